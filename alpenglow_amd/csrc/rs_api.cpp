// Host side of libalpenglow_rs.so: the C ABI declared in include/alpenglow_rs.h.  This file holds
// the context, the batch encode / decode and the per-call encoder / decoder with its mailbox
// server; rs_coder_api.cpp the coder, crypto_api.cpp the hashes, ciphers and signatures,
// wire_api.cpp the wire format.
//
// Mirrors three reference interfaces on top of the HIP kernels (the rs_*.hip TUs, rs_launch.hpp):
//   * the reed-solomon-simd 3.1.0 encoder/decoder API the reference wrapper calls
//     (reed_solomon.rs:9,64-66,96-125,150-180,214-226)
//   * ReedSolomonCoder (reed_solomon.rs:47-232) and the ValidatedShreds checks
//     (validated_shreds.rs:34-114) in front of it (rs_coder_api.cpp)
//   * batched, device-resident forms of the encode/decode for throughput
// All Reed-Solomon arithmetic runs on the GPU; the host does argument validation,
// padding/splitting (byte copies), pattern bookkeeping and table setup only.  There is
// no CPU compute fallback: without a device every call fails with AG_RS_ERR_NO_DEVICE.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstddef>
#include <cstdlib>
#include <cstring>
#include <new>
#include <utility>
#include <vector>

#include "../../include/alpenglow_rs.h"
#include "gf16.hpp"
#include "rs_ctx.hpp"
#include "rs_launch.hpp"
#include "rs_patterns.hpp"

using namespace ag::host;  // the context's buffers and the helpers shared with the other host files
using ag::lowrate_chunk;
using ag::mc_chunk;
using ag::padded_shard;
using ag::xform_points;

namespace {

// Host-memory calls: bytes (in + out) per staging group; two groups in flight.
constexpr size_t kStageGroupBytes = size_t{64} << 20;

// One codeword through the device, zero-copy: the kernels read the originals from and
// write the recovery shards to mapped pinned host memory (a 32-shard slice is 32 KiB each
// way; two DMA copies and their scheduling cost more than the kernel's PCIe accesses).
// The single-codeword calls (one slice per call, the reference's pattern) wait for their
// microseconds of device work by polling the stream: hipStreamSynchronize's blocking wait
// added ~9 us per call over the kernel time (profiles/r04_call_latency_hip_api_stats.csv).
int spin_sync(ag_rs_ctx* c) {
  for (;;) {
    const hipError_t e = hipStreamQuery(c->stream);
    if (e == hipSuccess) return AG_RS_OK;
    if (e != hipErrorNotReady) return AG_RS_ERR_DEVICE;
  }
}

// ---- per-call server: one single-tile 32-point job through the mailbox ----------------
// A 32:32 codeword of S <= 4 KiB (S % 64 == 0) is one tile of xform8: the resident server
// runs it without a kernel dispatch or completion signal (tools/latency: one slice's shred
// was dispatch + kernel + signal).  Started on first use, restarted when it has idled out.
constexpr uint64_t kServerIdleTicks = 2000000;  // 20 ms of the 100 MHz wall clock
bool server_fits(ag_rs_ctx* c, size_t k, size_t m, size_t S) {
  return !c->server_broken && k == 32 && m == 32 && S % 64 == 0 && S >= 64 && S <= 64 * 64;
}
ag::XformParams one_tile(uint8_t* in, size_t in_stride, uint8_t* out, size_t out_stride, size_t S) {
  ag::XformParams p = codeword_xform(in, in_stride, S, 1, S / 64);
  p.out = out;  // (not behind the inputs: each side of the staging has its own stride)
  p.out_block_stride = out_stride;
  p.n_in = 32;
  p.n_out = 32;
  return p;
}
// `stage`: the pinned buffer the job reads and writes (abandoned on a timeout).  `dp`: the
// kJobDecodePk parameters (then `p` is unused).
int server_job(ag_rs_ctx* c, uint32_t kind, const ag::XformParams& p, uint64_t mask, PinBuf& stage,
               const ag::DecodeXParams* dp = nullptr) {
  if (!c->mb) {
    void* h = nullptr;
    AG_HIP(hipHostMalloc(&h, sizeof(ag::LatencyMailbox), hipHostMallocMapped | hipHostMallocCoherent));
    std::memset(h, 0, sizeof(ag::LatencyMailbox));
    void* d = nullptr;
    if (hipHostGetDevicePointer(&d, h, 0) != hipSuccess ||
        hipStreamCreateWithFlags(&c->server_stream, hipStreamNonBlocking) != hipSuccess) {
      (void)hipHostFree(h);
      c->server_stream = nullptr;
      return AG_RS_ERR_DEVICE;
    }
    c->mb = static_cast<ag::LatencyMailbox*>(h);
    c->mb_dev = static_cast<ag::LatencyMailbox*>(d);
  }
  // the server caches part of the log table at launch (kJobDecodePk's locator)
  int st = c->ensure_tables();
  if (st) return st;
  ag::LatencyMailbox* mb = c->mb;
  // Retire a job that did not complete: a queued or slow server that wakes later finds a quit
  // job instead.  It may already be inside the job, so the staging buffer the job names is
  // abandoned (kept allocated, never reused: `stage` is left empty, and the encoder / decoder
  // that owned it drops its received shards, see pin_lost) and later calls take the launch path.
  auto retire = [&]() {
    c->server_broken = true;
    mb->kind = ag::kJobQuit;
    __atomic_store_n(&mb->doorbell, ++c->server_seq, __ATOMIC_RELEASE);
    c->abandoned_pins.push_back(std::move(stage));
    return AG_RS_ERR_DEVICE;
  };
  if (c->fail_next_server_job) {
    c->fail_next_server_job = false;
    return retire();
  }
  mb->kind = kind;
  mb->mask = mask;
  // parameters only when their bytes changed (the server reuses its copy of the same version;
  // a fresh server launch holds no copy and reads them)
  if (dp) {
    if (std::memcmp(static_cast<const void*>(&mb->dp), dp, sizeof *dp) != 0 || c->server_dp_seq == 0) {
      std::memcpy(static_cast<void*>(&mb->dp), dp, sizeof *dp);
      mb->dp_seq = ++c->server_dp_seq;
    }
  } else if (std::memcmp(static_cast<const void*>(&mb->p), &p, sizeof p) != 0 || c->server_p_seq == 0) {
    std::memcpy(static_cast<void*>(&mb->p), &p, sizeof p);
    mb->p_seq = ++c->server_p_seq;
  }
  if (kind < 4) ++c->server_jobs[kind];
  const uint32_t seq = ++c->server_seq;
  __atomic_store_n(&mb->doorbell, seq, __ATOMIC_RELEASE);  // x86: the job's fields are visible first
  const auto t0 = std::chrono::steady_clock::now();
  for (unsigned spins = 0;; ++spins) {
    if (__atomic_load_n(&mb->done, __ATOMIC_ACQUIRE) == seq) return AG_RS_OK;
    if (__atomic_load_n(&mb->alive, __ATOMIC_ACQUIRE) == 0) {
      // no server (first call, or it idled out -- possibly just after this doorbell)
      if (__atomic_load_n(&mb->done, __ATOMIC_ACQUIRE) == seq) return AG_RS_OK;
      __atomic_store_n(&mb->alive, 2u, __ATOMIC_RELEASE);
      if (ag::launch_latency_server(c->mb_dev, kServerIdleTicks, c->dtables().log, c->server_stream) != hipSuccess) {
        __atomic_store_n(&mb->alive, 0u, __ATOMIC_RELEASE);
        return AG_RS_ERR_DEVICE;
      }
    }
    if ((spins & 1023) == 1023 && std::chrono::steady_clock::now() - t0 > std::chrono::seconds(5))
      return retire();
    __builtin_ia32_pause();
  }
}

// One codeword staged in `pin` (originals at 0, recovery shards at k * S): the recovery shards
// are computed in place.
int run_one_encode(ag_rs_ctx* c, size_t k, size_t m, size_t S, PinBuf& pin) {
  int st;
  if ((st = c->enter())) return st;
  const size_t ob = k * S, rb = m * S;
  uint8_t* pd = pin.dev<uint8_t>();
  if (server_fits(c, k, m, S)) return server_job(c, ag::kJobEncode32, one_tile(pd, ob, pd + ob, rb, S), 0, pin);
  if ((st = encode_device(c, k, m, S, 1, pd, ob, pd + ob, rb))) return st;
  return spin_sync(c);
}

}  // namespace

namespace ag::host {
// One codeword decoded on the device, zero-copy like run_one_encode: originals and recovery
// shards staged in `pin` (originals at 0, recovery at k * S), restored originals written in
// place, and with `coding` the re-encode of every recovery shard from the completed originals
// (ReedSolomonCoder::deshred's encode_coding_from_data, reed_solomon.rs:206) at (k + m) * S
// -- or, when the received shards are exactly the m recovery shards, *coding_src points at
// those (the re-encode reproduces them bit for bit).  EXACT runs as ANY_K when exactly k
// shards are present: k shards fix the codeword, so both decoders return its originals for
// any input bytes.
int run_one_decode(ag_rs_ctx* c, size_t k, size_t m, size_t S, PinBuf& pin, const uint8_t* opres,
                   const uint8_t* rpres, int mode, bool coding, const uint8_t** coding_src) {
  int st;
  if ((st = c->enter())) return st;
  const size_t ob = k * S, rb = m * S;
  size_t present = 0;
  for (size_t i = 0; i < k; ++i) present += opres[i] != 0;
  for (size_t i = 0; i < m; ++i) present += rpres[i] != 0;
  if (present < k) return AG_RS_ERR_NOT_ENOUGH_SHARDS;
  if (present == k) mode = AG_RS_DECODE_ANY_K;
  uint8_t* pd = pin.dev<uint8_t>();
  // exactly k shards, all of them recovery shards: the completed codeword passes through
  // them, so its re-encoded recovery shards are the received ones (bit for bit)
  size_t nr = 0;
  for (size_t i = 0; i < m; ++i) nr += rpres[i] != 0;
  const bool reuse = coding && present == k && nr == m;
  if (coding_src) *coding_src = pin.as<uint8_t>() + (reuse ? ob : ob + rb);
  if (nr == m && (present == k || mode == AG_RS_DECODE_ANY_K) && server_fits(c, k, m, S)) {
    // the whole recovery set: the erased originals are one transform of it (the decode class
    // "none" route of decode_cols), run by the per-call server
    uint64_t mask = 0;
    for (size_t i = 0; i < k; ++i)
      if (!opres[i]) mask |= uint64_t{1} << i;
    std::fill(std::begin(c->last_classes), std::end(c->last_classes), uint64_t{0});
    ++c->last_classes[mask ? ag::kTransform : ag::kNone];
    if (mask && (st = server_job(c, (mask >> 16) ? ag::kJobDecode32 : ag::kJobDecode32Half,
                                 one_tile(pd + ob, rb, pd, ob, S), mask, pin)))
      return st;
    if (coding && !reuse &&
        (st = server_job(c, ag::kJobEncode32, one_tile(pd, ob, pd + ob + rb, rb, S), 0, pin)))
      return st;
    return AG_RS_OK;
  }
  const bool pk_size = S == 1024 || (S > 960 && S < 1024 && S % 2 == 0);  // 16 columns, tail included
  if (present == k && pk_size && k == 32 && m == 32 && !c->server_broken) {
    // exactly k = 32 of the 64 shreds of a 32:32 slice of 1 KiB shreds, or of 960 + T bytes
    // with a T >= 16-byte tail (the follower's deshred at its 32nd arriving shred):
    // decode_pk<-1>'s one-slice window decode on the server restores every absent data and
    // coding shred in place -- the codeword through the 32 survivors is unique, so the restored
    // coding shreds are the re-encode, bit for bit
    uint64_t pres = 0;
    for (size_t j = 0; j < m; ++j)
      if (rpres[j]) pres |= uint64_t{1} << j;
    for (size_t i = 0; i < k; ++i)
      if (opres[i]) pres |= uint64_t{1} << (32 + i);
    ag::DecodeXParams dp = codeword_decode_x(pd, (k + m) * S, S, 1, 16);
    dp.k = 32;
    dp.m = 32;
    dp.chunk = 32;
    dp.low_rate = 0;
    dp.per_lane = 1;
    dp.rows_w = 64;
    dp.any_k = 1;
    dp.fuse = 1;
    dp.tail_bytes = static_cast<uint32_t>(S % 64);
    std::fill(std::begin(c->last_classes), std::end(c->last_classes), uint64_t{0});
    ++c->last_classes[ag::kServerWindow64];
    if ((st = server_job(c, ag::kJobDecodePk, ag::XformParams{}, pres, pin, &dp))) return st;
    if (coding_src) *coding_src = pin.as<uint8_t>() + ob;  // the whole coding set, in place
    return AG_RS_OK;
  }
  if ((st = decode_device(c, k, m, S, 1, pd, ob, pd + ob, rb, opres, rpres, 1, mode))) return st;
  if (coding && !reuse && (st = encode_device(c, k, m, S, 1, pd, ob, pd + ob + rb, rb))) return st;
  return spin_sync(c);
}
}  // namespace ag::host

// =====================================================================================
// C ABI
// =====================================================================================
extern "C" {

const char* ag_rs_status_string(int s) {
  switch (s) {
    case AG_RS_OK: return "ok";
    case AG_RS_ERR_INVALID_SHARD_SIZE: return "invalid shard size";
    case AG_RS_ERR_DIFFERENT_SHARD_SIZE: return "different shard size";
    case AG_RS_ERR_TOO_FEW_ORIGINAL_SHARDS: return "too few original shards";
    case AG_RS_ERR_TOO_MANY_ORIGINAL_SHARDS: return "too many original shards";
    case AG_RS_ERR_INVALID_ORIGINAL_SHARD_INDEX: return "invalid original shard index";
    case AG_RS_ERR_INVALID_RECOVERY_SHARD_INDEX: return "invalid recovery shard index";
    case AG_RS_ERR_DUPLICATE_ORIGINAL_SHARD_INDEX: return "duplicate original shard index";
    case AG_RS_ERR_DUPLICATE_RECOVERY_SHARD_INDEX: return "duplicate recovery shard index";
    case AG_RS_ERR_NOT_ENOUGH_SHARDS: return "not enough shards";
    case AG_RS_ERR_UNSUPPORTED_SHARD_COUNT: return "unsupported shard count";
    case AG_RS_ERR_TOO_MUCH_DATA: return "too much data";
    case AG_RS_ERR_INVALID_PADDING: return "invalid padding";
    case AG_RS_ERR_INVALID_LAYOUT: return "invalid layout";
    case AG_RS_ERR_BAD_ENCODING: return "bad encoding";
    case AG_RS_ERR_INVALID_ARGUMENT: return "invalid argument";
    case AG_RS_ERR_NO_DEVICE: return "no HIP device";
    case AG_RS_ERR_DEVICE: return "HIP runtime error";
    case AG_RS_ERR_OUT_OF_MEMORY: return "out of device memory";
    case AG_RS_ERR_NOT_RESTORED: return "shard not restored";
    default: return "unknown status";
  }
}

int ag_rs_abi_version(void) { return AG_RS_ABI_VERSION; }

int ag_rs_device_count(int* count) {
  if (!count) return AG_RS_ERR_INVALID_ARGUMENT;
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) n = 0;
  *count = n;
  return AG_RS_OK;
}

int ag_rs_ctx_create(int device, ag_rs_ctx** out) {
  if (!out) return AG_RS_ERR_INVALID_ARGUMENT;
  *out = nullptr;
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return AG_RS_ERR_NO_DEVICE;
  if (device < 0 || device >= n) return AG_RS_ERR_NO_DEVICE;
  if (hipSetDevice(device) != hipSuccess) return AG_RS_ERR_DEVICE;
  auto* c = new (std::nothrow) ag_rs_ctx();
  if (!c) return AG_RS_ERR_OUT_OF_MEMORY;
  c->device = device;
  if (hipStreamCreate(&c->own_stream) != hipSuccess) {
    delete c;
    return AG_RS_ERR_DEVICE;
  }
  c->stream = c->own_stream;
  *out = c;
  return AG_RS_OK;
}

void ag_rs_ctx_destroy(ag_rs_ctx* c) { delete c; }

// A stream switch first drains the old stream (its queued kernels may still read the cached
// pattern uploads and scratch) and forgets the upload caches, whose copies were ordered on it.
static int switch_stream(ag_rs_ctx* c, hipStream_t s) {
  if (s == c->stream) return AG_RS_OK;
  if (c->enter() || hipStreamSynchronize(c->stream) != hipSuccess) return AG_RS_ERR_DEVICE;
  c->stream = s;
  c->forget_uploads();
  return AG_RS_OK;
}

int ag_rs_ctx_set_stream(ag_rs_ctx* c, void* s) {
  if (!c) return AG_RS_ERR_INVALID_ARGUMENT;
  return switch_stream(c, static_cast<hipStream_t>(s));
}

int ag_rs_ctx_reset_stream(ag_rs_ctx* c) {
  if (!c) return AG_RS_ERR_INVALID_ARGUMENT;
  return switch_stream(c, c->own_stream);
}

void* ag_rs_ctx_stream(ag_rs_ctx* c) { return c ? static_cast<void*>(c->stream) : nullptr; }

int ag_rs_ctx_synchronize(ag_rs_ctx* c) {
  if (!c) return AG_RS_ERR_INVALID_ARGUMENT;
  if (c->enter()) return AG_RS_ERR_DEVICE;
  return hipStreamSynchronize(c->stream) == hipSuccess ? AG_RS_OK : AG_RS_ERR_DEVICE;
}

int ag_rs_use_high_rate(size_t k, size_t m) {
  const int hr = ag::use_high_rate(k, m);
  return hr < 0 ? -AG_RS_ERR_UNSUPPORTED_SHARD_COUNT : hr;
}

// Test aid (not in the public header's contract): patterns per decoder class in the last
// decode on this context, indexed by ag::DecodeClass (rs_patterns.hpp).
int ag_rs_internal_last_decode_classes(ag_rs_ctx* c, uint64_t* out16) {
  if (!c || !out16) return AG_RS_ERR_INVALID_ARGUMENT;
  std::memcpy(out16, c->last_classes, sizeof c->last_classes);
  return AG_RS_OK;
}

// Test aid (not in the header): the W = 64 window kernels (DecodeXKernelBit) the last coder
// deshred batch on the context launched.
int ag_rs_internal_last_window_kernels(ag_rs_ctx* c, uint32_t* out) {
  if (!c || !out) return AG_RS_ERR_INVALID_ARGUMENT;
  *out = c->last_window_kernels;
  return AG_RS_OK;
}

// Test aid (not in the header): per-call server jobs posted on the context, per LatencyJob kind
// (encode, decode, decode half, decode_pk).
int ag_rs_internal_server_jobs(ag_rs_ctx* c, uint64_t* out4) {
  if (!c || !out4) return AG_RS_ERR_INVALID_ARGUMENT;
  std::copy(std::begin(c->server_jobs), std::end(c->server_jobs), out4);
  return AG_RS_OK;
}

// Test aid (not in the header): the context's next per-call server job takes the timeout path
// (retired, staging abandoned, server path off) without waiting 5 s.
int ag_rs_internal_fail_next_server_job(ag_rs_ctx* c) {
  if (!c) return AG_RS_ERR_INVALID_ARGUMENT;
  c->fail_next_server_job = true;
  return AG_RS_OK;
}

// Test aid (not in the header): the encode kernels (ag::EncodeKernelBit) the last
// ag_rs_encode_batch call on this context launched.
int ag_rs_internal_last_encode_kernels(ag_rs_ctx* c, uint32_t* out) {
  if (!c || !out) return AG_RS_ERR_INVALID_ARGUMENT;
  *out = c->last_encode_kernels;
  return AG_RS_OK;
}

// Test aid (not in the header): the leaf-kernel classes (ag::MerkleLeafKernelBit) the last Merkle
// build on this context launched -- uniform size with aligned rows, uniform size through the byte
// loader, or one size per slice.
int ag_rs_internal_last_merkle_kernels(ag_rs_ctx* c, uint32_t* out) {
  if (!c || !out) return AG_RS_ERR_INVALID_ARGUMENT;
  *out = c->last_merkle_kernels;
  return AG_RS_OK;
}

// Test aid (not in the header): out[0] = the slices the last composed deshred call on this
// context (ag_shredder_deshred_batch / _var / _kind) decoded again with EXACT, out[1] = the
// batched EXACT coder passes it made for them.
int ag_rs_internal_last_exact_rerun(ag_rs_ctx* c, uint64_t out[2]) {
  if (!c || !out) return AG_RS_ERR_INVALID_ARGUMENT;
  out[0] = c->last_rerun_slices;
  out[1] = c->last_rerun_passes;
  return AG_RS_OK;
}

int ag_rs_has_fast_path(size_t k, size_t m, size_t S) {
  // shard sizes that are not whole 64-byte chunks run restrided (padded) on the same kernels
  if (S == 0 || S % 2) return 0;
  const size_t Sp = padded_shard(S);
  return xform_points(k, m, Sp) || mc_chunk(k, m, Sp) || lowrate_chunk(k, m, Sp) ? 1 : 0;
}

int ag_rs_encode_batch(ag_rs_ctx* c, size_t k, size_t m, size_t S, size_t nblocks, const uint8_t* orig,
                       size_t ostride, uint8_t* rec, size_t rstride, int memory) {
  if (!c || (nblocks && (!orig || !rec))) return AG_RS_ERR_INVALID_ARGUMENT;
  int st = check_geometry(k, m, S);
  if (st) return st;
  if (ostride < k * S || rstride < m * S) return AG_RS_ERR_INVALID_ARGUMENT;
  if ((st = c->enter())) return st;
  c->last_encode_kernels = 0;
  if (memory == AG_RS_MEM_DEVICE) return encode_device(c, k, m, S, nblocks, orig, ostride, rec, rstride);
  if (memory != AG_RS_MEM_HOST) return AG_RS_ERR_INVALID_ARGUMENT;
  // host memory: groups of blocks through two device staging slots, H2D / compute / D2H
  // overlapped across groups (pinned host buffers give the full PCIe rate)
  const size_t in_b = k * S, out_b = m * S;
  const size_t group = std::max<size_t>(1, kStageGroupBytes / (in_b + out_b));
  if ((st = c->ensure_copy_streams())) return st;
  size_t g = 0;
  for (size_t b0 = 0; b0 < nblocks; b0 += group, ++g) {
    const size_t n = std::min(group, nblocks - b0);
    auto& sl = c->slot[g & 1];
    AG_HIP(hipStreamWaitEvent(c->h2d, sl.down, 0));  // slot free: its previous download is done
    if ((st = sl.in.ensure(group * in_b, c->h2d)) || (st = sl.out.ensure(group * out_b, c->h2d))) return st;
    AG_HIP(hipMemcpy2DAsync(sl.in.ptr, in_b, orig + b0 * ostride, ostride, in_b, n, hipMemcpyHostToDevice, c->h2d));
    AG_HIP(hipEventRecord(sl.up, c->h2d));
    AG_HIP(hipStreamWaitEvent(c->stream, sl.up, 0));
    if ((st = encode_device(c, k, m, S, n, sl.in.as<uint8_t>(), in_b, sl.out.as<uint8_t>(), out_b))) break;
    AG_HIP(hipEventRecord(sl.done, c->stream));
    AG_HIP(hipStreamWaitEvent(c->d2h, sl.done, 0));
    AG_HIP(hipMemcpy2DAsync(rec + b0 * rstride, rstride, sl.out.ptr, out_b, out_b, n, hipMemcpyDeviceToHost, c->d2h));
    AG_HIP(hipEventRecord(sl.down, c->d2h));
  }
  AG_HIP(hipStreamSynchronize(c->stream));
  AG_HIP(hipStreamSynchronize(c->d2h));
  return st;
}

int ag_rs_decode_batch(ag_rs_ctx* c, size_t k, size_t m, size_t S, size_t nblocks, uint8_t* orig, size_t ostride,
                       const uint8_t* rec, size_t rstride, const uint8_t* opres, const uint8_t* rpres, size_t npat,
                       int mode, int memory) {
  if (!c || !opres || !rpres || (nblocks && (!orig || !rec))) return AG_RS_ERR_INVALID_ARGUMENT;
  int st = check_geometry(k, m, S);
  if (st) return st;
  if (npat != 1 && npat != nblocks) return AG_RS_ERR_INVALID_ARGUMENT;
  if (mode != AG_RS_DECODE_EXACT && mode != AG_RS_DECODE_ANY_K) return AG_RS_ERR_INVALID_ARGUMENT;
  if (ostride < k * S || rstride < m * S) return AG_RS_ERR_INVALID_ARGUMENT;
  if ((st = c->enter())) return st;
  if (memory == AG_RS_MEM_DEVICE)
    return decode_device(c, k, m, S, nblocks, orig, ostride, rec, rstride, opres, rpres, npat, mode);
  if (memory != AG_RS_MEM_HOST) return AG_RS_ERR_INVALID_ARGUMENT;
  // pattern validity is checked up front so that an error leaves `orig` untouched
  for (size_t p = 0; p < npat; ++p) {
    size_t cnt = 0;
    for (size_t i = 0; i < k; ++i) cnt += opres[p * k + i] != 0;
    for (size_t i = 0; i < m; ++i) cnt += rpres[p * m + i] != 0;
    if (cnt < k) return AG_RS_ERR_NOT_ENOUGH_SHARDS;
  }
  const size_t o_b = k * S, r_b = m * S;
  const size_t group = std::max<size_t>(1, kStageGroupBytes / (o_b + r_b));
  if ((st = c->ensure_copy_streams())) return st;
  // One pattern: move only what the kernels read and write -- present originals up (none
  // when the transform path restores from the full recovery set), erased originals down.
  bool up_orig_all = npat > 1, down_all = npat > 1;
  bool need_orig = true;
  if (npat == 1) {
    size_t nr = 0, no = 0;
    for (size_t i = 0; i < m; ++i) nr += rpres[i] != 0;
    for (size_t i = 0; i < k; ++i) no += opres[i] != 0;
    if (no == k) return AG_RS_OK;  // nothing to restore
    need_orig = !ag::transform_restores(k, m, S, mode, nr);
  }
  size_t g = 0;
  for (size_t b0 = 0; b0 < nblocks; b0 += group, ++g) {
    const size_t n = std::min(group, nblocks - b0);
    auto& sl = c->slot[g & 1];
    AG_HIP(hipStreamWaitEvent(c->h2d, sl.down, 0));
    if ((st = sl.in.ensure(group * r_b, c->h2d)) || (st = sl.out.ensure(group * o_b, c->h2d))) return st;
    AG_HIP(hipMemcpy2DAsync(sl.in.ptr, r_b, rec + b0 * rstride, rstride, r_b, n, hipMemcpyHostToDevice, c->h2d));
    if (up_orig_all) {
      AG_HIP(hipMemcpy2DAsync(sl.out.ptr, o_b, orig + b0 * ostride, ostride, o_b, n, hipMemcpyHostToDevice, c->h2d));
    } else if (need_orig) {
      for (size_t i = 0; i < k; ++i)
        if (opres[i])
          AG_HIP(hipMemcpy2DAsync(sl.out.as<uint8_t>() + i * S, o_b, orig + b0 * ostride + i * S, ostride, S, n,
                                  hipMemcpyHostToDevice, c->h2d));
    }
    AG_HIP(hipEventRecord(sl.up, c->h2d));
    AG_HIP(hipStreamWaitEvent(c->stream, sl.up, 0));
    const uint8_t* op = npat > 1 ? opres + b0 * k : opres;
    const uint8_t* rp = npat > 1 ? rpres + b0 * m : rpres;
    if ((st = decode_device(c, k, m, S, n, sl.out.as<uint8_t>(), o_b, sl.in.as<uint8_t>(), r_b, op, rp,
                            npat > 1 ? n : 1, mode)))
      break;
    AG_HIP(hipEventRecord(sl.done, c->stream));
    AG_HIP(hipStreamWaitEvent(c->d2h, sl.done, 0));
    if (down_all) {
      AG_HIP(hipMemcpy2DAsync(orig + b0 * ostride, ostride, sl.out.ptr, o_b, o_b, n, hipMemcpyDeviceToHost, c->d2h));
    } else {
      for (size_t i = 0; i < k; ++i)
        if (!opres[i])
          AG_HIP(hipMemcpy2DAsync(orig + b0 * ostride + i * S, ostride, sl.out.as<uint8_t>() + i * S, o_b, S, n,
                                  hipMemcpyDeviceToHost, c->d2h));
    }
    AG_HIP(hipEventRecord(sl.down, c->d2h));
  }
  AG_HIP(hipStreamSynchronize(c->stream));
  AG_HIP(hipStreamSynchronize(c->d2h));
  return st;
}

int ag_rs_fill_splitmix(ag_rs_ctx* c, uint8_t* dst, size_t nblocks, size_t block_bytes, size_t dst_stride,
                        uint64_t seed_base) {
  if (!c || (nblocks && !dst) || block_bytes % 8 || dst_stride < block_bytes) return AG_RS_ERR_INVALID_ARGUMENT;
  if (c->enter()) return AG_RS_ERR_DEVICE;
  return ag::launch_fill_splitmix(dst, nblocks, block_bytes, dst_stride, seed_base, c->stream) == hipSuccess
             ? AG_RS_OK
             : AG_RS_ERR_DEVICE;
}

// ---- crate API mirror: ReedSolomonEncoder / ReedSolomonDecoder (the handles: rs_ctx.hpp) ----

int ag_rs_encoder_reset(ag_rs_encoder* e, size_t k, size_t m, size_t S) {
  if (!e) return AG_RS_ERR_INVALID_ARGUMENT;
  int st = check_geometry(k, m, S);
  if (st) return st;
  // the staging only grows; its bytes need no clearing (encode reads the k added originals)
  if ((k + m) * S > e->pin.size && ((st = e->ctx->enter()) || (st = e->pin.ensure((k + m) * S)))) return st;
  e->k = k;
  e->m = m;
  e->S = S;
  e->received = 0;
  e->encoded = false;
  return AG_RS_OK;
}

int ag_rs_encoder_new(ag_rs_ctx* c, size_t k, size_t m, size_t S, ag_rs_encoder** out) {
  if (!c || !out) return AG_RS_ERR_INVALID_ARGUMENT;
  *out = nullptr;
  auto* e = new (std::nothrow) ag_rs_encoder();
  if (!e) return AG_RS_ERR_OUT_OF_MEMORY;
  e->ctx = c;
  const int st = ag_rs_encoder_reset(e, k, m, S);
  if (st) {
    delete e;
    return st;
  }
  *out = e;
  return AG_RS_OK;
}

int ag_rs_encoder_new_on_device(int device, size_t k, size_t m, size_t S, ag_rs_encoder** out) {
  if (!out) return AG_RS_ERR_INVALID_ARGUMENT;
  *out = nullptr;
  ag_rs_ctx* c = nullptr;
  int st = ag_rs_ctx_create(device, &c);
  if (st) return st;
  if ((st = ag_rs_encoder_new(c, k, m, S, out))) {
    ag_rs_ctx_destroy(c);
    return st;
  }
  (*out)->owned.reset(c);
  return AG_RS_OK;
}

// A server job that timed out abandoned the object's staging (server_job: `stage` left
// empty): the shards it held are gone, so the object starts a new round in a fresh buffer.
static int encoder_pin_lost(ag_rs_encoder* e) {
  e->received = 0;
  e->encoded = false;
  int st = e->ctx->enter();
  return st ? st : e->pin.ensure((e->k + e->m) * e->S);
}

int ag_rs_encoder_add_original_shard(ag_rs_encoder* e, const uint8_t* shard, size_t len) {
  if (!e || (!shard && len)) return AG_RS_ERR_INVALID_ARGUMENT;
  if (!e->pin.ptr) {
    const int st = encoder_pin_lost(e);
    if (st) return st;
  }
  if (e->encoded) {  // the crate resets the received set once a result is dropped
    e->received = 0;
    e->encoded = false;
  }
  if (e->received == e->k) return AG_RS_ERR_TOO_MANY_ORIGINAL_SHARDS;
  if (len != e->S) return AG_RS_ERR_DIFFERENT_SHARD_SIZE;
  std::memcpy(e->orig() + e->received * e->S, shard, len);
  ++e->received;
  return AG_RS_OK;
}

int ag_rs_encoder_encode(ag_rs_encoder* e) {
  if (!e) return AG_RS_ERR_INVALID_ARGUMENT;
  if (!e->pin.ptr) e->received = 0;  // staging abandoned by a timed-out job: nothing received
  if (e->received != e->k) return AG_RS_ERR_TOO_FEW_ORIGINAL_SHARDS;
  const int st = run_one_encode(e->ctx, e->k, e->m, e->S, e->pin);
  if (st) {
    if (!e->pin.ptr) e->received = 0;
    e->encoded = false;
    return st;
  }
  e->encoded = true;
  return AG_RS_OK;
}

int ag_rs_encoder_recovery(const ag_rs_encoder* e, size_t index, const uint8_t** shard, size_t* len) {
  if (!e || !shard || !len) return AG_RS_ERR_INVALID_ARGUMENT;
  if (!e->encoded || index >= e->m) return AG_RS_ERR_INVALID_ARGUMENT;
  *shard = e->rec() + index * e->S;
  *len = e->S;
  return AG_RS_OK;
}

void ag_rs_encoder_free(ag_rs_encoder* e) { delete e; }

int ag_rs_decoder_reset(ag_rs_decoder* d, size_t k, size_t m, size_t S) {
  if (!d) return AG_RS_ERR_INVALID_ARGUMENT;
  int st = check_geometry(k, m, S);
  if (st) return st;
  if ((k + 2 * m) * S > d->pin.size && ((st = d->ctx->enter()) || (st = d->pin.ensure((k + 2 * m) * S))))
    return st;
  d->k = k;
  d->m = m;
  d->S = S;
  d->opres.assign(k, 0);
  d->rpres.assign(m, 0);
  d->restored.assign(k, 0);
  d->no = d->nr = 0;
  d->decoded = false;
  return AG_RS_OK;
}

int ag_rs_decoder_new(ag_rs_ctx* c, size_t k, size_t m, size_t S, ag_rs_decoder** out) {
  if (!c || !out) return AG_RS_ERR_INVALID_ARGUMENT;
  *out = nullptr;
  auto* d = new (std::nothrow) ag_rs_decoder();
  if (!d) return AG_RS_ERR_OUT_OF_MEMORY;
  d->ctx = c;
  const int st = ag_rs_decoder_reset(d, k, m, S);
  if (st) {
    delete d;
    return st;
  }
  *out = d;
  return AG_RS_OK;
}

int ag_rs_decoder_new_on_device(int device, size_t k, size_t m, size_t S, ag_rs_decoder** out) {
  if (!out) return AG_RS_ERR_INVALID_ARGUMENT;
  *out = nullptr;
  ag_rs_ctx* c = nullptr;
  int st = ag_rs_ctx_create(device, &c);
  if (st) return st;
  if ((st = ag_rs_decoder_new(c, k, m, S, out))) {
    ag_rs_ctx_destroy(c);
    return st;
  }
  (*out)->owned.reset(c);
  return AG_RS_OK;
}

// The decoder's counterpart of encoder_pin_lost: every received shard is dropped.
static int decoder_pin_lost(ag_rs_decoder* d) {
  std::fill(d->opres.begin(), d->opres.end(), 0);
  std::fill(d->rpres.begin(), d->rpres.end(), 0);
  std::fill(d->restored.begin(), d->restored.end(), 0);
  d->no = d->nr = 0;
  d->decoded = false;
  int st = d->ctx->enter();
  return st ? st : d->pin.ensure((d->k + 2 * d->m) * d->S);
}

static void decoder_begin_round(ag_rs_decoder* d) {
  if (!d->decoded) return;
  std::fill(d->opres.begin(), d->opres.end(), 0);
  std::fill(d->rpres.begin(), d->rpres.end(), 0);
  std::fill(d->restored.begin(), d->restored.end(), 0);
  d->no = d->nr = 0;
  d->decoded = false;
}

int ag_rs_decoder_add_original_shard(ag_rs_decoder* d, size_t index, const uint8_t* shard, size_t len) {
  if (!d || (!shard && len)) return AG_RS_ERR_INVALID_ARGUMENT;
  if (!d->pin.ptr) {
    const int st = decoder_pin_lost(d);
    if (st) return st;
  }
  decoder_begin_round(d);
  if (index >= d->k) return AG_RS_ERR_INVALID_ORIGINAL_SHARD_INDEX;
  if (d->opres[index]) return AG_RS_ERR_DUPLICATE_ORIGINAL_SHARD_INDEX;
  if (len != d->S) return AG_RS_ERR_DIFFERENT_SHARD_SIZE;
  std::memcpy(d->orig() + index * d->S, shard, len);
  d->opres[index] = 1;
  ++d->no;
  return AG_RS_OK;
}

int ag_rs_decoder_add_recovery_shard(ag_rs_decoder* d, size_t index, const uint8_t* shard, size_t len) {
  if (!d || (!shard && len)) return AG_RS_ERR_INVALID_ARGUMENT;
  if (!d->pin.ptr) {
    const int st = decoder_pin_lost(d);
    if (st) return st;
  }
  decoder_begin_round(d);
  if (index >= d->m) return AG_RS_ERR_INVALID_RECOVERY_SHARD_INDEX;
  if (d->rpres[index]) return AG_RS_ERR_DUPLICATE_RECOVERY_SHARD_INDEX;
  if (len != d->S) return AG_RS_ERR_DIFFERENT_SHARD_SIZE;
  std::memcpy(d->rec() + index * d->S, shard, len);
  d->rpres[index] = 1;
  ++d->nr;
  return AG_RS_OK;
}

int ag_rs_decoder_decode(ag_rs_decoder* d) {
  if (!d) return AG_RS_ERR_INVALID_ARGUMENT;
  if (!d->pin.ptr) {  // staging abandoned by a timed-out job: nothing received
    const int st = decoder_pin_lost(d);
    if (st) return st;
  }
  if (d->no + d->nr < d->k) return AG_RS_ERR_NOT_ENOUGH_SHARDS;
  std::fill(d->restored.begin(), d->restored.end(), 0);
  if (d->no < d->k) {
    // exact crate semantics: decode from every present shard
    const int st = run_one_decode(d->ctx, d->k, d->m, d->S, d->pin, d->opres.data(), d->rpres.data(),
                                  AG_RS_DECODE_EXACT, false, nullptr);
    if (st) {
      if (!d->pin.ptr) (void)decoder_pin_lost(d);
      return st;
    }
    for (size_t i = 0; i < d->k; ++i) d->restored[i] = d->opres[i] ? 0 : 1;
  }
  d->decoded = true;
  return AG_RS_OK;
}

int ag_rs_decoder_restored_original(const ag_rs_decoder* d, size_t index, const uint8_t** shard, size_t* len) {
  if (!d || !shard || !len) return AG_RS_ERR_INVALID_ARGUMENT;
  if (!d->decoded || index >= d->k || !d->restored[index]) return AG_RS_ERR_NOT_RESTORED;
  *shard = d->orig() + index * d->S;
  *len = d->S;
  return AG_RS_OK;
}

void ag_rs_decoder_free(ag_rs_decoder* d) { delete d; }

}  // extern "C"
