// Host side of libalpenglow_rs.so: the C ABI declared in include/alpenglow_rs.h.
//
// Mirrors three reference interfaces on top of the HIP kernels (the rs_*.hip TUs, rs_launch.hpp):
//   * the reed-solomon-simd 3.1.0 encoder/decoder API the reference wrapper calls
//     (reed_solomon.rs:9,64-66,96-125,150-180,214-226)
//   * ReedSolomonCoder (reed_solomon.rs:47-232) and the ValidatedShreds checks
//     (validated_shreds.rs:34-114) in front of it
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
#include <memory>
#include <new>
#include <vector>

#include "../../include/alpenglow_rs.h"
#include "gf16.hpp"
#include "cipher.hpp"
#include "ed25519.hpp"
#include "slice.hpp"
#include "wire.hpp"
#include "merkle.hpp"
#include "rs_ctx.hpp"
#include "rs_launch.hpp"
#include "rs_patterns.hpp"
#include "shredder.hpp"

using namespace ag::host;  // the context's buffers and the helpers shared with the other host files
using ag::count_flags;
using ag::lowrate_chunk;
using ag::mc_chunk;
using ag::pack_flags;
using ag::pack_present_words;
using ag::padded_shard;
using ag::xform_points;

namespace {

// Host-memory calls: bytes (in + out) per staging group; two groups in flight.
constexpr size_t kStageGroupBytes = size_t{64} << 20;

}  // namespace

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

// Test aid (not in the header): the encode kernels (ag::EncodeKernelBit) the last
// ag_rs_encode_batch call on this context launched.
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

// Diagnostic (not in the header): the in-kernel duration of the last per-call server job on the
// coder's context, doorbell seen -> its stores released, then its four phases (kind read,
// parameters + cache invalidate, tile, release): ns[5], 0 before any job.
int ag_rs_internal_coder_last_job_ns(ag_rs_coder* coder, uint64_t* ns);

// Test aid (not in the header): the context's next per-call server job takes the timeout path
// (retired, staging abandoned, server path off) without waiting 5 s.
int ag_rs_internal_fail_next_server_job(ag_rs_ctx* c) {
  if (!c) return AG_RS_ERR_INVALID_ARGUMENT;
  c->fail_next_server_job = true;
  return AG_RS_OK;
}

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

// ---- slice Merkle trees --------------------------------------------------------------

size_t ag_merkle_height(size_t n) {
  size_t h = 0;
  for (size_t len = n; len > 1; len = (len + 1) / 2) ++h;
  return h;
}

size_t ag_merkle_node_count(size_t n) {
  size_t total = n;
  for (size_t len = n; len > 1;) {
    len = (len + 1) / 2;
    total += len;
  }
  return total;
}

int ag_merkle_empty_root(size_t height, uint8_t out[32]) {
  if (!out || height >= static_cast<size_t>(ag::kMerkleMaxHeight)) return AG_RS_ERR_INVALID_ARGUMENT;
  uint32_t er[ag::kMerkleMaxHeight][8];
  ag::merkle_empty_roots(er);
  for (int i = 0; i < 8; ++i)
    for (int b = 0; b < 4; ++b) out[4 * i + b] = static_cast<uint8_t>(er[height][i] >> (24 - 8 * b));
  return AG_RS_OK;
}

}  // extern "C"

namespace ag::host {
int ensure_empty_roots(ag_rs_ctx* c) {
  if (c->d_empty_roots.ptr) return AG_RS_OK;
  uint32_t er[ag::kMerkleMaxHeight][8];
  ag::merkle_empty_roots(er);
  int st = c->d_empty_roots.ensure(sizeof er, c->stream);
  if (st) return st;
  AG_HIP(hipMemcpy(c->d_empty_roots.ptr, er, sizeof er, hipMemcpyHostToDevice));
  return AG_RS_OK;
}
}  // namespace ag::host

extern "C" {

int ag_merkle_build_batch(ag_rs_ctx* c, size_t n_leaves, size_t leaf_bytes, size_t nslices, const uint8_t* leaves,
                          size_t leaf_stride, size_t slice_stride, uint8_t* roots, uint8_t* nodes,
                          size_t nodes_stride, uint8_t* proofs, size_t proofs_stride) {
  if (!c || n_leaves == 0 || n_leaves > AG_MERKLE_MAX_LEAVES || leaf_bytes >= (size_t{1} << 28))
    return AG_RS_ERR_INVALID_ARGUMENT;
  if (nslices == 0) return AG_RS_OK;
  if ((leaf_bytes && !leaves) || !roots || (n_leaves > 1 && leaf_stride < leaf_bytes) ||
      (nslices > 1 && slice_stride < (n_leaves - 1) * leaf_stride + leaf_bytes))
    return AG_RS_ERR_INVALID_ARGUMENT;
  const size_t h = ag_merkle_height(n_leaves);
  if ((nodes && (nodes_stride % 16 || (nslices > 1 && nodes_stride < 32 * ag_merkle_node_count(n_leaves)))) ||
      (proofs && (proofs_stride % 16 || (nslices > 1 && proofs_stride < 32 * h * n_leaves))) ||
      reinterpret_cast<uintptr_t>(roots) % 16 || reinterpret_cast<uintptr_t>(nodes) % 16 ||
      reinterpret_cast<uintptr_t>(proofs) % 16)
    return AG_RS_ERR_INVALID_ARGUMENT;
  if (c->enter()) return AG_RS_ERR_DEVICE;
  int st = ensure_empty_roots(c);
  if (st) return st;
  ag::MerkleBuildParams p{};
  p.leaves = leaves;
  p.leaf_stride = leaf_stride;
  p.slice_stride = slice_stride;
  p.leaf_bytes = static_cast<uint32_t>(leaf_bytes);
  p.n_leaves = static_cast<uint32_t>(n_leaves);
  p.nslices = nslices;
  p.empty_roots = c->d_empty_roots.as<uint32_t>();
  p.roots = roots;
  p.proofs = proofs;
  p.proofs_stride = proofs_stride;
  if (!nodes) {  // the levels are built in memory: scratch when the caller wants no nodes
    nodes_stride = (32 * ag_merkle_node_count(n_leaves) + 255) / 256 * 256;
    if ((st = c->d_merkle_nodes.ensure(nslices * nodes_stride, c->stream))) return st;
    nodes = c->d_merkle_nodes.as<uint8_t>();
  }
  c->last_merkle_kernels = 0;
  return ag::launch_merkle_build(p, nodes, nodes_stride, c->stream, &c->last_merkle_kernels) == hipSuccess
             ? AG_RS_OK
             : AG_RS_ERR_DEVICE;
}

namespace {
constexpr size_t kMerkleVarMaxSlices = size_t{1} << 27;  // (the var coder's limit)

// ag_merkle_build_batch_var's host-side checks (sizes on the host): 0 or the status
int merkle_var_check(size_t nslices, const uint32_t* leaf_bytes, const uint8_t* leaves, size_t slice_stride,
                     const uint8_t* roots, const uint8_t* nodes, size_t nodes_stride, const uint8_t* proofs,
                     size_t proofs_stride) {
  if (!leaf_bytes || !leaves || !roots || nslices > kMerkleVarMaxSlices) return AG_RS_ERR_INVALID_ARGUMENT;
  size_t max_s = 0;
  for (size_t b = 0; b < nslices; ++b) {
    if (leaf_bytes[b] == 0 || leaf_bytes[b] % 2) return AG_RS_ERR_INVALID_SHARD_SIZE;
    if (leaf_bytes[b] > AG_RS_MAX_DATA_PER_SHRED) return AG_RS_ERR_TOO_MUCH_DATA;
    max_s = std::max<size_t>(max_s, leaf_bytes[b]);
  }
  constexpr size_t n = AG_MERKLE_MAX_LEAVES;
  if (slice_stride < n * max_s ||
      (nodes && (nodes_stride % 16 || nodes_stride < 32 * ag_merkle_node_count(n))) ||
      (proofs && (proofs_stride % 16 || proofs_stride < 32 * ag_merkle_height(n) * n)) ||
      reinterpret_cast<uintptr_t>(roots) % 16 || reinterpret_cast<uintptr_t>(nodes) % 16 ||
      reinterpret_cast<uintptr_t>(proofs) % 16)
    return AG_RS_ERR_INVALID_ARGUMENT;
  return AG_RS_OK;
}
}  // namespace
}  // extern "C"

namespace ag::host {
// The launches of ag_merkle_build_batch_var over sizes already on the device (d_sizes; checked by
// the caller on the host): the composed shred hands over the table its coder stage uploaded.
int merkle_var_launch(ag_rs_ctx* c, size_t nslices, const uint32_t* d_sizes, const uint8_t* leaves,
                      size_t slice_stride, uint8_t* roots, uint8_t* nodes, size_t nodes_stride, uint8_t* proofs,
                      size_t proofs_stride) {
  int st = ensure_empty_roots(c);
  if (st) return st;
  ag::MerkleBuildParams p{};
  p.leaves = leaves;
  p.slice_stride = slice_stride;
  p.n_leaves = AG_MERKLE_MAX_LEAVES;
  p.nslices = nslices;
  p.empty_roots = c->d_empty_roots.as<uint32_t>();
  p.roots = roots;
  p.proofs = proofs;
  p.proofs_stride = proofs_stride;
  p.leaf_sizes = d_sizes;
  if (!nodes) {
    nodes_stride = (32 * ag_merkle_node_count(AG_MERKLE_MAX_LEAVES) + 255) / 256 * 256;
    if ((st = c->d_merkle_nodes.ensure(nslices * nodes_stride, c->stream))) return st;
    nodes = c->d_merkle_nodes.as<uint8_t>();
  }
  c->last_merkle_kernels = 0;
  return ag::launch_merkle_build(p, nodes, nodes_stride, c->stream, &c->last_merkle_kernels) == hipSuccess
             ? AG_RS_OK
             : AG_RS_ERR_DEVICE;
}
}  // namespace ag::host

extern "C" {

int ag_merkle_build_batch_var(ag_rs_ctx* c, size_t nslices, const uint32_t* leaf_bytes, const uint8_t* leaves,
                              size_t slice_stride, uint8_t* roots, uint8_t* nodes, size_t nodes_stride,
                              uint8_t* proofs, size_t proofs_stride) {
  if (!c) return AG_RS_ERR_INVALID_ARGUMENT;
  if (nslices == 0) return AG_RS_OK;
  int st = merkle_var_check(nslices, leaf_bytes, leaves, slice_stride, roots, nodes, nodes_stride, proofs,
                            proofs_stride);
  if (st) return st;
  if ((st = c->enter())) return st;
  // the sizes go up through pinned staging of their own (the coder's payload lengths keep theirs),
  // rewritten once its last upload has completed
  if (c->leaf_sizes_ev) AG_HIP(hipEventSynchronize(c->leaf_sizes_ev));
  else AG_HIP(hipEventCreateWithFlags(&c->leaf_sizes_ev, hipEventDisableTiming));
  if ((st = c->h_leaf_sizes.ensure(4 * nslices)) || (st = c->d_leaf_sizes.ensure(4 * nslices, c->stream))) return st;
  std::memcpy(c->h_leaf_sizes.ptr, leaf_bytes, 4 * nslices);
  AG_HIP(hipMemcpyAsync(c->d_leaf_sizes.ptr, c->h_leaf_sizes.ptr, 4 * nslices, hipMemcpyHostToDevice, c->stream));
  AG_HIP(hipEventRecord(c->leaf_sizes_ev, c->stream));
  return merkle_var_launch(c, nslices, c->d_leaf_sizes.as<uint32_t>(), leaves, slice_stride, roots, nodes,
                           nodes_stride, proofs, proofs_stride);
}

int ag_merkle_verify_batch(ag_rs_ctx* c, size_t n, size_t leaf_bytes, const uint8_t* leaves, size_t leaf_stride,
                           const uint32_t* index, const uint8_t* roots, size_t roots_stride, const uint8_t* proofs,
                           size_t proofs_stride, size_t height, uint8_t* ok) {
  if (!c || leaf_bytes >= (size_t{1} << 28) || height > static_cast<size_t>(ag::kMerkleMaxHeight))
    return AG_RS_ERR_INVALID_ARGUMENT;
  if (n == 0) return AG_RS_OK;
  if ((leaf_bytes && !leaves) || !index || !roots || !ok || (height && !proofs) || roots_stride % 16 ||
      proofs_stride % 16 || reinterpret_cast<uintptr_t>(roots) % 16 || reinterpret_cast<uintptr_t>(proofs) % 16 ||
      (n > 1 && leaf_stride < leaf_bytes))
    return AG_RS_ERR_INVALID_ARGUMENT;
  if (c->enter()) return AG_RS_ERR_DEVICE;
  ag::MerkleVerifyParams p{};
  p.leaves = leaves;
  p.leaf_stride = leaf_stride;
  p.leaf_bytes = static_cast<uint32_t>(leaf_bytes);
  p.height = static_cast<uint32_t>(height);
  p.index = index;
  p.roots = roots;
  p.roots_stride = roots_stride;
  p.proofs = proofs;
  p.proofs_stride = proofs_stride;
  p.n = n;
  p.ok = ok;
  return ag::launch_merkle_verify(p, c->stream) == hipSuccess ? AG_RS_OK : AG_RS_ERR_DEVICE;
}

// ---- block trees: the double-Merkle tree over a block's slice roots -----------------------

int ag_block_tree_batch(ag_rs_ctx* c, size_t nblocks, const uint32_t* count, const uint8_t* slice_roots,
                        uint8_t* block_hashes, uint8_t* nodes, size_t nodes_stride, uint8_t* proofs,
                        size_t proofs_stride) {
  static_assert(AG_BLOCK_MAX_SLICES == ag::kBlockMaxSlices);
  if (!c) return AG_RS_ERR_INVALID_ARGUMENT;
  if (nblocks == 0) return AG_RS_OK;
  if (!count || !slice_roots || !block_hashes || nblocks > 0x7FFFFFFFull) return AG_RS_ERR_INVALID_ARGUMENT;
  uint32_t mx = 0;
  for (size_t b = 0; b < nblocks; ++b) {
    if (count[b] == 0 || count[b] > AG_BLOCK_MAX_SLICES) return AG_RS_ERR_INVALID_ARGUMENT;
    mx = std::max(mx, count[b]);
  }
  // node count and height * count both grow with the count: the largest block sets the strides
  if ((reinterpret_cast<uintptr_t>(slice_roots) | reinterpret_cast<uintptr_t>(block_hashes) |
       reinterpret_cast<uintptr_t>(nodes) | reinterpret_cast<uintptr_t>(proofs)) % 16 ||
      (nodes && (nodes_stride % 16 || (nblocks > 1 && nodes_stride < 32 * ag_merkle_node_count(mx)))) ||
      (proofs && (proofs_stride % 16 || (nblocks > 1 && proofs_stride < 32 * ag_merkle_height(mx) * mx))))
    return AG_RS_ERR_INVALID_ARGUMENT;
  int st = c->enter();
  if (st || (st = ensure_empty_roots(c))) return st;
  // offsets and counts go up through pinned staging on the context stream, as the coder's
  // payload lengths do: the staging is rewritten once its last upload has completed
  if (c->block_meta_ev) AG_HIP(hipEventSynchronize(c->block_meta_ev));
  else AG_HIP(hipEventCreateWithFlags(&c->block_meta_ev, hipEventDisableTiming));
  if ((st = c->h_block_meta.ensure(12 * nblocks)) || (st = c->d_block_meta.ensure(12 * nblocks, c->stream))) return st;
  uint64_t* first = c->h_block_meta.as<uint64_t>();
  uint32_t* cnt = reinterpret_cast<uint32_t*>(first + nblocks);
  uint64_t at = 0;
  for (size_t b = 0; b < nblocks; ++b) {
    first[b] = at;
    cnt[b] = count[b];
    at += count[b];
  }
  AG_HIP(hipMemcpyAsync(c->d_block_meta.ptr, c->h_block_meta.ptr, 12 * nblocks, hipMemcpyHostToDevice, c->stream));
  AG_HIP(hipEventRecord(c->block_meta_ev, c->stream));
  ag::BlockTreeParams p{};
  p.first = c->d_block_meta.as<uint64_t>();
  p.count = reinterpret_cast<const uint32_t*>(p.first + nblocks);
  p.nblocks = nblocks;
  p.slice_roots = slice_roots;
  p.empty_roots = c->d_empty_roots.as<uint32_t>();
  p.block_hashes = block_hashes;
  p.nodes = nodes;
  p.nodes_stride = nodes_stride;
  p.proofs = proofs;
  p.proofs_stride = proofs_stride;
  if (proofs && !nodes) {  // the proofs are gathered from the nodes: scratch when the caller wants none
    p.nodes_stride = (32 * ag_merkle_node_count(mx) + 255) / 256 * 256;
    if ((st = c->d_merkle_nodes.ensure(nblocks * p.nodes_stride, c->stream))) return st;
    p.nodes = c->d_merkle_nodes.as<uint8_t>();
  }
  return ag::launch_block_tree(p, c->stream) == hipSuccess ? AG_RS_OK : AG_RS_ERR_DEVICE;
}

int ag_block_proof_check_batch(ag_rs_ctx* c, size_t n, const uint8_t* slice_roots, size_t roots_stride,
                               const uint32_t* index, const uint8_t* block_hashes, size_t hashes_stride,
                               const uint8_t* proofs, size_t proofs_stride, const uint32_t* proof_len,
                               const uint8_t* last, uint8_t* ok) {
  if (!c) return AG_RS_ERR_INVALID_ARGUMENT;
  if (n == 0) return AG_RS_OK;
  // proofs may be null only with a zero stride, which holds no digest: any proof_len > 0 is then ok = 0
  if (!slice_roots || !index || !block_hashes || !proof_len || !ok || (!proofs && proofs_stride) ||
      hashes_stride % 16 || proofs_stride % 16 || reinterpret_cast<uintptr_t>(block_hashes) % 16 ||
      reinterpret_cast<uintptr_t>(proofs) % 16 || (n > 1 && roots_stride < 32))
    return AG_RS_ERR_INVALID_ARGUMENT;
  int st = c->enter();
  if (st || (st = ensure_empty_roots(c))) return st;
  ag::MerkleVerifyParams p{};
  p.leaves = slice_roots;
  p.leaf_stride = roots_stride;
  p.leaf_bytes = 32;
  p.index = index;
  p.roots = block_hashes;
  p.roots_stride = hashes_stride;
  p.proofs = proofs;
  p.proofs_stride = proofs_stride;
  p.n = n;
  p.ok = ok;
  p.proof_len = proof_len;
  p.last = last;
  p.empty_roots = c->d_empty_roots.as<uint32_t>();
  return ag::launch_merkle_verify(p, c->stream) == hipSuccess ? AG_RS_OK : AG_RS_ERR_DEVICE;
}

// ---- all-or-nothing payload transforms ------------------------------------------------

int ag_aes128_encrypt_block(const uint8_t key[16], const uint8_t in[16], uint8_t out[16]) {
  if (!key || !in || !out) return AG_RS_ERR_INVALID_ARGUMENT;
  ag::aes128_encrypt_block(key, in, out);
  return AG_RS_OK;
}

}  // extern "C"

namespace ag::host {
// lengths (host) -> device; the batch descriptor
int aon_batch(ag_rs_ctx* c, size_t n, uint8_t* buffers, size_t stride, const uint32_t* lens, uint32_t extra,
              ag::BufferBatch* bb) {
  uint32_t mx = 0;
  for (size_t b = 0; b < n; ++b) {
    if (lens[b] > (1u << 28)) return AG_RS_ERR_INVALID_ARGUMENT;
    mx = std::max(mx, lens[b]);
  }
  if (n > 1 && stride < static_cast<size_t>(mx) + extra) return AG_RS_ERR_INVALID_ARGUMENT;
  int st = c->d_aon_lens.ensure(n * 4, c->stream);
  if (st) return st;
  AG_HIP(hipStreamSynchronize(c->stream));  // a previous call's upload may still be pending
  AG_HIP(hipMemcpy(c->d_aon_lens.ptr, lens, n * 4, hipMemcpyHostToDevice));
  bb->base = buffers;
  bb->stride = stride;
  bb->lens = c->d_aon_lens.as<uint32_t>();
  bb->n = n;
  bb->max_len = mx;
  return AG_RS_OK;
}
}  // namespace ag::host

extern "C" {

int ag_cipher_apply_keystream_batch(ag_rs_ctx* c, size_t n, const uint8_t* keys, uint8_t* buffers, size_t stride,
                                    const uint32_t* lens) {
  if (!c || (n && (!keys || !buffers || !lens))) return AG_RS_ERR_INVALID_ARGUMENT;
  if (n == 0) return AG_RS_OK;
  if (c->enter()) return AG_RS_ERR_DEVICE;
  ag::BufferBatch bb;
  int st = aon_batch(c, n, buffers, stride, lens, 0, &bb);
  if (st) return st;
  return ag::launch_apply_keystream(bb, keys, 0, c->stream) == hipSuccess ? AG_RS_OK : AG_RS_ERR_DEVICE;
}

int ag_sha256_batch(ag_rs_ctx* c, size_t n, const uint8_t* buffers, size_t stride, const uint32_t* lens,
                    uint8_t* digests) {
  if (!c || (n && (!buffers || !lens || !digests))) return AG_RS_ERR_INVALID_ARGUMENT;
  if (n == 0) return AG_RS_OK;
  if (c->enter()) return AG_RS_ERR_DEVICE;
  ag::BufferBatch bb;
  int st = aon_batch(c, n, const_cast<uint8_t*>(buffers), stride, lens, 0, &bb);
  if (st) return st;
  return ag::launch_sha256(bb, 0, digests, c->stream) == hipSuccess ? AG_RS_OK : AG_RS_ERR_DEVICE;
}

int ag_aon_encrypt_batch(ag_rs_ctx* c, int scheme, size_t n, const uint8_t* keys, uint8_t* buffers, size_t stride,
                         const uint32_t* lens) {
  if (!c || (scheme != AG_AON_AONT && scheme != AG_AON_PETS) || (n && (!keys || !buffers || !lens)))
    return AG_RS_ERR_INVALID_ARGUMENT;
  if (n == 0) return AG_RS_OK;
  if (c->enter()) return AG_RS_ERR_DEVICE;
  ag::BufferBatch bb;
  int st = aon_batch(c, n, buffers, stride, lens, ag::kCipherKeyBytes, &bb);
  if (st) return st;
  const bool aont = scheme == AG_AON_AONT;
  if (aont && (st = c->d_aon_digests.ensure(n * 32, c->stream))) return st;
  if (ag::launch_apply_keystream(bb, keys, 0, c->stream) != hipSuccess) return AG_RS_ERR_DEVICE;
  if (aont && ag::launch_sha256(bb, 0, c->d_aon_digests.as<uint8_t>(), c->stream) != hipSuccess)
    return AG_RS_ERR_DEVICE;
  return ag::launch_write_key_tail(bb, aont, keys, aont ? c->d_aon_digests.as<uint8_t>() : nullptr, c->stream) ==
                 hipSuccess
             ? AG_RS_OK
             : AG_RS_ERR_DEVICE;
}

int ag_aon_decrypt_batch(ag_rs_ctx* c, int scheme, size_t n, uint8_t* buffers, size_t stride, const uint32_t* lens,
                         int64_t* plain_len_out) {
  if (!c || (scheme != AG_AON_AONT && scheme != AG_AON_PETS) || (n && (!buffers || !lens || !plain_len_out)))
    return AG_RS_ERR_INVALID_ARGUMENT;
  if (n == 0) return AG_RS_OK;
  if (c->enter()) return AG_RS_ERR_DEVICE;
  // buffers too short for a key: BadEncoding, left untouched (length 16 => empty payload)
  std::vector<uint32_t> lv(lens, lens + n);
  for (size_t b = 0; b < n; ++b) {
    plain_len_out[b] = lens[b] < ag::kCipherKeyBytes ? -AG_RS_ERR_BAD_ENCODING
                                                      : static_cast<int64_t>(lens[b]) - ag::kCipherKeyBytes;
    if (lens[b] < ag::kCipherKeyBytes) lv[b] = ag::kCipherKeyBytes;  // no-op (empty ciphertext, key unused)
  }
  ag::BufferBatch bb;
  int st = aon_batch(c, n, buffers, stride, lv.data(), 0, &bb);
  if (st) return st;
  const bool aont = scheme == AG_AON_AONT;
  if ((st = c->d_aon_keys.ensure(n * 16, c->stream))) return st;
  if (aont) {
    if ((st = c->d_aon_digests.ensure(n * 32, c->stream))) return st;
    if (ag::launch_sha256(bb, ag::kCipherKeyBytes, c->d_aon_digests.as<uint8_t>(), c->stream) != hipSuccess)
      return AG_RS_ERR_DEVICE;
  }
  if (ag::launch_derive_keys(bb, aont, aont ? c->d_aon_digests.as<uint8_t>() : nullptr, c->d_aon_keys.as<uint8_t>(),
                             c->stream) != hipSuccess ||
      ag::launch_apply_keystream(bb, c->d_aon_keys.as<uint8_t>(), ag::kCipherKeyBytes, c->stream) != hipSuccess)
    return AG_RS_ERR_DEVICE;
  AG_HIP(hipStreamSynchronize(c->stream));
  return AG_RS_OK;
}

}  // extern "C"

// =====================================================================================
// Crate API mirror: ReedSolomonEncoder / ReedSolomonDecoder (one codeword, host memory)
// =====================================================================================
// An object made by *_new_on_device owns its context (`owned`: created with it, destroyed by
// its _free), so objects made that way share no state and may run on different threads at
// once; *_new borrows the caller's context, shared with whatever else uses it.
// Each encoder / decoder stages its codeword in its own mapped pinned buffer (the shards are
// copied there by add_*_shard, the device reads and writes it in place, and the result
// accessors point into it), so no call re-copies or re-zeroes a 64 KiB slice.
struct ag_rs_encoder {
  ag_rs_ctx* ctx = nullptr;
  ag_rs_ctx* owned = nullptr;
  size_t k = 0, m = 0, S = 0;
  size_t received = 0;
  bool encoded = false;
  PinBuf pin;  // originals [k * S] then recovery shards [m * S]
  uint8_t* orig() const { return pin.as<uint8_t>(); }
  uint8_t* rec() const { return pin.as<uint8_t>() + k * S; }
  ~ag_rs_encoder() {
    pin.release();
    ag_rs_ctx_destroy(owned);
  }
};

struct ag_rs_decoder {
  ag_rs_ctx* ctx = nullptr;
  ag_rs_ctx* owned = nullptr;
  size_t k = 0, m = 0, S = 0;
  std::vector<uint8_t> opres, rpres;
  size_t no = 0, nr = 0;
  bool decoded = false;
  std::vector<uint8_t> restored;  // 1 where original i was restored by the last decode
  PinBuf pin;  // originals [k * S], recovery shards [m * S], re-encoded coding shards [m * S]
  uint8_t* orig() const { return pin.as<uint8_t>(); }
  uint8_t* rec() const { return pin.as<uint8_t>() + k * S; }
  ~ag_rs_decoder() {
    pin.release();
    ag_rs_ctx_destroy(owned);
  }
};

namespace {
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
ag::XformParams one_tile(const uint8_t* in, size_t in_stride, uint8_t* out, size_t out_stride, size_t S) {
  ag::XformParams p{};
  p.in = in;
  p.in_block_stride = in_stride;
  p.in_shard_stride = S;
  p.out = out;
  p.out_block_stride = out_stride;
  p.out_shard_stride = S;
  p.n_in = 32;
  p.n_out = 32;
  p.chunks_per_shard = static_cast<uint32_t>(S / 64);
  p.total_columns = S / 64;
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
    c->abandoned_pins.push_back(stage);
    stage = PinBuf{};
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
    ag::DecodeXParams dp{};
    dp.rec = pd + ob;
    dp.rec_block_stride = (k + m) * S;
    dp.rec_shard_stride = S;
    dp.orig = pd;
    dp.orig_block_stride = (k + m) * S;
    dp.orig_shard_stride = S;
    dp.k = 32;
    dp.m = 32;
    dp.chunk = 32;
    dp.low_rate = 0;
    dp.chunks_per_shard = 16;
    dp.total_columns = 16;
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
}  // namespace

extern "C" {

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
  (*out)->owned = c;
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
  (*out)->owned = c;
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

// =====================================================================================
// ReedSolomonCoder mirror (reed_solomon.rs:47-232)
// =====================================================================================
struct ag_rs_coder {
  ag_rs_ctx* ctx = nullptr;
  ag_rs_ctx* owned = nullptr;  // ag_rs_coder_new_on_device: shared by its encoder and decoder
  size_t num_coding = 0;
  ag_rs_encoder* enc = nullptr;
  ag_rs_decoder* dec = nullptr;
  ~ag_rs_coder() {
    ag_rs_encoder_free(enc);
    ag_rs_decoder_free(dec);
    ag_rs_ctx_destroy(owned);
  }
};

int ag_rs_internal_coder_last_job_ns(ag_rs_coder* coder, uint64_t* ns) {
  if (!coder || !coder->ctx || !ns) return AG_RS_ERR_INVALID_ARGUMENT;
  const ag::LatencyMailbox* mb = coder->ctx->mb;
  ns[0] = mb ? __atomic_load_n(&mb->job_ticks, __ATOMIC_ACQUIRE) * 10 : 0;  // 100 MHz wall clock
  for (int i = 0; i < 4; ++i) ns[1 + i] = mb ? uint64_t{__atomic_load_n(&mb->phase_ticks[i], __ATOMIC_ACQUIRE)} * 10 : 0;
  return AG_RS_OK;
}

namespace {
constexpr size_t kTotalShreds = AG_RS_TOTAL_SHREDS;
constexpr size_t kMaxAfterPadding = kDataShreds * AG_RS_MAX_DATA_PER_SHRED;
static_assert(kMaxPayload == kMaxAfterPadding - 1);

// encode_coding_from_data (reed_solomon.rs:211-231) of the 32 data shards already staged in
// the encoder's originals (S bytes each): the coding shards land in c->enc->rec()
// (the caller reset the encoder to (32, num_coding, S) before staging them)
int coder_encode_staged(ag_rs_coder* c) {
  c->enc->received = kDataShreds;
  c->enc->encoded = false;
  return ag_rs_encoder_encode(c->enc);
}
}  // namespace

extern "C" {

int ag_rs_coder_new(ag_rs_ctx* ctx, size_t num_coding, ag_rs_coder** out) {
  if (!ctx || !out) return AG_RS_ERR_INVALID_ARGUMENT;
  *out = nullptr;
  if (num_coding == 0 || num_coding > kTotalShreds) return AG_RS_ERR_UNSUPPORTED_SHARD_COUNT;
  auto* c = new (std::nothrow) ag_rs_coder();
  if (!c) return AG_RS_ERR_OUT_OF_MEMORY;
  c->ctx = ctx;
  c->num_coding = num_coding;
  int st = ag_rs_encoder_new(ctx, kDataShreds, num_coding, AG_RS_MAX_DATA_PER_SHRED, &c->enc);
  if (!st) st = ag_rs_decoder_new(ctx, kDataShreds, num_coding, AG_RS_MAX_DATA_PER_SHRED, &c->dec);
  if (st) {
    delete c;
    return st;
  }
  *out = c;
  return AG_RS_OK;
}

int ag_rs_coder_new_on_device(int device, size_t num_coding, ag_rs_coder** out) {
  if (!out) return AG_RS_ERR_INVALID_ARGUMENT;
  *out = nullptr;
  ag_rs_ctx* c = nullptr;
  int st = ag_rs_ctx_create(device, &c);
  if (st) return st;
  if ((st = ag_rs_coder_new(c, num_coding, out))) {
    ag_rs_ctx_destroy(c);
    return st;
  }
  (*out)->owned = c;
  return AG_RS_OK;
}

void ag_rs_coder_free(ag_rs_coder* c) { delete c; }

int ag_rs_coder_num_coding(const ag_rs_coder* c, size_t* out) {
  if (!c || !out) return AG_RS_ERR_INVALID_ARGUMENT;
  *out = c->num_coding;
  return AG_RS_OK;
}

int ag_rs_coder_shred(ag_rs_coder* c, const uint8_t* payload, size_t len, uint8_t* data_out, uint8_t* coding_out,
                      size_t* shred_bytes) {
  if (!c || (!payload && len) || !data_out || !coding_out || !shred_bytes) return AG_RS_ERR_INVALID_ARGUMENT;
  if (len > kMaxPayload) return AG_RS_ERR_TOO_MUCH_DATA;
  // padding 0x80 00.. to a multiple of 2 * DATA_SHREDS (reed_solomon.rs:94-106)
  const size_t padding = 2 * kDataShreds - len % (2 * kDataShreds);
  const size_t S = (len + padding) / kDataShreds;
  // padded payload straight into the encoder's pinned originals
  int st = ag_rs_encoder_reset(c->enc, kDataShreds, c->num_coding, S);
  if (st) return st;
  uint8_t* padded = c->enc->orig();
  if (len) std::memcpy(padded, payload, len);
  padded[len] = 0x80;
  std::memset(padded + len + 1, 0, padding - 1);
  if ((st = coder_encode_staged(c))) return st;
  std::memcpy(data_out, padded, len + padding);
  std::memcpy(coding_out, c->enc->rec(), c->num_coding * S);
  *shred_bytes = S;
  return AG_RS_OK;
}

int ag_rs_coder_deshred(ag_rs_coder* c, size_t data_shreds, const uint8_t* const* shreds, const size_t* lens,
                        const uint8_t* is_data, uint8_t* payload_out, size_t* payload_len, uint8_t* data_out,
                        uint8_t* coding_out, size_t* shred_bytes) {
  if (!c || !shreds || !lens || !payload_out || !payload_len || !data_out || !coding_out || !shred_bytes)
    return AG_RS_ERR_INVALID_ARGUMENT;
  if (data_shreds + c->num_coding != kTotalShreds) return AG_RS_ERR_INVALID_ARGUMENT;
  // Shredder::deshred: an empty set is too few shreds (shredder.rs:283-285)
  size_t present = 0, S = 0;
  for (size_t i = 0; i < kTotalShreds; ++i)
    if (shreds[i]) {
      if (!present) S = lens[i];
      ++present;
    }
  if (!present) return AG_RS_ERR_NOT_ENOUGH_SHARDS;
  // ValidatedShreds::try_new (validated_shreds.rs:34-70)
  if (S == 0 || S % 2) return AG_RS_ERR_INVALID_LAYOUT;
  for (size_t i = 0; i < kTotalShreds; ++i) {
    if (!shreds[i]) continue;
    if (lens[i] != S) return AG_RS_ERR_INVALID_LAYOUT;
    if (is_data && ((i < data_shreds) != (is_data[i] != 0))) return AG_RS_ERR_INVALID_LAYOUT;
  }
  // ReedSolomonCoder::deshred (reed_solomon.rs:140-208)
  if (present < kDataShreds) return AG_RS_ERR_NOT_ENOUGH_SHARDS;
  int st = ag_rs_decoder_reset(c->dec, kDataShreds, c->num_coding, S);
  if (st) return st;
  for (size_t i = 0; i < data_shreds; ++i)
    if (shreds[i] && (st = ag_rs_decoder_add_original_shard(c->dec, i, shreds[i], S))) return st;
  for (size_t j = data_shreds; j < kTotalShreds; ++j)
    if (shreds[j] && (st = ag_rs_decoder_add_recovery_shard(c->dec, j - data_shreds, shreds[j], S))) return st;
  ag_rs_decoder* dec = c->dec;
  if (dec->no + dec->nr < kDataShreds) return AG_RS_ERR_NOT_ENOUGH_SHARDS;
  // decode and the re-encode of every coding shard (:206) in one device round trip; the
  // completed originals (present ones as added, restored ones written back) are dec->orig()
  const uint8_t* coding = nullptr;
  const bool coded = dec->no < kDataShreds;
  if (coded && (st = run_one_decode(c->ctx, kDataShreds, c->num_coding, S, dec->pin, dec->opres.data(),
                                    dec->rpres.data(), AG_RS_DECODE_EXACT, true, &coding)))
    return st;
  // concatenation with the TooMuchData bound of :169-188 (exceeded iff 32 S > 32 768)
  if (kDataShreds * S > kMaxAfterPadding) return AG_RS_ERR_TOO_MUCH_DATA;
  const uint8_t* data = dec->orig();
  const size_t total = kDataShreds * S;
  // strip padding: trailing zeros then the 0x80 marker
  size_t zeros = 0;
  while (zeros < total && data[total - 1 - zeros] == 0) ++zeros;
  const size_t padding = zeros + 1;
  if (padding > total || data[total - padding] != 0x80) return AG_RS_ERR_INVALID_PADDING;
  const size_t plen = total - padding;
  if (!coded) {  // every data shred present: encode them (staged in the encoder)
    if ((st = ag_rs_encoder_reset(c->enc, kDataShreds, c->num_coding, S))) return st;
    std::memcpy(c->enc->orig(), data, total);
    if ((st = coder_encode_staged(c))) return st;
    coding = c->enc->rec();
  }
  std::memcpy(payload_out, data, plen);
  *payload_len = plen;
  std::memcpy(data_out, data, total);
  std::memcpy(coding_out, coding, c->num_coding * S);
  *shred_bytes = S;
  return AG_RS_OK;
}

int ag_rs_coder_shred_batch(ag_rs_ctx* c, size_t m, size_t n, size_t S, const uint8_t* payloads,
                            size_t payload_stride, const uint32_t* lens, uint8_t* cw, size_t cw_stride) {
  if (!c || (n && (!lens || !cw))) return AG_RS_ERR_INVALID_ARGUMENT;
  if (m == 0 || m > kTotalShreds) return AG_RS_ERR_UNSUPPORTED_SHARD_COUNT;
  if (S == 0 || S % 2 || S > AG_RS_MAX_DATA_PER_SHRED) return AG_RS_ERR_INVALID_SHARD_SIZE;
  if (cw_stride < (kDataShreds + m) * S) return AG_RS_ERR_INVALID_ARGUMENT;
  for (size_t b = 0; b < n; ++b) {
    if (lens[b] > kMaxPayload) return AG_RS_ERR_TOO_MUCH_DATA;
    const size_t padded = lens[b] + 2 * kDataShreds - lens[b] % (2 * kDataShreds);  // reed_solomon.rs:94-95
    if (padded / kDataShreds != S) return AG_RS_ERR_INVALID_ARGUMENT;
  }
  if (n == 0) return AG_RS_OK;
  int st = c->enter();
  if (st) return st;
  // the lengths go up through pinned staging on the context stream (ordered after a previous
  // call's pad kernel, which may still read d_lens); the staging is rewritten once its last
  // upload has completed -- no stream synchronisation before the call's work is enqueued
  if (c->lens_ev) AG_HIP(hipEventSynchronize(c->lens_ev));
  else AG_HIP(hipEventCreateWithFlags(&c->lens_ev, hipEventDisableTiming));
  if ((st = c->h_lens.ensure(n * 4))) return st;
  std::memcpy(c->h_lens.ptr, lens, n * 4);
  if ((st = c->d_lens.ensure(n * 4, c->stream))) return st;
  AG_HIP(hipMemcpyAsync(c->d_lens.ptr, c->h_lens.ptr, n * 4, hipMemcpyHostToDevice, c->stream));
  AG_HIP(hipEventRecord(c->lens_ev, c->stream));
  if (ag::launch_coder_pad(payloads, payload_stride, c->d_lens.as<uint32_t>(), cw, cw_stride,
                           static_cast<uint32_t>(kDataShreds * S), n, c->stream) != hipSuccess)
    return AG_RS_ERR_DEVICE;
  return encode_device(c, kDataShreds, m, S, n, cw, cw_stride, cw + kDataShreds * S, cw_stride);
}

namespace {
// ag_rs_coder_deshred_batch when every slice has the same present shreds (pattern = slice 0's).
int coder_deshred_uniform(ag_rs_ctx* c, size_t m, size_t n, size_t S, uint8_t* cw, size_t cw_stride,
                          const uint8_t* dpres, const uint8_t* cpres, int mode, int64_t* out) {
  const size_t nd = count_flags(dpres, kDataShreds), nc = count_flags(cpres, m);
  if (nd + nc < kDataShreds) {  // reed_solomon.rs:144: nothing decoded, coding untouched
    for (size_t b = 0; b < n; ++b) out[b] = -AG_RS_ERR_NOT_ENOUGH_SHARDS;
    return AG_RS_OK;
  }
  uint8_t* rec = cw + kDataShreds * S;
  int st = decode_device(c, kDataShreds, m, S, n, cw, cw_stride, rec, cw_stride, dpres, cpres, 1, mode);
  if (st) return st;
  if ((st = c->d_strip.ensure(n * 8, c->stream))) return st;
  if (ag::launch_coder_strip(cw, cw_stride, static_cast<uint32_t>(kDataShreds * S), n, c->d_strip.as<int64_t>(),
                             c->stream) != hipSuccess)
    return AG_RS_ERR_DEVICE;
  AG_HIP(hipMemcpyAsync(out, c->d_strip.ptr, n * 8, hipMemcpyDeviceToHost, c->stream));
  AG_HIP(hipStreamSynchronize(c->stream));
  for (size_t b = 0; b < n; ++b)
    if (out[b] < 0) out[b] = -AG_RS_ERR_INVALID_PADDING;
  // re-encode (encode_coding_from_data) the runs of slices that stripped; skipped when the
  // present shreds are exactly the 32 coding shreds (the re-encode reproduces them)
  if (m == kDataShreds && nd == 0 && nc == m) return AG_RS_OK;
  // LowRate 32:64 (CodingOnly) with exactly 32 kept shreds: the codeword is unique, so the
  // re-encode reproduces every kept coding shred.  When the absent ones all lie in one 32-shard
  // recovery chunk (the reference bench's shape: coding 32..63 kept), only that chunk is
  // encoded -- one 32-point transform under a store mask of its absent shreds instead of the
  // two-chunk 64-point one
  int lone = -1;
  if (m == 2 * kDataShreds && nd + nc == kDataShreds && S % 64 == 0 && !odd_layout(cw, cw, cw_stride, cw_stride)) {
    const uint64_t absent = ~pack_flags(cpres, m);
    const uint64_t lo = absent & 0xFFFFFFFFull, hi = absent >> 32;
    if (lo == 0 || hi == 0) {
      lone = lo == 0 ? 1 : 0;
      const uint64_t w = lo == 0 ? hi : lo;
      if ((st = c->d_reenc_mask.ensure(8, c->stream))) return st;
      AG_HIP(hipMemsetD32Async(c->d_reenc_mask.ptr, static_cast<int>(static_cast<uint32_t>(w)), 1, c->stream));
      AG_HIP(hipMemsetD32Async(c->d_reenc_mask.as<uint32_t>() + 1, 0, 1, c->stream));
    }
  }
  for (size_t b = 0; b < n;) {
    if (out[b] < 0) {
      ++b;
      continue;
    }
    size_t e = b;
    while (e < n && out[e] >= 0) ++e;
    if (lone >= 0) {
      ag::XformParams p{};
      p.in = cw + b * cw_stride;
      p.in_block_stride = cw_stride;
      p.in_shard_stride = S;
      p.out = rec + b * cw_stride + static_cast<size_t>(lone) * 32 * S;
      p.out_block_stride = cw_stride;
      p.out_shard_stride = S;
      p.out_mask = c->d_reenc_mask.as<uint64_t>();
      p.n_in = static_cast<uint32_t>(kDataShreds);
      p.n_out = 32;
      p.chunks_per_shard = static_cast<uint32_t>(S / 64);
      p.total_columns = static_cast<uint64_t>(e - b) * (S / 64);
      c->last_encode_kernels |= ag::kEkLowRate;
      if (ag::launch_xform_lowrate(32, static_cast<unsigned>(lone), p, c->stream) != hipSuccess) return AG_RS_ERR_DEVICE;
    } else if ((st = encode_device(c, kDataShreds, m, S, e - b, cw + b * cw_stride, cw_stride, rec + b * cw_stride,
                                   cw_stride))) {
      return st;
    }
    b = e;
  }
  AG_HIP(hipStreamSynchronize(c->stream));
  return AG_RS_OK;
}
}  // namespace

int ag_rs_coder_deshred_batch(ag_rs_ctx* c, size_t m, size_t n, size_t S, uint8_t* cw, size_t cw_stride,
                              const uint8_t* dpres, const uint8_t* cpres, int mode, int64_t* out) {
  if (!c || (n && (!cw || !dpres || !cpres || !out))) return AG_RS_ERR_INVALID_ARGUMENT;
  if (m == 0 || m > kTotalShreds) return AG_RS_ERR_UNSUPPORTED_SHARD_COUNT;
  if (mode != AG_RS_DECODE_EXACT && mode != AG_RS_DECODE_ANY_K) return AG_RS_ERR_INVALID_ARGUMENT;
  if (S == 0 || S % 2) return AG_RS_ERR_INVALID_SHARD_SIZE;
  if (kDataShreds * S > kMaxAfterPadding) return AG_RS_ERR_TOO_MUCH_DATA;  // reed_solomon.rs:183
  if (cw_stride < (kDataShreds + m) * S) return AG_RS_ERR_INVALID_ARGUMENT;
  if (n == 0) return AG_RS_OK;
  int st = c->enter();
  if (st) return st;
  c->last_encode_kernels = 0;  // the re-encode's kernels (test aid)
  c->last_window_kernels = 0;  // the window decode's kernels (test aid)
  // One pattern for the whole batch (a repair batch; the reference bench's shape): one
  // pattern word on the host, no per-slice bookkeeping past the strip results.
  bool uniform = true;
  for (size_t b = 1; b < n && uniform; ++b)
    uniform = std::memcmp(dpres, dpres + b * kDataShreds, kDataShreds) == 0 && std::memcmp(cpres, cpres + b * m, m) == 0;
  if (uniform) return coder_deshred_uniform(c, m, n, S, cw, cw_stride, dpres, cpres, mode, out);
  // Per-slice patterns of RegularShredder's 32:32 on whole-chunk shreds (the follower's
  // random arrival): one 64-bit present mask per slice goes to the device, and the window
  // patterns, locator constants, per-lane decode, padding strip and re-encode run there
  // (pipe_coder_deshred, the composed deshred's coder stage) -- no per-slice host work past
  // the packing.  ANY_K, or EXACT where no slice holds more than 32 shreds (k shreds fix the
  // codeword, so both decoders agree).  One pattern for the whole batch stays on the host
  // path below (a single transform launch).
  // CodingOnlyShredder's 32:64 and PetsShredder's 32:33 (LowRate, 32 < m <= 64) take the same
  // path with the W = 128 window (positions of coding shreds past m are simply never present).
  if (m >= kDataShreds && m <= 2 * kDataShreds && pipe_tail_ok(S, m, true) && n > 1 &&
      !odd_layout(cw, cw, cw_stride, cw_stride)) {
    const size_t wps = m == kDataShreds ? 1 : 2;  // present words per slice
    // packed straight into pinned staging, so the upload is one DMA with no pageable bounce
    // (once the previous call's upload of it has completed)
    if (c->present_ev) AG_HIP(hipEventSynchronize(c->present_ev));
    else AG_HIP(hipEventCreateWithFlags(&c->present_ev, hipEventDisableTiming));
    if ((st = c->h_present.ensure(wps * n * 8))) return st;
    uint64_t* pres = c->h_present.as<uint64_t>();
    // (uniform batches returned above)
    // ANY_K always takes the device path; EXACT when no slice keeps more than 32 shreds (both
    // decoders agree then).  (Packing a first ~1/8 range and the rest behind its decode
    // measured even with one whole-batch range, profiles/r05_ab_coder_ranges.jsonl.)
    bool full_data = false;
    const bool surplus = pack_present_words(dpres, cpres, m, n, pres, &full_data);
    if ((mode == AG_RS_DECODE_ANY_K || !surplus) && pipe_tail_ok(S, m, !surplus && !full_data)) {
      if ((st = c->d_present.ensure(wps * n * 8, c->stream))) return st;
      AG_HIP(hipMemcpyAsync(c->d_present.ptr, pres, wps * n * 8, hipMemcpyHostToDevice, c->stream));
      AG_HIP(hipEventRecord(c->present_ev, c->stream));
      // no surplus and no slice with every data shred: no store mask of the re-encode is set
      return pipe_coder_deshred(c, n, S, cw, cw_stride, c->d_present.as<uint64_t>(), out, m,
                                !surplus && !full_data);  // synchronous
    }
  }
  // slices with fewer than 32 shreds: reported, and decoded as "nothing missing" (untouched)
  std::vector<uint8_t> op(dpres, dpres + n * kDataShreds);
  std::vector<uint8_t> ok(n, 1);
  for (size_t b = 0; b < n; ++b) {
    const size_t cnt = count_flags(dpres + b * kDataShreds, kDataShreds) + count_flags(cpres + b * m, m);
    if (cnt < kDataShreds) {
      ok[b] = 0;
      out[b] = -AG_RS_ERR_NOT_ENOUGH_SHARDS;
      std::fill(op.begin() + b * kDataShreds, op.begin() + (b + 1) * kDataShreds, uint8_t{1});
    }
  }
  uint8_t* rec = cw + kDataShreds * S;
  if ((st = decode_device(c, kDataShreds, m, S, n, cw, cw_stride, rec, cw_stride, op.data(), cpres, n, mode)))
    return st;
  if ((st = c->d_strip.ensure(n * 8, c->stream))) return st;
  if (ag::launch_coder_strip(cw, cw_stride, static_cast<uint32_t>(kDataShreds * S), n, c->d_strip.as<int64_t>(),
                             c->stream) != hipSuccess)
    return AG_RS_ERR_DEVICE;
  std::vector<int64_t> lens(n);
  AG_HIP(hipMemcpyAsync(lens.data(), c->d_strip.ptr, n * 8, hipMemcpyDeviceToHost, c->stream));
  AG_HIP(hipStreamSynchronize(c->stream));
  for (size_t b = 0; b < n; ++b) {
    if (!ok[b]) continue;
    if (lens[b] < 0) {
      ok[b] = 0;
      out[b] = -AG_RS_ERR_INVALID_PADDING;
    } else {
      out[b] = lens[b];
    }
  }
  // re-encode all coding shards (encode_coding_from_data) of each run of good slices.  A
  // slice whose present shards are exactly its k = 32 coding shards (every data shred lost,
  // the reference bench's shape) is skipped: its re-encoded coding shards are the received
  // ones already in place, bit for bit.
  for (size_t b = 0; b < n; ++b)
    if (ok[b] && m == kDataShreds && count_flags(dpres + b * kDataShreds, kDataShreds) == 0 &&
        count_flags(cpres + b * m, m) == m)
      ok[b] = 0;
  for (size_t b = 0; b < n;) {
    if (!ok[b]) {
      ++b;
      continue;
    }
    size_t e = b;
    while (e < n && ok[e]) ++e;
    if ((st = encode_device(c, kDataShreds, m, S, e - b, cw + b * cw_stride, cw_stride, rec + b * cw_stride,
                            cw_stride)))
      return st;
    b = e;
  }
  AG_HIP(hipStreamSynchronize(c->stream));
  return AG_RS_OK;
}

// ---- Ed25519 shred signatures ------------------------------------------------------------

namespace {
int ensure_ed_base(ag_rs_ctx* c) {
  if (c->d_ed_base.ptr) return AG_RS_OK;
  int st = c->d_ed_base.ensure(ag::kEdBaseTableBytes, c->stream);
  if (st) return st;
  return ag::launch_ed25519_init(c->d_ed_base.as<int32_t>(), c->stream) == hipSuccess ? AG_RS_OK : AG_RS_ERR_DEVICE;
}
constexpr size_t kMaxSigBatch = size_t{1} << 31;
}  // namespace

int ag_ed25519_public_key_batch(ag_rs_ctx* c, size_t n, const uint8_t* seeds, uint8_t* pks) {
  if (!c || n >= kMaxSigBatch || (n && (!seeds || !pks))) return AG_RS_ERR_INVALID_ARGUMENT;
  if (n == 0) return AG_RS_OK;
  if (c->enter()) return AG_RS_ERR_DEVICE;
  int st = ensure_ed_base(c);
  if (st) return st;
  return ag::launch_ed25519_public_key(seeds, pks, n, c->d_ed_base.as<int32_t>(), c->stream) == hipSuccess
             ? AG_RS_OK
             : AG_RS_ERR_DEVICE;
}

int ag_ed25519_sign_batch(ag_rs_ctx* c, size_t n, const uint8_t* seeds, size_t seed_stride, const uint8_t* pks,
                          size_t pk_stride, const uint8_t* msgs, size_t msg_stride, size_t msg_len, uint8_t* sigs) {
  if (!c || n >= kMaxSigBatch || msg_len >= (size_t{1} << 28) ||
      (n && (!seeds || !pks || !sigs || (msg_len && !msgs))))
    return AG_RS_ERR_INVALID_ARGUMENT;
  if (n == 0) return AG_RS_OK;
  if (c->enter()) return AG_RS_ERR_DEVICE;
  int st = ensure_ed_base(c);
  if (st) return st;
  ag::EdSignParams p{};
  p.seeds = seeds;
  p.seed_stride = seed_stride;
  p.pks = pks;
  p.pk_stride = pk_stride;
  p.msgs = msgs;
  p.msg_stride = msg_stride;
  p.msg_len = static_cast<uint32_t>(msg_len);
  p.sigs = sigs;
  p.n = n;
  p.base_table = c->d_ed_base.as<int32_t>();
  return ag::launch_ed25519_sign(p, c->stream) == hipSuccess ? AG_RS_OK : AG_RS_ERR_DEVICE;
}

int ag_ed25519_verify_batch(ag_rs_ctx* c, size_t n, const uint8_t* pks, size_t pk_stride, const uint8_t* msgs,
                            size_t msg_stride, const uint32_t* msg_lens, size_t msg_len, const uint8_t* sigs,
                            size_t sig_stride, uint8_t* ok) {
  if (!c || n >= kMaxSigBatch || msg_len >= (size_t{1} << 28) || (n && (!pks || !sigs || !ok)) ||
      (n && !msgs && (msg_lens || msg_len)))
    return AG_RS_ERR_INVALID_ARGUMENT;
  if (n == 0) return AG_RS_OK;
  if (c->enter()) return AG_RS_ERR_DEVICE;
  int st = ensure_ed_base(c);
  if (st) return st;
  ag::EdVerifyParams p{};
  p.pks = pks;
  p.pk_stride = pk_stride;
  p.msgs = msgs;
  p.msg_stride = msg_stride;
  p.msg_lens = msg_lens;
  p.msg_len = static_cast<uint32_t>(msg_len);
  p.sigs = sigs;
  p.sig_stride = sig_stride;
  p.n = n;
  p.ok = ok;
  p.base_table = c->d_ed_base.as<int32_t>();
  return ag::launch_ed25519_verify(p, c->stream) == hipSuccess ? AG_RS_OK : AG_RS_ERR_DEVICE;
}

int ag_shred_validate_batch(ag_rs_ctx* c, size_t n, const uint8_t* data, size_t data_stride, size_t data_bytes,
                            const uint32_t* shred_index, const uint8_t* proofs, size_t proofs_stride, size_t height,
                            const uint64_t* slots, const uint64_t* slice_indices, const uint8_t* is_last,
                            const uint8_t* sigs, size_t sig_stride, const uint8_t* pk, const uint8_t* cached,
                            const uint8_t* has_cached, uint8_t* status, uint8_t* roots_out, uint8_t* commitments_out) {
  return shred_validate_impl(c, n, data, data_stride, data_bytes, shred_index, proofs, proofs_stride, height, slots,
                             slice_indices, is_last, sigs, sig_stride, pk, cached, has_cached, 1, nullptr, status,
                             roots_out, commitments_out);
}

}  // extern "C"

namespace ag::host {

// ag_shred_validate_batch with the cache entries shared by cached_group consecutive shreds
// (the composed deshred: one cached commitment per slice).
int shred_validate_impl(ag_rs_ctx* c, size_t n, const uint8_t* data, size_t data_stride, size_t data_bytes,
                        const uint32_t* shred_index, const uint8_t* proofs, size_t proofs_stride, size_t height,
                        const uint64_t* slots, const uint64_t* slice_indices, const uint8_t* is_last,
                        const uint8_t* sigs, size_t sig_stride, const uint8_t* pk, const uint8_t* cached,
                        const uint8_t* has_cached, uint32_t cached_group, const uint8_t* active, uint8_t* status,
                        uint8_t* roots_out, uint8_t* commitments_out, uint8_t* leaf_nodes, size_t leaf_nodes_stride,
                        uint32_t leaves_per_tree, size_t group_stride, uint32_t skip_row, bool roots_ready,
                        const uint32_t* leaf_sizes, uint32_t size_group) {
  // leaf_sizes / size_group (device, nullable): one shred size per size_group consecutive shreds
  // (MerkleVerifyParams; data_bytes then only bounds the sizes).
  // roots_ready: step 1 already ran (launch_derive_roots, e.g. on another stream): roots_out holds
  // every active shred's derived root
  if (roots_ready && !roots_out) return AG_RS_ERR_INVALID_ARGUMENT;
  if (!c || n >= kMaxSigBatch || data_bytes >= (size_t{1} << 28) ||
      height > static_cast<size_t>(ag::kMerkleMaxHeight) ||
      (n && (!shred_index || !slots || !slice_indices || !is_last || !sigs || !pk || !status ||
             (data_bytes && !data) || (height && !proofs))) ||
      (cached == nullptr) != (has_cached == nullptr) || proofs_stride % 16 ||
      reinterpret_cast<uintptr_t>(proofs) % 16 || (n > 1 && data_stride < data_bytes))
    return AG_RS_ERR_INVALID_ARGUMENT;
  if (n == 0) return AG_RS_OK;
  if (c->enter()) return AG_RS_ERR_DEVICE;
  int st = ensure_ed_base(c);
  if (st) return st;
  uint8_t* roots = roots_out;
  if (!roots) {
    if ((st = c->d_sh_roots.ensure(32 * n, c->stream))) return st;
    roots = c->d_sh_roots.as<uint8_t>();
  }
  uint8_t* commits = commitments_out;
  if (!commits) {
    if ((st = c->d_sh_commit.ensure(ag::kSliceCommitmentLen * n, c->stream))) return st;
    commits = c->d_sh_commit.as<uint8_t>();
  }
  if ((st = c->d_sh_onvalid.ensure(n, c->stream)) || (st = c->d_sh_list.ensure(4 * (n + 1), c->stream))) return st;
  uint32_t* list = c->d_sh_list.as<uint32_t>();
  uint32_t* count = list + n;
  // 1. Shred::slice_root (shredder.rs:168-175): derive_root from the Merkle path
  ag::MerkleVerifyParams mp{};
  mp.leaves = data;
  mp.leaf_stride = data_stride;
  mp.leaf_bytes = static_cast<uint32_t>(data_bytes);
  mp.height = static_cast<uint32_t>(height);
  mp.index = shred_index;
  mp.proofs = proofs;
  mp.proofs_stride = proofs_stride;
  mp.n = n;
  mp.roots_out = roots;
  mp.active = active;
  mp.list = list;  // scratch until the signature list below reuses it (stream order)
  mp.leaf_nodes = leaf_nodes;  // the leaf digests for a later Merkle rebuild over the same rows
  mp.leaf_nodes_stride = leaf_nodes_stride;
  mp.leaves_per_tree = leaves_per_tree;
  mp.group_stride = group_stride;
  mp.skip_row = skip_row;
  mp.leaf_sizes = leaf_sizes;
  mp.size_group = size_group;
  if (!roots_ready && ag::launch_merkle_verify(mp, c->stream) != hipSuccess) return AG_RS_ERR_DEVICE;
  // 2. SliceCommitment + cached-commitment rule (validated_shred.rs:57-64)
  AG_HIP(hipMemsetAsync(count, 0, 4, c->stream));
  ag::ShredCommitParams cp{};
  cp.slots = slots;
  cp.slice_indices = slice_indices;
  cp.is_last = is_last;
  cp.roots = roots;
  cp.cached = cached;
  cp.has_cached = has_cached;
  cp.cached_group = cached_group;
  cp.active = active;
  cp.n = n;
  cp.commitments = commits;
  cp.status = status;
  cp.on_valid = c->d_sh_onvalid.as<uint8_t>();
  cp.list = list;
  cp.list_count = count;
  if (ag::launch_shred_commit(cp, c->stream) != hipSuccess) return AG_RS_ERR_DEVICE;
  // 3. signature checks for the listed shreds (validated_shred.rs:65-77)
  ag::EdVerifyParams vp{};
  vp.pks = pk;
  vp.pk_stride = 0;
  vp.msgs = commits;
  vp.msg_stride = ag::kSliceCommitmentLen;
  vp.msg_len = ag::kSliceCommitmentLen;
  vp.sigs = sigs;
  vp.sig_stride = sig_stride;
  vp.n = n;
  vp.list = list;
  vp.list_count = count;
  vp.status = status;
  vp.on_valid = c->d_sh_onvalid.as<uint8_t>();
  vp.base_table = c->d_ed_base.as<int32_t>();
  return ag::launch_ed25519_verify(vp, c->stream) == hipSuccess ? AG_RS_OK : AG_RS_ERR_DEVICE;
}

}  // namespace ag::host

extern "C" {

int ag_slice_sign_batch(ag_rs_ctx* c, size_t nslices, const uint8_t* seed, const uint8_t* pk, const uint64_t* slots,
                        const uint64_t* slice_indices, const uint8_t* is_last, const uint8_t* roots, uint8_t* sigs,
                        uint8_t* commitments_out) {
  if (!c || nslices >= kMaxSigBatch ||
      (nslices && (!seed || !pk || !slots || !slice_indices || !is_last || !roots || !sigs)))
    return AG_RS_ERR_INVALID_ARGUMENT;
  if (nslices == 0) return AG_RS_OK;
  if (c->enter()) return AG_RS_ERR_DEVICE;
  int st = ensure_ed_base(c);
  if (st) return st;
  uint8_t* commits = commitments_out;
  if (!commits) {
    if ((st = c->d_sh_commit.ensure(ag::kSliceCommitmentLen * nslices, c->stream))) return st;
    commits = c->d_sh_commit.as<uint8_t>();
  }
  const size_t n = nslices;
  if ((st = c->d_sh_onvalid.ensure(2 * n, c->stream)) || (st = c->d_sh_list.ensure(4 * (n + 1), c->stream)))
    return st;
  uint32_t* list = c->d_sh_list.as<uint32_t>();
  AG_HIP(hipMemsetAsync(list + n, 0, 4, c->stream));
  // SliceCommitment::new (shredder.rs:206-215); no cache, so every slice is listed
  ag::ShredCommitParams cp{};
  cp.slots = slots;
  cp.slice_indices = slice_indices;
  cp.is_last = is_last;
  cp.roots = roots;
  cp.n = n;
  cp.commitments = commits;
  cp.status = c->d_sh_onvalid.as<uint8_t>() + n;
  cp.on_valid = c->d_sh_onvalid.as<uint8_t>();
  cp.list = list;
  cp.list_count = list + n;
  if (ag::launch_shred_commit(cp, c->stream) != hipSuccess) return AG_RS_ERR_DEVICE;
  // sk.sign_bytes(commitment) (shredder.rs:540)
  ag::EdSignParams p{};
  p.seeds = seed;
  p.seed_stride = 0;
  p.pks = pk;
  p.pk_stride = 0;
  p.msgs = commits;
  p.msg_stride = ag::kSliceCommitmentLen;
  p.msg_len = ag::kSliceCommitmentLen;
  p.sigs = sigs;
  p.n = n;
  p.base_table = c->d_ed_base.as<int32_t>();
  return ag::launch_ed25519_sign(p, c->stream) == hipSuccess ? AG_RS_OK : AG_RS_ERR_DEVICE;
}

// ---- shred wire format ----------------------------------------------------------------

namespace {
bool columns_ok(const ag_shred_columns* c) {
  return c && c->kind && c->slot && c->slice_index && c->is_last && c->shred_index && c->data_len && c->sig &&
         c->height && (c->data || c->data_stride == 0) && (c->proof || c->proof_stride == 0);
}
ag::ShredColumns to_columns(const ag_shred_columns* c) {
  ag::ShredColumns r{};
  r.kind = c->kind;
  r.slot = c->slot;
  r.slice_index = c->slice_index;
  r.is_last = c->is_last;
  r.shred_index = c->shred_index;
  r.data = c->data;
  r.data_stride = c->data_stride;
  r.data_len = c->data_len;
  r.sig = c->sig;
  r.proof = c->proof;
  r.proof_stride = c->proof_stride;
  r.height = c->height;
  return r;
}
}  // namespace

int ag_shred_deserialize_batch(ag_rs_ctx* c, size_t n, const uint8_t* packets, size_t packet_stride,
                               const uint32_t* packet_lens, const ag_shred_columns* cols, uint8_t* status) {
  if (!c || n >= kMaxSigBatch || (n && (!packets || !packet_lens || !status || !columns_ok(cols))))
    return AG_RS_ERR_INVALID_ARGUMENT;
  if (n == 0) return AG_RS_OK;
  if (c->enter()) return AG_RS_ERR_DEVICE;
  return ag::launch_shred_deserialize(packets, packet_stride, packet_lens, n, to_columns(cols), status, c->stream) ==
                 hipSuccess
             ? AG_RS_OK
             : AG_RS_ERR_DEVICE;
}

int ag_shred_serialize_batch(ag_rs_ctx* c, size_t n, const ag_shred_columns* cols, uint8_t* packets,
                             size_t packet_stride, uint32_t* packet_lens) {
  if (!c || n >= kMaxSigBatch || (n && (!packets || !packet_lens || !columns_ok(cols))))
    return AG_RS_ERR_INVALID_ARGUMENT;
  if (n == 0) return AG_RS_OK;
  if (c->enter()) return AG_RS_ERR_DEVICE;
  return ag::launch_shred_serialize(to_columns(cols), n, packets, packet_stride, packet_lens, c->stream) ==
                 hipSuccess
             ? AG_RS_OK
             : AG_RS_ERR_DEVICE;
}

int ag_shred_datagram_bytes(size_t shred_bytes, size_t proof_len, size_t* out) {
  if (!out || shred_bytes > ag::kMtuBytes || proof_len > ag::kMtuBytes / 32) return AG_RS_ERR_INVALID_ARGUMENT;
  const size_t len = ag::kShredHeadBytes + shred_bytes + 64 + 8 + 32 * proof_len;
  if (len > ag::kMtuBytes) return AG_RS_ERR_INVALID_ARGUMENT;
  *out = len;
  return AG_RS_OK;
}

int ag_slice_frame_batch(ag_rs_ctx* c, size_t nslices, size_t shred_bytes, const uint8_t* parent_flags,
                         const uint8_t* parent_ids, const uint8_t* data, size_t data_stride, const uint32_t* data_lens,
                         uint8_t* codewords, size_t codeword_stride, uint32_t* payload_lens_out) {
  if (!c) return AG_RS_ERR_INVALID_ARGUMENT;
  if (nslices == 0) return AG_RS_OK;
  if (!parent_flags || !parent_ids || !data_lens || !codewords || !payload_lens_out || nslices > 0x7FFFFFFFull ||
      shred_bytes == 0 || reinterpret_cast<uintptr_t>(codewords) % 4 || codeword_stride % 4 ||
      (nslices > 1 && codeword_stride < 32 * shred_bytes))
    return AG_RS_ERR_INVALID_ARGUMENT;
  size_t max_len = 0;
  for (size_t b = 0; b < nslices; ++b) {
    if (parent_flags[b] > 1) return AG_RS_ERR_INVALID_ARGUMENT;
    const size_t framed = 1 + (parent_flags[b] ? AG_SLICE_BLOCK_ID_BYTES : 0) + 8 + size_t{data_lens[b]};
    if (framed > AG_SLICE_MAX_DATA || framed >= 32 * shred_bytes) return AG_RS_ERR_TOO_MUCH_DATA;
    max_len = std::max<size_t>(max_len, data_lens[b]);
  }
  if (max_len && (!data || (nslices > 1 && data_stride < max_len))) return AG_RS_ERR_INVALID_ARGUMENT;
  if (c->enter()) return AG_RS_ERR_DEVICE;
  // metadata: flags | ids | lens, one upload
  const size_t off_ids = (nslices + 15) / 16 * 16, off_lens = off_ids + (nslices * AG_SLICE_BLOCK_ID_BYTES + 15) / 16 * 16;
  const size_t bytes = off_lens + 4 * nslices;
  int st = c->d_slice_meta.ensure(bytes, c->stream);
  if (st) return st;
  std::vector<uint8_t> meta(bytes, 0);
  std::memcpy(meta.data(), parent_flags, nslices);
  std::memcpy(meta.data() + off_ids, parent_ids, nslices * AG_SLICE_BLOCK_ID_BYTES);
  std::memcpy(meta.data() + off_lens, data_lens, 4 * nslices);
  AG_HIP(hipMemcpyAsync(c->d_slice_meta.ptr, meta.data(), bytes, hipMemcpyHostToDevice, c->stream));
  ag::SliceFrameParams p{};
  uint8_t* d = c->d_slice_meta.as<uint8_t>();
  p.parent_flags = d;
  p.parent_ids = d + off_ids;
  p.data_lens = reinterpret_cast<const uint32_t*>(d + off_lens);
  p.data = data;
  p.data_stride = data_stride;
  p.cw = codewords;
  p.cw_stride = codeword_stride;
  p.n = nslices;
  if (ag::launch_slice_frame(p, c->stream) != hipSuccess) return AG_RS_ERR_DEVICE;
  AG_HIP(hipStreamSynchronize(c->stream));  // the host metadata buffer goes out of scope
  for (size_t b = 0; b < nslices; ++b)
    payload_lens_out[b] = static_cast<uint32_t>(1 + (parent_flags[b] ? AG_SLICE_BLOCK_ID_BYTES : 0) + 8 + data_lens[b]);
  return AG_RS_OK;
}

int ag_slice_parse_batch(ag_rs_ctx* c, size_t nslices, const uint8_t* codewords, size_t codeword_stride,
                         const int64_t* payload_lens, uint8_t* status, uint8_t* parent_flags, uint8_t* parent_ids,
                         uint32_t* data_offsets, uint32_t* data_lens) {
  if (!c) return AG_RS_ERR_INVALID_ARGUMENT;
  if (nslices == 0) return AG_RS_OK;
  if (!codewords || !payload_lens || !status || !parent_flags || !parent_ids || !data_offsets || !data_lens ||
      nslices > 0x7FFFFFFFull)
    return AG_RS_ERR_INVALID_ARGUMENT;
  for (size_t b = 0; b < nslices; ++b)  // the bytes parsed must lie inside the codeword
    if (nslices > 1 && payload_lens[b] > 0 && static_cast<uint64_t>(payload_lens[b]) > codeword_stride)
      return AG_RS_ERR_INVALID_ARGUMENT;
  if (c->enter()) return AG_RS_ERR_DEVICE;
  // device layout: lens (8n) | status (n) | flags (n) | ids (40n) | offsets (4n) | data lens (4n)
  const size_t o_st = 8 * nslices, o_fl = o_st + nslices, o_id = o_fl + nslices,
               o_off = (o_id + AG_SLICE_BLOCK_ID_BYTES * nslices + 3) / 4 * 4, o_len = o_off + 4 * nslices;
  const size_t bytes = o_len + 4 * nslices;
  int st = c->d_slice_meta.ensure(bytes, c->stream);
  if (st) return st;
  uint8_t* d = c->d_slice_meta.as<uint8_t>();
  AG_HIP(hipMemcpyAsync(d, payload_lens, 8 * nslices, hipMemcpyHostToDevice, c->stream));
  ag::SliceParseParams p{};
  p.cw = codewords;
  p.cw_stride = codeword_stride;
  p.payload_lens = reinterpret_cast<const int64_t*>(d);
  p.status = d + o_st;
  p.parent_flags = d + o_fl;
  p.parent_ids = d + o_id;
  p.data_offsets = reinterpret_cast<uint32_t*>(d + o_off);
  p.data_lens = reinterpret_cast<uint32_t*>(d + o_len);
  p.n = nslices;
  if (ag::launch_slice_parse(p, c->stream) != hipSuccess) return AG_RS_ERR_DEVICE;
  // read back through pinned staging (a pageable destination costs a staged copy: ~0.3 ms more
  // for a 65 536-slice batch)
  if ((st = c->h_slice_meta.ensure(bytes - o_st))) return st;
  const uint8_t* out = c->h_slice_meta.as<uint8_t>();
  AG_HIP(hipMemcpyAsync(c->h_slice_meta.ptr, d + o_st, bytes - o_st, hipMemcpyDeviceToHost, c->stream));
  AG_HIP(hipStreamSynchronize(c->stream));
  std::memcpy(status, out, nslices);
  std::memcpy(parent_flags, out + (o_fl - o_st), nslices);
  std::memcpy(parent_ids, out + (o_id - o_st), AG_SLICE_BLOCK_ID_BYTES * nslices);
  std::memcpy(data_offsets, out + (o_off - o_st), 4 * nslices);
  std::memcpy(data_lens, out + (o_len - o_st), 4 * nslices);
  return AG_RS_OK;
}

}  // extern "C"

namespace {
// ReedSolomonCoder::deshred (reed_solomon.rs:140-208, ANY_K) over the kept shreds of every
// slice without a host round trip, for whole-chunk shreds (S % 64 == 0): the per-slice
// patterns come from the kept-shred masks on the device (launch_pipe_patterns), the per-lane
// window decoder restores the data shreds, coder_strip finds each payload's padding, and the
// 32-point encode rewrites the coding shreds of the slices that decoded and stripped (store
// masks per slice; the others keep theirs).  HighRate 32:32 also takes shreds with a tail of
// T = S mod 64 >= 16 bytes (pipe_tail_ok): the tail is the last column (decode_h8's TAIL
// variant, the TAIL encode).  plen[s] as ag_rs_coder_deshred_batch: the
// payload length, or -NotEnoughShreds / -InvalidPadding.
//
// pipe_coder_enqueue runs slices s0 .. s0 + n of a batch whose scratch pipe_coder_reserve
// sized (cw / d_present already at slice s0); pipe_coder_finish reads the results back.  The
// store-mask kernel writes each slice's final result (length or error) into the strip words.
int pipe_coder_reserve(ag_rs_ctx* c, size_t ntot, size_t m) {
  int st;
  if ((st = c->ensure_tables()) || (st = c->d_pipe_few.ensure(ntot, c->stream)) ||
      (st = c->d_pipe_mask.ensure(8 * ntot, c->stream)) || (st = c->d_strip.ensure(8 * ntot, c->stream)))
    return st;
  if (m > kDataShreds)
    return (st = c->x128.dev.ensure(10 * ntot * 8, c->stream)) ? st : c->d_rows128.ensure(ntot * 128 * 4, c->stream);
  if ((st = c->xmask.dev.ensure(3 * ntot * 8, c->stream)) || (st = c->d_rows.ensure(ntot * 64 * 4, c->stream))) return st;
  c->xmask.key.clear();  // xmask.dev / d_rows no longer hold decode_device's cached patterns
  c->xmask_w = 0;
  return AG_RS_OK;
}
// The same for CodingOnlyShredder's coder (LowRate 32:64, shredder.rs:362-395) and
// PetsShredder's (32:33, :403-444; its recovery shards are the first 33 of 32:64's): every slice
// decodes in the W = 128 window as the two per-lane decode_x16 passes (the class-8 patterns of
// decode_device, built on the device by launch_pipe_patterns128), then the strip, and the
// LowRate re-encode of both 32-shard recovery chunks under the per-slice store masks.
// present: two words per slice (launch_pipe_patterns128).
int pipe_coder_enqueue_lowrate(ag_rs_ctx* c, size_t s0, size_t n, size_t S, uint8_t* cw, size_t cw_stride,
                               const uint64_t* d_present, size_t m) {
  constexpr size_t k = kDataShreds;
  const size_t cps = S / 64;
  uint64_t* xm = c->x128.dev.as<uint64_t>() + 10 * s0;
  uint32_t* rows = c->d_rows128.as<uint32_t>() + 128 * s0;
  uint8_t* few = c->d_pipe_few.as<uint8_t>() + s0;
  uint64_t* mask = c->d_pipe_mask.as<uint64_t>() + s0;
  int64_t* strip = c->d_strip.as<int64_t>() + s0;
  if (ag::launch_pipe_patterns128(d_present, n, xm, few, c->stream) != hipSuccess ||
      ag::launch_decode_rows128(xm, static_cast<uint32_t>(n), c->dtables(), rows, c->stream) != hipSuccess)
    return AG_RS_ERR_DEVICE;
  ag::DecodeXParams p{};
  p.rec = cw + k * S;
  p.rec_block_stride = cw_stride;
  p.rec_shard_stride = S;
  p.orig = cw;
  p.orig_block_stride = cw_stride;
  p.orig_shard_stride = S;
  p.rows = rows;
  p.rows_w = 128;
  p.k = static_cast<uint32_t>(k);
  p.m = 32;  // recovery shards per window half (the kernel addresses the rest from p.rec)
  p.chunk = 32;
  p.low_rate = 1;
  p.chunks_per_shard = static_cast<uint32_t>(cps);
  p.total_columns = static_cast<uint64_t>(n) * cps;
  p.per_lane = 1;
  for (int pass = 1; pass <= 2; ++pass) {
    p.pmask = xm + (pass == 1 ? 6 : 8) * n;
    if (ag::launch_decode_x(128, pass, p, (p.total_columns + 63) / 64, c->stream) != hipSuccess)
      return AG_RS_ERR_DEVICE;
  }
  if (ag::launch_coder_strip(cw, cw_stride, static_cast<uint32_t>(k * S), n, strip, c->stream) != hipSuccess ||
      ag::launch_pipe_store_masks(few, strip, d_present, 2, n, mask, -AG_RS_ERR_NOT_ENOUGH_SHARDS,
                                  -AG_RS_ERR_INVALID_PADDING, c->stream) != hipSuccess)
    return AG_RS_ERR_DEVICE;
  for (unsigned j = 0; j * 32 < m;) {  // the recovery chunks, two per launch (encode_cols' LowRate loop)
    ag::XformParams xp{};
    xp.in = cw;
    xp.in_block_stride = cw_stride;
    xp.in_shard_stride = S;
    xp.out = cw + (k + 32 * j) * S;
    xp.out_block_stride = cw_stride;
    xp.out_shard_stride = S;
    xp.out_mask = mask;  // the slice's absent coding shreds, all, or none
    xp.pattern_per_block = 1;
    xp.n_in = static_cast<uint32_t>(k);
    xp.chunks_per_shard = static_cast<uint32_t>(cps);
    xp.total_columns = static_cast<uint64_t>(n) * cps;
    const bool pair = j % 2 == 0 && (j + 1) * 32 < m && j < 4;
    xp.n_out = static_cast<uint32_t>(std::min<size_t>(pair ? 64 : 32, m - 32 * j));
    if ((pair ? ag::launch_xform_lowrate2(j / 2, xp, c->stream) : ag::launch_xform_lowrate(32, j, xp, c->stream)) !=
        hipSuccess)
      return AG_RS_ERR_DEVICE;
    j += pair ? 2 : 1;
  }
  return AG_RS_OK;
}

int pipe_coder_enqueue(ag_rs_ctx* c, size_t s0, size_t n, size_t S, uint8_t* cw, size_t cw_stride,
                       const uint64_t* d_present, size_t m, bool no_surplus) {
  constexpr size_t k = kDataShreds;
  // whole 64-byte chunks, then (S mod 64 = T >= 16) the shard's T-byte tail as one more column
  const size_t cps = (S + 63) / 64;
  const uint32_t tail = static_cast<uint32_t>(S % 64);
  if (n == 0) return AG_RS_OK;
  if (m > kDataShreds) return pipe_coder_enqueue_lowrate(c, s0, n, S, cw, cw_stride, d_present, m);
  constexpr size_t W = 64;
  uint64_t* xm = c->xmask.dev.as<uint64_t>() + 3 * s0;
  uint32_t* rows = c->d_rows.as<uint32_t>() + W * s0;
  uint8_t* few = c->d_pipe_few.as<uint8_t>() + s0;
  uint64_t* mask = c->d_pipe_mask.as<uint64_t>() + s0;
  int64_t* strip = c->d_strip.as<int64_t>() + s0;
  // The window decode also restores the absent coding shreds of exactly-k slices (few 2): the
  // re-encode below skips those.  1 KiB shreds (every maximum slice) run the packed decoder
  // (decode_pk<-1>), the other whole-chunk sizes decode_h8<-1> (the full 64-point FFT).
  const bool fuse = true;
  if (ag::launch_pipe_patterns(d_present, n, xm, few, fuse, c->stream) != hipSuccess ||
      ag::launch_decode_rows(xm, xm + n, static_cast<uint32_t>(n), static_cast<uint32_t>(W), c->dtables(), rows, true,
                             c->stream) != hipSuccess)
    return AG_RS_ERR_DEVICE;
  ag::DecodeXParams p{};
  p.rec = cw + k * S;
  p.rec_block_stride = cw_stride;
  p.rec_shard_stride = S;
  p.orig = cw;
  p.orig_block_stride = cw_stride;
  p.orig_shard_stride = S;
  p.pmask = xm + n;
  p.rows = rows;
  p.k = static_cast<uint32_t>(k);
  p.m = 32;
  p.chunk = 32;
  p.low_rate = 0;
  p.chunks_per_shard = static_cast<uint32_t>(cps);
  p.total_columns = static_cast<uint64_t>(n) * cps;
  p.per_lane = 1;
  p.rows_w = static_cast<uint32_t>(W);
  p.any_k = 1;  // launch_pipe_patterns keeps exactly k survivors
  p.fuse = fuse ? 1u : 0u;
  p.tail_bytes = tail;
  if (ag::launch_decode_x(static_cast<unsigned>(W), 0, p, (p.total_columns + 63) / 64, c->stream,
                          &c->last_window_kernels) != hipSuccess)
    return AG_RS_ERR_DEVICE;
  if (ag::launch_coder_strip(cw, cw_stride, static_cast<uint32_t>(k * S), n, strip, c->stream) != hipSuccess ||
      ag::launch_pipe_store_masks(few, strip, d_present, 1, n, mask, -AG_RS_ERR_NOT_ENOUGH_SHARDS,
                                  -AG_RS_ERR_INVALID_PADDING, c->stream) != hipSuccess)
    return AG_RS_ERR_DEVICE;
  ag::XformParams xp{};
  xp.in = cw;
  xp.in_block_stride = cw_stride;
  xp.in_shard_stride = S;
  xp.out = cw + k * S;
  xp.out_block_stride = cw_stride;
  xp.out_shard_stride = S;
  xp.out_mask = mask;
  xp.pattern_per_block = 1;
  xp.n_in = static_cast<uint32_t>(k);
  xp.n_out = 32;
  xp.chunks_per_shard = static_cast<uint32_t>(cps);
  xp.total_columns = static_cast<uint64_t>(n) * cps;
  xp.skip_idle = fuse ? 1u : 0u;  // tiles of fused slices only: nothing to re-encode
  xp.tail_bytes = tail;
  // fused, no slice with surplus shreds and none with every data shred: every store mask is
  // zero (exactly 32 kept: restored by the decode; fewer, or a failed strip: untouched)
  if (fuse && no_surplus) return AG_RS_OK;
  if (ag::launch_xform(ag::XformKind::kEncode32, xp, c->stream) != hipSuccess) return AG_RS_ERR_DEVICE;
  return AG_RS_OK;
}
// plen[0 .. n) from the store-mask kernels' results (synchronous): read back through pinned
// staging (a pageable destination would take the runtime's bounce path)
int pipe_coder_finish(ag_rs_ctx* c, size_t n, int64_t* plen) {
  int st;
  if ((st = c->h_strip.ensure(8 * n))) return st;
  AG_HIP(hipMemcpyAsync(c->h_strip.ptr, c->d_strip.ptr, 8 * n, hipMemcpyDeviceToHost, c->stream));
  AG_HIP(hipStreamSynchronize(c->stream));
  std::memcpy(plen, c->h_strip.ptr, 8 * n);
  return AG_RS_OK;
}
}  // namespace

namespace ag::host {
// The whole batch in one range (the composed deshred's coder stage).  no_surplus: the caller
// knows that no slice keeps more than 32 shreds and none keeps all 32 data shreds.
int pipe_coder_deshred(ag_rs_ctx* c, size_t n, size_t S, uint8_t* cw, size_t cw_stride, const uint64_t* d_present,
                       int64_t* plen, size_t m, bool no_surplus) {
  int st;
  if ((st = pipe_coder_reserve(c, n, m)) ||
      (st = pipe_coder_enqueue(c, 0, n, S, cw, cw_stride, d_present, m, no_surplus)))
    return st;
  return pipe_coder_finish(c, n, plen);
}
// The device stages of ag_rs_coder_deshred_batch_var (32:32, ANY_K) over present words and the
// size / column table already on the device (d_sizes[n], d_col_base[n + 1] with total_columns its
// last entry): pipe_coder_enqueue's stages over the column table -- patterns and locator
// constants (they do not depend on S), the window decode with the fused coding restore, the
// strip, the store masks, and the re-encode when `reencode` (some slice has surplus shreds or
// every data shred; otherwise every store mask is zero).  Synchronous: plen[s] on return.  The
// caller has reset last_encode_kernels / last_window_kernels.
// exact: the crate's decoder over every kept shred instead (launch_pipe_patterns' exact masks, no
// fused coding restore): the same kernels -- var_decode runs the full 64-point window whatever
// the masks, and the store masks re-encode every coding shred of a surplus slice.
int pipe_coder_deshred_var(ag_rs_ctx* c, size_t n, uint8_t* cw, size_t cw_stride, const uint64_t* d_present,
                           const uint32_t* d_sizes, const uint32_t* d_col_base, uint32_t total_columns,
                           bool reencode, int64_t* plen, bool exact) {
  int st;
  if ((st = pipe_coder_reserve(c, n, kDataShreds))) return st;
  uint64_t* xm = c->xmask.dev.as<uint64_t>();
  uint32_t* rows = c->d_rows.as<uint32_t>();
  uint8_t* few = c->d_pipe_few.as<uint8_t>();
  uint64_t* mask = c->d_pipe_mask.as<uint64_t>();
  int64_t* strip = c->d_strip.as<int64_t>();
  if (ag::launch_pipe_patterns(d_present, n, xm, few, true, c->stream, exact) != hipSuccess ||
      ag::launch_decode_rows(xm, xm + n, static_cast<uint32_t>(n), 64, c->dtables(), rows, true, c->stream) !=
          hipSuccess)
    return AG_RS_ERR_DEVICE;
  ag::VarParams p{};
  p.cw = cw;
  p.stride = cw_stride;
  p.sizes = d_sizes;
  p.col_base = d_col_base;
  p.nslices = static_cast<uint32_t>(n);
  p.total_columns = total_columns;
  p.pmask = xm + n;
  p.rows = rows;
  c->last_window_kernels |= ag::kDxVar;
  if (ag::launch_var_decode(p, c->stream) != hipSuccess ||
      ag::launch_var_strip(cw, cw_stride, d_sizes, n, strip, c->stream) != hipSuccess ||
      ag::launch_pipe_store_masks(few, strip, d_present, 1, n, mask, -AG_RS_ERR_NOT_ENOUGH_SHARDS,
                                  -AG_RS_ERR_INVALID_PADDING, c->stream) != hipSuccess)
    return AG_RS_ERR_DEVICE;
  if (reencode) {
    p.out_mask = mask;
    c->last_encode_kernels |= ag::kEkVar;
    if (ag::launch_var_encode(p, c->stream) != hipSuccess) return AG_RS_ERR_DEVICE;
  }
  return pipe_coder_finish(c, n, plen);
}
// shred sizes pipe_coder_deshred decodes on the device: whole 64-byte chunks (any m of the
// device-pattern path), or for 32:32 a last chunk of T = S mod 64 bytes -- T >= 16 always, a
// shorter T when no slice needs the re-encode (no_reencode: no surplus shreds, no slice with
// every data shred; the TAIL encode takes T >= 16 only)
bool pipe_tail_ok(size_t S, size_t m, bool no_reencode) {
  const size_t T = S % 64;
  return T == 0 || (m == kDataShreds && S % 2 == 0 && (T >= 16 || no_reencode));
}
}  // namespace ag::host

extern "C" {

// ---- mixed shred sizes (ag_rs_coder_*_batch_var; kernels in rs_var.hip) -------------------
namespace {
// batches whose column table fits 32-bit column indices (16 columns per slice at most)
constexpr size_t kVarMaxSlices = size_t{1} << 27;

// sizes[0 .. n) and the column prefix col_base[0 .. n] (cols_b = ceil(S_b / 64)) behind it
void var_column_table(const uint32_t* S, size_t n, uint32_t* sizes, uint32_t* col_base) {
  uint32_t cols = 0;
  for (size_t b = 0; b < n; ++b) {
    sizes[b] = S[b];
    col_base[b] = cols;
    cols += (S[b] + 63) / 64;
  }
  col_base[n] = cols;
}

// S of ReedSolomonCoder::shred for a payload of len bytes (reed_solomon.rs:94-95)
size_t var_shred_size(size_t len) { return (len + 2 * kDataShreds - len % (2 * kDataShreds)) / kDataShreds; }

// the slow path hands runs of consecutive equal S_b to the uniform call: the end of b's run
size_t var_run_end(const uint32_t* S, size_t n, size_t b) {
  size_t e = b + 1;
  while (e < n && S[e] == S[b]) ++e;
  return e;
}
}  // namespace

int ag_rs_coder_shred_bytes(size_t len, size_t* shred_bytes) {
  if (!shred_bytes) return AG_RS_ERR_INVALID_ARGUMENT;
  if (len > kMaxPayload) return AG_RS_ERR_TOO_MUCH_DATA;
  *shred_bytes = var_shred_size(len);
  return AG_RS_OK;
}

int ag_rs_coder_shred_batch_var(ag_rs_ctx* c, size_t m, size_t n, const uint8_t* payloads, size_t payload_stride,
                                const uint32_t* lens, uint8_t* cw, size_t cw_stride, uint32_t* shred_bytes_out) {
  if (!c || (n && (!lens || !cw))) return AG_RS_ERR_INVALID_ARGUMENT;
  if (m == 0 || m > kTotalShreds) return AG_RS_ERR_UNSUPPORTED_SHARD_COUNT;
  if (n == 0) return AG_RS_OK;
  if (n > kVarMaxSlices) return AG_RS_ERR_INVALID_ARGUMENT;
  size_t max_s = 0;
  for (size_t b = 0; b < n; ++b) {
    if (lens[b] > kMaxPayload) return AG_RS_ERR_TOO_MUCH_DATA;
    max_s = std::max(max_s, var_shred_size(lens[b]));
  }
  if (cw_stride < (kDataShreds + m) * max_s) return AG_RS_ERR_INVALID_ARGUMENT;
  int st = c->enter();
  if (st) return st;
  // lens | sizes | col_base through the lengths' pinned staging, rewritten once its last upload
  // has completed (ag_rs_coder_shred_batch)
  if (c->lens_ev) AG_HIP(hipEventSynchronize(c->lens_ev));
  else AG_HIP(hipEventCreateWithFlags(&c->lens_ev, hipEventDisableTiming));
  const size_t words = 3 * n + 1;
  if ((st = c->h_lens.ensure(words * 4))) return st;
  uint32_t* h = c->h_lens.as<uint32_t>();
  std::memcpy(h, lens, n * 4);
  for (size_t b = 0; b < n; ++b) h[n + b] = static_cast<uint32_t>(var_shred_size(lens[b]));
  var_column_table(h + n, n, h + n, h + 2 * n);
  if (shred_bytes_out) std::memcpy(shred_bytes_out, h + n, n * 4);
  c->last_encode_kernels = 0;
  if (m != kDataShreds || odd_layout(cw, cw, cw_stride, cw_stride)) {
    const std::vector<uint32_t> S(h + n, h + 2 * n);  // (the uniform calls reuse the staging)
    for (size_t b = 0, e; b < n; b = e) {
      e = var_run_end(S.data(), n, b);
      if ((st = ag_rs_coder_shred_batch(c, m, e - b, S[b], payloads ? payloads + b * payload_stride : nullptr,
                                        payload_stride, lens + b, cw + b * cw_stride, cw_stride)))
        return st;
    }
    return AG_RS_OK;
  }
  if ((st = c->d_lens.ensure(words * 4, c->stream))) return st;
  AG_HIP(hipMemcpyAsync(c->d_lens.ptr, h, words * 4, hipMemcpyHostToDevice, c->stream));
  AG_HIP(hipEventRecord(c->lens_ev, c->stream));
  const uint32_t* d = c->d_lens.as<uint32_t>();
  if (ag::launch_var_pad(payloads, payload_stride, d, d + n, cw, cw_stride, n, c->stream) != hipSuccess)
    return AG_RS_ERR_DEVICE;
  ag::VarParams p{};
  p.cw = cw;
  p.stride = cw_stride;
  p.sizes = d + n;
  p.col_base = d + 2 * n;
  p.nslices = static_cast<uint32_t>(n);
  p.total_columns = h[3 * n];
  c->last_encode_kernels |= ag::kEkVar;
  return ag::launch_var_encode(p, c->stream) == hipSuccess ? AG_RS_OK : AG_RS_ERR_DEVICE;
}

int ag_rs_coder_deshred_batch_var(ag_rs_ctx* c, size_t m, size_t n, const uint32_t* S, uint8_t* cw, size_t cw_stride,
                                  const uint8_t* dpres, const uint8_t* cpres, int mode, int64_t* out) {
  if (!c || (n && (!S || !cw || !dpres || !cpres || !out))) return AG_RS_ERR_INVALID_ARGUMENT;
  if (m == 0 || m > kTotalShreds) return AG_RS_ERR_UNSUPPORTED_SHARD_COUNT;
  if (mode != AG_RS_DECODE_EXACT && mode != AG_RS_DECODE_ANY_K) return AG_RS_ERR_INVALID_ARGUMENT;
  if (n == 0) return AG_RS_OK;
  if (n > kVarMaxSlices) return AG_RS_ERR_INVALID_ARGUMENT;
  size_t max_s = 0;
  for (size_t b = 0; b < n; ++b) {
    if (S[b] == 0 || S[b] % 2) return AG_RS_ERR_INVALID_SHARD_SIZE;
    if (kDataShreds * S[b] > kMaxAfterPadding) return AG_RS_ERR_TOO_MUCH_DATA;  // reed_solomon.rs:183
    max_s = std::max<size_t>(max_s, S[b]);
  }
  if (cw_stride < (kDataShreds + m) * max_s) return AG_RS_ERR_INVALID_ARGUMENT;
  int st = c->enter();
  if (st) return st;
  c->last_encode_kernels = 0;
  c->last_window_kernels = 0;
  auto fallback = [&]() {
    uint32_t ek = 0, wk = 0;  // (each uniform call resets the records)
    int r = AG_RS_OK;
    for (size_t b = 0, e; b < n && !r; b = e) {
      e = var_run_end(S, n, b);
      r = ag_rs_coder_deshred_batch(c, m, e - b, S[b], cw + b * cw_stride, cw_stride, dpres + b * kDataShreds,
                                    cpres + b * m, mode, out + b);
      ek |= c->last_encode_kernels;
      wk |= c->last_window_kernels;
    }
    c->last_encode_kernels = ek;
    c->last_window_kernels = wk;
    return r;
  };
  if (m != kDataShreds || odd_layout(cw, cw, cw_stride, cw_stride)) return fallback();
  // present words | sizes | col_base, packed straight into the present words' pinned staging
  // (ag_rs_coder_deshred_batch's device-pattern path)
  if (c->present_ev) AG_HIP(hipEventSynchronize(c->present_ev));
  else AG_HIP(hipEventCreateWithFlags(&c->present_ev, hipEventDisableTiming));
  const size_t bytes = 8 * n + 4 * (2 * n + 1);
  if ((st = c->h_present.ensure(bytes))) return st;
  uint64_t* pres = c->h_present.as<uint64_t>();
  bool full_data = false;
  const bool surplus = pack_present_words(dpres, cpres, m, n, pres, &full_data);
  // EXACT with surplus shreds: the crate's decoder reads every kept shred (the uniform call's host path)
  if (mode != AG_RS_DECODE_ANY_K && surplus) return fallback();
  uint32_t* h = reinterpret_cast<uint32_t*>(pres + n);
  var_column_table(S, n, h, h + n);
  if ((st = c->d_present.ensure(bytes, c->stream))) return st;
  AG_HIP(hipMemcpyAsync(c->d_present.ptr, pres, bytes, hipMemcpyHostToDevice, c->stream));
  AG_HIP(hipEventRecord(c->present_ev, c->stream));
  const uint64_t* d_present = c->d_present.as<uint64_t>();
  const uint32_t* d = reinterpret_cast<const uint32_t*>(d_present + n);
  // no surplus and no slice with every data shred: every store mask is zero (pipe_coder_enqueue)
  return pipe_coder_deshred_var(c, n, cw, cw_stride, d_present, d, d + n, h[2 * n], surplus || full_data, out);
}

}  // extern "C"

namespace ag::host {
// sizes | column prefix of a batch of mixed shred sizes (checked by the caller: each even, 2 ..
// 1024) onto the device through the staging of ag_rs_coder_shred_batch_var's table (h_lens ->
// d_lens, rewritten once its last upload has completed): for the composed var deshred, whose
// kernels read the sizes from the first stage on, before any present words exist.  Valid on
// the stream until the next coder shred call on the context.
int upload_var_sizes(ag_rs_ctx* c, size_t n, const uint32_t* S, const uint32_t** d_sizes, const uint32_t** d_col_base,
                     uint32_t* total_columns) {
  if (n > kVarMaxSlices) return AG_RS_ERR_INVALID_ARGUMENT;
  if (c->lens_ev) AG_HIP(hipEventSynchronize(c->lens_ev));
  else AG_HIP(hipEventCreateWithFlags(&c->lens_ev, hipEventDisableTiming));
  const size_t words = 2 * n + 1;
  int st;
  if ((st = c->h_lens.ensure(words * 4)) || (st = c->d_lens.ensure(words * 4, c->stream))) return st;
  uint32_t* h = c->h_lens.as<uint32_t>();
  var_column_table(S, n, h, h + n);
  AG_HIP(hipMemcpyAsync(c->d_lens.ptr, h, words * 4, hipMemcpyHostToDevice, c->stream));
  AG_HIP(hipEventRecord(c->lens_ev, c->stream));
  *d_sizes = c->d_lens.as<uint32_t>();
  *d_col_base = *d_sizes + n;
  *total_columns = h[2 * n];
  return AG_RS_OK;
}
}  // namespace ag::host
