// The device context behind the C ABI (include/alpenglow_rs.h) and the helpers the host
// translation units share: rs_api.cpp, rs_coder_api.cpp, crypto_api.cpp and wire_api.cpp (the C
// ABI), rs_dispatch.cpp (the batch encode / decode dispatch), shredder_api.cpp, intake_api.cpp, repair_api.cpp and block_api.cpp.  Internal: not
// installed, included only by the host .cpp files; nothing here is exported from the shared object.
#pragma once
#include <hip/hip_runtime.h>

#include <chrono>
#include <cstddef>
#include <cstdint>
#include <memory>
#include <type_traits>
#include <utility>
#include <vector>

#include "../../include/alpenglow_rs.h"
#include "cipher.hpp"
#include "gf16.hpp"
#include "merkle.hpp"
#include "rs_launch.hpp"

#define AG_HIP(expr)                                  \
  do {                                                \
    if ((expr) != hipSuccess) return AG_RS_ERR_DEVICE; \
  } while (0)

namespace ag {
namespace host __attribute__((visibility("hidden"))) {

// Grow-only device buffer.  Owns its memory: move-only, freed on destruction.
struct DevBuf {
  void* ptr = nullptr;
  size_t size = 0;
  DevBuf() = default;
  DevBuf(DevBuf&& o) noexcept : ptr(std::exchange(o.ptr, nullptr)), size(std::exchange(o.size, 0)) {}
  DevBuf& operator=(DevBuf&& o) noexcept {  // (declaring the moves deletes the copies)
    if (this != &o) release();
    ptr = std::exchange(o.ptr, nullptr);
    size = std::exchange(o.size, 0);
    return *this;
  }
  ~DevBuf() { release(); }
  int ensure(size_t n, hipStream_t stream) {
    if (n <= size) return AG_RS_OK;
    if (ptr) {
      if (hipStreamSynchronize(stream) != hipSuccess) return AG_RS_ERR_DEVICE;
      release();
    }
    if (hipMalloc(&ptr, n) != hipSuccess) return AG_RS_ERR_OUT_OF_MEMORY;
    size = n;
    return AG_RS_OK;
  }
  template <typename T>
  T* as() const {
    return static_cast<T*>(ptr);
  }
  void release() {
    if (ptr) (void)hipFree(ptr);
    ptr = nullptr;
    size = 0;
  }
};
static_assert(!std::is_copy_constructible_v<DevBuf> && !std::is_copy_assignable_v<DevBuf>);

// The typed sections of one buffer, each 256-byte aligned, in the order they are taken.  A call's
// scratch layout is a struct of typed pointers and a carve function that fills it; the function
// runs twice, over a null base for the size the buffer is grown to, then over the buffer.
struct Carver {
  uint8_t* base;
  size_t used = 0;
  template <typename T>
  T* take(size_t count) {
    T* out = base ? reinterpret_cast<T*>(base + used) : nullptr;
    used += (count * sizeof(T) + 255) / 256 * 256;
    return out;
  }
};

// Grow-only pinned host buffer, mapped and coherent (fine-grained: never cached in the GPU's
// L2, so one call's kernels cannot read another call's stale bytes): the crate-API
// single-call kernels read and write it directly (zero-copy).  Owns its memory like DevBuf.
struct PinBuf {
  void* ptr = nullptr;
  size_t size = 0;
  void* dptr = nullptr;
  PinBuf() = default;
  PinBuf(PinBuf&& o) noexcept { *this = std::move(o); }
  PinBuf& operator=(PinBuf&& o) noexcept {
    if (this != &o) release();
    ptr = std::exchange(o.ptr, nullptr);
    size = std::exchange(o.size, 0);
    dptr = std::exchange(o.dptr, nullptr);
    return *this;
  }
  ~PinBuf() { release(); }
  int ensure(size_t n) {
    if (n <= size) return AG_RS_OK;
    release();
    if (hipHostMalloc(&ptr, n, hipHostMallocMapped | hipHostMallocCoherent) != hipSuccess) {
      ptr = nullptr;
      return AG_RS_ERR_OUT_OF_MEMORY;
    }
    if (hipHostGetDevicePointer(&dptr, ptr, 0) != hipSuccess) {
      release();
      return AG_RS_ERR_DEVICE;
    }
    size = n;
    return AG_RS_OK;
  }
  template <typename T>
  T* as() const {
    return static_cast<T*>(ptr);
  }
  template <typename T>
  T* dev() const {  // the same bytes as the device addresses them (zero-copy over PCIe)
    return static_cast<T*>(dptr);
  }
  void release() {
    if (ptr) (void)hipHostFree(ptr);
    leak();
  }
  // Forgets the memory without freeing it: for staging that a device kernel which never quit
  // may still write (ag_rs_ctx::server_stop).
  void leak() {
    ptr = dptr = nullptr;
    size = 0;
  }
};
static_assert(!std::is_copy_constructible_v<PinBuf> && !std::is_copy_assignable_v<PinBuf>);

// "Upload only when the pattern set changed": a device buffer and the host key of what it
// holds.  While the key matches (steady-state batches) a call neither copies nor waits.
template <typename K>
struct UploadCache {
  std::vector<K> key;  // what `dev` holds; the context-owned source of upload()'s asynchronous copy
  DevBuf dev;
  bool holds(const std::vector<K>& k) const { return k == key; }
  // A miss: one stream synchronisation (a pending upload may still read `key`, queued kernels
  // `dev`), then `dev` grown to `bytes`.  The key is dropped -- every key has at least one
  // entry, so it matches nothing until the caller has filled `dev` and set it again.
  int renew(size_t bytes, hipStream_t stream) {
    AG_HIP(hipStreamSynchronize(stream));
    key.clear();
    return dev.ensure(bytes, stream);
  }
  // The key is the uploaded data: copied on the stream from the cache's own vector.
  int upload(std::vector<K>&& words, hipStream_t stream) {
    key = std::move(words);
    if (hipMemcpyAsync(dev.ptr, key.data(), key.size() * sizeof(K), hipMemcpyHostToDevice, stream) == hipSuccess)
      return AG_RS_OK;
    key.clear();
    return AG_RS_ERR_DEVICE;
  }
  int put(std::vector<K>&& words, hipStream_t stream) {
    if (holds(words)) return AG_RS_OK;
    const int st = renew(words.size() * sizeof(K), stream);
    return st ? st : upload(std::move(words), stream);
  }
};

// "Fill on the host, upload behind the queued work": pinned staging, the device buffer it is
// copied to, and the event recorded after the copy.  No stream synchronisation: the staging may
// be rewritten only once its last upload has completed, so host() waits for that event; a caller
// that returns between host() and send() has uploaded nothing and leaves the event as it was.
struct StagedUpload {
  PinBuf pin;
  DevBuf dev;
  hipEvent_t ev = nullptr;  // recorded after the last upload
  ~StagedUpload() {  // (the members free after it: once the last upload has read the staging)
    if (!ev) return;
    (void)hipEventSynchronize(ev);
    (void)hipEventDestroy(ev);
  }
  // *out: `bytes` of staging for the caller to fill.  `dev` is not touched: growing it may
  // synchronise the stream, which a caller that ends up uploading nothing must not pay for.
  template <typename T>
  int host(size_t bytes, T** out) {
    if (ev) AG_HIP(hipEventSynchronize(ev));
    else AG_HIP(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
    const int st = pin.ensure(bytes);
    *out = pin.as<T>();
    return st;
  }
  // The first `bytes` of the staging to `dst` on the stream, or to `dev`, grown to hold them.
  int send(size_t bytes, hipStream_t stream, void* dst = nullptr) {
    if (!dst) {
      const int st = dev.ensure(bytes, stream);
      if (st) return st;
      dst = dev.ptr;
    }
    AG_HIP(hipMemcpyAsync(dst, pin.ptr, bytes, hipMemcpyHostToDevice, stream));
    AG_HIP(hipEventRecord(ev, stream));
    return AG_RS_OK;
  }
};

}  // namespace host
}  // namespace ag

using ag::host::Carver;
using ag::host::DevBuf;
using ag::host::PinBuf;
using ag::host::StagedUpload;
using ag::host::UploadCache;

struct ag_rs_ctx {
  int device = 0;
  hipStream_t own_stream = nullptr;
  hipStream_t stream = nullptr;
  bool tables_ready = false;
  DevBuf d_exp, d_log, d_skew, d_log_walsh;
  DevBuf scratch;                         // generic-kernel work rows
  DevBuf d_flags, d_loc, d_blocks;          // generic decode: flags, locators, block ids
  // pattern uploads of the decoder classes (rs_dispatch.cpp), each cache with what is derived from it
  UploadCache<uint64_t> mask;               // store-mask words of the transform launches
  UploadCache<uint64_t> stage_mask;         // restride store / pack masks (sizes not whole 64-byte chunks)
  UploadCache<uint64_t> xmask;              // W <= 64 window masks, for W = xmask_w
  size_t xmask_w = 0;
  bool xmask_poly = false;                  // d_rows holds polynomial-basis constants (per-lane)
  DevBuf d_rows, d_xblocks;                 // their constants / matrices; window block ids (W = 128 too)
  UploadCache<uint64_t> x128;               // W = 128 two-pass masks
  DevBuf d_rows128;                         // their constants
  std::vector<uint32_t> x128_ids;           // host source of the W = 128 block-id upload (d_xblocks)
  UploadCache<uint8_t> syn;                 // syndrome patterns, key (k, m, present flags)
  DevBuf d_synblocks;                       // their block ids
  UploadCache<uint8_t> corr;                // correction patterns, key (k, m, present flags)
  DevBuf d_corrk, d_corrblocks;             // their K picks, block ids
  static constexpr int kClassSlots = 16;    // the test aid's out16: one counter per ag::DecodeClass value
  uint64_t last_classes[kClassSlots] = {};  // patterns per decoder class of the last decode call
  int decode_depth = 0;                     // decode_device nesting (tail restrides decode inside)
  uint32_t last_encode_kernels = 0;         // EncodeKernelBit of the last ag_rs_encode_batch / coder deshred batch
  uint32_t last_window_kernels = 0;         // DecodeXKernelBit of the last coder deshred batch's window decode
  DevBuf d_empty_roots;                     // Merkle EMPTY_ROOTS [32][8] words
  DevBuf d_merkle_nodes;                    // Merkle node scratch (callers without a nodes buffer)
  uint32_t last_merkle_kernels = 0;         // MerkleLeafKernelBit of the last Merkle build's leaf kernel
  StagedUpload leaf_sizes;                  // ag_merkle_build_batch_var: leaf size per slice
  StagedUpload block_meta;                  // block trees: first[nblocks] (u64), then count[nblocks] (u32)
  DevBuf d_aon_lens, d_aon_digests, d_aon_keys;  // all-or-nothing transforms
  DevBuf d_aon_lens2;                            // the side stream's SHA-256 lengths (AONT deshred)
  hipStream_t side = nullptr;                    // a second compute stream: used through SideScope only
  hipEvent_t side_fork = nullptr, side_join = nullptr;
  bool side_open = false;                        // a SideScope is open (they share the events: no nesting)
  DevBuf d_slice_meta;                           // slice framing / parsing metadata
  DevBuf stage_pad;                              // restrided shards (sizes not whole 64-byte chunks)
  StagedUpload lens;                        // coder shred batches: payload lengths (var: | sizes | column prefix)
  DevBuf d_strip;                           // coder batches: strip results
  DevBuf d_reenc_mask;                      // uniform coder deshreds: the re-encode's store mask word
  DevBuf d_pipe_few, d_pipe_mask;           // composed deshred: too-few flags, re-encode store masks
  StagedUpload present;                     // coder batches: per-slice present masks
  PinBuf h_strip;                           // coder deshred batches: pinned staging of the results
  PinBuf h_slice_meta;                      // slice parse batches: pinned staging of the results
  PinBuf h_pipe_meta;                       // composed deshreds: pinned staging of the per-slice columns
  StagedUpload rerun;                       // their EXACT re-run: list | sizes | column prefix (sent into d_pipe_rerun)
  uint64_t last_rerun_slices = 0, last_rerun_passes = 0;  // the last composed deshred's EXACT re-run (test aid)
  DevBuf d_ed_base;                         // Ed25519 fixed-base table (ed25519.hpp)
  DevBuf d_pipe;                            // composed shredders: one call's scratch, grown at entry (shredder_api.cpp carves it up)
  DevBuf d_pipe_rerun;                      // their EXACT re-run's scratch: grown in mid-call, so never part of d_pipe
  DevBuf d_sh_roots, d_sh_commit, d_sh_onvalid, d_sh_list;  // shred validation scratch
  DevBuf d_intake;                          // shred / repair intake scratch (intake_scratch.hpp carves it up)
  StagedUpload intake_win;                  // shred intake: slot ids ascending (u64), then their indices (u32);
                                            // repair intake: its blocks' slot ids (u64), in the caller's order
  PinBuf h_intake;                          // pinned staging of their per-row host outputs
  DevBuf d_block;                           // block assembly scratch and staged outputs (block_api.cpp carves it up)
  StagedUpload block_cols;                  // its host columns: data lengths | parent ids | row_ok | parent flags
  PinBuf h_block;                           // pinned staging of its host outputs
  // host-memory calls: two staging slots, H2D / D2H streams next to the compute stream
  struct Slot {
    DevBuf in, out;
    hipEvent_t up = nullptr, done = nullptr, down = nullptr;
  } slot[2];
  hipStream_t h2d = nullptr, d2h = nullptr;
  DevBuf one_in, one_out;                 // crate-API single codeword
  // per-call server (latency_server_kernel): mailbox in mapped host memory, its own stream
  ag::LatencyMailbox* mb = nullptr;
  ag::LatencyMailbox* mb_dev = nullptr;
  hipStream_t server_stream = nullptr;
  uint32_t server_seq = 0;
  uint32_t server_p_seq = 0, server_dp_seq = 0;  // versions of the parameters last posted
  bool server_broken = false;  // a job timed out: the server path is off for this context
  bool fail_next_server_job = false;  // test aid: the next server job takes the timeout path
  uint64_t server_jobs[4] = {};        // jobs posted per LatencyJob kind (test aid)
  std::vector<PinBuf> abandoned_pins;  // staging a timed-out job named (freed once the server is gone)

  // A stream switch forgets the pattern uploads: their copies were ordered on the old stream.
  void forget_uploads() {
    mask.key.clear();
    stage_mask.key.clear();
    xmask.key.clear();
    x128.key.clear();
    syn.key.clear();
    corr.key.clear();
  }

  int enter() { return hipSetDevice(device) == hipSuccess ? AG_RS_OK : AG_RS_ERR_DEVICE; }

  int ensure_tables() {
    if (tables_ready) return AG_RS_OK;
    const ag::Gf16Tables& t = ag::gf16_tables();
    // log_walsh: Walsh-Hadamard transform (mod 65535) of the log table with log[0] := 0
    // (crate engine/tables.rs initialize_log_walsh).
    std::vector<uint16_t> lw(t.log, t.log + ag::kGfOrder);
    lw[0] = 0;
    for (size_t dist = 1; dist < ag::kGfOrder; dist <<= 1)
      for (size_t r = 0; r < ag::kGfOrder; r += 2 * dist)
        for (size_t i = r; i < r + dist; ++i) {
          const uint32_t a = lw[i], b = lw[i + dist];
          const uint32_t s = a + b, d = a - b;
          lw[i] = static_cast<uint16_t>(s + (s >> 16));
          lw[i + dist] = static_cast<uint16_t>(d + (d >> 16));
        }
    int st;
    if ((st = d_exp.ensure(sizeof t.exp, stream)) || (st = d_log.ensure(sizeof t.log, stream)) ||
        (st = d_skew.ensure(sizeof t.skew, stream)) || (st = d_log_walsh.ensure(lw.size() * 2, stream)))
      return st;
    AG_HIP(hipMemcpy(d_exp.ptr, t.exp, sizeof t.exp, hipMemcpyHostToDevice));
    AG_HIP(hipMemcpy(d_log.ptr, t.log, sizeof t.log, hipMemcpyHostToDevice));
    AG_HIP(hipMemcpy(d_skew.ptr, t.skew, sizeof t.skew, hipMemcpyHostToDevice));
    AG_HIP(hipMemcpy(d_log_walsh.ptr, lw.data(), lw.size() * 2, hipMemcpyHostToDevice));
    tables_ready = true;
    return AG_RS_OK;
  }

  ag::GfDeviceTables dtables() const {
    return {d_exp.as<uint16_t>(), d_log.as<uint16_t>(), d_skew.as<uint16_t>(), d_log_walsh.as<uint16_t>()};
  }

  int ensure_side_stream() {
    if (side) return AG_RS_OK;
    AG_HIP(hipStreamCreateWithFlags(&side, hipStreamNonBlocking));
    AG_HIP(hipEventCreateWithFlags(&side_fork, hipEventDisableTiming));
    AG_HIP(hipEventCreateWithFlags(&side_join, hipEventDisableTiming));
    return AG_RS_OK;
  }

  int ensure_copy_streams() {
    if (h2d) return AG_RS_OK;
    AG_HIP(hipStreamCreateWithFlags(&h2d, hipStreamNonBlocking));
    AG_HIP(hipStreamCreateWithFlags(&d2h, hipStreamNonBlocking));
    for (Slot& s : slot) {
      AG_HIP(hipEventCreateWithFlags(&s.up, hipEventDisableTiming));
      AG_HIP(hipEventCreateWithFlags(&s.done, hipEventDisableTiming));
      AG_HIP(hipEventCreateWithFlags(&s.down, hipEventDisableTiming));
      AG_HIP(hipEventRecord(s.down, d2h));  // slots start free
    }
    return AG_RS_OK;
  }

  void server_stop() {
    if (!mb) return;
    (void)hipSetDevice(device);
    const auto t0 = std::chrono::steady_clock::now();
    if (__atomic_load_n(&mb->alive, __ATOMIC_ACQUIRE) != 0) {
      mb->kind = ag::kJobQuit;
      __atomic_store_n(&mb->doorbell, ++server_seq, __ATOMIC_RELEASE);
      while (__atomic_load_n(&mb->alive, __ATOMIC_ACQUIRE) != 0 &&
             std::chrono::steady_clock::now() - t0 < std::chrono::seconds(2)) {
      }
    }
    if (__atomic_load_n(&mb->alive, __ATOMIC_ACQUIRE) != 0) {
      // a server that neither served nor quit (server_broken): waiting on its stream could
      // block forever, and it may still write the mailbox or an abandoned staging buffer,
      // so those stay allocated
      mb = mb_dev = nullptr;
      server_stream = nullptr;
      for (PinBuf& b : abandoned_pins) b.leak();
      abandoned_pins.clear();
      return;
    }
    (void)hipStreamSynchronize(server_stream);  // the server has exited (quit or idle timeout)
    abandoned_pins.clear();
    (void)hipStreamDestroy(server_stream);
    (void)hipHostFree(mb);
    mb = mb_dev = nullptr;
    server_stream = nullptr;
  }

  // The buffers free themselves, after this body: it drains every stream first, so no queued
  // work or pending upload can touch a member when its destructor runs.
  ~ag_rs_ctx() {
    (void)hipSetDevice(device);
    server_stop();
    if (side) {
      (void)hipStreamSynchronize(side);
      (void)hipEventDestroy(side_fork);
      (void)hipEventDestroy(side_join);
      (void)hipStreamDestroy(side);
    }
    if (own_stream) (void)hipStreamSynchronize(own_stream);
    if (h2d) {
      (void)hipStreamSynchronize(h2d);
      (void)hipStreamSynchronize(d2h);
      for (Slot& s : slot)
        for (hipEvent_t e : {s.up, s.done, s.down})
          if (e) (void)hipEventDestroy(e);
      (void)hipStreamDestroy(h2d);
      (void)hipStreamDestroy(d2h);
    }
    if (own_stream) (void)hipStreamDestroy(own_stream);
  }
};

// Work on the context's side stream beside its main stream, and the one rule that goes with it: a
// call never returns while the side stream still runs work it enqueued, since that work reads and
// writes buffers the caller gets back.  open() forks the side stream from the main stream's
// current point, the launches in between go to stream(), close() marks their end and join() makes
// the main stream wait for it.  A scope destroyed between open() and join() -- any error return
// in between, written as a plain `return st;` -- waits for the side stream on the host.  The
// context's two events are shared, so scopes do not nest.  Nothing else touches c->side,
// side_fork or side_join.
namespace ag {
namespace host __attribute__((visibility("hidden"))) {
class SideScope {
 public:
  explicit SideScope(ag_rs_ctx* c) : c_(c) {}
  SideScope(const SideScope&) = delete;
  SideScope& operator=(const SideScope&) = delete;
  ~SideScope() {
    if (!open_) return;
    (void)hipStreamSynchronize(c_->side);
    c_->side_open = false;
  }
  int open() {
    if (c_->side_open) return AG_RS_ERR_DEVICE;
    const int st = c_->ensure_side_stream();
    if (st) return st;
    AG_HIP(hipEventRecord(c_->side_fork, c_->stream));
    AG_HIP(hipStreamWaitEvent(c_->side, c_->side_fork, 0));
    c_->side_open = open_ = true;
    return AG_RS_OK;
  }
  bool is_open() const { return open_; }
  hipStream_t stream() const { return c_->side; }
  int close() {
    AG_HIP(hipEventRecord(c_->side_join, c_->side));
    return AG_RS_OK;
  }
  int join() {
    AG_HIP(hipStreamWaitEvent(c_->stream, c_->side_join, 0));
    c_->side_open = open_ = false;
    return AG_RS_OK;
  }

 private:
  ag_rs_ctx* c_;
  bool open_ = false;
};
}  // namespace host
}  // namespace ag

// =====================================================================================
// Crate API mirror: ReedSolomonEncoder / ReedSolomonDecoder (one codeword, host memory)
// =====================================================================================
// An object made by *_new_on_device owns its context (`owned`: created with it, destroyed by
// its _free), so objects made that way share no state and may run on different threads at
// once; *_new borrows the caller's context, shared with whatever else uses it.
// Each encoder / decoder stages its codeword in its own mapped pinned buffer (the shards are
// copied there by add_*_shard, the device reads and writes it in place, and the result
// accessors point into it), so no call re-copies or re-zeroes a 64 KiB slice.
// `owned` is declared first, so it is destroyed last: the staging is freed before its context.
namespace ag {
namespace host __attribute__((visibility("hidden"))) {
struct CtxDestroy {
  void operator()(ag_rs_ctx* c) const { ag_rs_ctx_destroy(c); }
};
using OwnedCtx = std::unique_ptr<ag_rs_ctx, CtxDestroy>;
}  // namespace host
}  // namespace ag

struct ag_rs_encoder {
  ag::host::OwnedCtx owned;
  ag_rs_ctx* ctx = nullptr;
  size_t k = 0, m = 0, S = 0;
  size_t received = 0;
  bool encoded = false;
  PinBuf pin;  // originals [k * S] then recovery shards [m * S]
  uint8_t* orig() const { return pin.as<uint8_t>(); }
  uint8_t* rec() const { return pin.as<uint8_t>() + k * S; }
};

struct ag_rs_decoder {
  ag::host::OwnedCtx owned;
  ag_rs_ctx* ctx = nullptr;
  size_t k = 0, m = 0, S = 0;
  std::vector<uint8_t> opres, rpres;
  size_t no = 0, nr = 0;
  bool decoded = false;
  std::vector<uint8_t> restored;  // 1 where original i was restored by the last decode
  PinBuf pin;  // originals [k * S], recovery shards [m * S], re-encoded coding shards [m * S]
  uint8_t* orig() const { return pin.as<uint8_t>(); }
  uint8_t* rec() const { return pin.as<uint8_t>() + k * S; }
};

// What the host translation units call in each other; each is documented where it is defined.
namespace ag {
namespace host __attribute__((visibility("hidden"))) {

// rs_dispatch.cpp: the batch encode / decode over device memory
int check_geometry(size_t k, size_t m, size_t S);
bool odd_layout(const void* a, const void* b, size_t sa, size_t sb);
int encode_device(ag_rs_ctx* c, size_t k, size_t m, size_t S, size_t nblocks, const uint8_t* orig, size_t ostride,
                  uint8_t* rec, size_t rstride);
int decode_device(ag_rs_ctx* c, size_t k, size_t m, size_t S, size_t nblocks, uint8_t* orig, size_t ostride,
                  const uint8_t* rec, size_t rstride, const uint8_t* opres, const uint8_t* rpres, size_t npat,
                  int mode);

constexpr size_t kDataShreds = AG_RS_DATA_SHREDS;
constexpr size_t kTotalShreds = AG_RS_TOTAL_SHREDS;
constexpr size_t kMaxAfterPadding = kDataShreds * AG_RS_MAX_DATA_PER_SHRED;
constexpr size_t kMaxPayload = kMaxAfterPadding - 1;
constexpr size_t kMaxSigBatch = size_t{1} << 31;  // shreds / slices per signature, validation or wire call

// rs_api.cpp: what the coder handle (rs_coder_api.cpp) calls
int run_one_decode(ag_rs_ctx* c, size_t k, size_t m, size_t S, PinBuf& pin, const uint8_t* opres,
                   const uint8_t* rpres, int mode, bool coding, const uint8_t** coding_src);

// rs_coder_api.cpp: what the composed shredders (shredder_api.cpp) and the per-call server call
ag::XformParams codeword_xform(uint8_t* cw, size_t cw_stride, size_t S, size_t n, size_t cps);
ag::DecodeXParams codeword_decode_x(uint8_t* cw, size_t cw_stride, size_t S, size_t n, size_t cps);
int pipe_coder_deshred(ag_rs_ctx* c, size_t n, size_t S, uint8_t* cw, size_t cw_stride, const uint64_t* d_present,
                       int64_t* plen, size_t m, bool no_surplus = false);
int pipe_coder_deshred_var(ag_rs_ctx* c, size_t n, uint8_t* cw, size_t cw_stride, const uint64_t* d_present,
                           const uint32_t* d_sizes, const uint32_t* d_col_base, uint32_t total_columns,
                           bool reencode, int64_t* plen, bool exact = false);
int upload_var_sizes(ag_rs_ctx* c, size_t n, const uint32_t* S, const uint32_t** d_sizes, const uint32_t** d_col_base,
                     uint32_t* total_columns);
bool pipe_tail_ok(size_t S, size_t m, bool no_reencode = false);

// crypto_api.cpp: what the composed shredders and the intake call
int ensure_empty_roots(ag_rs_ctx* c);
int ensure_ed_base(ag_rs_ctx* c);
int merkle_var_launch(ag_rs_ctx* c, size_t nslices, const uint32_t* d_sizes, const uint8_t* leaves,
                      size_t slice_stride, uint8_t* roots, uint8_t* nodes, size_t nodes_stride, uint8_t* proofs,
                      size_t proofs_stride);
int aon_batch(ag_rs_ctx* c, size_t n, uint8_t* buffers, size_t stride, const uint32_t* lens, uint32_t extra,
              ag::BufferBatch* bb);
int shred_validate_impl(ag_rs_ctx* c, const ag::MerkleVerifyParams& merkle, const uint64_t* slots,
                        const uint64_t* slice_indices, const uint8_t* is_last, const uint8_t* sigs, size_t sig_stride,
                        const uint8_t* pk, const uint8_t* cached, const uint8_t* has_cached, uint32_t cached_group,
                        uint8_t* status, uint8_t* roots_out, uint8_t* commitments_out, bool roots_ready);
int slice_sign_prepare(ag_rs_ctx* c, size_t nslices, const uint8_t* seed, const uint8_t* pk, const uint64_t* slots,
                       const uint64_t* slice_indices, const uint8_t* is_last, const uint8_t* roots,
                       const uint8_t* sigs, const uint8_t* commitments_out);
int slice_sign_enqueue(ag_rs_ctx* c, size_t nslices, const uint8_t* seed, const uint8_t* pk, const uint64_t* slots,
                       const uint64_t* slice_indices, const uint8_t* is_last, const uint8_t* roots, uint8_t* sigs,
                       uint8_t* commitments_out, hipStream_t stream);

}  // namespace host
}  // namespace ag
