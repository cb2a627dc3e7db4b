// The C ABI of the ReedSolomonCoder mirror (include/alpenglow_rs.h): the per-call coder handle,
// the batched shred / deshred over device codewords of one shred size (ag_rs_coder_*_batch) and
// of mixed sizes (*_batch_var), and the device stages of the deshred that the composed shredders
// (shredder_api.cpp) chain.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <new>
#include <vector>

#include "../../include/alpenglow_rs.h"
#include "rs_ctx.hpp"
#include "rs_launch.hpp"
#include "rs_patterns.hpp"
#include "shredder.hpp"

using namespace ag::host;
using ag::count_flags;
using ag::pack_flags;
using ag::pack_present_words;

// =====================================================================================
// ReedSolomonCoder mirror (reed_solomon.rs:47-232)
// =====================================================================================
struct ag_rs_coder {
  OwnedCtx owned;  // ag_rs_coder_new_on_device: shared by its encoder and decoder, destroyed after them
  ag_rs_ctx* ctx = nullptr;
  size_t num_coding = 0;
  ag_rs_encoder* enc = nullptr;
  ag_rs_decoder* dec = nullptr;
  ~ag_rs_coder() {
    ag_rs_encoder_free(enc);
    ag_rs_decoder_free(dec);
  }
};

namespace {
// encode_coding_from_data (reed_solomon.rs:211-231) of the 32 data shards already staged in
// the encoder's originals (S bytes each): the coding shards land in c->enc->rec()
// (the caller reset the encoder to (32, num_coding, S) before staging them)
int coder_encode_staged(ag_rs_coder* c) {
  c->enc->received = kDataShreds;
  c->enc->encoded = false;
  return ag_rs_encoder_encode(c->enc);
}

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
      ag::XformParams p = codeword_xform(cw + b * cw_stride, cw_stride, S, e - b, S / 64);
      p.out += static_cast<size_t>(lone) * 32 * S;
      p.out_mask = c->d_reenc_mask.as<uint64_t>();
      p.n_in = static_cast<uint32_t>(kDataShreds);
      p.n_out = 32;
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
  ag::DecodeXParams p = codeword_decode_x(cw, cw_stride, S, n, cps);
  p.rows = rows;
  p.rows_w = 128;
  p.k = static_cast<uint32_t>(k);
  p.m = 32;  // recovery shards per window half (the kernel addresses the rest from p.rec)
  p.chunk = 32;
  p.low_rate = 1;
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
    ag::XformParams xp = codeword_xform(cw, cw_stride, S, n, cps);
    xp.out += 32 * j * S;
    xp.out_mask = mask;  // the slice's absent coding shreds, all, or none
    xp.pattern_per_block = 1;
    xp.n_in = static_cast<uint32_t>(k);
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
  if (ag::launch_pipe_patterns(d_present, n, xm, few, true, c->stream) != hipSuccess ||
      ag::launch_decode_rows(xm, xm + n, static_cast<uint32_t>(n), static_cast<uint32_t>(W), c->dtables(), rows, true,
                             c->stream) != hipSuccess)
    return AG_RS_ERR_DEVICE;
  ag::DecodeXParams p = codeword_decode_x(cw, cw_stride, S, n, cps);
  p.pmask = xm + n;
  p.rows = rows;
  p.k = static_cast<uint32_t>(k);
  p.m = 32;
  p.chunk = 32;
  p.low_rate = 0;
  p.per_lane = 1;
  p.rows_w = static_cast<uint32_t>(W);
  p.any_k = 1;  // launch_pipe_patterns keeps exactly k survivors
  p.fuse = 1;
  p.tail_bytes = tail;
  if (ag::launch_decode_x(static_cast<unsigned>(W), 0, p, (p.total_columns + 63) / 64, c->stream,
                          &c->last_window_kernels) != hipSuccess)
    return AG_RS_ERR_DEVICE;
  if (ag::launch_coder_strip(cw, cw_stride, static_cast<uint32_t>(k * S), n, strip, c->stream) != hipSuccess ||
      ag::launch_pipe_store_masks(few, strip, d_present, 1, n, mask, -AG_RS_ERR_NOT_ENOUGH_SHARDS,
                                  -AG_RS_ERR_INVALID_PADDING, c->stream) != hipSuccess)
    return AG_RS_ERR_DEVICE;
  // fused, no slice with surplus shreds and none with every data shred: every store mask is
  // zero (exactly 32 kept: restored by the decode; fewer, or a failed strip: untouched)
  if (no_surplus) return AG_RS_OK;
  ag::XformParams xp = codeword_xform(cw, cw_stride, S, n, cps);
  xp.out_mask = mask;
  xp.pattern_per_block = 1;
  xp.n_in = static_cast<uint32_t>(k);
  xp.n_out = 32;
  xp.skip_idle = 1;  // tiles of fused slices only: nothing to re-encode
  xp.tail_bytes = tail;
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

// ---- mixed shred sizes (ag_rs_coder_*_batch_var; kernels in rs_var.hip) -------------------
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

namespace ag::host {
// The codeword layout of the coder batches in the transform / window-decode parameters: block b
// at cw + b * cw_stride, its 32 data shreds of S bytes first, the coding shreds behind them; n
// blocks of cps columns.  Everything else stays value-initialised for the caller to set.
ag::XformParams codeword_xform(uint8_t* cw, size_t cw_stride, size_t S, size_t n, size_t cps) {
  ag::XformParams p{};
  p.in = cw;
  p.in_block_stride = cw_stride;
  p.in_shard_stride = S;
  p.out = cw + kDataShreds * S;
  p.out_block_stride = cw_stride;
  p.out_shard_stride = S;
  p.chunks_per_shard = static_cast<uint32_t>(cps);
  p.total_columns = static_cast<uint64_t>(n) * cps;
  return p;
}
ag::DecodeXParams codeword_decode_x(uint8_t* cw, size_t cw_stride, size_t S, size_t n, size_t cps) {
  ag::DecodeXParams p{};
  p.rec = cw + kDataShreds * S;
  p.rec_block_stride = cw_stride;
  p.rec_shard_stride = S;
  p.orig = cw;
  p.orig_block_stride = cw_stride;
  p.orig_shard_stride = S;
  p.chunks_per_shard = static_cast<uint32_t>(cps);
  p.total_columns = static_cast<uint64_t>(n) * cps;
  return p;
}

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

// sizes | column prefix of a batch of mixed shred sizes (checked by the caller: each even, 2 ..
// 1024) onto the device through the staging of ag_rs_coder_shred_batch_var's table (the
// context's `lens`): for the composed var deshred, whose
// kernels read the sizes from the first stage on, before any present words exist.  Valid on
// the stream until the next coder shred call on the context.
int upload_var_sizes(ag_rs_ctx* c, size_t n, const uint32_t* S, const uint32_t** d_sizes, const uint32_t** d_col_base,
                     uint32_t* total_columns) {
  if (n > kVarMaxSlices) return AG_RS_ERR_INVALID_ARGUMENT;
  const size_t words = 2 * n + 1;
  int st;
  uint32_t* h;
  if ((st = c->lens.host(words * 4, &h))) return st;
  var_column_table(S, n, h, h + n);
  if ((st = c->lens.send(words * 4, c->stream))) return st;
  *d_sizes = c->lens.dev.as<uint32_t>();
  *d_col_base = *d_sizes + n;
  *total_columns = h[2 * n];
  return AG_RS_OK;
}
}  // namespace ag::host

extern "C" {

// Diagnostic (not in the header): the in-kernel duration of the last per-call server job on the
// coder's context, doorbell seen -> its stores released, then its four phases (kind read,
// parameters + cache invalidate, tile, release): ns[5], 0 before any job.
int ag_rs_internal_coder_last_job_ns(ag_rs_coder* coder, uint64_t* ns) {
  if (!coder || !coder->ctx || !ns) return AG_RS_ERR_INVALID_ARGUMENT;
  const ag::LatencyMailbox* mb = coder->ctx->mb;
  ns[0] = mb ? __atomic_load_n(&mb->job_ticks, __ATOMIC_ACQUIRE) * 10 : 0;  // 100 MHz wall clock
  for (int i = 0; i < 4; ++i) ns[1 + i] = mb ? uint64_t{__atomic_load_n(&mb->phase_ticks[i], __ATOMIC_ACQUIRE)} * 10 : 0;
  return AG_RS_OK;
}

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
  (*out)->owned.reset(c);
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
  // call's pad kernel, which may still read lens.dev) -- no stream synchronisation before the
  // call's work is enqueued
  uint32_t* h;
  if ((st = c->lens.host(n * 4, &h))) return st;
  std::memcpy(h, lens, n * 4);
  if ((st = c->lens.send(n * 4, c->stream))) return st;
  if (ag::launch_coder_pad(payloads, payload_stride, c->lens.dev.as<uint32_t>(), cw, cw_stride,
                           static_cast<uint32_t>(kDataShreds * S), n, c->stream) != hipSuccess)
    return AG_RS_ERR_DEVICE;
  return encode_device(c, kDataShreds, m, S, n, cw, cw_stride, cw + kDataShreds * S, cw_stride);
}

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
    uint64_t* pres;
    if ((st = c->present.host(wps * n * 8, &pres))) return st;
    // (uniform batches returned above)
    // ANY_K always takes the device path; EXACT when no slice keeps more than 32 shreds (both
    // decoders agree then).  (Packing a first ~1/8 range and the rest behind its decode
    // measured even with one whole-batch range, profiles/r05_ab_coder_ranges.jsonl.)
    bool full_data = false;
    const bool surplus = pack_present_words(dpres, cpres, m, n, pres, &full_data);
    if ((mode == AG_RS_DECODE_ANY_K || !surplus) && pipe_tail_ok(S, m, !surplus && !full_data)) {
      if ((st = c->present.send(wps * n * 8, c->stream))) return st;
      // no surplus and no slice with every data shred: no store mask of the re-encode is set
      return pipe_coder_deshred(c, n, S, cw, cw_stride, c->present.dev.as<uint64_t>(), out, m,
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
  // lens | sizes | col_base through the lengths' staging (ag_rs_coder_shred_batch's)
  const size_t words = 3 * n + 1;
  uint32_t* h;
  if ((st = c->lens.host(words * 4, &h))) return st;
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
  if ((st = c->lens.send(words * 4, c->stream))) return st;
  const uint32_t* d = c->lens.dev.as<uint32_t>();
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
  const size_t bytes = 8 * n + 4 * (2 * n + 1);
  uint64_t* pres;
  if ((st = c->present.host(bytes, &pres))) return st;
  bool full_data = false;
  const bool surplus = pack_present_words(dpres, cpres, m, n, pres, &full_data);
  // EXACT with surplus shreds: the crate's decoder reads every kept shred (the uniform call's host path)
  if (mode != AG_RS_DECODE_ANY_K && surplus) return fallback();
  uint32_t* h = reinterpret_cast<uint32_t*>(pres + n);
  var_column_table(S, n, h, h + n);
  if ((st = c->present.send(bytes, c->stream))) return st;
  const uint64_t* d_present = c->present.dev.as<uint64_t>();
  const uint32_t* d = reinterpret_cast<const uint32_t*>(d_present + n);
  // no surplus and no slice with every data shred: every store mask is zero (pipe_coder_enqueue)
  return pipe_coder_deshred_var(c, n, cw, cw_stride, d_present, d, d + n, h[2 * n], surplus || full_data, out);
}

}  // extern "C"
