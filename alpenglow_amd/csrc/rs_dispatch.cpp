// The batch encode / decode over device memory behind the C ABI (rs_api.cpp and rs_coder_api.cpp
// call encode_device / decode_device): which kernel serves a geometry and a shard size, the
// restride of sizes that are not whole 64-byte chunks, and one launcher per decoder class
// (rs_patterns.cpp's classify_patterns decides the class of every erasure pattern; this file
// uploads what the class's kernel reads and launches it).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <vector>

#include "gf16.hpp"
#include "rs_ctx.hpp"
#include "rs_launch.hpp"
#include "rs_patterns.hpp"
#include "shredder.hpp"

namespace ag {
namespace host {

int check_geometry(size_t k, size_t m, size_t S) {
  if (use_high_rate(k, m) < 0) return AG_RS_ERR_UNSUPPORTED_SHARD_COUNT;
  if (S == 0 || S % 2) return AG_RS_ERR_INVALID_SHARD_SIZE;
  if (S > 0xFFFFFFFEull) return AG_RS_ERR_INVALID_ARGUMENT;
  return AG_RS_OK;
}

// Byte-odd buffers or strides: every shard goes through the restride (its byte path)
bool odd_layout(const void* a, const void* b, size_t sa, size_t sb) {
  return ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b) | sa | sb) & 1) != 0;
}

namespace {

// Scratch budget of the generic kernels (per launch).
constexpr size_t kGenericScratchBytes = size_t{512} << 20;

// Restrided shard buffer (shard sizes that are not whole 64-byte chunks), per group.
constexpr size_t kRestrideGroupBytes = size_t{2048} << 20;

// Origin, recovery and strides of the parameter structs that name them orig / rec: block b's
// shards at orig + b * ostride and rec + b * rstride, sstride bytes apart.
template <typename P, typename O, typename R>
P shard_params(O* orig, size_t ostride, R* rec, size_t rstride, size_t sstride) {
  P p{};
  p.orig = orig;
  p.orig_block_stride = ostride;
  p.orig_shard_stride = sstride;
  p.rec = rec;
  p.rec_block_stride = rstride;
  p.rec_shard_stride = sstride;
  return p;
}

// The same for the transforms: n_in shards in, n_out out, cps 64-byte chunks per shard.
XformParams xform_params(const uint8_t* in, size_t in_stride, size_t n_in, uint8_t* out, size_t out_stride,
                         size_t n_out, size_t sstride, size_t cps, size_t nblocks) {
  XformParams p{};
  p.in = in;
  p.in_block_stride = in_stride;
  p.in_shard_stride = sstride;
  p.out = out;
  p.out_block_stride = out_stride;
  p.out_shard_stride = sstride;
  p.n_in = static_cast<uint32_t>(n_in);
  p.n_out = static_cast<uint32_t>(n_out);
  p.chunks_per_shard = static_cast<uint32_t>(cps);
  p.total_columns = static_cast<uint64_t>(nblocks) * cps;
  return p;
}

// Shard sizes that are not whole 64-byte chunks (a slice's tail, reed_solomon.rs:94-95):
// the whole chunks of every shard run in place on the bitsliced kernels (shard stride S,
// chunks_per_shard = S / 64: the kernels take any alignment), and only the T = S mod 64 tail
// bytes of each shard -- in the crate's tail layout exactly a T-byte shard --
// are restrided into a padded 64-byte chunk per shard (restride_kernel), run there and
// restrided back.  Taken when the padded geometry has a bitsliced path.
//
// Virtual shards of Sv bytes at byte `off` of every shard (shard stride sstride) are packed
// into padded shards, encoded there, and the recovery shards' pieces unpacked.
int encode_restrided(ag_rs_ctx* c, size_t k, size_t m, size_t Sv, size_t sstride, size_t off, size_t nblocks,
                     const uint8_t* orig, size_t ostride, uint8_t* rec, size_t rstride) {
  const size_t Sp = padded_shard(Sv), per_block = (k + m) * Sp;
  const size_t group = std::max<size_t>(1, kRestrideGroupBytes / per_block);
  int st = c->stage_pad.ensure(std::min(group, nblocks) * per_block, c->stream);
  if (st) return st;
  c->last_encode_kernels |= kEkRestride;
  uint8_t* pad = c->stage_pad.as<uint8_t>();
  for (size_t b0 = 0; b0 < nblocks; b0 += group) {
    const size_t nb = std::min(group, nblocks - b0);
    if (launch_restride(orig + b0 * ostride + off, ostride, sstride, pad, per_block, Sp, static_cast<uint32_t>(Sv),
                        static_cast<uint32_t>(k), nb, false, nullptr, false, c->stream) != hipSuccess)
      return AG_RS_ERR_DEVICE;
    if ((st = encode_device(c, k, m, Sp, nb, pad, per_block, pad + k * Sp, per_block))) return st;
    if (launch_restride(pad + k * Sp, per_block, Sp, rec + b0 * rstride + off, rstride, sstride,
                        static_cast<uint32_t>(Sv), static_cast<uint32_t>(m), nb, true, nullptr, false,
                        c->stream) != hipSuccess)
      return AG_RS_ERR_DEVICE;
  }
  return AG_RS_OK;
}

// The encode over the first S bytes of every shard (S % 64 == 0 on the bitsliced paths;
// shards sstride >= S bytes apart).
int encode_cols(ag_rs_ctx* c, size_t k, size_t m, size_t S, size_t sstride, size_t nblocks, const uint8_t* orig,
                size_t ostride, uint8_t* rec, size_t rstride) {
  const unsigned npts = xform_points(k, m, S);
  const unsigned mc = mc_chunk(k, m, S);
  const unsigned lr = lowrate_chunk(k, m, S);
  if (npts || mc || lr) {
    const XformParams p = xform_params(orig, ostride, k, rec, rstride, m, sstride, S / 64, nblocks);
    hipError_t e = hipSuccess;
    if (npts) {
      c->last_encode_kernels |= npts == 32 ? encode32_kernel(p) : kEkXformH8;
      e = launch_xform(npts == 32 ? XformKind::kEncode32 : XformKind::kEncode64, p, c->stream);
    } else if (mc) {
      c->last_encode_kernels |= kEkEncodeMc;
      e = launch_encode_mc(mc, p, c->stream);
    } else {
      for (size_t j = 0; j * lr < m && e == hipSuccess;) {  // one launch per recovery chunk
        XformParams pj = p;
        pj.out = rec + j * lr * sstride;
        if (lr == 32 && j % 2 == 0 && (j + 1) * lr < m && j < 4) {  // chunks j, j + 1 in one launch
          pj.n_out = static_cast<uint32_t>(std::min<size_t>(2 * lr, m - j * lr));
          c->last_encode_kernels |= kEkLowRate2;
          e = launch_xform_lowrate2(static_cast<unsigned>(j / 2), pj, c->stream);
          j += 2;
          continue;
        }
        pj.n_out = static_cast<uint32_t>(std::min<size_t>(lr, m - j * lr));
        c->last_encode_kernels |= kEkLowRate;
        e = launch_xform_lowrate(lr, static_cast<unsigned>(j), pj, c->stream);
        ++j;
      }
    }
    return e == hipSuccess ? AG_RS_OK : AG_RS_ERR_DEVICE;
  }
  int st = c->ensure_tables();
  if (st) return st;
  const int hr = use_high_rate(k, m);
  const size_t chunk = hr ? next_pow2(m) : next_pow2(k);
  const size_t cover = hr ? k : m;
  const size_t rows = std::max(chunk, (cover + chunk - 1) / chunk * chunk);
  const size_t nsym = S / 2;
  const size_t per_block = rows * nsym * 2;
  const size_t per_launch = std::max<size_t>(1, kGenericScratchBytes / per_block);
  if ((st = c->scratch.ensure(std::min(per_launch, nblocks) * per_block, c->stream))) return st;
  for (size_t b0 = 0; b0 < nblocks; b0 += per_launch) {
    auto p = shard_params<GenericEncodeParams>(orig + b0 * ostride, ostride, rec + b0 * rstride, rstride, sstride);
    p.k = static_cast<uint32_t>(k);
    p.m = static_cast<uint32_t>(m);
    p.high_rate = static_cast<uint32_t>(hr);
    p.chunk = static_cast<uint32_t>(chunk);
    p.rows = static_cast<uint32_t>(rows);
    p.shard_bytes = static_cast<uint32_t>(S);
    p.nsym = static_cast<uint32_t>(nsym);
    p.nblocks = std::min(per_launch, nblocks - b0);
    p.scratch = c->scratch.as<uint16_t>();
    p.t = c->dtables();
    c->last_encode_kernels |= kEkGeneric;
    if (launch_generic_encode(p, c->stream) != hipSuccess) return AG_RS_ERR_DEVICE;
  }
  return AG_RS_OK;
}

// A 32-point transform over shards of S bytes that end in a split tail chunk (S % 64 != 0, S
// even), one launch on the caller's buffers (no restride): chunks_per_shard = ceil(S / 64), the
// last chunk of every shard read and written as 16-byte windows of its tail (rs_xform.hpp
// tile_io_g).  (Two launches -- the whole chunks with the tails skipped, then the tails alone
// -- measured slower: 3.76 / 4.06 TB/s at S = 1000 against 3.8-4.0 / 4.2-4.4; the whole-chunk
// pass alone ran at 4.35 TB/s, its shards' last 64-byte sectors left partial for the second
// pass to complete, profiles/r05_tail_split_kernel_stats.csv.)
XformParams tail_params(const uint8_t* in, size_t in_stride, size_t n_in, uint8_t* out, size_t out_stride,
                        size_t n_out, size_t S, size_t nblocks) {
  XformParams p = xform_params(in, in_stride, n_in, out, out_stride, n_out, S, padded_shard(S) / 64, nblocks);
  p.tail_bytes = static_cast<uint32_t>(S % 64);
  return p;
}

int encode_tail32(ag_rs_ctx* c, size_t k, size_t m, size_t S, size_t nblocks, const uint8_t* orig, size_t ostride,
                  uint8_t* rec, size_t rstride) {
  const XformParams p = tail_params(orig, ostride, k, rec, rstride, m, S, nblocks);
  c->last_encode_kernels |= encode32_kernel(p);
  return launch_xform(XformKind::kEncode32, p, c->stream) == hipSuccess ? AG_RS_OK : AG_RS_ERR_DEVICE;
}

}  // namespace

int encode_device(ag_rs_ctx* c, size_t k, size_t m, size_t S, size_t nblocks, const uint8_t* orig, size_t ostride,
                  uint8_t* rec, size_t rstride) {
  if (nblocks == 0) return AG_RS_OK;
  const size_t Sp = padded_shard(S);
  if (S % 2 == 0 && (xform_points(k, m, Sp) || mc_chunk(k, m, Sp) || lowrate_chunk(k, m, Sp))) {
    if (odd_layout(orig, rec, ostride, rstride))
      return encode_restrided(c, k, m, S, S, 0, nblocks, orig, ostride, rec, rstride);
    const size_t full = S / 64 * 64, tail = S - full;
    if (tail >= 16 && xform_points(k, m, Sp) == 32)  // (tail windows are 16 bytes of the tail itself)
      return encode_tail32(c, k, m, S, nblocks, orig, ostride, rec, rstride);
    int st;
    if (full && (st = encode_cols(c, k, m, full, S, nblocks, orig, ostride, rec, rstride))) return st;
    if (tail && (st = encode_restrided(c, k, m, tail, S, full, nblocks, orig, ostride, rec, rstride))) return st;
    return AG_RS_OK;
  }
  return encode_cols(c, k, m, S, S, nblocks, orig, ostride, rec, rstride);
}

namespace {

// One decode over the first S bytes of every shard (shards sstride >= S bytes apart).
struct DecodeCall {
  ag_rs_ctx* c;
  size_t k, m, S, sstride, nblocks;
  uint8_t* orig;
  size_t ostride;
  const uint8_t* rec;
  size_t rstride;
  const uint8_t *opres, *rpres;
  int mode;
};

uint64_t low_bits(size_t n) { return n >= 64 ? ~uint64_t{0} : (uint64_t{1} << n) - 1; }

// The decode counterpart of encode_restrided: originals and recovery shards of a group of
// blocks go to one padded buffer, the bitsliced decoders run there, and only the restored
// originals are restrided back (a store mask per pattern).
int decode_restrided(ag_rs_ctx* c, size_t k, size_t m, size_t Sv, size_t sstride, size_t off, size_t nblocks,
                     uint8_t* orig, size_t ostride, const uint8_t* rec, size_t rstride, const uint8_t* opres,
                     const uint8_t* rpres, size_t npat, int mode) {
  const size_t Sp = padded_shard(Sv), per_block = (k + m) * Sp;
  // store masks: the absent originals of each pattern (k <= 64 on every bitsliced path)
  // and the pack masks: only present shards are packed (decoders never read absent ones)
  std::vector<uint64_t> mask(3 * npat);
  const uint64_t kmask = low_bits(k);
  const bool rmask = m <= 64;
  if (k == 32 && m == 32) {  // the flags packed 32 at a time (AVX2 where the host has it)
    std::vector<uint64_t> w(npat);
    bool full_data = false;
    (void)pack_present_words(opres, rpres, m, npat, w.data(), &full_data);
    for (size_t p = 0; p < npat; ++p) {
      if (__builtin_popcountll(w[p]) < 32) return AG_RS_ERR_NOT_ENOUGH_SHARDS;  // nothing launched yet
      mask[p] = ~w[p] & kmask;
      mask[npat + p] = w[p] & kmask;
      mask[2 * npat + p] = w[p] >> 32;
    }
  } else {
    for (size_t p = 0; p < npat; ++p)  // NotEnoughShards before anything is launched
      if (count_flags(opres + p * k, k) + count_flags(rpres + p * m, m) < k) return AG_RS_ERR_NOT_ENOUGH_SHARDS;
    for (size_t p = 0; p < npat; ++p) {
      mask[p] = ~pack_flags(opres + p * k, k) & kmask;
      mask[npat + p] = pack_flags(opres + p * k, k);
      mask[2 * npat + p] = rmask ? pack_flags(rpres + p * m, m) : 0;
    }
  }
  int st;
  if ((st = c->stage_mask.put(std::move(mask), c->stream))) return st;
  const uint64_t* d_store = c->stage_mask.dev.as<uint64_t>();
  const uint64_t* d_omask = d_store + npat;
  const uint64_t* d_rmask = rmask ? d_store + 2 * npat : nullptr;
  const size_t group = std::max<size_t>(1, kRestrideGroupBytes / per_block);
  if ((st = c->stage_pad.ensure(std::min(group, nblocks) * per_block, c->stream))) return st;
  uint8_t* pad = c->stage_pad.as<uint8_t>();
  for (size_t b0 = 0; b0 < nblocks; b0 += group) {
    const size_t nb = std::min(group, nblocks - b0);
    const size_t p0 = npat > 1 ? b0 : 0, np = npat > 1 ? nb : 1;
    if (launch_restride(orig + b0 * ostride + off, ostride, sstride, pad, per_block, Sp, static_cast<uint32_t>(Sv),
                        static_cast<uint32_t>(k), nb, false, d_omask + p0, npat > 1, c->stream) != hipSuccess ||
        launch_restride(rec + b0 * rstride + off, rstride, sstride, pad + k * Sp, per_block, Sp,
                        static_cast<uint32_t>(Sv), static_cast<uint32_t>(m), nb, false,
                        d_rmask ? d_rmask + p0 : nullptr, npat > 1, c->stream) != hipSuccess)
      return AG_RS_ERR_DEVICE;
    if ((st = decode_device(c, k, m, Sp, nb, pad, per_block, pad + k * Sp, per_block, opres + p0 * k, rpres + p0 * m,
                            np, mode)))
      return st;
    if (launch_restride(pad, per_block, Sp, orig + b0 * ostride + off, ostride, sstride, static_cast<uint32_t>(Sv),
                        static_cast<uint32_t>(k), nb, true, d_store + p0, npat > 1, c->stream) != hipSuccess)
      return AG_RS_ERR_DEVICE;
  }
  return AG_RS_OK;
}

// The 32-point full-recovery reconstruct (decode class "transform") of shards ending in a split
// tail chunk: xform8's TAIL variant restores the erased originals, tail included, in place.
// It shares the store-mask cache with run_transform and run_lowrate_chunk.
int decode_tail32(const DecodeCall& d, size_t npat) {
  ag_rs_ctx* c = d.c;
  if (npat > 1) {
    bool same = true;
    for (size_t p = 1; p < npat && same; ++p) same = std::memcmp(d.opres, d.opres + p * d.k, d.k) == 0;
    if (same) npat = 1;
  }
  std::vector<uint64_t> mask(npat);
  bool any = false, low_half = true;
  for (size_t p = 0; p < npat; ++p) {
    mask[p] = ~pack_flags(d.opres + p * d.k, d.k) & low_bits(d.k);
    ++c->last_classes[mask[p] ? kTransform : kNone];
    any = any || mask[p];
    low_half = low_half && (mask[p] >> 16) == 0;
  }
  if (!any) return AG_RS_OK;
  const int st = c->mask.put(std::move(mask), c->stream);
  if (st) return st;
  XformParams p = tail_params(d.rec, d.rstride, d.m, d.orig, d.ostride, d.k, d.S, d.nblocks);
  p.out_mask = c->mask.dev.as<uint64_t>();
  p.pattern_per_block = npat > 1 ? 1u : 0u;
  p.out_low_half = low_half;
  return launch_xform(XformKind::kDecode32, p, c->stream) == hipSuccess ? AG_RS_OK : AG_RS_ERR_DEVICE;
}

// Origin, recovery, strides and the columns of a bitsliced decoder's launch.
template <typename P>
P decode_params(const DecodeCall& d, size_t cps) {
  P p = shard_params<P>(d.orig, d.ostride, d.rec, d.rstride, d.sstride);
  p.k = static_cast<uint32_t>(d.k);
  p.chunks_per_shard = static_cast<uint32_t>(cps);
  p.total_columns = static_cast<uint64_t>(d.nblocks) * cps;
  return p;
}

constexpr int kNotApplicable = -1;

// Per-block patterns of the 32:32 code on tiles that straddle blocks (chunks per shard not a
// multiple of 64: the follower's slices, tail shreds' whole chunks and their restrided tails),
// ANY_K, where some recovery shards are lost: the per-lane window decode with its masks built
// on the device (launch_pipe_patterns, the coder batches' kernel), so the host only packs the
// presence flags (AVX2) -- the per-pattern classification, window masks and mask compares cost
// ~25 ns per pattern and call on the host, 3-7 ms per 131 072-block call
// (profiles/r06_kt_tail_lose4_kernel_stats.csv against the call's wall time).  kNotApplicable
// when some pattern has its full recovery set and lost data (the transform decodes those) --
// the host route (decode_cols) takes the call then.
// d.S = 64 C, or 64 C + T with a tail of T >= 16 bytes as the last column (decode_h8 TAIL).
int decode_cols_device_patterns(const DecodeCall& d) {
  constexpr size_t k = 32, m = 32, W = 64;
  ag_rs_ctx* c = d.c;
  const size_t n = d.nblocks;
  int st;
  uint64_t* pres;
  if ((st = c->present.host(n * 8, &pres))) return st;
  bool full_data = false;
  (void)pack_present_words(d.opres, d.rpres, m, n, pres, &full_data);
  size_t restore = 0;
  for (size_t b = 0; b < n; ++b) {
    const uint64_t w = pres[b];
    if (__builtin_popcountll(w) < static_cast<int>(k)) return AG_RS_ERR_NOT_ENOUGH_SHARDS;  // nothing launched
    const bool data_full = (w & 0xFFFFFFFFull) == 0xFFFFFFFFull;
    if (!data_full && (w >> 32) == 0xFFFFFFFFull) return kNotApplicable;
    restore += data_full ? 0 : 1;
  }
  c->last_classes[kNone] += n - restore;
  c->last_classes[kWindow64] += restore;
  if (!restore) return AG_RS_OK;
  if ((st = c->ensure_tables()) || (st = c->present.dev.ensure(n * 8, c->stream)) ||
      (st = c->d_pipe_few.ensure(n, c->stream)) || (st = c->xmask.dev.ensure(3 * n * 8, c->stream)) ||
      (st = c->d_rows.ensure(n * W * 4, c->stream)))
    return st;
  c->xmask.key.clear();  // xmask.dev / d_rows no longer hold run_window64's cached patterns
  c->xmask_w = 0;
  if ((st = c->present.send(n * 8, c->stream))) return st;  // (the device buffer grown above: the old order)
  uint64_t* xm = c->xmask.dev.as<uint64_t>();
  uint32_t* rows = c->d_rows.as<uint32_t>();
  if (launch_pipe_patterns(c->present.dev.as<uint64_t>(), n, xm, c->d_pipe_few.as<uint8_t>(), false, c->stream) !=
          hipSuccess ||
      launch_decode_rows(xm, xm + n, static_cast<uint32_t>(n), static_cast<uint32_t>(W), c->dtables(), rows, true,
                         c->stream) != hipSuccess)
    return AG_RS_ERR_DEVICE;
  auto p = decode_params<DecodeXParams>(d, padded_shard(d.S) / 64);
  p.pmask = xm + n;
  p.rows = rows;
  p.m = static_cast<uint32_t>(m);
  p.chunk = 32;
  p.low_rate = 0;
  p.per_lane = 1;
  p.rows_w = static_cast<uint32_t>(W);
  p.any_k = 1;  // launch_pipe_patterns keeps exactly k survivors
  p.tail_bytes = static_cast<uint32_t>(d.S % 64);
  if (launch_decode_x(static_cast<unsigned>(W), 0, p, (p.total_columns + 63) / 64, c->stream) != hipSuccess)
    return AG_RS_ERR_DEVICE;
  return AG_RS_OK;
}

// ---- the steps the class launchers share ----

// Store-mask word per pattern: restore original i iff the pattern has class cl (and, for
// kLowRateChunk, restores from recovery chunk `chunk`) and i is absent.
std::vector<uint64_t> store_masks(const DecodeCall& d, const DecodePlan& pl, DecodeClass cl, int chunk = -1) {
  std::vector<uint64_t> mask(pl.npat, 0);
  const uint64_t kmask = low_bits(d.k);  // k <= 64 on the transform paths
  for (size_t p = 0; p < pl.npat; ++p)
    if (pl.cls[p] == cl && (chunk < 0 || pl.lr_chunk[p] == chunk)) mask[p] = ~pack_flags(d.opres + p * d.k, d.k) & kmask;
  return mask;
}

// Cache key of the pattern tables built from the flags: (k, m), then the present flags of the
// patterns of class cl (the other patterns' tables are zero, and so is their part of the key).
std::vector<uint8_t> flags_key(const DecodeCall& d, const DecodePlan& pl, DecodeClass cl) {
  const size_t k = d.k, m = d.m;
  std::vector<uint8_t> key(16 + pl.npat * (k + m));
  const uint64_t km[2] = {k, m};
  std::memcpy(key.data(), km, 16);
  for (size_t p = 0; p < pl.npat; ++p) {
    if (pl.cls[p] != cl) continue;
    std::memcpy(&key[16 + p * (k + m)], d.opres + p * k, k);
    std::memcpy(&key[16 + p * (k + m) + k], d.rpres + p * m, m);
  }
  return key;
}

std::vector<uint32_t> class_blocks(const DecodePlan& pl, DecodeClass cl, size_t nblocks) {
  std::vector<uint32_t> ids;
  for (size_t b = 0; b < nblocks; ++b)
    if (pl.cls[b] == cl) ids.push_back(static_cast<uint32_t>(b));
  return ids;
}

// Block selection of a per_block launch: the ids of the blocks of class cl, uploaded to `buf`
// unless they are all the blocks (*block_ids stays null: blocks 0..).  With `owned`, a vector
// of the context, the ids move there and the copy is asynchronous; else it is synchronous.
int select_blocks(const DecodeCall& d, const DecodePlan& pl, DecodeClass cl, DevBuf& buf, std::vector<uint32_t>* owned,
                  const uint32_t** block_ids, size_t* count) {
  ag_rs_ctx* c = d.c;
  std::vector<uint32_t> ids = class_blocks(pl, cl, d.nblocks);
  *count = ids.size();
  if (ids.size() == d.nblocks) return AG_RS_OK;
  AG_HIP(hipStreamSynchronize(c->stream));  // a previous id upload may be pending (and read *owned)
  const int st = buf.ensure(ids.size() * 4, c->stream);
  if (st) return st;
  if (owned) {
    *owned = std::move(ids);
    AG_HIP(hipMemcpyAsync(buf.ptr, owned->data(), owned->size() * 4, hipMemcpyHostToDevice, c->stream));
  } else {
    AG_HIP(hipMemcpy(buf.ptr, ids.data(), ids.size() * 4, hipMemcpyHostToDevice));
  }
  *block_ids = buf.as<uint32_t>();
  return AG_RS_OK;
}

// Tiling of a bitsliced decoder's launch over 64-column tiles: one pattern -- every tile of the
// batch; per-lane patterns (tiles straddle blocks; lanes of blocks outside the class find
// all-zero masks: no loads, no stores) -- the same tiles; else per block, the tiles of the
// class's blocks only.
template <typename P>
int set_tiling(const DecodeCall& d, const DecodePlan& pl, DecodeClass cl, DevBuf& idbuf, std::vector<uint32_t>* owned,
               P& p, uint64_t* ntiles) {
  *ntiles = (p.total_columns + 63) / 64;
  if (pl.npat == 1) return AG_RS_OK;
  if constexpr (requires { p.per_lane; }) {
    if (pl.per_lane) {
      p.per_lane = 1;
      return AG_RS_OK;
    }
  }
  p.per_block = 1;
  p.tiles_per_block = static_cast<uint32_t>(pl.cps / 64);
  size_t count = 0;
  const int st = select_blocks(d, pl, cl, idbuf, owned, &p.block_ids, &count);
  *ntiles = static_cast<uint64_t>(count) * p.tiles_per_block;
  return st;
}

// ---- one launcher per decoder class ----

int run_transform(const DecodeCall& d, const DecodePlan& pl) {
  ag_rs_ctx* c = d.c;
  std::vector<uint64_t> mask = store_masks(d, pl, kTransform);
  // all restored originals among shards 0..15: the output-pruned 32-point transform
  // (64-point: every restored original among shards 0..31, xform_h8's pruned FFT)
  const unsigned half = pl.npts / 2;
  const bool low_half = std::all_of(mask.begin(), mask.end(), [half](uint64_t w) { return (w >> half) == 0; });
  const int st = c->mask.put(std::move(mask), c->stream);
  if (st) return st;
  XformParams p = xform_params(d.rec, d.rstride, d.m, d.orig, d.ostride, d.k, d.sstride, pl.cps, d.nblocks);
  p.out_mask = c->mask.dev.as<uint64_t>();
  p.pattern_per_block = pl.npat > 1 ? 1u : 0u;
  p.out_low_half = low_half;
  const auto kind = pl.npts == 32 ? XformKind::kDecode32 : XformKind::kDecode64;
  return launch_xform(kind, p, c->stream) == hipSuccess ? AG_RS_OK : AG_RS_ERR_DEVICE;
}

// One launch per recovery chunk in use; store masks select that chunk's patterns.
int run_lowrate_chunk(const DecodeCall& d, const DecodePlan& pl) {
  ag_rs_ctx* c = d.c;
  for (unsigned j = 0; j < 4; ++j) {
    std::vector<uint64_t> mask = store_masks(d, pl, kLowRateChunk, static_cast<int>(j));
    if (std::all_of(mask.begin(), mask.end(), [](uint64_t w) { return w == 0; })) continue;  // chunk not in use
    const int st = c->mask.put(std::move(mask), c->stream);
    if (st) return st;
    XformParams p = xform_params(d.rec + size_t{32} * j * d.sstride, d.rstride, 32, d.orig, d.ostride, d.k, d.sstride,
                                 pl.cps, d.nblocks);
    p.out_mask = c->mask.dev.as<uint64_t>();
    p.pattern_per_block = pl.npat > 1 ? 1u : 0u;
    if (launch_xform_lowrate_decode(j, p, c->stream) != hipSuccess) return AG_RS_ERR_DEVICE;
  }
  return AG_RS_OK;
}

int run_syndrome(const DecodeCall& d, const DecodePlan& pl) {
  ag_rs_ctx* c = d.c;
  int st;
  std::vector<uint8_t> key = flags_key(d, pl, kSyndrome);
  if (!c->syn.holds(key)) {
    const size_t bytes = pl.npat * sizeof(SynPattern);
    if ((st = c->syn.renew(bytes, c->stream))) return st;
    AG_HIP(hipMemcpy(c->syn.dev.ptr, pl.syn.data(), bytes, hipMemcpyHostToDevice));
    c->syn.key = std::move(key);
  }
  auto p = decode_params<DecodeSynParams>(d, pl.cps);
  p.pat = c->syn.dev.as<SynPattern>();
  if ((st = set_tiling(d, pl, kSyndrome, c->d_synblocks, nullptr, p, &p.ntiles))) return st;
  return launch_decode_syn(pl.syn_chunk, p, c->stream) == hipSuccess ? AG_RS_OK : AG_RS_ERR_DEVICE;
}

int run_correction(const DecodeCall& d, const DecodePlan& pl) {
  ag_rs_ctx* c = d.c;
  int st;
  std::vector<uint8_t> key = flags_key(d, pl, kCorrection);
  if (!c->corr.holds(key)) {
    std::vector<CorrPattern> corr(pl.npat);
    std::vector<uint32_t> pool;
    for (size_t p = 0; p < pl.npat; ++p) {
      if (pl.cls[p] != kCorrection) {
        std::memset(&corr[p], 0, sizeof corr[p]);
        continue;
      }
      // corr_fits admitted the pattern; the MDS property makes N invertible
      if (!build_corr_pattern(d.k, d.opres + p * d.k, d.rpres + p * d.m, &corr[p], pool)) return AG_RS_ERR_DEVICE;
    }
    if ((st = c->corr.renew(pl.npat * sizeof(CorrPattern), c->stream))) return st;
    if ((st = c->d_corrk.ensure(std::max<size_t>(pool.size(), 1) * 4, c->stream))) return st;
    AG_HIP(hipMemcpy(c->corr.dev.ptr, corr.data(), pl.npat * sizeof(CorrPattern), hipMemcpyHostToDevice));
    if (!pool.empty()) AG_HIP(hipMemcpy(c->d_corrk.ptr, pool.data(), pool.size() * 4, hipMemcpyHostToDevice));
    c->corr.key = std::move(key);
  }
  auto p = decode_params<DecodeCParams>(d, pl.cps);
  p.pat = c->corr.dev.as<CorrPattern>();
  p.kpool = c->d_corrk.as<uint32_t>();
  if ((st = set_tiling(d, pl, kCorrection, c->d_corrblocks, nullptr, p, &p.ntiles))) return st;
  return launch_decode_c(p, c->stream) == hipSuccess ? AG_RS_OK : AG_RS_ERR_DEVICE;
}

int run_window64(const DecodeCall& d, const DecodePlan& pl) {
  ag_rs_ctx* c = d.c;
  const size_t npat = pl.npat, xw = pl.xw;
  const bool any_k = d.mode == AG_RS_DECODE_ANY_K;
  int st;
  if ((st = c->ensure_tables())) return st;
  // per pattern: [erased (locator) | present (loaded) | restored] position bits
  std::vector<uint64_t> xm(3 * npat, 0);
  for (size_t p = 0; p < npat; ++p) {
    if (pl.cls[p] != kWindow64) continue;
    window64_masks(pl.hr == 1, d.k, d.m, pl.xchunk, pl.xm_rec, d.opres + p * d.k, d.rpres + p * d.m, any_k, &xm[p],
                   &xm[npat + 2 * p], &xm[npat + 2 * p + 1]);
  }
  // polynomial-basis constants (one word per position) for decode_x16 (W = 64) and for
  // per-lane patterns; bitsliced matrices for decode_x's wave-uniform four-Russians products
  const bool poly = xw == 64 || pl.per_lane;
  if (!c->xmask.holds(xm) || xw != c->xmask_w || poly != c->xmask_poly) {
    if ((st = c->xmask.renew(xm.size() * 8, c->stream)) ||
        (st = c->d_rows.ensure(npat * xw * (poly ? 1 : 16) * 4, c->stream)) ||
        (st = c->xmask.upload(std::move(xm), c->stream)))
      return st;
    c->xmask_w = xw;
    c->xmask_poly = poly;
    const uint64_t* dx = c->xmask.dev.as<uint64_t>();
    if (launch_decode_rows(dx, dx + npat, static_cast<uint32_t>(npat), static_cast<uint32_t>(xw), c->dtables(),
                           c->d_rows.as<uint32_t>(), poly, c->stream) != hipSuccess) {
      c->xmask.key.clear();  // d_rows does not hold these patterns' constants
      return AG_RS_ERR_DEVICE;
    }
  }
  auto p = decode_params<DecodeXParams>(d, pl.cps);
  p.pmask = c->xmask.dev.as<uint64_t>() + npat;
  p.rows = c->d_rows.as<uint32_t>();
  p.m = static_cast<uint32_t>(pl.xm_rec);
  p.chunk = static_cast<uint32_t>(pl.xchunk);
  p.low_rate = pl.hr == 1 ? 0u : 1u;
  p.rows_w = static_cast<uint32_t>(xw);
  p.any_k = any_k ? 1u : 0u;
  uint64_t ntiles;
  if ((st = set_tiling(d, pl, kWindow64, c->d_xblocks, nullptr, p, &ntiles))) return st;
  return launch_decode_x(static_cast<unsigned>(xw), 0, p, ntiles, c->stream) == hipSuccess ? AG_RS_OK
                                                                                           : AG_RS_ERR_DEVICE;
}

int run_window128(const DecodeCall& d, const DecodePlan& pl) {
  ag_rs_ctx* c = d.c;
  const size_t npat = pl.npat;
  int st;
  if ((st = c->ensure_tables())) return st;
  // device: m6 [npat][6] = {erased, present, restored} as (positions 0..63, 64..127) pairs, then
  // the two passes' (present in the loaded half, restored) pairs: pass 1 [npat][2], pass 2 [npat][2]
  std::vector<uint64_t> dev(10 * npat, 0);
  for (size_t p = 0; p < npat; ++p) {
    if (pl.cls[p] != kWindow128) continue;
    uint64_t q[10];
    window128_masks(pl.hr == 1, d.k, d.m, pl.c128, d.opres + p * d.k, d.rpres + p * d.m, q);
    std::copy(q, q + 6, &dev[6 * p]);
    std::copy(q + 6, q + 8, &dev[6 * npat + 2 * p]);
    std::copy(q + 8, q + 10, &dev[8 * npat + 2 * p]);
  }
  // upload (and rebuild the constants) only when the masks changed; the copy is ordered on
  // the stream and reads the context's own host vector, so nothing waits for it
  if (!c->x128.holds(dev)) {
    if ((st = c->x128.renew(dev.size() * 8, c->stream)) || (st = c->d_rows128.ensure(npat * 128 * 4, c->stream)) ||
        (st = c->x128.upload(std::move(dev), c->stream)))
      return st;
    if (launch_decode_rows128(c->x128.dev.as<uint64_t>(), static_cast<uint32_t>(npat), c->dtables(),
                              c->d_rows128.as<uint32_t>(), c->stream) != hipSuccess) {
      c->x128.key.clear();  // d_rows128 does not hold these patterns' constants
      return AG_RS_ERR_DEVICE;
    }
  }
  const uint64_t* d6 = c->x128.dev.as<uint64_t>();
  auto p = decode_params<DecodeXParams>(d, pl.cps);
  p.rows = c->d_rows128.as<uint32_t>();
  p.rows_w = 128;
  p.chunk = static_cast<uint32_t>(pl.c128);
  p.low_rate = pl.hr == 1 ? 0u : 1u;
  // recovery shards beyond the window half the kernel loads are addressed from p.rec with
  // the window position; launch_decode_x checks the geometry
  p.m = static_cast<uint32_t>(std::min<size_t>(d.m, p.chunk));
  uint64_t ntiles;
  if ((st = set_tiling(d, pl, kWindow128, c->d_xblocks, &c->x128_ids, p, &ntiles))) return st;
  for (int pass = 1; pass <= 2; ++pass) {
    p.pmask = d6 + (pass == 1 ? 6 : 8) * npat;
    if (launch_decode_x(128, pass, p, ntiles, c->stream) != hipSuccess) return AG_RS_ERR_DEVICE;
  }
  return AG_RS_OK;
}

int run_generic(const DecodeCall& d, const DecodePlan& pl) {
  ag_rs_ctx* c = d.c;
  const size_t k = d.k, m = d.m, npat = pl.npat;
  const int hr = pl.hr;
  int st;
  if ((st = c->ensure_tables())) return st;
  const size_t chunk = hr ? next_pow2(m) : next_pow2(k);
  const size_t end = chunk + (hr ? k : m);
  const size_t W = next_pow2(end);
  // per-pattern device copies of the present flags, then the erasure flags over the transform
  // window (crate decoder_high/low.rs)
  const size_t flag_bytes = npat * (k + m + W);
  std::vector<uint8_t> hostflags(flag_bytes, 0);
  std::memcpy(hostflags.data(), d.opres, npat * k);
  std::memcpy(hostflags.data() + npat * k, d.rpres, npat * m);
  for (size_t p = 0; p < npat; ++p) {
    if (pl.cls[p] != kGeneric) continue;
    uint8_t* e = &hostflags[npat * (k + m) + p * W];
    const size_t opos = hr ? chunk : 0, rpos = hr ? 0 : chunk;
    for (size_t i = 0; i < k; ++i) e[opos + i] = d.opres[p * k + i] ? 0 : 1;
    for (size_t i = 0; i < m; ++i) e[rpos + i] = d.rpres[p * m + i] ? 0 : 1;
    if (hr) {
      for (size_t i = m; i < chunk; ++i) e[i] = 1;  // virtual recovery points
    } else {
      for (size_t i = end; i < W; ++i) e[i] = 1;  // beyond the recovery block
    }
  }
  if ((st = c->d_flags.ensure(flag_bytes, c->stream))) return st;
  if ((st = c->d_loc.ensure(npat * W * 2, c->stream))) return st;
  uint8_t* dflags = c->d_flags.as<uint8_t>();
  AG_HIP(hipMemcpyAsync(dflags, hostflags.data(), flag_bytes, hipMemcpyHostToDevice, c->stream));
  if (launch_locator(dflags + npat * (k + m), static_cast<uint32_t>(npat), static_cast<uint32_t>(W),
                     hr ? 65536u : static_cast<uint32_t>(end), c->d_log_walsh.as<uint16_t>(),
                     c->d_loc.as<uint16_t>(), c->stream) != hipSuccess)
    return AG_RS_ERR_DEVICE;
  // blocks handled by the generic kernel (always by id with per-block patterns)
  std::vector<uint32_t> ids;
  if (npat > 1) {
    ids = class_blocks(pl, kGeneric, d.nblocks);
    if ((st = c->d_blocks.ensure(ids.size() * 4, c->stream))) return st;
    AG_HIP(hipMemcpyAsync(c->d_blocks.ptr, ids.data(), ids.size() * 4, hipMemcpyHostToDevice, c->stream));
  }
  const size_t ngen = npat > 1 ? ids.size() : d.nblocks;
  const size_t nsym = d.S / 2;
  const size_t per_block = W * nsym * 2;
  const size_t per_launch = std::max<size_t>(1, kGenericScratchBytes / per_block);
  if ((st = c->scratch.ensure(std::min(per_launch, ngen) * per_block, c->stream))) return st;
  for (size_t b0 = 0; b0 < ngen; b0 += per_launch) {
    auto p = shard_params<GenericDecodeParams>(d.orig, d.ostride, d.rec, d.rstride, d.sstride);
    p.orig_present = dflags;
    p.rec_present = dflags + npat * k;
    p.pattern_per_block = npat > 1 ? 1u : 0u;
    p.block_ids = npat > 1 ? c->d_blocks.as<uint32_t>() + b0 : nullptr;
    p.block_base = npat > 1 ? 0 : b0;
    p.loc = c->d_loc.as<uint16_t>();
    p.k = static_cast<uint32_t>(k);
    p.m = static_cast<uint32_t>(m);
    p.high_rate = static_cast<uint32_t>(hr);
    p.chunk = static_cast<uint32_t>(chunk);
    p.end = static_cast<uint32_t>(end);
    p.W = static_cast<uint32_t>(W);
    p.shard_bytes = static_cast<uint32_t>(d.S);
    p.nsym = static_cast<uint32_t>(nsym);
    p.nblocks = std::min(per_launch, ngen - b0);
    p.scratch = c->scratch.as<uint16_t>();
    p.t = c->dtables();
    if (launch_generic_decode(p, c->stream) != hipSuccess) return AG_RS_ERR_DEVICE;
  }
  // host vectors above are read by async copies: finish before they go out of scope
  AG_HIP(hipStreamSynchronize(c->stream));
  return AG_RS_OK;
}

// The decode over the first S bytes of every shard (S % 64 == 0 on the bitsliced paths;
// shards sstride >= S bytes apart; any alignment).
int decode_cols(const DecodeCall& d, size_t npat) {
  ag_rs_ctx* c = d.c;
  // (collapsed here for the device-pattern route; classify_patterns finds nothing left to collapse)
  if (npat > 1 && patterns_equal(d.k, d.m, npat, d.opres, d.rpres)) npat = 1;
  if (npat > 1 && npat == d.nblocks && d.k == 32 && d.m == 32 && d.mode == AG_RS_DECODE_ANY_K && d.S % 64 == 0 &&
      d.S / 64 % 64 != 0) {
    const int st = decode_cols_device_patterns(d);
    if (st != kNotApplicable) return st;
  }
  const DecodePlan pl = classify_patterns(d.k, d.m, d.S, d.nblocks, npat, d.mode, d.opres, d.rpres);
  if (pl.status) return pl.status;  // nothing launched yet
  for (size_t p = 0; p < pl.npat; ++p) ++c->last_classes[pl.cls[p]];
  int st;
  if (pl.uses(kTransform) && (st = run_transform(d, pl))) return st;
  if (pl.uses(kLowRateChunk) && (st = run_lowrate_chunk(d, pl))) return st;
  if (pl.uses(kSyndrome) && (st = run_syndrome(d, pl))) return st;
  if (pl.uses(kCorrection) && (st = run_correction(d, pl))) return st;
  if (pl.uses(kWindow64) && (st = run_window64(d, pl))) return st;
  if (pl.uses(kWindow128) && (st = run_window128(d, pl))) return st;
  if (pl.uses(kGeneric) && (st = run_generic(d, pl))) return st;
  return AG_RS_OK;
}

int decode_device_body(ag_rs_ctx* c, size_t k, size_t m, size_t S, size_t nblocks, uint8_t* orig, size_t ostride,
                       const uint8_t* rec, size_t rstride, const uint8_t* opres, const uint8_t* rpres, size_t npat,
                       int mode) {
  if (nblocks == 0) return AG_RS_OK;
  DecodeCall d{c, k, m, S, S, nblocks, orig, ostride, rec, rstride, opres, rpres, mode};
  const bool odd = odd_layout(orig, rec, ostride, rstride);
  if (k <= 64 && (S % 64 != 0 || odd) && S % 2 == 0) {
    const size_t Sp = padded_shard(S);
    const int hr = use_high_rate(k, m);
    const size_t xw = hr == 1 ? next_pow2(next_pow2(m) + k) : 0;
    if (xform_points(k, m, Sp) || mc_chunk(k, m, Sp) || lowrate_chunk(k, m, Sp) || xw == 32 || xw == 64) {
      if (odd) return decode_restrided(c, k, m, S, S, 0, nblocks, orig, ostride, rec, rstride, opres, rpres, npat, mode);
      const size_t full = S / 64 * 64, tail = S - full;
      // every pattern restores from the full 32-point recovery set (or restores nothing): the
      // TAIL transform decodes the whole shards, tail included, in place in one launch
      if (tail >= 16 && xform_points(k, m, Sp) == 32 && m == 32 && mode == AG_RS_DECODE_ANY_K) {
        bool all_full = true;
        for (size_t p = 0; p < npat && all_full; ++p) all_full = count_flags(rpres + p * m, m) == m;
        if (all_full) return decode_tail32(d, npat);
      }
      int st;
      // per-block 32:32 patterns with lost recovery shards (ANY_K): the per-lane window decode
      // takes the whole shards, the T-byte tail as one more column (decode_h8 TAIL), no restride
      if (tail != 0 && npat > 1 && npat == nblocks && k == 32 && m == 32 && hr == 1 && mode == AG_RS_DECODE_ANY_K) {
        st = decode_cols_device_patterns(d);
        if (st != kNotApplicable) return st;
      }
      d.S = full;
      if (full && (st = decode_cols(d, npat))) return st;
      return decode_restrided(c, k, m, tail, S, full, nblocks, orig, ostride, rec, rstride, opres, rpres, npat, mode);
    }
  }
  return decode_cols(d, npat);
}

}  // namespace

// last_classes counts every pattern of the outermost call: the whole-chunk decode and the
// tail restride's inner decode of a shard size with S % 64 != 0 add up (reset once per call)
int decode_device(ag_rs_ctx* c, size_t k, size_t m, size_t S, size_t nblocks, uint8_t* orig, size_t ostride,
                  const uint8_t* rec, size_t rstride, const uint8_t* opres, const uint8_t* rpres, size_t npat,
                  int mode) {
  if (c->decode_depth == 0) std::fill(std::begin(c->last_classes), std::end(c->last_classes), uint64_t{0});
  ++c->decode_depth;
  const int st = decode_device_body(c, k, m, S, nblocks, orig, ostride, rec, rstride, opres, rpres, npat, mode);
  --c->decode_depth;
  return st;
}

}  // namespace host
}  // namespace ag
