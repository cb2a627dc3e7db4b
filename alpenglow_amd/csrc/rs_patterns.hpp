// Host-only pattern bookkeeping of the decoders (no HIP calls): presence flags -> masks, the
// per-pattern tables of the syndrome (decode_syn) and correction (decode_c) decoders, and the
// window masks of the locator decoders (decode_x / decode_h8 / decode_x16), and the classifier
// that decides which decoder restores each pattern (rs_dispatch.cpp launches what it plans).
// Kept apart from the HIP host code so the CPU suite can run it under AddressSanitizer /
// UndefinedBehaviorSanitizer (tests/native/patterns_selfcheck.cpp, tests/test_sanitizers.py).
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../include/alpenglow_rs.h"
#include "gf16.hpp"
#include "rs_launch.hpp"

namespace ag {

// Single-chunk HighRate geometries served by the bitsliced N-point transform kernel:
// k <= N, next_pow2(m) == N, N in {32, 64}, whole 64-byte chunks.  Returns N or 0.
// (HighRate with a single chunk implies next_pow2(k) == N and k <= m.)
inline unsigned xform_points(size_t k, size_t m, size_t S) {
  if (S == 0 || S % 64 || use_high_rate(k, m) != 1) return 0;
  const size_t n = next_pow2(m);
  return (n == 32 || n == 64) && k <= n ? static_cast<unsigned>(n) : 0;
}

// Multi-chunk HighRate encode with a small recovery chunk (encode_mc kernel): returns the
// chunk next_pow2(m) in {1, 2, 4} when k > chunk, k <= 64, whole 64-byte chunks; else 0.
inline unsigned mc_chunk(size_t k, size_t m, size_t S) {
  if (S == 0 || S % 64 || use_high_rate(k, m) != 1 || k > 64) return 0;
  const size_t c = next_pow2(m);
  return c <= 4 && k > c ? static_cast<unsigned>(c) : 0;
}

// LowRate encode through the transform kernel, one launch per recovery chunk: returns the
// chunk next_pow2(k) in {32, 64} when the recovery chunks fit the launcher, else 0.
inline unsigned lowrate_chunk(size_t k, size_t m, size_t S) {
  if (S == 0 || S % 64 || use_high_rate(k, m) != 0) return 0;
  const size_t c = next_pow2(k);
  const size_t chunks = (m + c - 1) / c;
  if (c == 32 && chunks <= 4) return 32;
  if (c == 64 && chunks <= 3) return 64;
  return 0;
}

// A shard size rounded up to whole 64-byte chunks.
inline size_t padded_shard(size_t S) { return (S + 63) / 64 * 64; }

// Host flag arrays (0 / nonzero bytes, one per shard) -> bit masks, 8 flags per step:
// the per-pattern bookkeeping of a 65 536-slice batch stays well under a millisecond.
inline uint64_t pack_flags(const uint8_t* f, size_t n) {  // n <= 64
  uint64_t bits = 0;
  size_t i = 0;
  for (; i + 8 <= n; i += 8) {
    uint64_t x;
    std::memcpy(&x, f + i, 8);
    // high bit of each byte <- byte != 0, then gather the 8 high bits (multiply trick)
    const uint64_t nz = ((((x & 0x7F7F7F7F7F7F7F7Full) + 0x7F7F7F7F7F7F7F7Full) | x) & 0x8080808080808080ull) >> 7;
    bits |= ((nz * 0x0102040810204080ull) >> 56) << i;
  }
  for (; i < n; ++i) bits |= uint64_t{f[i] != 0} << i;
  return bits;
}
inline size_t count_flags(const uint8_t* f, size_t n) {
  if (n <= 64) return static_cast<size_t>(__builtin_popcountll(pack_flags(f, n)));
  size_t c = 0;
  for (size_t i = 0; i < n; ++i) c += f[i] != 0;
  return c;
}

// Syndrome-decoder pattern (decode_syn_kernel): restore the erased originals from the
// first e present recovery shards; G = the k x m HighRate generator (hr_generator).  False
// if the pattern does not fit (more than 4 erased, too few recovery shards) or the e x e
// system is singular (cannot happen for an MDS code); the caller then takes another decoder.
bool build_syn_pattern(size_t k, size_t m, const uint8_t* opres, const uint8_t* rpres, const uint16_t* G,
                       SynPattern* sp);

// In-place Gauss-Jordan inverse of an n x n matrix over GF(2^16) (row-major, stride n).
// Returns false if singular.
bool gf_invert(size_t n, uint16_t* A);

// X = the 32-point full-recovery transform as a matrix (the inverse of the 32:32 encoder).
const uint16_t* full_window_x32();

// decode_c: whether a 32:m=32 pattern takes the correction decoder (no = present originals,
// nr = present recovery shards), and its pattern (K picks appended to `pool`).
bool corr_fits(size_t k, size_t no, size_t nr);
bool build_corr_pattern(size_t k, const uint8_t* opres, const uint8_t* rpres, CorrPattern* cp,
                        std::vector<uint32_t>& pool);

// The W <= 64 locator window of one pattern (decode_x / decode_h8 / decode_x16 PASS 0):
// erased (locator) / present (loaded) / restored position bits.  HighRate (hr): recovery j <
// xchunk at j, original i at xchunk + i; LowRate sub-window: original i at i, recovery j at
// xchunk + j (j < xm_rec).  any_k: exactly k survivors -- the present originals, then the
// recovery shards in index order (the surplus counts as erased).
void window64_masks(bool hr, size_t k, size_t m, size_t xchunk, size_t xm_rec, const uint8_t* opres,
                    const uint8_t* rpres, bool any_k, uint64_t* e, uint64_t* in, uint64_t* out);

// The W = 128 window of one pattern as two 64-point passes (exactly k survivors): q[0..5] =
// {erased, present, restored} as (positions 0..63, 64..127) pairs, q[6..7] = pass 1's (present
// in the loaded half, restored), q[8..9] = pass 2's.  c128 = next_pow2(m) (HighRate, 64) or
// next_pow2(k) (LowRate).
void window128_masks(bool hr, size_t k, size_t m, size_t c128, const uint8_t* opres, const uint8_t* rpres,
                     uint64_t q[10]);

// Per-slice present words of the coder deshreds' device-pattern paths (32 data shreds, m coding
// shreds): word 0 = data flags | coding 0..31 << 32 (and word 1 = coding 32..m-1 when m > 32).
// Returns whether any slice keeps more than 32 shreds; *any_full_data: some slice holds every
// data shred (its decode is skipped, so its absent coding shreds come from the re-encode).
bool pack_present_words(const uint8_t* dpres, const uint8_t* cpres, size_t m, size_t n, uint64_t* pres,
                        bool* any_full_data);

// The decoder that restores a pattern.  The values are fixed: last_classes[] is indexed by
// them and Python names them (rs.DECODE_CLASSES).
enum DecodeClass : uint8_t {
  kNone = 0,            // no original lost
  kTransform = 1,       // full recovery set: the N-point transform inverts the encoder
  kGeneric = 2,         // table-driven generic kernel
  kWindow64 = 3,        // W <= 64 locator window (decode_x / decode_h8 / decode_x16)
  kSyndrome = 4,        // encode_mc geometries, at most 4 originals lost (decode_syn)
  kLowRateChunk = 5,    // LowRate, one fully present 32-shard recovery chunk: its transform
  kCorrection = 6,      // 32-point full window with few lost recovery shards (decode_c)
  kWindow128 = 8,       // W = 128 window as two 64-point passes
  kServerWindow64 = 9,  // the per-call server's one-slice window decode
};

// One erasure pattern repeated for every block (a repair batch, a uniform loss) is one
// pattern: uniform store masks, and the bitsliced kernels regardless of block alignment.
bool patterns_equal(size_t k, size_t m, size_t npat, const uint8_t* opres, const uint8_t* rpres);

// Whether the transform restores a pattern with nr recovery shards present (kTransform): it
// inverts the encoder only when all N recovery points exist (m == N; with m < N the points
// m..N-1 were never stored), and then reads no original.
inline bool transform_restores(size_t k, size_t m, size_t S, int mode, size_t nr) {
  const unsigned npts = xform_points(k, m, S);
  return mode == AG_RS_DECODE_ANY_K && npts != 0 && m == npts && nr == m;
}

// What classify_patterns decides for one decode over the first S bytes of every shard.
struct DecodePlan {
  int status = AG_RS_OK;          // or AG_RS_ERR_NOT_ENOUGH_SHARDS: nothing else is set then
  size_t npat = 0;                // patterns after the equal-patterns collapse
  std::vector<uint8_t> cls;       // DecodeClass per pattern
  std::vector<uint8_t> lr_chunk;  // kLowRateChunk patterns: the recovery chunk they restore from
  std::vector<SynPattern> syn;    // kSyndrome patterns (all zero for the others); empty without syn_chunk
  uint32_t used = 0;              // bit c: some pattern has class c
  int hr = 0;                     // use_high_rate(k, m)
  unsigned npts = 0;              // xform_points(k, m, S)
  unsigned syn_chunk = 0;         // mc_chunk(k, m, S) where the syndrome decoder's tiling allows it
  size_t xchunk = 0, xw = 0;      // W <= 64 window: chunk and width (0: no such window)
  size_t xm_rec = 0;              // recovery shards inside that window
  size_t c128 = 0;                // W = 128 window: next_pow2(m) (HighRate) or next_pow2(k) (LowRate)
  size_t cps = 0;                 // S / 64
  bool per_lane = false;          // per-block patterns on tiles that straddle blocks (cps % 64 != 0)
  bool uses(DecodeClass c) const { return (used >> c) & 1u; }
};

// Classifies every pattern of a decode call (npat == 1 or npat == nblocks; mode AG_RS_DECODE_*):
// one pass over the flags, no allocation per pattern.  Each pattern takes the first class of
// none, transform, lowrate_chunk, syndrome, correction, window64, window128, generic that
// admits it.
DecodePlan classify_patterns(size_t k, size_t m, size_t S, size_t nblocks, size_t npat, int mode,
                             const uint8_t* opres, const uint8_t* rpres);

}  // namespace ag
