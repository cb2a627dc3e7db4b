// Test infrastructure (not part of the library): the host-only decoder bookkeeping of
// rs_patterns.cpp and the field code of gf16.cpp, built with AddressSanitizer and
// UndefinedBehaviorSanitizer by tests/test_sanitizers.py and checked against the field's own
// definitions -- no GPU, no HIP call.
//   * gf_invert: A * A^-1 = I for random invertible matrices (n = 1..32);
//   * full_window_x32: X * G = I for the 32:32 HighRate generator G;
//   * build_syn_pattern: Minv * (syndromes) restores the erased originals of 16:4 codewords;
//   * build_corr_pattern: (X r')_E + K s restores the erased originals of 32:32 codewords
//     with lost recovery shards (K read back from the kernel's table picks);
//   * window64_masks / window128_masks: exactly k survivors under ANY_K, no erased position
//     loaded, every restored position erased;
//   * pack_flags / count_flags against a byte loop;
//   * classify_patterns: a table of geometries and patterns with the decoder class each must
//     take, and the rules every class obeys over random patterns.
// Prints "ok" and exits 0, or names the first failing check and exits 1.
#include <cstdio>
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <random>
#include <utility>
#include <vector>

#include "gf16.hpp"
#include "rs_patterns.hpp"

using namespace ag;

static int g_fail = 0;
#define CHECK(cond, ...)                         \
  do {                                           \
    if (!(cond)) {                               \
      std::fprintf(stderr, "FAIL %s:%d: ", __FILE__, __LINE__); \
      std::fprintf(stderr, __VA_ARGS__);         \
      std::fprintf(stderr, "\n");                \
      ++g_fail;                                  \
      return;                                    \
    }                                            \
  } while (0)

static uint16_t mulv(uint16_t a, uint16_t b) { return gf_mul_elem(gf16_tables(), a, b); }

// y = M x over GF(2^16), M n x n row-major
static void matvec(size_t n, const uint16_t* M, const uint16_t* x, uint16_t* y) {
  for (size_t r = 0; r < n; ++r) {
    uint16_t acc = 0;
    for (size_t c = 0; c < n; ++c) acc ^= mulv(M[r * n + c], x[c]);
    y[r] = acc;
  }
}

static void check_invert(std::mt19937_64& rng) {
  for (size_t n = 1; n <= 32; ++n) {
    std::vector<uint16_t> A(n * n), B;
    for (int attempt = 0;; ++attempt) {
      for (auto& v : A) v = static_cast<uint16_t>(rng());
      B = A;
      if (gf_invert(n, B.data())) break;
      CHECK(attempt < 8, "no invertible random %zux%zu matrix", n, n);
    }
    for (size_t r = 0; r < n; ++r)
      for (size_t c = 0; c < n; ++c) {
        uint16_t acc = 0;
        for (size_t i = 0; i < n; ++i) acc ^= mulv(A[r * n + i], B[i * n + c]);
        CHECK(acc == (r == c ? 1 : 0), "A * A^-1 != I (n=%zu)", n);
      }
  }
  std::vector<uint16_t> Z(9, 0);
  CHECK(!gf_invert(3, Z.data()), "singular matrix inverted");
}

static void check_x32() {
  const uint16_t* X = full_window_x32();
  CHECK(X != nullptr, "full_window_x32 failed");
  std::vector<uint16_t> G(32 * 32);
  hr_generator(32, 32, G.data());
  for (size_t r = 0; r < 32; ++r)
    for (size_t c = 0; c < 32; ++c) {
      uint16_t acc = 0;
      for (size_t i = 0; i < 32; ++i) acc ^= mulv(X[r * 32 + i], G[i * 32 + c]);
      CHECK(acc == (r == c ? 1 : 0), "X * G != I");
    }
}

// 16x16 GF(2) matrix (rows[o] bit i) applied to a field element
static uint16_t bitmat(const uint32_t* rows, uint16_t x) {
  uint16_t y = 0;
  for (unsigned o = 0; o < 16; ++o) y |= static_cast<uint16_t>((__builtin_popcount(rows[o] & x) & 1) << o);
  return y;
}

static void check_syn(std::mt19937_64& rng) {
  const size_t k = 16, m = 4;
  std::vector<uint16_t> G(m * k);
  hr_generator(k, m, G.data());
  for (int it = 0; it < 400; ++it) {
    uint16_t d[16], r[4];
    for (auto& v : d) v = static_cast<uint16_t>(rng());
    for (size_t j = 0; j < m; ++j) {
      r[j] = 0;
      for (size_t i = 0; i < k; ++i) r[j] ^= mulv(G[j * k + i], d[i]);
    }
    uint8_t op[16], rp[4];
    for (auto& v : op) v = 1;
    for (auto& v : rp) v = rng() & 1;
    const size_t e = rng() % 5;
    for (size_t i = 0; i < e; ++i) op[rng() % k] = 0;
    SynPattern sp;
    const size_t ne = k - count_flags(op, k), nr = count_flags(rp, m);
    const bool ok = build_syn_pattern(k, m, op, rp, G.data(), &sp);
    CHECK(ok == (ne <= nr), "build_syn_pattern admitted %d with ne=%zu nr=%zu", ok, ne, nr);
    if (!ok) continue;
    CHECK(sp.e == ne, "syn e");
    // syndromes: received recovery minus the re-encoded present originals at the used rows
    uint16_t S[4] = {};
    for (size_t b = 0; b < sp.e; ++b) {
      const size_t j = sp.rec[b];
      CHECK(rp[j], "syn uses an absent recovery shard");
      uint16_t acc = r[j];
      for (size_t i = 0; i < k; ++i)
        if (op[i]) acc ^= mulv(G[j * k + i], d[i]);
      S[b] = acc;
    }
    for (size_t a = 0; a < sp.e; ++a) {
      uint16_t got = 0;
      for (size_t b = 0; b < sp.e; ++b) got ^= bitmat(sp.rows[a][b], S[b]);
      CHECK(got == d[sp.out[a]], "syn restore mismatch");
    }
  }
}

static void check_corr(std::mt19937_64& rng) {
  const uint16_t* X = full_window_x32();
  std::vector<uint16_t> G(32 * 32);
  hr_generator(32, 32, G.data());
  for (int it = 0; it < 300; ++it) {
    const size_t k = 17 + rng() % 16;  // 17..32
    uint16_t d[32] = {}, r[32];
    for (size_t i = 0; i < k; ++i) d[i] = static_cast<uint16_t>(rng());
    matvec(32, G.data(), d, r);  // the k-code is the 32-code with originals k..31 zero
    uint8_t op[32], rp[32];
    for (size_t i = 0; i < k; ++i) op[i] = 1;
    for (auto& v : rp) v = 1;
    const size_t nl = 1 + rng() % 16;
    for (size_t i = 0; i < nl; ++i) rp[rng() % 32] = 0;
    const size_t ne = 1 + rng() % 16;
    for (size_t i = 0; i < ne; ++i) op[rng() % k] = 0;
    const size_t no = count_flags(op, k), nr = count_flags(rp, 32);
    if (no + nr < k) continue;
    CorrPattern cp;
    std::vector<uint32_t> pool;
    const bool fits = corr_fits(k, no, nr);
    const bool ok = build_corr_pattern(k, op, rp, &cp, pool);
    CHECK(ok == fits, "build_corr_pattern %d vs corr_fits %d", ok, fits);
    if (!ok) continue;
    uint16_t rz[32], xr[32];
    for (size_t j = 0; j < 32; ++j) rz[j] = rp[j] ? r[j] : 0;
    matvec(32, X, rz, xr);
    // syndromes at the points of smask in position order
    uint16_t s[32];
    size_t ns = 0;
    for (size_t i = 0; i < 32; ++i)
      if ((cp.smask >> i) & 1) s[ns++] = static_cast<uint16_t>(d[i] ^ xr[i]);
    CHECK(ns == cp.ns, "corr syndrome count");
    const uint32_t* K = pool.data() + cp.kofs;
    size_t a = 0;
    for (size_t i = 0; i < k; ++i) {
      if (!((cp.emask >> i) & 1)) continue;
      uint16_t got = xr[i];
      for (size_t b = 0; b < ns; ++b) {
        const uint32_t* pk = K + kCorrPairWords * (a * ns + b);
        uint32_t rows[16];
        for (unsigned o = 0; o < 16; ++o)
          rows[o] = pk[2 * o] | (pk[2 * o + 1] << 4) | (pk[32 + 2 * o] << 8) | (pk[32 + 2 * o + 1] << 12);
        got ^= bitmat(rows, s[b]);
      }
      CHECK(got == d[i], "corr restore mismatch (k=%zu |L|=%u |E|=%u)", k, cp.ns, cp.ne);
      ++a;
    }
  }
}

static void check_windows(std::mt19937_64& rng) {
  for (int it = 0; it < 2000; ++it) {
    // HighRate 32:32 (xchunk 32) and the LowRate sub-window of 32:64 (xchunk 32, xm_rec 32)
    const bool hr = it & 1;
    const size_t k = 32, m = hr ? 32 : 64, xchunk = 32, xm_rec = 32;
    uint8_t op[32], rp[64];
    for (auto& v : op) v = rng() & 1;
    for (auto& v : rp) v = (rng() % 3) != 0;
    const size_t no = count_flags(op, k), nr = count_flags(rp, xm_rec);
    if (no + nr < k) continue;
    uint64_t e, in, out;
    window64_masks(hr, k, m, xchunk, xm_rec, op, rp, true, &e, &in, &out);
    CHECK(static_cast<size_t>(__builtin_popcountll(in)) == k, "ANY_K window loads %d, not k", __builtin_popcountll(in));
    CHECK((in & e) == 0, "a loaded position is erased");
    CHECK((out & ~e) == 0, "a restored position is not erased");
    CHECK(static_cast<size_t>(__builtin_popcountll(out)) == k - no, "restored count");
    uint64_t e2, in2, out2;
    window64_masks(hr, k, m, xchunk, xm_rec, op, rp, false, &e2, &in2, &out2);
    CHECK(static_cast<size_t>(__builtin_popcountll(in2)) == no + nr, "EXACT window must load every present shard");
    // W = 128: HighRate 64:64, LowRate 32:64 over both recovery chunks
    const size_t k2 = hr ? 64 : 32, m2 = 64, c128 = 64 / (hr ? 1 : 2);
    uint8_t op2[64], rp2[64];
    for (size_t i = 0; i < k2; ++i) op2[i] = rng() & 1;
    for (auto& v : rp2) v = rng() & 1;
    if (count_flags(op2, k2) + count_flags(rp2, m2) < k2) continue;
    uint64_t q[10];
    window128_masks(hr, k2, m2, hr ? 64 : c128, op2, rp2, q);
    const int nin = __builtin_popcountll(q[2]) + __builtin_popcountll(q[3]);
    CHECK(static_cast<size_t>(nin) == k2, "W=128 loads %d, not k", nin);
    CHECK(((q[2] & q[0]) | (q[3] & q[1])) == 0, "W=128 loaded position erased");
    CHECK(((q[4] & ~q[0]) | (q[5] & ~q[1])) == 0, "W=128 restored position not erased");
  }
}

static void check_flags(std::mt19937_64& rng) {
  for (int it = 0; it < 5000; ++it) {
    const size_t n = rng() % 65;
    std::vector<uint8_t> f(n);
    uint64_t want = 0;
    for (size_t i = 0; i < n; ++i) {
      f[i] = (rng() & 3) ? static_cast<uint8_t>(rng()) : 0;
      if (f[i]) want |= uint64_t{1} << i;
    }
    CHECK(pack_flags(f.data(), n) == want, "pack_flags");
    CHECK(count_flags(f.data(), n) == static_cast<size_t>(__builtin_popcountll(want)), "count_flags");
  }
}

// n flags, all present but the [from, to) ranges
static std::vector<uint8_t> flags(size_t n, std::initializer_list<std::pair<size_t, size_t>> lost) {
  std::vector<uint8_t> f(n, 1);
  for (const auto& r : lost)
    for (size_t i = r.first; i < r.second; ++i) f[i] = 0;
  return f;
}

struct ClassCase {
  size_t k, m, S, nblocks;
  int mode;
  std::vector<std::vector<uint8_t>> op, rp;  // one entry per pattern
  int status;
  std::vector<uint8_t> cls;  // expected class per pattern (after the collapse)
  int lr_chunk;              // of the kLowRateChunk patterns; -1: none expected
};

static void check_classify_table() {
  const int A = AG_RS_DECODE_ANY_K, E = AG_RS_DECODE_EXACT;
  const auto lose16 = flags(32, {{0, 16}}), all32 = flags(32, {});
  // mixed per-block patterns of the 32:32 code: nothing lost / full recovery set / 4 recovery
  // shards lost / 17 recovery shards lost
  const std::vector<std::vector<uint8_t>> mix_o = {all32, lose16, lose16, flags(32, {{0, 8}})};
  const std::vector<std::vector<uint8_t>> mix_r = {flags(32, {{0, 5}}), all32, flags(32, {{0, 4}}),
                                                   flags(32, {{4, 21}})};
  // 32:64: nothing lost / recovery chunk 0 whole / chunk 1 whole / enough inside the W = 64
  // sub-window / only both chunks together
  const std::vector<std::vector<uint8_t>> lr_o = {all32, flags(32, {{0, 32}}), flags(32, {{0, 32}}),
                                                  flags(32, {{0, 8}}), lose16};
  const std::vector<std::vector<uint8_t>> lr_r = {flags(64, {{0, 3}}), flags(64, {{40, 64}}), flags(64, {{0, 32}}),
                                                  flags(64, {{0, 3}, {40, 44}}), flags(64, {{0, 24}, {40, 44}})};
  const std::vector<ClassCase> cases = {
      {32, 32, 4096, 1, A, {lose16}, {all32}, AG_RS_OK, {kTransform}, -1},
      {32, 32, 4096, 1, E, {lose16}, {all32}, AG_RS_OK, {kWindow64}, -1},
      // the correction decoder from 64 * 256 columns on (64 columns per block here)
      {32, 32, 4096, 256, A, {lose16}, {flags(32, {{0, 4}})}, AG_RS_OK, {kCorrection}, -1},
      {32, 32, 4096, 255, A, {lose16}, {flags(32, {{0, 4}})}, AG_RS_OK, {kWindow64}, -1},
      {16, 4, 4096, 1, A, {flags(16, {{0, 2}})}, {flags(4, {})}, AG_RS_OK, {kSyndrome}, -1},
      {16, 4, 4096, 1, E, {flags(16, {{0, 2}})}, {flags(4, {})}, AG_RS_OK, {kWindow64}, -1},
      {32, 64, 1024, 1, A, {flags(32, {{0, 32}})}, {flags(64, {{0, 32}})}, AG_RS_OK, {kLowRateChunk}, 1},
      {64, 64, 4096, 1, A, {flags(64, {{0, 16}})}, {flags(64, {{0, 8}})}, AG_RS_OK, {kWindow128}, -1},
      {100, 100, 1024, 1, A, {flags(100, {{0, 10}})}, {flags(100, {{0, 5}})}, AG_RS_OK, {kGeneric}, -1},
      {100, 100, 1024, 1, E, {flags(100, {{0, 10}})}, {flags(100, {{0, 5}})}, AG_RS_OK, {kGeneric}, -1},
      // no original lost: none, whatever the geometry
      {32, 32, 4096, 1, A, {all32}, {flags(32, {{0, 9}})}, AG_RS_OK, {kNone}, -1},
      {100, 100, 1024, 1, E, {flags(100, {})}, {flags(100, {{0, 50}})}, AG_RS_OK, {kNone}, -1},
      // fewer than k shards present
      {32, 32, 4096, 1, A, {lose16}, {flags(32, {{0, 17}})}, AG_RS_ERR_NOT_ENOUGH_SHARDS, {}, -1},
      {16, 4, 4096, 1, A, {flags(16, {{0, 3}})}, {flags(4, {{0, 2}})}, AG_RS_ERR_NOT_ENOUGH_SHARDS, {}, -1},
      // per-block patterns, mixed classes in one call: 64 tiles per block, then per-lane tiles
      {32, 32, 4096 * 64, 4, A, mix_o, mix_r, AG_RS_OK, {kNone, kTransform, kCorrection, kWindow64}, -1},
      {32, 32, 4096 * 64, 4, E, mix_o, mix_r, AG_RS_OK, {kNone, kWindow64, kWindow64, kWindow64}, -1},
      {32, 32, 192, 4, A, mix_o, mix_r, AG_RS_OK, {kNone, kTransform, kWindow64, kWindow64}, -1},
      {64, 64, 4096, 3, A, {flags(64, {}), flags(64, {{0, 16}}), flags(64, {{0, 16}})},
       {flags(64, {{0, 3}}), flags(64, {}), flags(64, {{0, 8}})}, AG_RS_OK, {kNone, kTransform, kWindow128}, -1},
      {64, 64, 4096, 3, E, {flags(64, {}), flags(64, {{0, 16}}), flags(64, {{0, 16}})},
       {flags(64, {{0, 3}}), flags(64, {}), flags(64, {{0, 8}})}, AG_RS_OK, {kNone, kGeneric, kGeneric}, -1},
      {32, 64, 4096, 5, E, lr_o, lr_r, AG_RS_OK, {kNone, kGeneric, kWindow128, kGeneric, kGeneric}, -1},
      // equal patterns collapse to one
      {32, 32, 4096, 3, A, {lose16, lose16, lose16}, {all32, all32, all32}, AG_RS_OK, {kTransform}, -1},
  };
  for (size_t ci = 0; ci < cases.size(); ++ci) {
    const ClassCase& t = cases[ci];
    std::vector<uint8_t> op, rp;
    for (const auto& v : t.op) op.insert(op.end(), v.begin(), v.end());
    for (const auto& v : t.rp) rp.insert(rp.end(), v.begin(), v.end());
    const DecodePlan pl = classify_patterns(t.k, t.m, t.S, t.nblocks, t.op.size(), t.mode, op.data(), rp.data());
    CHECK(pl.status == t.status, "classify case %zu: status %d, expected %d", ci, pl.status, t.status);
    if (t.status) continue;
    CHECK(pl.npat == t.cls.size() && pl.cls == t.cls, "classify case %zu (%zu:%zu): class %d...", ci, t.k, t.m,
          pl.cls.empty() ? -1 : pl.cls[0]);
    uint32_t used = 0;
    for (size_t p = 0; p < pl.npat; ++p) {
      used |= 1u << pl.cls[p];
      if (pl.cls[p] == kLowRateChunk) CHECK(pl.lr_chunk[p] == t.lr_chunk, "classify case %zu: chunk %d", ci, pl.lr_chunk[p]);
    }
    CHECK(pl.used == used, "classify case %zu: used %x", ci, pl.used);
  }
  // the 32:64 row above under ANY_K, with both chunk choices in one call
  std::vector<uint8_t> op, rp;
  for (const auto& v : lr_o) op.insert(op.end(), v.begin(), v.end());
  for (const auto& v : lr_r) rp.insert(rp.end(), v.begin(), v.end());
  const DecodePlan pl = classify_patterns(32, 64, 4096, 5, 5, A, op.data(), rp.data());
  const std::vector<uint8_t> want = {kNone, kLowRateChunk, kLowRateChunk, kWindow64, kWindow128};
  CHECK(pl.status == AG_RS_OK && pl.cls == want, "classify 32:64 per block");
  CHECK(pl.lr_chunk[1] == 0 && pl.lr_chunk[2] == 1, "classify 32:64 chunks %d %d", pl.lr_chunk[1], pl.lr_chunk[2]);
  CHECK(pl.hr == 0 && pl.xchunk == 32 && pl.xw == 64 && pl.xm_rec == 32 && pl.c128 == 32 && pl.cps == 64 && !pl.per_lane,
        "classify 32:64 geometry");
}

// The rules of the classes over random patterns: what a class may be given, read off the
// decoders' own requirements, not off the classifier.
static void check_classify_random(std::mt19937_64& rng) {
  const size_t geos[][2] = {{32, 32}, {32, 64}, {32, 33}, {16, 4}, {64, 64}, {40, 64}, {20, 80}};
  for (const auto& g : geos) {
    const size_t k = g[0], m = g[1];
    std::vector<uint16_t> G;
    if (use_high_rate(k, m) == 1) {
      G.resize(m * k);
      hr_generator(k, m, G.data());
    }
    for (int it = 0; it < 40; ++it) {
      // 64 tiles per block with the column threshold of the correction class met (it % 4 ==
      // 0) or not, per-lane tiles, one pattern
      const size_t S = it % 4 == 2 ? 192 : 4096, nblocks = it % 4 == 0 ? 256 : 16;
      const size_t npat = it % 4 == 3 ? 1 : nblocks;
      const int mode = it & 4 ? AG_RS_DECODE_EXACT : AG_RS_DECODE_ANY_K;
      const unsigned lo = rng() % 5, lr = rng() % 5;
      std::vector<uint8_t> op(npat * k), rp(npat * m);
      for (size_t p = 0; p < npat; ++p) {
        // a valid pattern: redrawn until k shards are present; some with nothing lost, some
        // with the full recovery set, some with one whole 32-shard recovery chunk
        do {
          for (size_t i = 0; i < k; ++i) op[p * k + i] = rng() % 8 >= lo ? static_cast<uint8_t>(1 + rng() % 255) : 0;
          for (size_t i = 0; i < m; ++i) rp[p * m + i] = rng() % 8 >= lr;
          const unsigned pick = rng() % 8;
          if (pick == 0) std::fill_n(&op[p * k], k, 1);
          if (pick == 1) std::fill_n(&rp[p * m], m, 1);
          if (pick == 2 && m >= 64) std::fill_n(&rp[p * m + 32 * (rng() % 2)], 32, 1);
        } while (count_flags(&op[p * k], k) + count_flags(&rp[p * m], m) < k);
      }
      const DecodePlan pl = classify_patterns(k, m, S, nblocks, npat, mode, op.data(), rp.data());
      CHECK(pl.status == AG_RS_OK && pl.npat == npat && pl.cls.size() == npat, "classify %zu:%zu: plan shape", k, m);
      const unsigned npts = xform_points(k, m, S);
      uint32_t used = 0;
      for (size_t p = 0; p < npat; ++p) {
        const uint8_t *o = &op[p * k], *r = &rp[p * m];
        const size_t no = count_flags(o, k), nr = count_flags(r, m);
        const uint8_t c = pl.cls[p];
        used |= 1u << c;
        // exactly one class, and a named one
        CHECK(c == kNone || c == kTransform || c == kGeneric || c == kWindow64 || c == kSyndrome ||
                  c == kLowRateChunk || c == kCorrection || c == kWindow128,
              "classify %zu:%zu: class %d", k, m, c);
        CHECK((c == kNone) == (no == k), "classify %zu:%zu: none iff no original lost", k, m);
        if (c == kTransform)
          CHECK(mode == AG_RS_DECODE_ANY_K && nr == m && npts != 0 && m == npts, "classify %zu:%zu: transform", k, m);
        if (c == kSyndrome) {
          SynPattern sp;
          CHECK(!G.empty() && build_syn_pattern(k, m, o, r, G.data(), &sp), "classify %zu:%zu: syndrome", k, m);
          CHECK(std::memcmp(&sp, &pl.syn[p], sizeof sp) == 0, "classify %zu:%zu: syndrome pattern", k, m);
        }
        if (c == kCorrection)
          CHECK(corr_fits(k, no, nr) && nblocks * (S / 64) >= 64 * 256, "classify %zu:%zu: correction", k, m);
        if (c == kLowRateChunk) {
          const size_t j = pl.lr_chunk[p];
          CHECK(32 * (j + 1) <= m && count_flags(r + 32 * j, 32) == 32, "classify %zu:%zu: chunk %zu not whole", k, m, j);
        }
        // the class of a pattern does not depend on the other patterns of the call
        if (npat > 1 && p % 16 == 0) {
          std::vector<uint8_t> o2(o, o + k), r2(r, r + m);
          for (size_t q = 1; q < npat; ++q) {  // the same call with every other pattern replaced
            o2.insert(o2.end(), k, 1);
            r2.insert(r2.end(), m, q & 1);
          }
          o2[k] = 0;  // (and never equal patterns: pattern 1 loses original 0 alone)
          r2[m] = 1;
          const DecodePlan alone = classify_patterns(k, m, S, nblocks, npat, mode, o2.data(), r2.data());
          CHECK(alone.status == AG_RS_OK && alone.npat == npat && alone.cls[0] == c,
                "classify %zu:%zu: class %d of a pattern became %d among other patterns", k, m, c, alone.cls[0]);
        }
      }
      CHECK(pl.used == used, "classify %zu:%zu: used", k, m);
    }
  }
}

static void check_present_words(std::mt19937_64& rng) {
  for (size_t m : {size_t{32}, size_t{33}, size_t{64}}) {
    const size_t n = 37, wps = m == 32 ? 1 : 2;
    std::vector<uint8_t> d(n * 32), c(n * m);
    for (auto& v : d) v = (rng() & 3) ? static_cast<uint8_t>(rng() | 1) : 0;
    for (auto& v : c) v = (rng() & 1) ? static_cast<uint8_t>(rng() | 1) : 0;
    std::fill_n(&d[5 * 32], 32, 1);
    std::vector<uint64_t> w(n * wps);
    bool full = false, surplus = false;
    const bool got = pack_present_words(d.data(), c.data(), m, n, w.data(), &full);
    for (size_t b = 0; b < n; ++b) {
      const uint64_t w0 = pack_flags(&d[b * 32], 32) | (pack_flags(&c[b * m], 32) << 32);
      CHECK(w[wps * b] == w0, "pack_present_words word 0 (m=%zu)", m);
      if (wps == 2) CHECK(w[2 * b + 1] == pack_flags(&c[b * m + 32], m - 32), "pack_present_words word 1 (m=%zu)", m);
      surplus |= count_flags(&d[b * 32], 32) + count_flags(&c[b * m], m) > 32;
    }
    CHECK(got == surplus && full, "pack_present_words flags (m=%zu)", m);
  }
}

static void check_classify(std::mt19937_64& rng) {
  check_classify_table();
  check_classify_random(rng);
}

int main() {
  std::mt19937_64 rng(0xA19E);
  check_flags(rng);
  check_invert(rng);
  check_x32();
  check_syn(rng);
  check_corr(rng);
  check_windows(rng);
  check_classify(rng);
  check_present_words(rng);
  if (g_fail) return 1;
  std::printf("ok\n");
  return 0;
}
