// decode_pk's tile body (the packed W = 64 window decoder) with its LDS lists, the per-call
// server's locator tables and the Z/65535 Walsh helpers of the locator route.  Shared by
// decode_pk_kernel's grid and decode_rows (rs_window.hip) and the per-call server's
// random-arrival job (rs_tile64.hip).  gfx950 / CDNA4 only.
#pragma once
#include <hip/hip_runtime.h>

#include "rs_device.hpp"
#include "rs_launch.hpp"
#include "rs_xform.hpp"

namespace ag {
namespace {

using dev::static_for;

__device__ __forceinline__ uint32_t m65535_add(uint32_t a, uint32_t b) {
  const uint32_t s = a + b;
  return s >= 65535u ? s - 65535u : s;
}
__device__ __forceinline__ uint32_t m65535_sub(uint32_t a, uint32_t b) { return a >= b ? a - b : a + 65535u - b; }
__device__ __forceinline__ uint32_t m65535_mul(uint32_t a, uint32_t b) {  // canonical a, b < 65535
  const uint32_t p = a * b;
  uint32_t s = (p & 0xFFFFu) + (p >> 16);  // 2^16 = 1 (mod 65535)
  s = (s & 0xFFFFu) + (s >> 16);
  return s >= 65535u ? s - 65535u : s;
}
// the unnormalised Walsh transform over the 64 lanes (one residue per lane)
__device__ __forceinline__ uint32_t walsh64(uint32_t v, int lane) {
  static_for<6>([&](auto B) {
    constexpr int d = 1 << decltype(B)::value;
    const uint32_t o = static_cast<uint32_t>(__shfl_xor(static_cast<int>(v), d));
    v = (lane & d) ? m65535_sub(o, v) : m65535_add(v, o);
  });
  return v;
}
// 128 points: position lane in v0, lane + 64 in v1
__device__ __forceinline__ void walsh128(uint32_t& v0, uint32_t& v1, int lane) {
  v0 = walsh64(v0, lane);
  v1 = walsh64(v1, lane);
  const uint32_t a = v0;
  v0 = m65535_add(a, v1);
  v1 = m65535_sub(a, v1);
}
__device__ __forceinline__ uint16_t locator_log(uint32_t loc, bool in) {  // exp of +loc (present), -loc (restored)
  return static_cast<uint16_t>(in ? loc : 65535u - loc);
}

// =====================================================================================
// decode_pk<OUTH>: decode_h8's W = 64 window for per-slice patterns on 1 KiB shreds (16 chunks
// per shard: a 32-column tile is two slices) with the locator products packed.  In decode_h8 a
// wave-slot holds four 16-lane groups -- two slices x two positions (lane half) -- and runs the
// per-lane Horner product when ANY group's position is present: with random 32-of-64 arrival
// that is ~94 % of the slots where 50 % carry data, and likewise for the restored outputs.
// Here the products run on packed items instead (item = one slice's 16 columns of one position,
// 1 KiB):
//   1. the workgroup ranks each slice's survivors and restored positions (LDS lists);
//   2. item i of the survivors (i < 64: ANY_K keeps at most 32 per slice) is loaded by row
//      group i & 3 of slot (i >> 2) & 1 of wave i >> 3, bitsliced, multiplied by its locator
//      constant and written to the 64 KiB exchange buffer;
//   3. every lane reads its layout-A slots from there (absent positions are zero) and the
//      transform runs as decode_h8's (swaps, derivative, the half-pruned FFT);
//   4. the live waves write their restored positions' values as packed items, and each item is
//      multiplied, converted to bytes and stored by one row group.
// Survivor and restored counts bound the product work instead of the slot count: per 2-slice
// tile 64 input items on 16 wave-slots (decode_h8: ~30 of 32) and the restored items on the
// live waves' 16 wave-slots.  OUTH: the window half of the restored originals (1 HighRate chunk
// 32, 0 the LowRate sub-window); only those geometries launch it.  Requires any_k (at most k
// survivors per pattern) and 16 chunks per shard.
// =====================================================================================
// The transform's multiplies use the subset-greedy programs (TAB 1, rs_device.hpp mul_acc): with
// the cancellation programs this kernel's allocation spills (14 VGPRs).
// The tile body (decode_pk_kernel, and the per-call server's random-arrival job with one slice):
// `lds` is the 64 KiB exchange buffer (packed items [item][q][16 lanes] or swap regions), `sh`
// the tile's lists.  p.pmask / p.rows may address LDS (the server stages them there).
struct PkShared {
  uint32_t lcoef[2 * 64];         // the two slices' locator constants (polynomial basis)
  uint64_t smask[2][2];           // per slice: positions present (loaded), restored
  uint8_t ilist[2][64], olist[2][64];  // per slice: survivor / restored positions by rank
};
// The per-call server's locator tables (built once per server launch): log x for the window's
// 64 positions, and a^i, a^(256 i) (i < 256) in the polynomial basis, where a constant of the
// decoder is to_poly(exp[l]) = a^l (the basis map sends exp[l] to the l-th power of the
// polynomial generator, a^16 = a^5 + a^3 + a^2 + 1; checked for every l by
// tests/test_oracle.py::test_poly_basis_powers) -- so the server needs no table lookups in HBM.
struct PkLocTables {
  uint16_t log64[64];
  uint16_t apow_lo[256], apow_hi[256];
};
__device__ __forceinline__ uint32_t poly_mul(uint32_t a, uint32_t b) {  // GF(2)[a] / (a^16 + a^5 + a^3 + a^2 + 1)
  uint32_t r = 0;
  for (int i = 0; i < 16; ++i) r ^= ((b >> i) & 1) ? a << i : 0u;
  for (int i = 30; i >= 16; --i) r ^= ((r >> i) & 1) ? (1u << i) ^ (0x2Du << (i - 16)) : 0u;
  return r;
}
__device__ __forceinline__ uint32_t poly_pow_a(const PkLocTables& t, uint32_t l) {  // a^l, l <= 65535
  return poly_mul(t.apow_hi[l >> 8], t.apow_lo[l & 255]);
}

// SRV: the per-call server's one-slice job; the locator constants of slice 0 are computed in
// the list phase by wave 0 (decode_rows' Walsh route over `loc`) instead of read from p.rows.
// TAIL: shreds of S = 960 + T bytes (16 <= T < 64): column 15 of an item is the shred's T-byte
// tail, moved whole by its lanes (load_tail_chunk / store_tail_chunk, as decode_h8's TAIL).
template <int OUTH, bool SRV = false, bool TAIL = false>
__device__ __forceinline__ void decode_pk_tile(const DecodeXParams& p, uint32_t tile, uint4* lds, X8Flags* fl,
                                               PkShared& sh, const PkLocTables* loc = nullptr) {
  static_assert(OUTH >= -1 && OUTH <= 1, "OUTH: the restored positions' window half, -1 both");
  constexpr int W = 64, kSl = 16;           // positions, columns per slice
  constexpr int D = 2;                      // derivative epochs 4, 5; FFT swaps 4 + D ..
  X8Flags& flags = *fl;
  uint32_t* lcoef = sh.lcoef;
  auto& smask = sh.smask;
  auto& ilist = sh.ilist;
  auto& olist = sh.olist;
  const int lane = threadIdx.x & 63;
  const int h = lane >> 5;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const uint64_t sb0 = static_cast<uint64_t>(tile) * 2;  // the tile's first slice (block)
  const uint64_t nblk = p.total_columns / kSl;
  const uint32_t opos = p.low_rate ? 0 : p.chunk, rpos = p.low_rate ? p.chunk : 0;
  if (threadIdx.x < 2 * W) {
    const uint32_t sl = threadIdx.x >> 6, j = threadIdx.x & 63;
    uint64_t im = 0, om = 0;
    if (sb0 + sl < nblk) {
      im = p.pmask[2 * (sb0 + sl)];
      om = p.pmask[2 * (sb0 + sl) + 1];
      if constexpr (SRV) {
        // wave 0 (slice 0): loc(x) = sum over erased e != x of log(x ^ e), as H(H(L) H(I)) / 64
        const uint64_t e = ~im;
        const uint32_t hl = m65535_mul(walsh64(j ? loc->log64[j] : 0u, static_cast<int>(j)), 1024u);
        const uint32_t hi = walsh64(static_cast<uint32_t>((e >> j) & 1), static_cast<int>(j));
        const uint32_t acc = walsh64(m65535_mul(hl, hi), static_cast<int>(j));
        lcoef[threadIdx.x] = poly_pow_a(*loc, locator_log(acc, (im >> j) & 1));
      } else if (((im | om) >> j) & 1) {
        lcoef[threadIdx.x] = p.rows[(sb0 + sl) * p.rows_w + j];
      }
    }
    const uint64_t below = (uint64_t{1} << j) - 1;
    if ((im >> j) & 1) ilist[sl][__builtin_popcountll(im & below)] = static_cast<uint8_t>(j);
    if ((om >> j) & 1) olist[sl][__builtin_popcountll(om & below)] = static_cast<uint8_t>(j);
    if (j == 0) {
      smask[sl][0] = im;
      smask[sl][1] = om;
    }
  }
  if (threadIdx.x < 16) reinterpret_cast<uint32_t*>(&flags)[threadIdx.x] = 0;
  __syncthreads();
  const uint64_t imA = smask[0][0], imB = smask[1][0], omA = smask[0][1], omB = smask[1][1];
  const uint32_t nA = static_cast<uint32_t>(__builtin_popcountll(imA));
  const uint32_t nin = nA + static_cast<uint32_t>(__builtin_popcountll(imB));
  const uint32_t noA = static_cast<uint32_t>(__builtin_popcountll(omA));
  const uint32_t nout = noA + static_cast<uint32_t>(__builtin_popcountll(omB));
  if (nout == 0) return;  // nothing restored in either slice (workgroup-uniform)
  const int col = lane & 15, row = lane >> 4;
  const bool tail_lane = TAIL && col == kSl - 1;
  // the byte offset of position g's shard of slice sl, column col (recovery shards below the
  // originals in HighRate)
  auto src_of = [&](uint32_t sl, uint32_t g) -> const uint8_t* {
    const bool is_rec = p.low_rate ? g >= p.chunk : g < p.chunk;
    const uint64_t blk = sb0 + sl;
    return is_rec ? p.rec + (g - rpos) * p.rec_shard_stride + blk * p.rec_block_stride + col * 64
                  : p.orig + (g - opos) * p.orig_shard_stride + blk * p.orig_block_stride + col * 64;
  };
  // 2. packed input products: item i on row group i & 3 of wave (i >> 2) & 7, slot i >> 5 (a
  // one-slice tile's 32 items fill all eight waves' first slot).  Both items' loads are issued
  // before either product (one HBM round trip per wave, not two)
  uint32_t v[2][16];
  static_for<2>([&](auto U) {
    constexpr int u = decltype(U)::value;
    const uint32_t i = u * 32 + wave * 4 + row;
    if (i < nin) {
      const uint32_t sl = i < nA ? 0u : 1u;
      const uint8_t* src = src_of(sl, ilist[sl][i - (sl ? nA : 0u)]);
      if (tail_lane) {
        load_tail_chunk(src, p.tail_bytes, v[u]);
      } else {
        static_for<4>([&](auto Q) {
          constexpr int q = decltype(Q)::value;
          const uint4 x = ld_piece(src + 16 * q);
          v[u][4 * q] = x.x;
          v[u][4 * q + 1] = x.y;
          v[u][4 * q + 2] = x.z;
          v[u][4 * q + 3] = x.w;
        });
      }
    } else {
      static_for<16>([&](auto P) { v[u][decltype(P)::value] = 0; });
    }
  });
  static_for<2>([&](auto U) {
    constexpr int u = decltype(U)::value;
    if (static_cast<uint32_t>(u * 32 + wave * 4) < nin) {  // wave-uniform
      const uint32_t i = u * 32 + wave * 4 + row;
      const bool ok = i < nin;
      const uint32_t sl = i < nA ? 0u : 1u;
      const uint32_t j = ok ? ilist[sl][i - (sl ? nA : 0u)] : 0u;
      dev::planes_from_raw(v[u]);
      dev::mul_rt_poly(v[u], lcoef[sl * W + j]);
      if (ok) {
        static_for<4>([&](auto Q) {
          constexpr int q = decltype(Q)::value;
          lds[(i * 4 + q) * kSl + col] = make_uint4(v[u][4 * q], v[u][4 * q + 1], v[u][4 * q + 2], v[u][4 * q + 3]);
        });
      }
    }
  });
  __syncthreads();
  // 3. layout A from the packed items: lane column c = lane & 31 (slice c >> 4), slot t holds
  // position t | h << 2 | wave << 3
  const uint32_t lsl = static_cast<uint32_t>((lane & 31) >> 4);
  const uint64_t in_mask = lsl ? imB : imA, out_mask = lsl ? omB : omA;
  auto posA = [&](int t) -> uint32_t {
    return static_cast<uint32_t>((t & 1) | ((t >> 1) << 1) | (h << 2) | (wave << 3));
  };
  Regs4 r;
  static_for<4>([&](auto T) {
    constexpr int t = decltype(T)::value;
    const uint32_t j = posA(t);
    if ((in_mask >> j) & 1) {
      const uint32_t i = static_cast<uint32_t>(__builtin_popcountll(in_mask & ((uint64_t{1} << j) - 1))) + (lsl ? nA : 0u);
      static_for<4>([&](auto Q) {
        constexpr int q = decltype(Q)::value;
        const uint4 x = lds[(i * 4 + q) * kSl + col];
        r[t][4 * q] = x.x;
        r[t][4 * q + 1] = x.y;
        r[t][4 * q + 2] = x.z;
        r[t][4 * q + 3] = x.w;
      });
    } else {
      static_for<16>([&](auto P) { r[t][decltype(P)::value] = 0; });
    }
  });
  __syncthreads();  // every item read: the buffer becomes the swap regions
  // IFFT_64
  h8_layer0<true, 0, 1>(wave, h, r);
  h8_relayout(r);
  x8_layer_t<LB, 1, true, 0, 1>(wave, r);
  x8_layer_t<LB, 2, true, 0, 1>(wave, r);
  x8_swap<1, 0, 1, 0xF, false>(wave, lane, lds, &flags, r);
  x8_layer_t<LC, 3, true, 0, 1>(wave, r);
  x8_swap<0, 1, 2, 0xF, false>(wave, lane, lds, &flags, r);
  x8_layer_t<LD, 4, true, 0, 1>(wave, r);
  x8_swap<1, 2, 3, 0xF, false>(wave, lane, lds, &flags, r);
  x8_layer_t<LE, 5, true, 0, 1>(wave, r);
  // formal derivative in E (decode_h8's, epochs 4 and 5)
  auto wait_readers = [&](int x, uint32_t e) __attribute__((always_inline)) {
    static_for<3>([&](auto Bb) {
      constexpr int b = decltype(Bb)::value;
      if ((x >> b) & 1) x8_wait_ge(&flags.done[x & ~(1 << b)], e);
    });
  };
  static_for<2>([&](auto Rho) {
    constexpr int rho = decltype(Rho)::value;
    constexpr uint32_t e = 4 + rho;
    if constexpr (rho == 1) wait_readers(wave, e - 1);
    static_for<2>([&](auto U) { lds_put(lds, 2 * wave + decltype(U)::value, lane, r[2 * rho + decltype(U)::value]); });
    x8_signal(&flags.ready[wave], e, lane);
    static_for<2>([&](auto U) {
      constexpr int t = 2 * rho + decltype(U)::value;
      uint32_t hi[16];
      static_for<16>([&](auto P) {
        constexpr int q = decltype(P)::value;
        hi[q] = __builtin_amdgcn_permlane32_swap(r[t][q], 0u, false, false)[1];
      });
      if constexpr (!(t & 1)) dev::xor_planes(r[t], r[t | 1]);
      if constexpr (!(t & 2)) dev::xor_planes(r[t], r[t | 2]);
      dev::xor_planes(r[t], hi);
    });
    static_for<3>([&](auto Bb) {
      constexpr int b = decltype(Bb)::value;
      if (!((wave >> b) & 1)) {
        const int pw = wave | (1 << b);
        x8_wait_ge(&flags.ready[pw], e);
        static_for<2>([&](auto U) { lds_get_xor(lds, 2 * pw + decltype(U)::value, lane, r[2 * rho + decltype(U)::value]); });
      }
    });
    x8_signal(&flags.done[wave], e, lane);
  });
  // FFT_64 down to A; the waves of the other window half hand over their live slots and retire
  x8_layer_t<LE, 5, false, 0, 1>(wave, r);
  x8_layer_t<LE, 4, false, 0, 1>(wave, r);
  wait_readers(wave ^ 4, 5);
  if constexpr (OUTH < 0) {
    // restored positions in both halves (fused coding restore): every wave finishes the FFT
    x8_swap<1, 2, 4 + D, 0xF, false>(wave, lane, lds, &flags, r);
  } else {
    const int partner = wave ^ 4;
    if (((wave >> 2) & 1) != OUTH) {
      x8_wait_ge(&flags.done[partner], 3 + D);
      static_for<4>([&](auto T) {
        constexpr int t = decltype(T)::value;
        if constexpr (((t >> 1) & 1) == OUTH) {
          lds_put(lds, 2 * partner + (t & 1), lane, r[t]);
          __asm__ volatile("; pk put %0" ::"n"(t));
        }
      });
      x8_signal(&flags.ready[wave], 4 + D, lane);
      return;
    }
    x8_wait_ge(&flags.ready[partner], 4 + D);
    static_for<4>([&](auto T) {
      constexpr int t = decltype(T)::value;
      if constexpr (((t >> 1) & 1) != OUTH) {
        lds_get(lds, 2 * wave + (t & 1), lane, r[t]);
        __asm__ volatile("; pk get %0" ::"n"(t));
      }
    });
    x8_signal(&flags.done[wave], 4 + D, lane);
  }
  x8_layer_t<LD, 3, false, 0, 1>(wave, r);
  x8_swap<0, 1, 5 + D, 0xF, false>(wave, lane, lds, &flags, r);
  x8_layer_t<LC, 2, false, 0, 1>(wave, r);
  x8_swap<1, 0, 6 + D, 0xF, false>(wave, lane, lds, &flags, r);
  x8_layer_t<LB, 1, false, 0, 1>(wave, r);
  h8_relayout(r);
  h8_layer0<false, 0, 1>(wave, h, r);
  // 4. packed output products.  Every live wave's last swap read is done before any item
  // overwrites a region; items written, then every live wave's items visible before reads.
  constexpr int kLive = OUTH < 0 ? 8 : 4;     // live waves: all, or wave bit 2 == OUTH
  constexpr int kHi = OUTH < 0 ? 0 : OUTH << 2;
  const int lw = wave & (kLive - 1);
  static_for<kLive>([&](auto Wv) {
    constexpr int w2 = decltype(Wv)::value;
    x8_wait_ge(&flags.done[w2 | kHi], 6 + D);
  });
  static_for<4>([&](auto T) {
    constexpr int t = decltype(T)::value;
    // recomputed here: otherwise layout A's rank masks stay live across the transform and
    // the fused variant (kLive 8) spills them
    uint32_t j = posA(t);
    __asm__ volatile("" : "+v"(j));
    if ((out_mask >> j) & 1) {
      const uint32_t o = static_cast<uint32_t>(__builtin_popcountll(out_mask & ((uint64_t{1} << j) - 1))) + (lsl ? noA : 0u);
      static_for<4>([&](auto Q) {
        constexpr int q = decltype(Q)::value;
        lds[(o * 4 + q) * kSl + col] = make_uint4(r[t][4 * q], r[t][4 * q + 1], r[t][4 * q + 2], r[t][4 * q + 3]);
      });
    }
  });
  x8_signal(&flags.ready[wave], 7 + D, lane);
  static_for<kLive>([&](auto Wv) {
    constexpr int w2 = decltype(Wv)::value;
    x8_wait_ge(&flags.ready[w2 | kHi], 7 + D);
  });
  // item o on row group o & 3 of live wave (o >> 2) % kLive, slot o / (4 kLive) (the first
  // 4 kLive items spread over every live wave)
  constexpr int kPer = 64 / kLive;  // items per live wave
  static_for<kPer / 4>([&](auto U) {
    constexpr int u = decltype(U)::value;
    if (static_cast<uint32_t>(u * 4 * kLive + lw * 4) < nout) {  // wave-uniform
      const uint32_t o = u * 4 * kLive + lw * 4 + row;
      if (o < nout) {
        const uint32_t sl = o < noA ? 0u : 1u;
        const uint32_t j = olist[sl][o - (sl ? noA : 0u)];
        uint32_t v[16];
        static_for<4>([&](auto Q) {
          constexpr int q = decltype(Q)::value;
          const uint4 x = lds[(o * 4 + q) * kSl + col];
          v[4 * q] = x.x;
          v[4 * q + 1] = x.y;
          v[4 * q + 2] = x.z;
          v[4 * q + 3] = x.w;
        });
        dev::mul_rt_poly(v, lcoef[sl * W + j]);
        if (tail_lane) {
          dev::transpose8(v);
          dev::transpose8(v + 8);
          store_tail_chunk(const_cast<uint8_t*>(src_of(sl, j)), p.tail_bytes, v);
        } else {
          dev::store_chunk<true>(const_cast<uint8_t*>(src_of(sl, j)), v);
        }
      }
    }
  });
}

}  // namespace

}  // namespace ag
