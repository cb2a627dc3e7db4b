// ReedSolomonCoder batches whose slices have their own shred sizes (gfx950 / CDNA4):
// ag_rs_coder_shred_batch_var / ag_rs_coder_deshred_batch_var, RegularShredder's 32:32.
//
// The code works column by column (one 64-byte chunk across the 32 shards of a window half),
// and a column needs only its slice's base address, shard stride and tail length.  Slice b has
// cols_b = ceil(S_b / 64) columns; col_base[0 .. n] is their prefix sum (VarParams).  A tile of
// 64 (encode) or 32 (window decode) consecutive columns finds the slice of its first column
// with one wave-uniform binary search in col_base; its lanes then walk forward from there (at
// most one step per column of the tile: every slice has at least one column).
//
// Kernels
//   var_pad_kernel     coder_pad_kernel with the data region 32 * S_b of each slice
//   var_encode_kernel  xform_kernel<32, 0>'s 32-point HighRate encode; lane = one whole
//                      column; optional per-slice store masks (the deshred's re-encode)
//   var_decode_kernel  decode_h8_kernel<-1, 0, 0, 0>'s W = 64 per-lane window decode with the
//                      fused coding restore
//   var_strip_kernel   coder_strip_kernel with the data region 32 * S_b
//
// Tail chunks: the last column of a slice with T_b = S_b mod 64 != 0 is the crate's split tail
// (T/2 low bytes, then T/2 high bytes).  T differs from lane to lane here, so
// var_load_tail / var_store_tail are per-lane forms of load_tail_chunk / store_tail_chunk:
// 16-byte windows for T >= 16 that start where their run starts (the memory system does the
// large shifts) with the last one moved down to end at T and shifted per lane over registers
// (shr_bytes_pl), 2-byte parts for a shorter tail; every access stays inside [0, T) of its shard.  All even T from 2 to 62 run in
// place on both the encode and the decode side.
#include <hip/hip_runtime.h>

#include "rs_device.hpp"
#include "rs_launch.hpp"
#include "rs_xform.hpp"
#include "unaligned.hpp"

namespace ag {
namespace {

using dev::static_for;

// ---- column table -------------------------------------------------------------------

// The slice of column c < col_base[n]: the largest b with col_base[b] <= c.  Wave-uniform c
// (the loads of col_base are uniform).
__device__ __forceinline__ uint32_t var_find(const uint32_t* __restrict__ cb, uint32_t n, uint32_t c) {
  uint32_t lo = 0, hi = n;  // cb[lo] <= c < cb[hi]
  while (hi - lo > 1) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (cb[mid] <= c) lo = mid;
    else hi = mid;
  }
  return lo;
}

struct VarLane {
  uint64_t off;  // byte offset of this lane's chunk in shard 0 of its slice's codeword
  uint32_t blk;  // slice
  uint32_t S;    // shard stride = shred size of the slice
  uint32_t T;    // != 0: the chunk is the slice's tail chunk of T bytes
  bool ok;       // the column exists
};
// Column c0 + i of the batch (c0 wave-uniform, i < 64 per lane).
__device__ __forceinline__ VarLane var_lane(const VarParams& p, uint32_t c0, uint32_t i) {
  VarLane g{};
  const uint32_t gc = c0 + i;
  g.ok = gc < p.total_columns;
  if (!g.ok) return g;
  uint32_t b = var_find(p.col_base, p.nslices, __builtin_amdgcn_readfirstlane(c0));
  uint32_t next = p.col_base[b + 1];
  while (gc >= next) next = p.col_base[++b + 1];  // <= i steps; col_base[n] = total_columns > gc
  const uint32_t first = p.col_base[b];
  const uint32_t col = gc - first;
  g.blk = b;
  g.S = p.sizes[b];
  g.T = col + 1 == next - first ? g.S % 64 : 0;
  g.off = static_cast<uint64_t>(b) * p.stride + static_cast<uint64_t>(col) * 64;
  return g;
}

// ---- per-lane byte shifts ---------------------------------------------------------------

// out[0 .. NO) = bytes [j, j + 4 NO) of the NI-word little-endian value `in`, zeros past its
// end; j < 4 << STAGES differs per lane: a barrel shift over words (bit selects), then one
// v_alignbyte_b32 per output word.
template <int NI, int NO, int STAGES>
__device__ __forceinline__ void shr_bytes_pl(const uint32_t* in, uint32_t j, uint32_t* out) {
  constexpr int N = NO + (1 << STAGES);
  uint32_t t[N + 1];
  static_for<N + 1>([&](auto I) {
    constexpr int i = decltype(I)::value;
    if constexpr (i < NI) t[i] = in[i];
    else t[i] = 0u;
  });
  const uint32_t w = j >> 2;
  static_for<STAGES>([&](auto K) {
    constexpr int s = 1 << (STAGES - 1 - decltype(K)::value);
    // (bit selects, not ?: on array elements: LLVM turns those into one load through a
    // selected address, which sends the array to scratch)
    const uint32_t m = (w & s) ? ~0u : 0u;
    static_for<N + 1>([&](auto I) {  // ascending: t[i + s] is still this stage's input
      constexpr int i = decltype(I)::value;
      if constexpr (i + s <= N) t[i] = dev::bfi(m, t[i + s], t[i]);
      else t[i] &= ~m;
    });
  });
  const uint32_t b = j & 3;
  static_for<NO>([&](auto I) {
    constexpr int i = decltype(I)::value;
    out[i] = __builtin_amdgcn_alignbyte(t[i + 1], t[i], b);
  });
}
// keep the low `len` bytes of the WORDS-word value v (len per lane)
template <int WORDS>
__device__ __forceinline__ void keep_bytes_pl(uint32_t* v, uint32_t len) {
  static_for<WORDS>([&](auto K) {
    constexpr int k = decltype(K)::value;
    const int keep = static_cast<int>(len) - 4 * k;
    const uint32_t m = keep >= 4 ? ~0u : keep <= 0 ? 0u : (1u << (8 * keep)) - 1;
    v[k] &= m;
  });
}

// One lane's tail chunk of T bytes (2 <= T < 64, even, per lane; h = T / 2 symbols) as raw
// chunk words v[16]: low bytes of symbols 0..31 in words 0..7, high bytes in 8..15, symbols >= h
// zero.  The tail holds its h low bytes then its h high bytes.  load_tail_chunk's windows with
// the memory system doing the large shifts (a window starts where its run starts) and a per-lane
// shift of under 16 bytes only for the window that has to end at T.
__device__ __forceinline__ void var_load_tail(const uint8_t* src, uint32_t T, uint32_t* v) {
  const uint32_t h = T / 2;
  auto ld = [&](uint32_t off, uint32_t* out) __attribute__((always_inline)) {
    const uint4 x = ld16u(src + off);
    out[0] = x.x; out[1] = x.y; out[2] = x.z; out[3] = x.w;
  };
  static_for<16>([&](auto I) { v[decltype(I)::value] = 0u; });
  uint32_t w[4] = {0u, 0u, 0u, 0u};
  if (T >= 32) {  // low [0, 16) [16, h), high [0, 16) at h and [16, h) from the last window
    ld(0, v);
    ld(16, v + 4);
    ld(h, v + 8);
    ld(T - 16, w);
    shr_bytes_pl<4, 4, 3>(w, 32 - h, v + 12);  // high byte 16 sits at 32 - h (1 .. 16) of the window
    keep_bytes_pl<4>(v + 4, h - 16);
    keep_bytes_pl<4>(v + 12, h - 16);
  } else if (T >= 16) {  // low [0, h) from the first window, high [0, h) at 16 - h of the last
    ld(0, v);
    ld(T - 16, w);
    shr_bytes_pl<4, 4, 2>(w, 16 - h, v + 8);  // 1 .. 8
    keep_bytes_pl<4>(v, h);
    keep_bytes_pl<4>(v + 8, h);
  } else {  // 2-byte parts (static word indices: T differs per lane)
    static_for<7>([&](auto I) {
      constexpr uint32_t i = decltype(I)::value;
      if (2 * i < T) w[i / 2] |= ld2u(src + 2 * i) << (16 * (i & 1));
    });
    static_for<4>([&](auto I) { v[decltype(I)::value] = w[decltype(I)::value]; });
    shr_bytes_pl<4, 4, 1>(w, h, v + 8);  // h <= 7
    keep_bytes_pl<4>(v, h);
    keep_bytes_pl<4>(v + 8, h);
  }
}
// The inverse: the T bytes of a tail chunk from raw chunk words (symbols >= h are ignored).
// Every access lies inside [0, T).  For T >= 32 the low run's second window also covers bytes
// [h, 32), which the high run's first window (stored after it by the same lane) rewrites; all
// other overlapping windows carry equal bytes.
__device__ __forceinline__ void var_store_tail(uint8_t* dst, uint32_t T, const uint32_t* v) {
  const uint32_t h = T / 2;
  auto st = [&](uint32_t off, const uint32_t* x) __attribute__((always_inline)) {
    st16u(dst + off, make_uint4(x[0], x[1], x[2], x[3]));
  };
  if (T >= 32) {
    st(0, v);       // low [0, 16)
    st(16, v + 4);  // low [16, h)
    st(h, v + 8);   // high [0, 16) at [h, h + 16)
    uint32_t w[4];
    shr_bytes_pl<8, 4, 2>(v + 8, h - 16, w);  // high [h - 16, h) at [T - 16, T)
    st(T - 16, w);
    return;
  }
  // T < 32: the tail as one value X = low [0, h) ++ high [0, h); the high bytes move up by h
  // (bytes [16 - h, 32 - h) of 16 zero bytes ++ high)
  uint32_t lo[4] = {v[0], v[1], v[2], v[3]}, X[8];
  keep_bytes_pl<4>(lo, h);
  const uint32_t z[8] = {0u, 0u, 0u, 0u, v[8], v[9], v[10], v[11]};
  if (T >= 16) {
    shr_bytes_pl<8, 4, 2>(z, 16 - h, X);          // 1 .. 8
    shr_bytes_pl<4, 4, 2>(v + 8, 16 - h, X + 4);  // high [16 - h, 16) at byte 16
    static_for<4>([&](auto I) { X[decltype(I)::value] |= lo[decltype(I)::value]; });
    uint32_t w[4];
    shr_bytes_pl<8, 4, 2>(X, T - 16, w);  // 0 .. 15
    st(0, X);
    st(T - 16, w);
  } else {
    shr_bytes_pl<8, 4, 2>(z, 16 - h, X);  // 9 .. 15
    static_for<4>([&](auto I) { X[decltype(I)::value] |= lo[decltype(I)::value]; });
    static_for<7>([&](auto I) {
      constexpr uint32_t i = decltype(I)::value;
      if (2 * i < T) st2u(dst + 2 * i, X[i / 2] >> (16 * (i & 1)));
    });
  }
}

// this lane's whole chunk of one shard -> bit planes (a tail chunk when T != 0)
__device__ __forceinline__ void var_load_planes(const uint8_t* src, uint32_t T, uint32_t* v) {
  if (T) {
    var_load_tail(src, T, v);
  } else {
    static_for<4>([&](auto Q) {
      constexpr int q = decltype(Q)::value;
      const uint4 x = ld16u(src + 16 * q);
      v[4 * q] = x.x;
      v[4 * q + 1] = x.y;
      v[4 * q + 2] = x.z;
      v[4 * q + 3] = x.w;
    });
  }
  dev::planes_from_raw(v);
}
__device__ __forceinline__ void var_store_planes(uint8_t* dst, uint32_t T, const uint32_t* planes) {
  uint32_t v[16];
  static_for<16>([&](auto P) { v[decltype(P)::value] = planes[decltype(P)::value]; });
  dev::transpose8(v);
  dev::transpose8(v + 8);
  if (T) {
    var_store_tail(dst, T, v);
  } else {
    static_for<4>([&](auto Q) {
      constexpr int q = decltype(Q)::value;
      st16u(dst + 16 * q, make_uint4(v[4 * q], v[4 * q + 1], v[4 * q + 2], v[4 * q + 3]));
    });
  }
}

// ---- padding writer and strip ----------------------------------------------------------

// coder_pad_kernel (rs_coder_kernels.hip) with the data region 32 * sizes[b] of each slice: with a
// payload source one workgroup copies one slice (the piece holding byte `len` merged with 0x80
// 00..); in place only the pieces from that one on are written, one wave per slice.
__global__ __launch_bounds__(256) void var_pad_kernel(const uint8_t* __restrict__ payload, uint64_t payload_stride,
                                                      const uint32_t* __restrict__ lens,
                                                      const uint32_t* __restrict__ sizes, uint8_t* cw,
                                                      uint64_t cw_stride, uint64_t nslices) {
  const uint64_t b = payload ? blockIdx.x : static_cast<uint64_t>(blockIdx.x) * 4 + (threadIdx.x >> 6);
  if (b >= nslices) return;
  const uint32_t tid = payload ? threadIdx.x : (threadIdx.x & 63), nt = payload ? blockDim.x : 64;
  const uint32_t per = 32 * sizes[b] / 16;
  const uint32_t len = lens[b];
  uint8_t* base = cw + b * cw_stride;
  const uint8_t* src = payload ? payload + b * payload_stride : nullptr;
  for (uint32_t piece = (src ? 0u : len / 16) + tid; piece < per; piece += nt) {
    const uint32_t j = piece * 16;
    uint8_t* dst = base + j;
    if (j + 16 <= len) {  // whole payload piece (only with a source)
      st16u(dst, ld16u(src + j));
      continue;
    }
    if (j >= len + 1) {  // padding zeros only
      st16u(dst, make_uint4(0, 0, 0, 0));
      continue;
    }
    uint8_t v[16];
    for (int i = 0; i < 16; ++i) {
      const uint32_t pos = j + i;
      v[i] = pos < len ? (src ? src[pos] : dst[i]) : (pos == len ? 0x80 : 0);
    }
    for (int i = 0; i < 16; ++i) dst[i] = v[i];
  }
}

// coder_strip_kernel with the data region 32 * sizes[b]: out[b] = the index of the 0x80 marker
// (the payload length), or -1.  One wave per slice, 1 KiB windows from the end.
__global__ __launch_bounds__(256) void var_strip_kernel(const uint8_t* __restrict__ cw, uint64_t cw_stride,
                                                        const uint32_t* __restrict__ sizes, uint64_t nslices,
                                                        int64_t* out) {
  const uint64_t b = static_cast<uint64_t>(blockIdx.x) * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (b >= nslices) return;  // wave-uniform
  const uint8_t* d = cw + b * cw_stride;
  const int64_t data_bytes = 32 * static_cast<int64_t>(sizes[b]);  // % 64 == 0
  int64_t found = -1;
  for (int64_t hi = data_bytes; hi > 0 && found < 0; hi -= 1024) {
    const int64_t i0 = hi - 1024 + 16 * static_cast<int64_t>(lane);
    int32_t last = -1;  // highest nonzero byte of this lane's piece
    if (i0 >= 0) {
      const uint4 x = ld16u(d + i0);
      const uint32_t w[4] = {x.x, x.y, x.z, x.w};
      for (int q = 0; q < 4; ++q)
        if (w[q]) last = 4 * q + (31 - __builtin_clz(w[q])) / 8;
    }
    const uint64_t any = __builtin_amdgcn_ballot_w64(last >= 0);
    if (any) {
      const int top = 63 - __builtin_clzll(any);
      const int32_t l = __shfl(last, top);
      found = hi - 1024 + 16 * top + l;
    }
  }
  if (lane == 0) out[b] = (found < 0 || d[found] != 0x80) ? -1 : found;
}

// ---- 32-point HighRate encode over the column table ------------------------------------

// xform_kernel<32, 0> (rs_tile64.hip) with lane = one whole column of the batch: 4 waves x
// 64 lanes, wave w owns data shards 8 w + t in passes A and C.  out_mask (optional): one word
// per slice, bit s set => coding shard s is stored; a tile whose slices store nothing exits
// before loading.
__global__ __launch_bounds__(256, 2) void var_encode_kernel(const VarParams p) {
  __shared__ uint4 lds[16 * 4 * kXfLanes];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const uint32_t tile = dev::xcd_tile(blockIdx.x, gridDim.x);
  const VarLane g = var_lane(p, tile * kXfLanes, lane);
  uint32_t mask = g.ok ? 0xFFFFFFFFu : 0u;
  if (p.out_mask && g.ok) mask = static_cast<uint32_t>(p.out_mask[g.blk]);
  // (every wave holds the same columns: the exit is uniform over the workgroup)
  if (__builtin_amdgcn_ballot_w64(mask != 0) == 0) return;
  const uint8_t* in = p.cw + g.off;
  Regs8 ra;
  static_for<8>([&](auto T) {
    constexpr int t = decltype(T)::value;
    const uint32_t s = 8 * wave + t;
    if (g.ok) var_load_planes(in + static_cast<uint64_t>(s) * g.S, g.T, ra[t]);
    else static_for<16>([&](auto P) { ra[t][decltype(P)::value] = 0u; });
  });
  xf_pass_a<32>(wave, ra);
  Regs8 rb;
  xf_exchange_ab(wave, lane, lds, ra, rb);
  xf_pass_b<32, 0>(rb);
  xf_exchange_bc(wave, lane, lds, rb, ra);
  const uint32_t mine = (mask >> (8 * wave)) & 0xFFu;  // this wave's coding shards
  if (__builtin_amdgcn_ballot_w64(mine != 0) == 0) return;
  xf_pass_c<0>(wave, ra);
  uint8_t* out = p.cw + g.off + 32ull * g.S;
  static_for<8>([&](auto T) {
    constexpr int t = decltype(T)::value;
    const uint32_t s = 8 * wave + t;
    if ((mine >> t) & 1) var_store_planes(out + static_cast<uint64_t>(s) * g.S, g.T, ra[t]);
  });
}

// ---- W = 64 window decode over the column table ----------------------------------------

// decode_h8_kernel<-1, 0, 0, 0> (rs_window.hip: layouts A .. E, the swaps' epoch flags, the
// formal derivative) for HighRate 32:32 with the fused coding restore: window position j < 32
// is coding shred j, 32 + i data shred i.  32-column tiles; lanes l and l + 32 hold column
// l & 31.  pmask [slice][2]: positions loaded, positions restored; rows [slice][64]: the
// polynomial-basis locator constants (decode_rows_kernel), staged in LDS for the <= 32 slices
// of the tile.
__global__ __launch_bounds__(512, 4) void var_decode_kernel(const VarParams p) {
  constexpr int W = 64, kCols = 32;
  __shared__ uint4 lds[16 * 4 * kXfLanes];  // 8 waves x 2 slots x 4 KiB
  __shared__ X8Flags flags;
  __shared__ uint32_t lcoef[kCols * W];
  const int lane = threadIdx.x & 63;
  const int h = lane >> 5;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const uint32_t tile = dev::xcd_tile(blockIdx.x, gridDim.x);
  const uint32_t c0 = tile * kCols;
  const uint32_t c1 = c0 + kCols - 1 < p.total_columns ? c0 + kCols - 1 : p.total_columns - 1;
  const uint32_t sb0 = var_find(p.col_base, p.nslices, c0);
  {
    const uint32_t nbt = var_find(p.col_base, p.nslices, c1) - sb0 + 1;  // <= 32
    for (uint32_t i = threadIdx.x; i < nbt * W; i += blockDim.x)
      lcoef[i] = p.rows[static_cast<uint64_t>(sb0 + i / W) * W + i % W];
  }
  if (threadIdx.x < 16) reinterpret_cast<uint32_t*>(&flags)[threadIdx.x] = 0;
  __syncthreads();
  const VarLane g = var_lane(p, c0, lane & 31);
  const uint64_t in_mask = g.ok ? p.pmask[2 * static_cast<uint64_t>(g.blk)] : 0;
  const uint64_t out_mask = g.ok ? p.pmask[2 * static_cast<uint64_t>(g.blk) + 1] : 0;
  const uint32_t* coef = lcoef + (g.ok ? g.blk - sb0 : 0u) * W;
  // window position j of this lane's column: coding shred j (j < 32) or data shred j - 32
  auto shard = [&](uint32_t j) -> uint8_t* {
    return p.cw + g.off + static_cast<uint64_t>(j < 32 ? 32 + j : j - 32) * g.S;
  };
  auto posA = [&](int t) -> uint32_t {
    return static_cast<uint32_t>((t & 1) | ((t >> 1) << 1) | (h << 2) | (wave << 3));
  };
  Regs4 r;
  static_for<4>([&](auto T) {
    constexpr int t = decltype(T)::value;
    const uint32_t j = posA(t);
    if ((in_mask >> j) & 1) {
      var_load_planes(shard(j), g.T, r[t]);
      dev::mul_rt_poly(r[t], coef[j]);
    } else {
      static_for<16>([&](auto P) { r[t][decltype(P)::value] = 0; });
    }
  });
  // IFFT_64
  h8_layer0<true, 0>(wave, h, r);
  h8_relayout(r);
  x8_layer_t<LB, 1, true, 0>(wave, r);
  x8_layer_t<LB, 2, true, 0>(wave, r);
  x8_swap<1, 0, 1>(wave, lane, lds, &flags, r);
  x8_layer_t<LC, 3, true, 0>(wave, r);
  x8_swap<0, 1, 2>(wave, lane, lds, &flags, r);
  x8_layer_t<LD, 4, true, 0>(wave, r);
  x8_swap<1, 2, 3>(wave, lane, lds, &flags, r);
  x8_layer_t<LE, 5, true, 0>(wave, r);
  // formal derivative in E (decode_h8_kernel): each wave publishes its two pre-derivative
  // slots of round rho in its own region; the waves with a wave bit b clear add the region of
  // their partner w | 2^b
  auto wait_readers = [&](int x, uint32_t e) __attribute__((always_inline)) {
    static_for<3>([&](auto Bb) {
      constexpr int b = decltype(Bb)::value;
      if ((x >> b) & 1) x8_wait_ge(&flags.done[x & ~(1 << b)], e);
    });
  };
  static_for<2>([&](auto Rho) {
    constexpr int rho = decltype(Rho)::value;
    constexpr uint32_t e = 4 + rho;
    if constexpr (rho == 1) wait_readers(wave, e - 1);  // round 0's readers of this region
    static_for<2>([&](auto U) { lds_put(lds, 2 * wave + decltype(U)::value, lane, r[2 * rho + decltype(U)::value]); });
    x8_signal(&flags.ready[wave], e, lane);
    static_for<2>([&](auto U) {
      constexpr int t = 2 * rho + decltype(U)::value;
      // p0 term: the lower half (p0 clear) adds the upper half's pre-derivative value
      uint32_t hi[16];
      static_for<16>([&](auto P) {
        constexpr int q = decltype(P)::value;
        hi[q] = __builtin_amdgcn_permlane32_swap(r[t][q], 0u, false, false)[1];
      });
      // slot bits, ascending t: partners t | 1, t | 2 > t still hold pre-derivative values
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
  // FFT_64, ending in A.  The first swap writes the partner's region: its last derivative
  // round's readers must be done with it.
  x8_layer_t<LE, 5, false, 0>(wave, r);
  x8_layer_t<LE, 4, false, 0>(wave, r);
  wait_readers(wave ^ 4, 5);
  x8_swap<1, 2, 6>(wave, lane, lds, &flags, r);
  x8_layer_t<LD, 3, false, 0>(wave, r);
  x8_swap<0, 1, 7>(wave, lane, lds, &flags, r);
  x8_layer_t<LC, 2, false, 0>(wave, r);
  x8_swap<1, 0, 8>(wave, lane, lds, &flags, r);
  x8_layer_t<LB, 1, false, 0>(wave, r);
  // the store predicates, packed before the first store (bit t: slot t restores its position)
  uint32_t qall = 0;
  static_for<4>([&](auto T) { qall |= static_cast<uint32_t>((out_mask >> posA(decltype(T)::value)) & 1) << decltype(T)::value; });
  if (__builtin_amdgcn_ballot_w64(qall != 0) == 0) return;  // nothing to restore in this wave
  h8_relayout(r);
  h8_layer0<false, 0>(wave, h, r);
  static_for<4>([&](auto T) {
    constexpr int t = decltype(T)::value;
    const uint32_t j = posA(t);
    if ((qall >> t) & 1) {
      dev::mul_rt_poly(r[t], coef[j]);
      var_store_planes(shard(j), g.T, r[t]);
    }
  });
}

}  // namespace

hipError_t launch_var_pad(const uint8_t* payload, uint64_t payload_stride, const uint32_t* lens, const uint32_t* sizes,
                          uint8_t* cw, uint64_t cw_stride, uint64_t nslices, hipStream_t stream) {
  if (nslices == 0) return hipSuccess;
  if (nslices > 0x7FFFFFFFull) return hipErrorInvalidValue;
  const uint64_t groups = payload ? nslices : (nslices + 3) / 4;
  hipLaunchKernelGGL(var_pad_kernel, dim3(static_cast<unsigned>(groups)), dim3(256), 0, stream, payload,
                     payload_stride, lens, sizes, cw, cw_stride, nslices);
  return hipGetLastError();
}

hipError_t launch_var_strip(const uint8_t* cw, uint64_t cw_stride, const uint32_t* sizes, uint64_t nslices,
                            int64_t* out, hipStream_t stream) {
  if (nslices == 0) return hipSuccess;
  const uint64_t groups = (nslices + 3) / 4;  // one wave per slice
  if (groups > 0x7FFFFFFFull) return hipErrorInvalidValue;
  hipLaunchKernelGGL(var_strip_kernel, dim3(static_cast<unsigned>(groups)), dim3(256), 0, stream, cw, cw_stride,
                     sizes, nslices, out);
  return hipGetLastError();
}

hipError_t launch_var_encode(const VarParams& p, hipStream_t stream) {
  if (p.total_columns == 0) return hipSuccess;
  const uint32_t tiles = (p.total_columns + kXfLanes - 1) / kXfLanes;
  hipLaunchKernelGGL(var_encode_kernel, dim3(tiles), dim3(256), 0, stream, p);
  return hipGetLastError();
}

hipError_t launch_var_decode(const VarParams& p, hipStream_t stream) {
  if (p.total_columns == 0) return hipSuccess;
  const uint32_t tiles = (p.total_columns + 31) / 32;
  hipLaunchKernelGGL(var_decode_kernel, dim3(tiles), dim3(512), 0, stream, p);
  return hipGetLastError();
}

}  // namespace ag
