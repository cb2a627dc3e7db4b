// The Reed-Solomon kernels on 64-column tiles (TileIO / tile_io_g, rs_xform.hpp) and the
// per-call server, gfx950 / CDNA4.  What they replace: the reed-solomon-simd 3.1.0 calls inside
// ReedSolomonCoder (encode, decode, re-encode).  Arithmetic: GF(2^16) Leopard additive FFT
// (SURVEY.md App. A).
//
// Kernels
//   xform_kernel       32-point FFT(IFFT(in)), 4 waves x 8 slots, passes A / B / C: HighRate
//                      encode (the headline), LowRate encode / decode per 32-point chunk
//   xform8_kernel      the same transform on 8 waves x 4 slots with epoch-flag swaps (tile body
//                      in rs_xform8.hpp): decode from a full recovery set, small batches
//   xform8_stream_kernel   xform8 with the streamed intake: the 32:32 full-recovery reconstruct
//   decode_x_kernel    W = 32 window decoder on xform_kernel's layout
//   decode_x16_kernel  W = 64 / 128 window decoder on 16 waves x 4 slots, one pattern per tile
//   encode_mc_kernel, decode_syn_kernel   chunk <= 4 (16:4): one wave per tile, no LDS
//   latency_server_kernel   one resident workgroup running single-slice jobs from a host
//                      mailbox: xform8's tiles and decode_pk's tile (rs_decode_pk.hpp)
// These families share one TU because their code depends on it: LLVM specialises the shared
// non-template helpers (tile_io_g, lds_put, ...) on all their callers in the TU before it
// inlines them, so a family compiled apart from the others gets different instructions
// (tools/kernel_isa_diff.py).  The window decoders on 32-column tiles are rs_window.hip.
#include <hip/hip_runtime.h>

#include "rs_decode_pk.hpp"
#include "rs_device.hpp"
#include "rs_launch.hpp"
#include "rs_xform.hpp"
#include "rs_xform8.hpp"

namespace ag {
namespace {

using dev::static_for;

// One 64-chunk tile per workgroup of 4 waves; 64 KiB LDS, two workgroups per CU.
// TAIL 1: shards end in the crate's split tail chunk (XformParams::tail_bytes, rs_xform.hpp).
template <int DIN, int DOUT, int TAIL = 0>
__global__ __launch_bounds__(256, 2) void xform_kernel(const XformParams p) {
  __shared__ uint4 lds[16 * 4 * kXfLanes];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const uint32_t tile = dev::xcd_tile(blockIdx.x, gridDim.x);
  if (p.skip_idle) {  // per-block masks: a tile none of whose blocks stores anything exits
    const uint64_t col = static_cast<uint64_t>(tile) * kXfLanes + lane;
    const uint64_t m = col < p.total_columns ? p.out_mask[col / p.chunks_per_shard] : 0;
    if (__builtin_amdgcn_ballot_w64(m != 0) == 0) return;
  }
  Regs8 ra;
  xf_load_raw<TAIL>(p, tile_io<TAIL>(p, tile, lane, p.in_block_stride), wave, ra);
  // Store-mask words, fetched now so their latency hides under the data loads.  With
  // one pattern for the batch the word is wave-uniform (scalar load).
  uint64_t mask[4] = {~0ull, ~0ull, ~0ull, ~0ull};
  if (p.out_mask) {
    if (!p.pattern_per_block) {
      const uint64_t m = p.out_mask[0];
      mask[0] = mask[1] = mask[2] = mask[3] = m;
    } else {
      const TileIO io = tile_io<TAIL>(p, tile, lane, p.out_block_stride);  // the stores' column order
      static_for<4>([&](auto Q) {
        constexpr int q = decltype(Q)::value;
        mask[q] = p.out_mask[io.blk[q]];
      });
    }
  }

  if constexpr (TAIL == 1) {
    const TileIO in_io = tile_io<TAIL>(p, tile, lane, p.in_block_stride);
    static_for<8>([&](auto T) { tail_fix_all<TAIL>(in_io, ra[decltype(T)::value]); });
  }
  static_for<8>([&](auto T) {
    swap_halves(ra[decltype(T)::value]);
    dev::planes_from_raw(ra[decltype(T)::value]);
  });
  xf_pass_a<DIN>(wave, ra);
  Regs8 rb;
  xf_exchange_ab(wave, lane, lds, ra, rb);
  xf_pass_b<DIN, DOUT>(rb);
  xf_exchange_bc(wave, lane, lds, rb, ra);

  // pass C only where some lane of the wave stores one of its 8 shards (a decode restores
  // only the erased originals)
  const TileIO out_io = tile_io<TAIL>(p, tile, lane, p.out_block_stride);
  const uint32_t qall = qmask_all<8>(out_io, mask, 8 * wave, p.n_out);  // 32 bits: 8 shards x 4 pieces
  if (__builtin_amdgcn_ballot_w64(qall != 0) == 0) return;
  xf_pass_c<DOUT>(wave, ra);
  static_for<8>([&](auto T) {
    constexpr int t = decltype(T)::value;
    const uint32_t s = 8 * wave + t;  // wave-uniform
    const uint32_t q = (qall >> (4 * t)) & 15u;
    // a slot no lane stores skips its planes -> bytes conversion (a decode restores a subset)
    if (s < p.n_out && __builtin_amdgcn_ballot_w64(q != 0) != 0)
      store_shard<false, TAIL>(p.out + s * p.out_shard_stride, out_io, q, ra[t]);
  });
}

template <int DIN, int DOUT, bool HALF = false, int TAIL = 0>
__global__ __launch_bounds__(512, 4) void xform8_kernel(const XformParams p) {
  __shared__ uint4 lds[16 * 4 * kXfLanes];  // 8 waves x 2 slots x 4 KiB
  __shared__ X8Flags flags;
  if (threadIdx.x < 16) reinterpret_cast<uint32_t*>(&flags)[threadIdx.x] = 0;
  __syncthreads();
  xform8_tile<DIN, DOUT, HALF, TAIL>(p, dev::xcd_tile(blockIdx.x, gridDim.x), lds, &flags);
}

// xform8_kernel on the streamed intake (xform8_stream_tile, rs_xform8.hpp): every input shard
// exists, whole chunks, store masks given
template <int DIN, int DOUT, bool HALF>
__global__ __launch_bounds__(512, 4) void xform8_stream_kernel(const XformParams p) {
  __shared__ uint4 lds[16 * 4 * kXfLanes];  // 8 waves x 2 slots x 4 KiB
  __shared__ X8Flags flags;
  if (threadIdx.x < 16) reinterpret_cast<uint32_t*>(&flags)[threadIdx.x] = 0;
  __syncthreads();
  xform8_stream_tile<DIN, DOUT, HALF>(p, dev::xcd_tile(blockIdx.x, gridDim.x), lds, &flags);
}

// =====================================================================================
// decode_x: the crate's HighRate decoder for any erasure pattern,
// bitsliced, over a W = 32 point window (W = next_pow2(chunk + k)):
//   pass A : load present positions (recovery j < chunk, original chunk + i), multiply by
//            the pattern's locator constant (runtime 16x16 GF(2) matrix), IFFT dist 1..4
//   pass B : IFFT dist 8.., formal derivative, FFT ..8
//   pass C : FFT dist 4..1, multiply erased originals by the inverse locator, store
// Position j sits where shard j sits in xform_kernel.  The formal derivative
//   w'[j] = w[j] ^ XOR_{b : bit b of j clear} w[j | 2^b]     (all terms pre-derivative)
// splits in layout B into slot bits (in-lane) and wave bits (partner waves through LDS).
// Pattern constants come from decode_rows_kernel; one pattern per tile (either one
// pattern for the batch, or tiles that never straddle blocks).
// =====================================================================================

// x <- M x for a runtime 16x16 GF(2) matrix (rows[o] bit i = M[o][i], wave-uniform rows) by
// four Russians: per group of 4 input planes, the 16 XOR combinations (11 XORs); output plane
// o is then the XOR of 4 combinations picked by the row's nibbles.  The nibbles are
// wave-uniform, so each pick is one v_movrels (M0 index) instead of 4 bitop3s: 44 + 16 * 5
// VALU per multiply instead of 256 masked XORs (+ the mask extraction).
__device__ __forceinline__ void mul_rt4(uint32_t* x, const uint32_t* __restrict__ rows) {
  uint32_t t0[16], t1[16], t2[16], t3[16];
  auto build = [&](uint32_t* t, uint32_t a, uint32_t b, uint32_t c, uint32_t d) {
    t[0] = 0;
    t[1] = a;
    t[2] = b;
    t[3] = a ^ b;
    t[4] = c;
    t[5] = a ^ c;
    t[6] = b ^ c;
    t[7] = dev::xor3(a, b, c);
    t[8] = d;
    t[9] = a ^ d;
    t[10] = b ^ d;
    t[11] = dev::xor3(a, b, d);
    t[12] = c ^ d;
    t[13] = dev::xor3(a, c, d);
    t[14] = dev::xor3(b, c, d);
    t[15] = dev::xor3(t[3], c, d);
  };
  build(t0, x[0], x[1], x[2], x[3]);
  build(t1, x[4], x[5], x[6], x[7]);
  build(t2, x[8], x[9], x[10], x[11]);
  build(t3, x[12], x[13], x[14], x[15]);
  static_for<16>([&](auto O) {
    constexpr int o = decltype(O)::value;
    const uint32_t r = __builtin_amdgcn_readfirstlane(rows[o]);
    x[o] = dev::xor3(t0[r & 15], t1[(r >> 4) & 15], t2[(r >> 8) & 15]) ^ t3[(r >> 12) & 15];
  });
}

// Formal derivative in layout B (slot t of wave w = position w + 4t).
__device__ __forceinline__ void xf_derivative(int wave, int lane, uint4* lds, Regs8& r) {
  static_for<2>([&](auto Rho) {
    constexpr int rho = decltype(Rho)::value;
    static_for<4>([&](auto U) { lds_put(lds, 4 * wave + decltype(U)::value, lane, r[4 * rho + decltype(U)::value]); });
    __syncthreads();
    // slot bits, ascending t: partners t | 2^tb > t still hold pre-derivative values
    static_for<4>([&](auto U) {
      constexpr int t = 4 * rho + decltype(U)::value;
      static_for<3>([&](auto TB) {
        constexpr int tb = decltype(TB)::value;
        if constexpr (!((t >> tb) & 1)) dev::xor_planes(r[t], r[t | (1 << tb)]);
      });
    });
    // wave bits: partner waves' pre-derivative slots from LDS
    static_for<2>([&](auto B) {  // the two wave bits
      constexpr int b = decltype(B)::value;
      if (!((wave >> b) & 1)) {
        const int pw = wave | (1 << b);
        static_for<4>([&](auto U) { lds_get_xor(lds, 4 * pw + decltype(U)::value, lane, r[4 * rho + decltype(U)::value]); });
      }
    });
    __syncthreads();
  });
}

// PL: per-lane patterns (tiles straddle blocks: shard sizes below 4 KiB, e.g. the 1 KiB
// shreds of the reference's slices).  Every lane then owns one whole 64-byte chunk of one
// block (four 16-byte loads of its own chunk, no lane exchange), reads its block's pattern
// masks and matrices, and multiplies with mul_rt_lane; the transform itself is unchanged
// (its skew constants never depend on the pattern).
template <bool PL = false>
__global__ __launch_bounds__(256, 2) void decode_x_kernel(const DecodeXParams p) {
  constexpr int W = 32;
  __shared__ uint4 lds[16 * 4 * kXfLanes];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const uint32_t tile = dev::xcd_tile(blockIdx.x, gridDim.x);
  uint64_t in_mask, out_mask;
  const uint32_t* rows;
  TileIO io_r, io_o;
  uint64_t off_r = 0, off_o = 0;
  if constexpr (PL) {
    const uint64_t g0 = static_cast<uint64_t>(tile) * kXfLanes;  // wave-uniform: one scalar division
    const uint64_t b0 = g0 / p.chunks_per_shard;
    const uint32_t cc = static_cast<uint32_t>(g0 - b0 * p.chunks_per_shard) + lane;
    const bool ok = g0 + lane < p.total_columns;
    const uint32_t d = ok ? cc / p.chunks_per_shard : 0;
    const uint64_t blk = ok ? b0 + d : 0;
    const uint64_t col = ok ? cc - d * p.chunks_per_shard : 0;
    in_mask = ok ? p.pmask[2 * blk] : 0;
    out_mask = ok ? p.pmask[2 * blk + 1] : 0;
    rows = p.rows + blk * W;  // polynomial-basis constants, one word per position
    off_r = blk * p.rec_block_stride + col * 64;
    off_o = blk * p.orig_block_stride + col * 64;
  } else {
    // tile -> (pattern, address tile)
    uint64_t vtile = tile, pat = 0;
    if (p.per_block) {
      const uint64_t bi = tile / p.tiles_per_block;
      const uint64_t blk = p.block_ids ? p.block_ids[bi] : bi;
      vtile = blk * p.tiles_per_block + (tile - bi * p.tiles_per_block);
      pat = blk;
    }
    in_mask = p.pmask[2 * pat];
    out_mask = p.pmask[2 * pat + 1];
    rows = p.rows + pat * (W * 16);
    io_r = tile_io_g(p.total_columns, p.chunks_per_shard, vtile, lane, p.rec_block_stride);
    io_o = tile_io_g(p.total_columns, p.chunks_per_shard, vtile, lane, p.orig_block_stride);
  }

  Regs8 ra;
  static_for<8>([&](auto T) {
    constexpr int t = decltype(T)::value;
    const uint32_t j = 8 * wave + t;  // wave-uniform
    if ((in_mask >> j) & 1) {          // PL: per lane
      const uint32_t opos = p.low_rate ? 0 : p.chunk, rpos = p.low_rate ? p.chunk : 0;
      const bool is_rec = p.low_rate ? j >= p.chunk : j < p.chunk;
      const uint8_t* base = is_rec ? p.rec + (j - rpos) * p.rec_shard_stride : p.orig + (j - opos) * p.orig_shard_stride;
      static_for<4>([&](auto Q) {
        constexpr int q = decltype(Q)::value;
        const uint8_t* src;
        if constexpr (PL) src = base + (is_rec ? off_r : off_o) + 16 * q;
        else src = base + (is_rec ? io_r.off[q] : io_o.off[q]);
        const uint4 x = ld_piece(src);
        ra[t][4 * q] = x.x;
        ra[t][4 * q + 1] = x.y;
        ra[t][4 * q + 2] = x.z;
        ra[t][4 * q + 3] = x.w;
      });
    } else {
      static_for<16>([&](auto P) { ra[t][decltype(P)::value] = 0; });
    }
  });
  static_for<8>([&](auto T) {
    constexpr int t = decltype(T)::value;
    const uint32_t j = 8 * wave + t;
    if ((in_mask >> j) & 1) {
      if constexpr (!PL) swap_halves(ra[t]);
      dev::planes_from_raw(ra[t]);
      if constexpr (PL) dev::mul_rt_poly(ra[t], rows[j]); else mul_rt4(ra[t], rows + j * 16);
    }
  });
  xf_pass_a<0>(wave, ra);
  Regs8 rb;
  xf_exchange_ab(wave, lane, lds, ra, rb);
  xf_pass_b_ifft<0>(rb);
  xf_derivative(wave, lane, lds, rb);
  xf_pass_b_fft<0>(rb);
  xf_exchange_bc(wave, lane, lds, rb, ra);
  const uint32_t mine = static_cast<uint32_t>(out_mask >> (8 * wave)) & 0xFF;
  if constexpr (PL) {
    if (__builtin_amdgcn_ballot_w64(mine != 0) == 0) return;  // nothing to restore in this wave
  } else {
    if (mine == 0) return;
  }
  xf_pass_c<0>(wave, ra);
  static_for<8>([&](auto T) {
    constexpr int t = decltype(T)::value;
    const uint32_t j = 8 * wave + t;
    if ((out_mask >> j) & 1) {
      uint8_t* dst = p.orig + (j - (p.low_rate ? 0 : p.chunk)) * p.orig_shard_stride;
      if constexpr (PL) {
        dev::mul_rt_poly(ra[t], rows[j]);
        dev::store_chunk(dst + off_o, ra[t]);
      } else {
        mul_rt4(ra[t], rows + j * 16);
        store_shard(dst, io_o, io_o.valid, ra[t]);
      }
    }
  });
}

// =====================================================================================
// decode_x16<PASS, DIN, DOUT>: the window decoder (decode_x's algorithm) on the 16-wave
// layout: 16 waves x 4 slots, one 1024-thread workgroup per CU at 4 waves/SIMD (an 8-wave decode_x
// keeps 8 slots per lane at 216 VGPRs: 2 waves/SIMD, latency-bound).
// Positions by layout (X8Lay: slot bits | wave bits):
//   G0 slots p0 p1 | waves p2 p3 p4 p5   loads + locator multiplies, IFFT b0 b1; FFT b0, stores
//   G1 slots p2 p1 | waves p0 p3 p4 p5   IFFT b2 / FFT b1
//   G2 slots p2 p3 | waves p0 p1 p4 p5   IFFT b3 / FFT b2
//   G3 slots p4 p3 | waves p0 p1 p2 p5   IFFT b4 / FFT b3
//   G4 slots p4 p5 | waves p0 p1 p2 p3   IFFT b5, formal derivative, FFT b5 b4
// The derivative w'[j] = w[j] ^ XOR_{b : bit b of j clear} w[j | 2^b] (pre-derivative terms)
// in G4: slot bits in-lane, wave bits from the partner waves' pre-derivative copies in LDS,
// two slots per round (2 x 128 KiB would not fit).
//
// PASS 0: the W <= 64 window (DIN = DOUT = 0).
// PASS 1 / 2: the W = 128 window as two 64-point passes.  With u_h = IFFT_64 of window half h
// (skew delta 64 h) and P = the derivative without its self term (D = I + P), the crate's
// IFFT_128 -> derivative -> FFT_128 gives output half o as FFT_64,64o(P u_o ^ u_{1-o}): the
// size-128 layer's skew factor (index 63) is zero, so the halves meet only there
// (tests/test_oracle.py pins the identity against the oracle's 128-point decoder).  Pass 1
// (DIN = the other half, DOUT = the output half): IFFT, no derivative, FFT, the partial
// stored unmultiplied.  Pass 2 (DIN = DOUT = the output half): IFFT, P, FFT, + the stored
// partial (in planes), output multiply (linear: one product per restored original).  Loads
// and masks are the pass's loaded half (window positions DIN + j); outputs are window
// positions DOUT + j.  One pattern per tile (tiles never straddle blocks): the constants are
// wave-uniform words, multiplied by the Horner scheme in the polynomial basis with the
// coefficient bits tested on the scalar unit (mul_rt_poly_u: a clear bit costs no VALU).
// Per-lane patterns run on decode_h8.
// =====================================================================================
template <int PASS, int DIN, int DOUT>
__global__ __launch_bounds__(1024, 4) void decode_x16_kernel(const DecodeXParams p) {
  using G0 = X8Lay<0, 1, 2, 3, 4, 5>;
  using G1 = X8Lay<2, 1, 0, 3, 4, 5>;
  using G2 = X8Lay<2, 3, 0, 1, 4, 5>;
  using G3 = X8Lay<4, 3, 0, 1, 2, 5>;
  using G4 = X8Lay<4, 5, 0, 1, 2, 3>;
  static_assert(PASS != 0 || (DIN == 0 && DOUT == 0), "the one-pass window starts at 0");
  static_assert(PASS != 2 || DIN == DOUT, "pass 2 loads its output half");
  __shared__ uint4 lds[32 * 4 * kXfLanes];  // 16 waves x 2 slots x 4 KiB
  __shared__ XFlags<16> flags;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const uint32_t tile = dev::xcd_tile(blockIdx.x, gridDim.x);
  const uint32_t rw = p.rows_w;  // constants per pattern (64 or 128)
  if (threadIdx.x < 32) reinterpret_cast<uint32_t*>(&flags)[threadIdx.x] = 0;
  __syncthreads();
  uint64_t vtile = tile, pat = 0;
  if (p.per_block) {
    const uint64_t bi = tile / p.tiles_per_block;
    const uint64_t blk = p.block_ids ? p.block_ids[bi] : bi;
    vtile = blk * p.tiles_per_block + (tile - bi * p.tiles_per_block);
    pat = blk;
  }
  const uint64_t in_mask = p.pmask[2 * pat];
  const uint64_t out_mask = p.pmask[2 * pat + 1];
  const uint32_t* coef = p.rows + pat * rw + DIN;
  const uint32_t* coef_out = p.rows + pat * rw + DOUT;
  const TileIO io_r = tile_io_g(p.total_columns, p.chunks_per_shard, vtile, lane, p.rec_block_stride);
  const TileIO io_o = tile_io_g(p.total_columns, p.chunks_per_shard, vtile, lane, p.orig_block_stride);
  const uint32_t opos = p.low_rate ? 0 : p.chunk, rpos = p.low_rate ? p.chunk : 0;
  Regs4 r;
  static_for<4>([&](auto T) {
    constexpr int t = decltype(T)::value;
    const uint32_t j = 4 * wave + t;  // G0 position in the pass (wave-uniform)
    if ((in_mask >> j) & 1) {
      const uint32_t g = DIN + j;  // window position (recovery shards below the originals in HighRate)
      const bool is_rec = p.low_rate ? g >= p.chunk : g < p.chunk;
      const uint8_t* base = is_rec ? p.rec + (g - rpos) * p.rec_shard_stride : p.orig + (g - opos) * p.orig_shard_stride;
      static_for<4>([&](auto Q) {
        constexpr int q = decltype(Q)::value;
        const uint4 x = ld_piece(base + (is_rec ? io_r.off[q] : io_o.off[q]));
        r[t][4 * q] = x.x;
        r[t][4 * q + 1] = x.y;
        r[t][4 * q + 2] = x.z;
        r[t][4 * q + 3] = x.w;
      });
    } else {
      static_for<16>([&](auto P) { r[t][decltype(P)::value] = 0; });
    }
  });
  static_for<4>([&](auto T) {
    constexpr int t = decltype(T)::value;
    const uint32_t j = 4 * wave + t;
    if ((in_mask >> j) & 1) {
      swap_halves(r[t]);
      dev::planes_from_raw(r[t]);
      dev::mul_rt_poly_u(r[t], coef[j]);  // wave-uniform constant: scalar-branch Horner
    }
  });
  // IFFT_64 (skew delta DIN)
  x8_layer_t<G0, 0, true, DIN>(wave, r);
  x8_layer_t<G0, 1, true, DIN>(wave, r);
  x8_swap<0, 0, 1>(wave, lane, lds, &flags, r);
  x8_layer_t<G1, 2, true, DIN>(wave, r);
  x8_swap<1, 1, 2>(wave, lane, lds, &flags, r);
  x8_layer_t<G2, 3, true, DIN>(wave, r);
  x8_swap<0, 2, 3>(wave, lane, lds, &flags, r);
  x8_layer_t<G3, 4, true, DIN>(wave, r);
  x8_swap<1, 3, 4>(wave, lane, lds, &flags, r);
  x8_layer_t<G4, 5, true, DIN>(wave, r);
  if constexpr (PASS != 1) {
    // formal derivative in G4 (slot t: position bits p4 = t & 1, p5 = t >> 1; wave bits p0..p3)
    __syncthreads();  // every wave's swap reads are done: the exchange buffer is free
    static_for<2>([&](auto Rho) {
      constexpr int rho = decltype(Rho)::value;
      // slot = 2 * wave + u holds this wave's pre-derivative slot 2 rho + u
      static_for<2>([&](auto U) { lds_put(lds, 2 * wave + decltype(U)::value, lane, r[2 * rho + decltype(U)::value]); });
      // slot-bit terms of slots 2 rho, 2 rho + 1 from pre-derivative partners (ascending t: a
      // partner t | 2^i > t is unmodified; slots 2, 3 are untouched until round 1)
      static_for<2>([&](auto U) {
        constexpr int t = 2 * rho + decltype(U)::value;
        if constexpr (PASS == 2) {
          // P = D ^ I: the partner terms only (the slot's own value stays in LDS for the
          // partner waves; lower slots never need a higher slot's register after this)
          static_for<16>([&](auto P) {
            constexpr int q = decltype(P)::value;
            if constexpr (!(t & 1) && !(t & 2)) r[t][q] = r[t | 1][q] ^ r[t | 2][q];
            else if constexpr (!(t & 1)) r[t][q] = r[t | 1][q];
            else if constexpr (!(t & 2)) r[t][q] = r[t | 2][q];
            else r[t][q] = 0;
          });
        } else {
          if constexpr (!(t & 1)) dev::xor_planes(r[t], r[t | 1]);
          if constexpr (!(t & 2)) dev::xor_planes(r[t], r[t | 2]);
        }
      });
      __syncthreads();
      static_for<4>([&](auto B) {
        constexpr int b = decltype(B)::value;
        if (!((wave >> b) & 1)) {
          const int pw = wave | (1 << b);
          static_for<2>([&](auto U) { lds_get_xor(lds, 2 * pw + decltype(U)::value, lane, r[2 * rho + decltype(U)::value]); });
        }
      });
      __syncthreads();
    });
  }
  // FFT_64 (skew delta DOUT), ending in G0
  x8_layer_t<G4, 5, false, DOUT>(wave, r);
  x8_layer_t<G4, 4, false, DOUT>(wave, r);
  x8_swap<1, 3, 5>(wave, lane, lds, &flags, r);
  x8_layer_t<G3, 3, false, DOUT>(wave, r);
  x8_swap<0, 2, 6>(wave, lane, lds, &flags, r);
  x8_layer_t<G2, 2, false, DOUT>(wave, r);
  x8_swap<1, 1, 7>(wave, lane, lds, &flags, r);
  x8_layer_t<G1, 1, false, DOUT>(wave, r);
  x8_swap<0, 0, 8>(wave, lane, lds, &flags, r);
  const uint32_t mine = static_cast<uint32_t>(out_mask >> (4 * wave)) & 0xF;  // wave-uniform
  if (mine == 0) return;
  x8_layer_t<G0, 0, false, DOUT>(wave, r);
  static_for<4>([&](auto T) {
    constexpr int t = decltype(T)::value;
    const uint32_t j = 4 * wave + t;
    if ((mine >> t) & 1) {
      uint8_t* dst = p.orig + (DOUT + j - opos) * p.orig_shard_stride;
      if constexpr (PASS == 2) {
        // + pass 1's partial, in planes (the youngest memory operation when waited on, as in
        // decode_h8)
        uint32_t o[16];
        static_for<4>([&](auto Q) {
          constexpr int q = decltype(Q)::value;
          const uint4 x = ld_piece(dst + io_o.off[q]);
          o[4 * q] = x.x;
          o[4 * q + 1] = x.y;
          o[4 * q + 2] = x.z;
          o[4 * q + 3] = x.w;
        });
        swap_halves(o);
        dev::planes_from_raw(o);
        dev::xor_planes(r[t], o);
      }
      // the output multiply is linear: pass 1 stores its unmultiplied partial, pass 2 has
      // added it in planes and multiplies once
      if constexpr (PASS != 1) dev::mul_rt_poly_u(r[t], coef_out[j]);
      store_shard(dst, io_o, io_o.valid, r[t]);
    }
  });
}

// =====================================================================================
// encode_mc<C>: multi-chunk HighRate encode for small recovery sets (chunk C = next_pow2(m)
// in {1, 2, 4}, k <= kMcMaxK).  One wave per 64-column tile, no LDS: the wave streams the
// k/C original chunks (next chunk's loads issued before this chunk's math), runs each
// chunk's in-lane IFFT_C (skew delta C*(c+1)), XOR-accumulates, and ends with FFT_C (delta
// 0) on the accumulator -- the crate's HighRate encoder.
// =====================================================================================
constexpr int kMcMaxK = 64;

template <int C>
constexpr int ilog2c() { return C <= 1 ? 0 : 1 + ilog2c<C / 2>(); }

template <int C, int DELTA, bool INV>
__device__ __forceinline__ void xform_lane(uint32_t (&r)[C][16]) {
  constexpr int LC = ilog2c<C>();
  static_for<LC>([&](auto Lx) {
    constexpr int L = INV ? decltype(Lx)::value : LC - 1 - decltype(Lx)::value;  // IFFT ascending
    constexpr int d = 1 << L;
    static_for<C / 2>([&](auto I) {
      constexpr int i = decltype(I)::value;
      constexpr int g = (i / d) * 2 * d;
      constexpr int u = g + i % d;
      bfly<g + d + DELTA - 1, INV>(r[u], r[u + d]);
    });
  });
}

template <int C>
__device__ __forceinline__ void mc_load(const XformParams& p, const TileIO& io, uint32_t s0, uint32_t (&raw)[C][16]) {
  static_for<C>([&](auto T) {
    constexpr int t = decltype(T)::value;
    if (s0 + t < p.n_in) {  // wave-uniform
      const uint8_t* base = p.in + (s0 + t) * p.in_shard_stride;
      static_for<4>([&](auto Q) {
        constexpr int q = decltype(Q)::value;
        const uint4 x = ld_piece(base + io.off[q]);
        raw[t][4 * q] = x.x;
        raw[t][4 * q + 1] = x.y;
        raw[t][4 * q + 2] = x.z;
        raw[t][4 * q + 3] = x.w;
      });
    } else {
      static_for<16>([&](auto P) { raw[t][decltype(P)::value] = 0; });
    }
  });
}

template <int C>
__global__ __launch_bounds__(256, 2) void encode_mc_kernel(const XformParams p) {
  constexpr int NCMAX = kMcMaxK / C;
  const int lane = threadIdx.x & 63;
  const uint64_t tile = static_cast<uint64_t>(dev::xcd_tile(blockIdx.x, gridDim.x)) * 4 + (threadIdx.x >> 6);
  if (tile * kXfLanes >= p.total_columns) return;  // whole wave
  const TileIO io = tile_io(p, tile, lane, p.in_block_stride);
  const uint32_t nc = (p.n_in + C - 1) / C;
  uint32_t acc[C][16];
  uint32_t raw[2][C][16];
  mc_load<C>(p, io, 0, raw[0]);
  static_for<NCMAX>([&](auto Cc) {
    constexpr int c = decltype(Cc)::value;
    if (c < nc) {
      if (c + 1 < nc) mc_load<C>(p, io, (c + 1) * C, raw[(c + 1) & 1]);
      auto& cur = raw[c & 1];
      static_for<C>([&](auto T) {
        swap_halves(cur[decltype(T)::value]);
        dev::planes_from_raw(cur[decltype(T)::value]);
      });
      xform_lane<C, C * (c + 1), true>(cur);
      static_for<C>([&](auto T) {
        constexpr int t = decltype(T)::value;
        static_for<16>([&](auto P) {
          constexpr int q = decltype(P)::value;
          if constexpr (c == 0) acc[t][q] = cur[t][q]; else acc[t][q] ^= cur[t][q];
        });
      });
    }
  });
  xform_lane<C, 0, false>(acc);
  const TileIO out_io = tile_io(p, tile, lane, p.out_block_stride);
  static_for<C>([&](auto T) {
    constexpr int t = decltype(T)::value;
    if (t < p.n_out) store_shard(p.out + t * p.out_shard_stride, out_io, out_io.valid, acc[t]);
  });
}

// =====================================================================================
// decode_syn<C>: syndrome decoder for small recovery sets (chunk C = next_pow2(m) <= 4,
// k <= kMcMaxK).  One wave per 64-column tile, no LDS.  The wave re-encodes the present
// originals exactly as encode_mc does (erased originals read as zero), adds e received
// recovery shards (syndromes S_b = received_b ^ re-encoded_b = sum over erased a of
// G[b][a] * original_a) and restores original E[a] = sum_b Minv[a][b] S_b with e^2 runtime
// multiplies.  Any correct decoder returns the crate's originals on a valid codeword (MDS).
// =====================================================================================
typedef uint32_t u32x16 __attribute__((ext_vector_type(16)));

// the 16 XOR combinations of planes x[0..3] (entry v = XOR of x[i] for the bits i of v)
__device__ __forceinline__ u32x16 syn_table(const uint32_t* x) {
  const uint32_t a = x[0], b = x[1], c = x[2], d = x[3];
  const uint32_t ab = a ^ b, cd = c ^ d;
  return u32x16{0u, a, b, ab, c, a ^ c, b ^ c, ab ^ c, d, a ^ d, b ^ d, ab ^ d, cd, a ^ cd, b ^ cd, ab ^ cd};
}

// acc ^= M x for a runtime 16x16 GF(2) matrix in (wave-uniform) global memory
__device__ __forceinline__ void mul_rt_acc(uint32_t* acc, const uint32_t* x, const uint32_t* __restrict__ rows) {
  static_for<16>([&](auto O) {
    constexpr int o = decltype(O)::value;
    const uint32_t r = __builtin_amdgcn_readfirstlane(rows[o]);
    uint32_t a = acc[o];
    static_for<16>([&](auto I) {
      constexpr int i = decltype(I)::value;
      const uint32_t msk = static_cast<uint32_t>(static_cast<int32_t>(r << (31 - i)) >> 31);
      a = __builtin_amdgcn_bitop3_b32(a, x[i], msk, 0x78);  // a ^ (x & msk)
    });
    acc[o] = a;
  });
}

template <int C>
__device__ __forceinline__ void syn_load(const DecodeSynParams& p, const TileIO& io, uint64_t dmask, uint32_t s0,
                                         uint32_t (&raw)[C][16]) {
  static_for<C>([&](auto T) {
    constexpr int t = decltype(T)::value;
    const uint32_t s = s0 + t;
    if (s < p.k && ((dmask >> s) & 1)) {  // wave-uniform
      const uint8_t* base = p.orig + s * p.orig_shard_stride;
      static_for<4>([&](auto Q) {
        constexpr int q = decltype(Q)::value;
        const uint4 x = ld_piece(base + io.off[q]);
        raw[t][4 * q] = x.x;
        raw[t][4 * q + 1] = x.y;
        raw[t][4 * q + 2] = x.z;
        raw[t][4 * q + 3] = x.w;
      });
    } else {
      static_for<16>([&](auto P) { raw[t][decltype(P)::value] = 0; });
    }
  });
}

template <int C>
__global__ __launch_bounds__(256, 2) void decode_syn_kernel(const DecodeSynParams p) {
  constexpr int NCMAX = kMcMaxK / C;
  const int lane = threadIdx.x & 63;
  const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  uint64_t tile = static_cast<uint64_t>(dev::xcd_tile(blockIdx.x, gridDim.x)) * 4 + wave;
  if (tile >= p.ntiles) return;  // whole wave
  uint64_t pat = 0;
  if (p.per_block) {
    const uint64_t bi = tile / p.tiles_per_block;
    const uint64_t blk = p.block_ids ? p.block_ids[bi] : bi;
    tile = blk * p.tiles_per_block + (tile - bi * p.tiles_per_block);
    pat = blk;
  }
  const SynPattern* sp = p.pat + pat;
  const uint64_t dmask = sp->dmask;
  const uint32_t e = sp->e;
  const TileIO io = tile_io_g(p.total_columns, p.chunks_per_shard, tile, lane, p.orig_block_stride);
  const TileIO rio = tile_io_g(p.total_columns, p.chunks_per_shard, tile, lane, p.rec_block_stride);
  const uint32_t nc = (p.k + C - 1) / C;
  // recovery positions used for the syndromes (wave-uniform)
  uint32_t used = 0;
  for (uint32_t b = 0; b < e; ++b) used |= 1u << sp->rec[b];
  // Stage 0 streams the used received recovery shards R (zero elsewhere) and starts the
  // accumulator at IFFT_C,0(R); stages 1..nc stream the present originals' chunks as encode_mc.
  // The final FFT_C,0 then yields re-encoded ^ R = the syndromes at the used positions
  // (linearity), so no dependent recovery load sits between the stream and the correction.
  uint32_t acc[C][16];
  uint32_t raw[2][C][16];
  static_for<C>([&](auto T) {
    constexpr int t = decltype(T)::value;
    if ((used >> t) & 1) {
      const uint8_t* base = p.rec + t * p.rec_shard_stride;
      static_for<4>([&](auto Q) {
        constexpr int q = decltype(Q)::value;
        const uint4 x = ld_piece(base + rio.off[q]);
        raw[0][t][4 * q] = x.x;
        raw[0][t][4 * q + 1] = x.y;
        raw[0][t][4 * q + 2] = x.z;
        raw[0][t][4 * q + 3] = x.w;
      });
    } else {
      static_for<16>([&](auto P) { raw[0][t][decltype(P)::value] = 0; });
    }
  });
  static_for<NCMAX + 1>([&](auto Sg) {
    constexpr int sg = decltype(Sg)::value;
    if (sg <= nc) {
      if (sg < nc) syn_load<C>(p, io, dmask, sg * C, raw[(sg + 1) & 1]);
      auto& cur = raw[sg & 1];
      static_for<C>([&](auto T) {
        swap_halves(cur[decltype(T)::value]);
        dev::planes_from_raw(cur[decltype(T)::value]);
      });
      if constexpr (sg == 0) {
        xform_lane<C, 0, true>(cur);
      } else {
        xform_lane<C, C * sg, true>(cur);
      }
      static_for<C>([&](auto T) {
        constexpr int t = decltype(T)::value;
        static_for<16>([&](auto P) {
          constexpr int q = decltype(P)::value;
          if constexpr (sg == 0) acc[t][q] = cur[t][q]; else acc[t][q] ^= cur[t][q];
        });
      });
    }
  });
  xform_lane<C, 0, false>(acc);  // syndromes S_b at positions rec[b]
  // Four Russians in registers (mul_rt4's scheme): per syndrome b, the 16 XOR combinations
  // of each 4-plane group (44 VALU) serve all e outputs; output plane o of Minv[a][b] S_b is
  // the XOR of 4 entries picked by row o's wave-uniform nibbles (one v_movrels each).
  // Syndromes, tables and outputs stay in VGPRs (2 waves per SIMD: 256 available).
  uint32_t out[C][16];
  static_for<C>([&](auto A) { static_for<16>([&](auto P) { out[decltype(A)::value][decltype(P)::value] = 0; }); });
  // one set of 4 tables reused for every syndrome: LLVM promotes these allocas to VGPRs
  // (dynamic picks = v_movrels) within its promote-alloca budget; a set per syndrome
  // overflows the budget and lands in scratch
  uint32_t t0[16], t1[16], t2[16], t3[16];
  static_for<C>([&](auto J) {
    constexpr int j = decltype(J)::value;
    if ((used >> j) & 1) {
      uint32_t b = 0;
      while (b + 1 < e && sp->rec[b] != j) ++b;  // wave-uniform: the syndrome index of position j
      const uint32_t* x = acc[j];
      auto fill = [&](uint32_t* t, const uint32_t* v) {
        const u32x16 c = syn_table(v);
        static_for<16>([&](auto V) { t[decltype(V)::value] = c[decltype(V)::value]; });
      };
      fill(t0, x);
      fill(t1, x + 4);
      fill(t2, x + 8);
      fill(t3, x + 12);
      static_for<C>([&](auto A) {
        constexpr int a = decltype(A)::value;
        if (a < e) {
          const uint32_t* rows = sp->rows[a][b];
          static_for<16>([&](auto O) {
            constexpr int o = decltype(O)::value;
            const uint32_t r = __builtin_amdgcn_readfirstlane(rows[o]);
            out[a][o] = dev::xor3(out[a][o], t0[r & 15], t1[(r >> 4) & 15]) ^
                        dev::xor3(t2[(r >> 8) & 15], t3[(r >> 12) & 15], 0u);
          });
        }
      });
    }
  });
  static_for<C>([&](auto A) {
    constexpr int a = decltype(A)::value;
    if (a < e) store_shard(p.orig + sp->out[a] * p.orig_shard_stride, io, io.valid, out[a]);
  });
}

}  // namespace

// ---- launchers ----------------------------------------------------------------------
bool xform_supported(unsigned n) { return n == 32 || n == 64; }

hipError_t launch_xform_lowrate(unsigned n, unsigned j, const XformParams& p, hipStream_t stream) {
  if (p.total_columns == 0) return hipSuccess;
  const uint64_t tiles = (p.total_columns + 63) / 64;
  if (tiles > 0x7FFFFFFFull) return hipErrorInvalidValue;
  const dim3 grid(static_cast<unsigned>(tiles));
  if (n == 32) {
    switch (j) {
      case 0: hipLaunchKernelGGL((xform_kernel<0, 32>), grid, dim3(256), 0, stream, p); break;
      case 1: hipLaunchKernelGGL((xform_kernel<0, 64>), grid, dim3(256), 0, stream, p); break;
      case 2: hipLaunchKernelGGL((xform_kernel<0, 96>), grid, dim3(256), 0, stream, p); break;
      case 3: hipLaunchKernelGGL((xform_kernel<0, 128>), grid, dim3(256), 0, stream, p); break;
      default: return hipErrorInvalidValue;
    }
  } else if (n == 64) {
    switch (j) {
      case 0: return launch_xform64(0, 64, p, stream);
      case 1: return launch_xform64(0, 128, p, stream);
      case 2: return launch_xform64(0, 192, p, stream);
      default: return hipErrorInvalidValue;
    }
  } else {
    return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

hipError_t launch_xform_lowrate_decode(unsigned j, const XformParams& p, hipStream_t stream) {
  if (p.total_columns == 0) return hipSuccess;
  const uint64_t tiles = (p.total_columns + 63) / 64;
  if (tiles > 0x7FFFFFFFull) return hipErrorInvalidValue;
  const dim3 grid(static_cast<unsigned>(tiles));
  switch (j) {
    case 0: hipLaunchKernelGGL((xform_kernel<32, 0>), grid, dim3(256), 0, stream, p); break;
    case 1: hipLaunchKernelGGL((xform_kernel<64, 0>), grid, dim3(256), 0, stream, p); break;
    case 2: hipLaunchKernelGGL((xform_kernel<96, 0>), grid, dim3(256), 0, stream, p); break;
    case 3: hipLaunchKernelGGL((xform_kernel<128, 0>), grid, dim3(256), 0, stream, p); break;
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

hipError_t launch_xform(XformKind kind, const XformParams& p, hipStream_t stream) {
  if (p.total_columns == 0) return hipSuccess;
  const uint64_t groups = (p.total_columns + kXfLanes - 1) / kXfLanes;
  if (groups > 0x7FFFFFFFull) return hipErrorInvalidValue;
  const dim3 grid(static_cast<unsigned>(groups));
  switch (kind) {
    // 32-point: xform_kernel encodes (it runs at its load/store skeleton's speed), xform8
    // reconstructs (half the exposed arithmetic per wave: -8% time), with the pruned FFT when
    // every restored original is < 16.
    case XformKind::kEncode32:
      if (p.tail_bytes) {  // shards ending in a split tail chunk: the TAIL kernels, same dispatch
        if (encode32_kernel(p) == kEkXform8)
          hipLaunchKernelGGL((xform8_kernel<32, 0, false, 1>), grid, dim3(512), 0, stream, p);
        else
          hipLaunchKernelGGL((xform_kernel<32, 0, 1>), grid, dim3(256), 0, stream, p);
        break;
      }
      // batches of fewer tiles than CUs (a single slice per call: one tile) are latency-bound:
      // xform8 spreads a tile's transform over 8 waves of 4 slots, half xform_kernel's instruction
      // stream per wave.  Shards of 8 and 16 KiB (2 or 4 tiles per shard) also take xform8:
      // xform_kernel drops to 5.49-5.77 TB/s there while xform8 runs 5.93-6.18, and xform_kernel wins
      // by 0.03-0.31 TB/s at every other measured size (profiles/r04_encode_kernel_grid.txt; a
      // copy with either kernel's load/store skeleton shows no such dip, tools/membench/
      // membench7.hip, so it is the kernel's access order against that stride)
      if (encode32_kernel(p) == kEkXform8)
        hipLaunchKernelGGL((xform8_kernel<32, 0>), grid, dim3(512), 0, stream, p);
      else
        hipLaunchKernelGGL((xform_kernel<32, 0>), grid, dim3(256), 0, stream, p);
      break;
    case XformKind::kDecode32:
      // (xform_kernel with the same skipped conversions: random-16 reconstruct 5.37 TB/s against
      // xform8's 5.43-5.51, one box)
      if (p.tail_bytes) {
        if (p.out_low_half)
          hipLaunchKernelGGL((xform8_kernel<0, 32, true, 1>), grid, dim3(512), 0, stream, p);
        else
          hipLaunchKernelGGL((xform8_kernel<0, 32, false, 1>), grid, dim3(512), 0, stream, p);
        break;
      }
      // the full recovery set of a 32:32 code (every input shard exists) with store masks: the
      // streamed intake (headline reconstruct 1.09 -> 1.03-1.04 ms, profiles/stream_intake_ab.txt)
      if (p.n_in == 32 && p.out_mask) {
        if (p.out_low_half)
          hipLaunchKernelGGL((xform8_stream_kernel<0, 32, true>), grid, dim3(512), 0, stream, p);
        else
          hipLaunchKernelGGL((xform8_stream_kernel<0, 32, false>), grid, dim3(512), 0, stream, p);
        break;
      }
      if (p.out_low_half)
        hipLaunchKernelGGL((xform8_kernel<0, 32, true>), grid, dim3(512), 0, stream, p);
      else
        hipLaunchKernelGGL((xform8_kernel<0, 32>), grid, dim3(512), 0, stream, p);
      break;
    // 64-point: xform_h8 (32-column tiles, lane-linear I/O, two workgroups per CU)
    case XformKind::kEncode64:
      return launch_xform64(64, 0, p, stream);
    case XformKind::kDecode64:
      return launch_xform64(0, 64, p, stream);
    default:
      return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

// decode_x / decode_x16 for launch_decode_x (rs_window.hip), which checks the geometry and
// picks the kernel
hipError_t launch_decode_x32(bool per_lane, dim3 grid, const DecodeXParams& p, hipStream_t stream) {
  if (per_lane) hipLaunchKernelGGL((decode_x_kernel<true>), grid, dim3(256), 0, stream, p);
  else hipLaunchKernelGGL((decode_x_kernel<>), grid, dim3(256), 0, stream, p);
  return hipGetLastError();
}

hipError_t launch_decode_x16(int pass, unsigned din, unsigned dout, dim3 grid, const DecodeXParams& p,
                             hipStream_t stream) {
#define AG_X16(PS, DI, DO) hipLaunchKernelGGL((decode_x16_kernel<PS, DI, DO>), grid, dim3(1024), 0, stream, p)
  if (pass == 0 && din == 0 && dout == 0) AG_X16(0, 0, 0);
  else if (pass == 1 && din == 64 && dout == 0) AG_X16(1, 64, 0);
  else if (pass == 2 && din == 0 && dout == 0) AG_X16(2, 0, 0);
  else if (pass == 1 && din == 0 && dout == 64) AG_X16(1, 0, 64);
  else if (pass == 2 && din == 64 && dout == 64) AG_X16(2, 64, 64);
  else return hipErrorInvalidValue;
#undef AG_X16
  return hipGetLastError();
}

hipError_t launch_encode_mc(unsigned chunk, const XformParams& p, hipStream_t stream) {
  if (p.total_columns == 0) return hipSuccess;
  if (p.n_in > static_cast<uint32_t>(kMcMaxK) || p.n_out > chunk) return hipErrorInvalidValue;
  const uint64_t tiles = (p.total_columns + kXfLanes - 1) / kXfLanes;
  const uint64_t groups = (tiles + 3) / 4;
  if (groups > 0x7FFFFFFFull) return hipErrorInvalidValue;
  const dim3 grid(static_cast<unsigned>(groups));
  switch (chunk) {
    case 1: hipLaunchKernelGGL((encode_mc_kernel<1>), grid, dim3(256), 0, stream, p); break;
    case 2: hipLaunchKernelGGL((encode_mc_kernel<2>), grid, dim3(256), 0, stream, p); break;
    case 4: hipLaunchKernelGGL((encode_mc_kernel<4>), grid, dim3(256), 0, stream, p); break;
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

hipError_t launch_decode_syn(unsigned chunk, const DecodeSynParams& p, hipStream_t stream) {
  if (p.ntiles == 0) return hipSuccess;
  if (p.k > static_cast<uint32_t>(kMcMaxK)) return hipErrorInvalidValue;
  const uint64_t groups = (p.ntiles + 3) / 4;
  if (groups > 0x7FFFFFFFull) return hipErrorInvalidValue;
  const dim3 grid(static_cast<unsigned>(groups));
  switch (chunk) {
    case 1: hipLaunchKernelGGL((decode_syn_kernel<1>), grid, dim3(256), 0, stream, p); break;
    case 2: hipLaunchKernelGGL((decode_syn_kernel<2>), grid, dim3(256), 0, stream, p); break;
    case 4: hipLaunchKernelGGL((decode_syn_kernel<4>), grid, dim3(256), 0, stream, p); break;
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

// ---- per-call server --------------------------------------------------------------
// One workgroup of xform8's shape, resident between per-slice calls (LatencyMailbox in
// rs_launch.hpp).  Thread 0 polls the doorbell with system-scope loads (vector memory; the
// host memory is fine-grained, so nothing is cached across jobs) and every wave invalidates
// its caches at job start; each wave releases its stores at system scope before thread 0
// publishes done.  Every wave leaves the loop together on kJobQuit or the idle timeout.
__device__ __forceinline__ uint32_t sys_load(const uint32_t* a) {
  return __hip_atomic_load(a, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}
__global__ __launch_bounds__(512, 1) void latency_server_kernel(LatencyMailbox* mb, uint64_t idle_ticks,
                                                                const uint16_t* log_t) {
  __shared__ uint4 lds[16 * 4 * kXfLanes];
  __shared__ X8Flags flags;
  constexpr unsigned kXw = sizeof(XformParams) / 4, kDw = sizeof(DecodeXParams) / 4;
  __shared__ __attribute__((aligned(16))) uint32_t job[kXw];    // the transform jobs' XformParams
  __shared__ __attribute__((aligned(16))) uint32_t jobd[kDw];   // kJobDecodePk's DecodeXParams
  __shared__ uint64_t mask;
  __shared__ uint32_t cmd, reload;
  __shared__ PkShared pk;                 // kJobDecodePk: the tile's lists
  __shared__ uint64_t pk_mask[4];         // slice 0: present, restored; slice 1: none
  __shared__ PkLocTables loc;             // kJobDecodePk: the locator's tables
  static_assert(sizeof(XformParams) % 4 == 0 && kXw <= 512, "params copy");
  static_assert(sizeof(DecodeXParams) % 4 == 0 && kDw <= 512, "decode params copy");
  // the locator tables, once per launch: log x (x < 64) from the device table, a^i and a^(256 i)
  // by square-and-multiply
  if (threadIdx.x < 64) loc.log64[threadIdx.x] = log_t[threadIdx.x];
  if (threadIdx.x < 256) {
    uint32_t b = 2, bh = 2;  // a^(2^i) and a^(256 * 2^i) at step i
    for (int q = 0; q < 8; ++q) bh = poly_mul(bh, bh);
    uint32_t lo = 1, hi = 1;
    for (int i = 0; i < 8; ++i) {
      if ((threadIdx.x >> i) & 1) {
        lo = poly_mul(lo, b);
        hi = poly_mul(hi, bh);
      }
      b = poly_mul(b, b);
      bh = poly_mul(bh, bh);
    }
    loc.apow_lo[threadIdx.x] = static_cast<uint16_t>(lo);
    loc.apow_hi[threadIdx.x] = static_cast<uint16_t>(hi);
  }
  uint32_t last = 0;
  uint64_t t_job = 0, t_kind = 0, t_par = 0, t_tile = 0;  // thread 0: phase boundaries of the job
  uint32_t have_p = 0, have_dp = 0;  // thread 0: versions of the parameter copies in LDS (0: none)
  if (threadIdx.x == 0) {
    last = sys_load(&mb->done);
    __hip_atomic_store(&mb->alive, 1u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
  }
  for (;;) {
    if (threadIdx.x == 0) {
      const uint64_t t0 = wall_clock64();
      uint32_t kind = kJobQuit;
      for (;;) {
        const uint32_t d = __hip_atomic_load(&mb->doorbell, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_SYSTEM);
        if (d != last) {
          t_job = wall_clock64();
          last = d;
          // one round trip: the job's header words are loaded together (no load depends on another)
          kind = sys_load(&mb->kind);
          const uint32_t* m = reinterpret_cast<const uint32_t*>(&mb->mask);
          const uint32_t m0 = sys_load(m), m1 = sys_load(m + 1), ps = sys_load(&mb->p_seq), ds = sys_load(&mb->dp_seq);
          mask = static_cast<uint64_t>(m0) | static_cast<uint64_t>(m1) << 32;
          const uint32_t seq = kind == kJobDecodePk ? ds : ps;
          uint32_t& have = kind == kJobDecodePk ? have_dp : have_p;
          reload = seq != have ? 1u : 0u;
          have = seq;
          t_kind = wall_clock64();
          break;
        }
        if (wall_clock64() - t0 > idle_ticks) break;
        __builtin_amdgcn_s_sleep(2);
      }
      cmd = kind;
    }
    __syncthreads();
    const uint32_t kind = __builtin_amdgcn_readfirstlane(cmd);
    if (kind >= kJobQuit) break;
    if (__builtin_amdgcn_readfirstlane(reload)) {
      if (kind == kJobDecodePk) {
        if (threadIdx.x < kDw) jobd[threadIdx.x] = sys_load(reinterpret_cast<const uint32_t*>(&mb->dp) + threadIdx.x);
      } else if (threadIdx.x < kXw) {
        job[threadIdx.x] = sys_load(reinterpret_cast<const uint32_t*>(&mb->p) + threadIdx.x);
      }
    }
    if (threadIdx.x >= 128 && threadIdx.x < 144) reinterpret_cast<uint32_t*>(&flags)[threadIdx.x - 128] = 0;
    __syncthreads();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "");  // system scope: no stale input bytes in this CU's caches
    if (threadIdx.x == 0) t_par = wall_clock64();
    if (kind == kJobDecodePk) {
      // the tile reads its parameters from the LDS copy: a private copy would be indexed by the
      // rec / orig selects and land in scratch
      DecodeXParams& dp = *reinterpret_cast<DecodeXParams*>(jobd);
      if (threadIdx.x == 0) {
        pk_mask[0] = mask;   // present positions
        pk_mask[1] = ~mask;  // restored: every absent data and coding position
        pk_mask[2] = pk_mask[3] = 0;
        dp.pmask = pk_mask;
      }
      __syncthreads();
      if (dp.tail_bytes) decode_pk_tile<-1, true, true>(dp, 0, lds, &flags, pk, &loc);  // S = 960 + T, T < 64
      else decode_pk_tile<-1, true>(dp, 0, lds, &flags, pk, &loc);
      if (threadIdx.x == 0) t_tile = wall_clock64();
      __threadfence_system();
      __syncthreads();
      if (threadIdx.x == 0) {
        const uint64_t t_end = wall_clock64();
        __hip_atomic_store(&mb->phase_ticks[0], static_cast<uint32_t>(t_kind - t_job), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        __hip_atomic_store(&mb->phase_ticks[1], static_cast<uint32_t>(t_par - t_kind), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        __hip_atomic_store(&mb->phase_ticks[2], static_cast<uint32_t>(t_tile - t_par), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        __hip_atomic_store(&mb->phase_ticks[3], static_cast<uint32_t>(t_end - t_tile), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        __hip_atomic_store(&mb->job_ticks, t_end - t_job, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        __hip_atomic_store(&mb->done, last, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
      }
      continue;
    }
    XformParams p;
    uint32_t* pw = reinterpret_cast<uint32_t*>(&p);
    for (unsigned i = 0; i < sizeof(XformParams) / 4; ++i) pw[i] = __builtin_amdgcn_readfirstlane(job[i]);
    p.out_mask = kind == kJobEncode32 ? nullptr : &mask;
    p.pattern_per_block = 0;
    if (kind == kJobEncode32)
      xform8_tile<32, 0>(p, 0, lds, &flags);
    else if (kind == kJobDecode32)
      xform8_tile<0, 32>(p, 0, lds, &flags);
    else
      xform8_tile<0, 32, true>(p, 0, lds, &flags);
    if (threadIdx.x == 0) t_tile = wall_clock64();
    __threadfence_system();  // this wave's stores reach the host before done is published
    __syncthreads();
    if (threadIdx.x == 0) {
      const uint64_t t_end = wall_clock64();
      __hip_atomic_store(&mb->phase_ticks[0], static_cast<uint32_t>(t_kind - t_job), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
      __hip_atomic_store(&mb->phase_ticks[1], static_cast<uint32_t>(t_par - t_kind), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
      __hip_atomic_store(&mb->phase_ticks[2], static_cast<uint32_t>(t_tile - t_par), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
      __hip_atomic_store(&mb->phase_ticks[3], static_cast<uint32_t>(t_end - t_tile), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
      __hip_atomic_store(&mb->job_ticks, t_end - t_job, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
      __hip_atomic_store(&mb->done, last, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
  }
  if (threadIdx.x == 0) __hip_atomic_store(&mb->alive, 0u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

hipError_t launch_latency_server(LatencyMailbox* mb_dev, uint64_t idle_ticks, const uint16_t* log_t,
                                 hipStream_t stream) {
  if (!log_t) return hipErrorInvalidValue;
  hipLaunchKernelGGL(latency_server_kernel, dim3(1), dim3(512), 0, stream, mb_dev, idle_ticks, log_t);
  return hipGetLastError();
}

}  // namespace ag
