// The window decoders on 32-column tiles of the Reed-Solomon shredder path (gfx950 / CDNA4): the
// crate's HighRate / LowRate decoder for any erasure pattern, bitsliced, over a W-point window
// -- locator multiply, IFFT_W, formal derivative, FFT_W, inverse locator multiply -- and
// launch_decode_x, which picks the window decoder (decode_x and decode_x16, on 64-column tiles,
// are in rs_tile64.hip).
// What they replace: the reed-solomon-simd 3.1.0 calls inside ReedSolomonCoder (encode,
// decode, re-encode).  Arithmetic: GF(2^16) Leopard additive FFT.
//
// Kernels
//   decode_h8_kernel       W = 64 / 128 on 32-column tiles, per-lane patterns
//   decode_pk_kernel       W = 64 for 1 KiB shreds, locator products on packed items (tile body
//                          in rs_decode_pk.hpp)
//   decode_rows_kernel, decode_rows128_kernel   the patterns' locator constants (Walsh route
//                          over Z/65535)
#include <hip/hip_runtime.h>

#include "rs_decode_pk.hpp"
#include "rs_device.hpp"
#include "rs_launch.hpp"
#include "rs_xform.hpp"

namespace ag {
namespace {

using dev::static_for;

// =====================================================================================
// decode_h8<OUTH>: the W = 64 per-lane window decoder (decode_x16<true, 0>'s algorithm) on
// 32-column tiles with the lane half as a position bit: 8 waves x 4 slots x 2 lane halves,
// 64 KiB of swap buffer, so two workgroups share a CU and one's loads, swaps and barriers
// overlap the other's arithmetic (decode_x16 runs one 1024-thread workgroup per CU).
// Lane l holds column l & 31 of the tile; h = l >> 5 is a position bit.  Layouts (slot bits
// | lane half | wave bits):
//   A  slots p0 p1 | h p2 | waves p3 p4 p5   loads, locator multiplies, IFFT b0; FFT b0, stores
//   B  slots p2 p1 | h p0 | waves p3 p4 p5   IFFT b1 b2 / FFT b1      (A <-> B: v_permlane32_swap)
//   C  slots p2 p3 | h p0 | waves p1 p4 p5   IFFT b3 / FFT b2
//   D  slots p4 p3 | h p0 | waves p1 p2 p5   IFFT b4 / FFT b3
//   E  slots p4 p5 | h p0 | waves p1 p2 p3   IFFT b5, formal derivative, FFT b5 b4
// A layer-b skew constant depends on the position bits above b.  From B on the lane half is
// p0, below every layer's bit; layer 0 in A has a constant per lane half (both halves' XOR
// programs run under the exec mask).  The derivative's p0 term crosses lane halves
// (v_permlane32_swap of the pre-derivative slot).  OUTH = the window half (p5) holding the
// restored originals (1 HighRate chunk 32, 0 the LowRate sub-window, -1 both): after FFT b4
// the waves whose p5 is the other half send their live slots and retire.
// PASS 1 / 2: the W = 128 window as decode_x16's two 64-point passes (loaded half DIN, output
// half DOUT), with the output multiply deferred: pass 1 stores FFT(u_other) unmultiplied,
// pass 2 adds it to FFT(P u_out) in planes and multiplies once (the multiply is linear), so a
// restored original costs one runtime product instead of two.
// Each lane loads its own whole chunk (four 16-byte pieces of one chunk).  A lane-linear
// option (xform_h8's piece order + quad_exchange) measured slower on the follower's batches
// (14.0-14.1 vs 14.4-14.6 M slices/s, profiles/r03_h8_ll_ab.jsonl) and was removed.
// The derivative's regions are handed over by the swaps' epoch flags (no workgroup barriers):
// ready = published, done = this wave's reads finished; a region is rewritten once every
// reader of its last epoch is done.  Epochs: swaps 1-3, derivative rounds 4-5, swaps 6-8.
// TAIL: shards of S = 64 C + T bytes (16 <= T < 64; p.chunks_per_shard = C + 1): the lanes of
// column C move their block's T-byte tail chunk whole (load_tail_chunk / store_tail_chunk:
// 16-byte accesses inside the tail only), so the follower's slices of any even shred size with
// T >= 16 decode in place, with no restride.
template <int OUTH, int PASS, int DIN, int DOUT, bool TAIL = false>
__global__ __launch_bounds__(512, 4) void decode_h8_kernel(const DecodeXParams p) {
  static_assert(PASS != 0 || (DIN == 0 && DOUT == 0), "the one-pass window starts at 0");
  static_assert(PASS != 2 || DIN == DOUT, "pass 2 loads its output half");
  static_assert(!TAIL || PASS == 0, "tail chunks on the one-pass window");
  constexpr int W = 64, kCols = 32;
  __shared__ uint4 lds[16 * 4 * kXfLanes];  // 8 waves x 2 slots x 4 KiB
  __shared__ X8Flags flags;
  __shared__ uint32_t lcoef[kCols * W];     // the constants of the <= 32 blocks of the tile
  const int lane = threadIdx.x & 63;
  const int h = lane >> 5;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const uint32_t tile = dev::xcd_tile(blockIdx.x, gridDim.x);
  const uint64_t c0 = static_cast<uint64_t>(tile) * kCols;
  const uint64_t c1 = c0 + kCols - 1 < p.total_columns ? c0 + kCols - 1 : p.total_columns - 1;
  const uint64_t sb0 = c0 / p.chunks_per_shard;
  {
    const uint32_t nbt = static_cast<uint32_t>(c1 / p.chunks_per_shard - sb0 + 1);  // <= 32
    for (uint32_t i = threadIdx.x; i < nbt * W; i += blockDim.x) lcoef[i] = p.rows[(sb0 + i / W) * p.rows_w + DIN + i % W];
  }
  if (threadIdx.x < 16) reinterpret_cast<uint32_t*>(&flags)[threadIdx.x] = 0;
  __syncthreads();
  const uint64_t gc = c0 + (lane & 31);
  const bool ok = gc < p.total_columns;
  const uint32_t cc = static_cast<uint32_t>(c0 - sb0 * p.chunks_per_shard) + (lane & 31);  // 32-bit per lane
  const uint32_t d = ok ? cc / p.chunks_per_shard : 0;
  const uint64_t blk = sb0 + d;
  const uint64_t col = ok ? cc - d * p.chunks_per_shard : 0;
  const bool tail_lane = TAIL && ok && col + 1 == p.chunks_per_shard;
  const uint64_t in_mask = ok ? p.pmask[2 * blk] : 0;
  const uint64_t out_mask = ok ? p.pmask[2 * blk + 1] : 0;
  const uint32_t* coef = lcoef + (blk - sb0) * W;
  const uint64_t off_r = blk * p.rec_block_stride + col * 64;
  const uint64_t off_o = blk * p.orig_block_stride + col * 64;
  const uint32_t opos = p.low_rate ? 0 : p.chunk, rpos = p.low_rate ? p.chunk : 0;
  // layout A position of slot t in this lane
  auto posA = [&](int t) -> uint32_t {
    return static_cast<uint32_t>((t & 1) | ((t >> 1) << 1) | (h << 2) | (wave << 3));
  };
  Regs4 r;
  static_for<4>([&](auto T) {
    constexpr int t = decltype(T)::value;
    const uint32_t j = posA(t);
    const uint32_t g = DIN + j;  // window position
    const bool is_rec = p.low_rate ? g >= p.chunk : g < p.chunk;
    if ((in_mask >> j) & 1) {
      const uint8_t* src = is_rec ? p.rec + (g - rpos) * p.rec_shard_stride + off_r
                                  : p.orig + (g - opos) * p.orig_shard_stride + off_o;
      if (tail_lane) {
        load_tail_chunk(src, p.tail_bytes, r[t]);
      } else {
        static_for<4>([&](auto Q) {
          constexpr int q = decltype(Q)::value;
          const uint4 x = ld_piece(src + 16 * q);
          r[t][4 * q] = x.x;
          r[t][4 * q + 1] = x.y;
          r[t][4 * q + 2] = x.z;
          r[t][4 * q + 3] = x.w;
        });
      }
    } else {
      static_for<16>([&](auto P) { r[t][decltype(P)::value] = 0; });
    }
  });
  static_for<4>([&](auto T) {
    constexpr int t = decltype(T)::value;
    const uint32_t j = posA(t);
    if ((in_mask >> j) & 1) {
      dev::planes_from_raw(r[t]);
      dev::mul_rt_poly(r[t], coef[j]);
    }
  });
  // IFFT_64 (skew delta DIN)
  h8_layer0<true, DIN>(wave, h, r);
  h8_relayout(r);
  x8_layer_t<LB, 1, true, DIN>(wave, r);
  x8_layer_t<LB, 2, true, DIN>(wave, r);
  x8_swap<1, 0, 1>(wave, lane, lds, &flags, r);
  x8_layer_t<LC, 3, true, DIN>(wave, r);
  x8_swap<0, 1, 2>(wave, lane, lds, &flags, r);
  x8_layer_t<LD, 4, true, DIN>(wave, r);
  x8_swap<1, 2, 3>(wave, lane, lds, &flags, r);
  x8_layer_t<LE, 5, true, DIN>(wave, r);
  // formal derivative in E (slot t: p4 = t & 1, p5 = t >> 1; lane half p0; waves p1 p2 p3);
  // PASS 2: P = the derivative without its self term; PASS 1: none.  Each wave publishes its
  // two pre-derivative slots of round rho in its own region (its swap inbox); the waves with
  // a wave bit b clear add the region of their partner w | 2^b.
  constexpr int D = PASS != 1 ? 2 : 0;  // FFT swap epochs 4 + D ..
  // the readers of region x in a derivative round: x with one of its set wave bits cleared
  auto wait_readers = [&](int x, uint32_t e) __attribute__((always_inline)) {
    static_for<3>([&](auto Bb) {
      constexpr int b = decltype(Bb)::value;
      if ((x >> b) & 1) x8_wait_ge(&flags.done[x & ~(1 << b)], e);
    });
  };
  if constexpr (PASS != 1) {
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
        if constexpr (PASS == 2) {
          static_for<16>([&](auto P) {
            constexpr int q = decltype(P)::value;
            uint32_t v = hi[q];
            if constexpr (!(t & 1)) v ^= r[t | 1][q];
            if constexpr (!(t & 2)) v ^= r[t | 2][q];
            r[t][q] = v;
          });
        } else {
          if constexpr (!(t & 1)) dev::xor_planes(r[t], r[t | 1]);
          if constexpr (!(t & 2)) dev::xor_planes(r[t], r[t | 2]);
          dev::xor_planes(r[t], hi);
        }
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
  }
  // FFT_64 (skew delta DOUT), ending in A.  The first swap writes the partner's region: its
  // last derivative round's readers must be done with it.
  x8_layer_t<LE, 5, false, DOUT>(wave, r);
  x8_layer_t<LE, 4, false, DOUT>(wave, r);
  if constexpr (D != 0) wait_readers(wave ^ 4, 5);
  if constexpr (OUTH < 0) {
    x8_swap<1, 2, 4 + D>(wave, lane, lds, &flags, r);
  } else {
    // E -> D: slot bit 1 (p5) <-> wave bit 2 (p3).  After it a wave's slots all have p5 =
    // its wave bit 2; the other half's waves only send the slots the live partner needs.
    const int partner = wave ^ 4;
    if (((wave >> 2) & 1) != OUTH) {
      x8_wait_ge(&flags.done[partner], 3 + D);
      static_for<4>([&](auto T) {
        constexpr int t = decltype(T)::value;
        if constexpr (((t >> 1) & 1) == (OUTH > 0 ? 1 : 0)) {
          lds_put(lds, 2 * partner + (t & 1), lane, r[t]);
          __asm__ volatile("; h8 put %0" ::"n"(t));
        }
      });
      x8_signal(&flags.ready[wave], 4 + D, lane);
      return;
    }
    x8_wait_ge(&flags.ready[partner], 4 + D);
    static_for<4>([&](auto T) {
      constexpr int t = decltype(T)::value;
      if constexpr (((t >> 1) & 1) != (OUTH > 0 ? 1 : 0)) {
        lds_get(lds, 2 * wave + (t & 1), lane, r[t]);
        __asm__ volatile("; h8 get %0" ::"n"(t));
      }
    });
    x8_signal(&flags.done[wave], 4 + D, lane);
  }
  x8_layer_t<LD, 3, false, DOUT>(wave, r);
  x8_swap<0, 1, 5 + D>(wave, lane, lds, &flags, r);
  x8_layer_t<LC, 2, false, DOUT>(wave, r);
  x8_swap<1, 0, 6 + D>(wave, lane, lds, &flags, r);
  x8_layer_t<LB, 1, false, DOUT>(wave, r);
  // the store predicates, packed before the first load or store of the store phase (bit t:
  // slot t restores its position in this lane's block)
  uint32_t qall = 0;
  static_for<4>([&](auto T) { qall |= static_cast<uint32_t>((out_mask >> posA(decltype(T)::value)) & 1) << decltype(T)::value; });
  if (__builtin_amdgcn_ballot_w64(qall != 0) == 0) return;  // nothing to restore in this wave
  h8_relayout(r);
  h8_layer0<false, DOUT>(wave, h, r);
  static_for<4>([&](auto T) {
    constexpr int t = decltype(T)::value;
    const uint32_t j = posA(t);
    if ((qall >> t) & 1) {
      uint8_t* dst = p.orig + (DOUT + j - opos) * p.orig_shard_stride + off_o;
      if constexpr (PASS == 0 && OUTH < 0) {
        // fused coding restore (p.fuse, HighRate): an absent recovery position's value is the
        // re-encoded coding shard; it goes back to its own slot (the ANY_K patterns of other
        // callers never restore recovery positions)
        if (DOUT + j < p.chunk) dst = const_cast<uint8_t*>(p.rec) + (DOUT + j) * p.rec_shard_stride + off_r;
      }
      if constexpr (PASS == 2) {
        // + pass 1's partial, in planes.  The load is the youngest memory operation when it is
        // waited on (vmcnt(0)): the earlier slots' stores may alias it, so it is not hoisted
        // above them (tools/scan_waitcnt.py)
        uint32_t o[16];
        static_for<4>([&](auto Q) {
          constexpr int q = decltype(Q)::value;
          const uint4 x = ld_piece(dst + 16 * q);
          o[4 * q] = x.x;
          o[4 * q + 1] = x.y;
          o[4 * q + 2] = x.z;
          o[4 * q + 3] = x.w;
        });
        dev::planes_from_raw(o);
        dev::xor_planes(r[t], o);
      }
      if constexpr (PASS != 1) dev::mul_rt_poly(r[t], coef[j]);
      if (tail_lane) {
        uint32_t raw[16];
        static_for<16>([&](auto P) { raw[decltype(P)::value] = r[t][decltype(P)::value]; });
        dev::transpose8(raw);
        dev::transpose8(raw + 8);
        store_tail_chunk(dst, p.tail_bytes, raw);
      } else {
        dev::store_chunk<true>(dst, r[t]);  // PASS 1: the unmultiplied partial
      }
    }
  });
}

template <int OUTH, bool TAIL = false>
__global__ __launch_bounds__(512, 4) void decode_pk_kernel(const DecodeXParams p) {
  __shared__ uint4 lds[16 * 4 * kXfLanes];
  __shared__ X8Flags flags;
  __shared__ PkShared sh;
  decode_pk_tile<OUTH, false, TAIL>(p, dev::xcd_tile(blockIdx.x, gridDim.x), lds, &flags, sh);
}

// Per pattern and window position x: the decoder's locator constant as a bitsliced
// multiply matrix.  loc(x) = sum_{e erased, e != x} log(x ^ e) (mod 65535) -- the crate's
// eval_poly over the window up to one constant factor, which cancels between the input
// multiply (present x: exp(loc)) and the output multiply (restored x: exp(-loc)).
// poly: one word per position instead -- the constant in the polynomial basis (mul_rt_poly).
//
// loc is the XOR convolution of L(z) = log z (L(0) = 0, which drops e = x; log[0] = 65535 is
// the same residue) with the erasure indicator, so it comes out of Walsh-Hadamard transforms
// over Z/65535 (the crate's own error-locator route, on the window instead of the field):
// loc = H(H(L) * H(I)) / N.  The window's L is zero past W, so an N-point transform
// (N = 64, or 128 with two positions per lane) serves every W <= N.  One wave per pattern,
// lane-shuffle stages, no loop over the erased positions; exp depends only on the residue
// (exp[65535] = exp[0]), so the constants are the loop form's bit for bit.

__global__ __launch_bounds__(256) void decode_rows_kernel(const uint64_t* __restrict__ emask,
                                                          const uint64_t* __restrict__ pmask, uint32_t npat,
                                                          uint32_t W, const uint16_t* __restrict__ log_t,
                                                          const uint16_t* __restrict__ exp_t, uint32_t* rows,
                                                          uint32_t poly) {
  const uint64_t pat = static_cast<uint64_t>(blockIdx.x) * 4 + (threadIdx.x >> 6);
  if (pat >= npat) return;  // wave-uniform
  const int lane = threadIdx.x & 63;
  const uint32_t x = static_cast<uint32_t>(lane);
  const uint64_t e = emask[pat], in = pmask[2 * pat], out = pmask[2 * pat + 1];
  // H(L) / 64 (64^-1 = 1024: 2^16 = 1)
  const uint32_t hl = m65535_mul(walsh64(x && x < W ? log_t[x] : 0u, lane), 1024u);
  const uint32_t hi = walsh64(x < W ? static_cast<uint32_t>((e >> x) & 1) : 0u, lane);
  const uint32_t acc = walsh64(m65535_mul(hl, hi), lane);
  if (x >= W) return;
  const bool is_in = (in >> x) & 1, is_out = (out >> x) & 1;
  if (!is_in && !is_out) return;
  const uint16_t lg = locator_log(acc, is_in);
  if (poly) {
    rows[pat * W + x] = dev::to_poly(exp_t[lg]);  // exp[lg] = the constant
    return;
  }
  uint32_t* dst = rows + (pat * W + x) * 16;
  uint32_t r[16] = {};
  for (int i = 0; i < 16; ++i) {
    const uint16_t prod = dev::gmul(exp_t, log_t, static_cast<uint16_t>(1u << i), lg);
    for (int o = 0; o < 16; ++o) r[o] |= ((prod >> o) & 1u) << i;
  }
  for (int o = 0; o < 16; ++o) dst[o] = r[o];
}

}  // namespace

// ---- launchers ----------------------------------------------------------------------
hipError_t launch_decode_x(unsigned W, int pass, const DecodeXParams& p, uint64_t ntiles, hipStream_t stream,
                           uint32_t* which) {
  if (ntiles == 0) return hipSuccess;
  auto rec = [&](uint32_t bit) {
    if (which) *which |= bit;
  };
  if (ntiles > 0x7FFFFFFFull) return hipErrorInvalidValue;
  if (p.k + p.chunk > W || p.m > p.chunk || (p.low_rate && (p.k > p.chunk || p.m + p.chunk > W)))
    return hipErrorInvalidValue;
  const dim3 grid(static_cast<unsigned>(ntiles));
  const bool pl = p.per_lane != 0;
  if (W == 32 && pass == 0) {
    return launch_decode_x32(pl, grid, p, stream);
  }
  // per-lane patterns run on decode_h8 (32-column tiles over every column; the caller's
  // ntiles counts 64-column ones), one pattern per tile on decode_x16
  const uint64_t t32 = (p.total_columns + 31) / 32;
  if (t32 > 0x7FFFFFFFull) return hipErrorInvalidValue;
  const dim3 g32(static_cast<unsigned>(t32));
#define AG_H8(O, PS, DI, DO) hipLaunchKernelGGL((decode_h8_kernel<O, PS, DI, DO>), g32, dim3(512), 0, stream, p)
#define AG_H8T(O) hipLaunchKernelGGL((decode_h8_kernel<O, 0, 0, 0, true>), g32, dim3(512), 0, stream, p)
  hipError_t x16 = hipSuccess;  // decode_x16 lives with the 64-column-tile kernels (rs_tile64.hip)
#define AG_X16(PS, DI, DO) x16 = launch_decode_x16(PS, DI, DO, grid, p, stream)
  if (W == 64 && pass == 0) {
    if (p.rows_w != 64) return hipErrorInvalidValue;
    if (p.tail_bytes) {
      // shards with a T-byte tail chunk (per-lane HighRate chunk 32): decode_h8's TAIL variant
      if (!pl || p.low_rate || p.chunk != 32 || p.tail_bytes >= 64 || p.tail_bytes % 2) return hipErrorInvalidValue;
      if (p.any_k && p.chunks_per_shard == 16) {  // S = 960 + T: the packed decoder, tail column 15
        if (p.fuse) hipLaunchKernelGGL((decode_pk_kernel<-1, true>), g32, dim3(512), 0, stream, p);
        else hipLaunchKernelGGL((decode_pk_kernel<1, true>), g32, dim3(512), 0, stream, p);
        rec(p.fuse ? kDxPkFused : kDxPk);
        return hipGetLastError();
      }
      if (p.fuse) AG_H8T(-1);
      else AG_H8T(1);
      rec(p.fuse ? kDxH8Fused : kDxH8);
      return hipGetLastError();
    }
    const bool packed = pl && p.any_k && p.chunks_per_shard == 16 && (p.low_rate || p.chunk == 32);
    // fused coding restore: the caller's patterns restore absent coding positions too and skip
    // those slices in the re-encode, which decode_pk<-1> and the full-FFT decode_h8<-1> honour
    // (per-lane HighRate chunk 32 only)
    if (p.fuse && (p.low_rate || !pl || p.chunk != 32)) return hipErrorInvalidValue;
    if (packed) {
      if (p.low_rate) hipLaunchKernelGGL((decode_pk_kernel<0>), g32, dim3(512), 0, stream, p);
      else if (p.fuse) hipLaunchKernelGGL((decode_pk_kernel<-1>), g32, dim3(512), 0, stream, p);
      else hipLaunchKernelGGL((decode_pk_kernel<1>), g32, dim3(512), 0, stream, p);
      rec(p.fuse ? kDxPkFused : kDxPk);
    } else if (!pl) {
      AG_X16(0, 0, 0);
      rec(kDxX16);
    } else if (p.low_rate) {
      AG_H8(0, 0, 0, 0);
      rec(kDxH8);
    } else if (p.chunk == 32 && !p.fuse) {
      AG_H8(1, 0, 0, 0);
      rec(kDxH8);
    } else {
      AG_H8(-1, 0, 0, 0);  // (fused: restored positions in both window halves)
      rec(p.fuse ? kDxH8Fused : kDxH8);
    }
  } else if (W == 128 && (pass == 1 || pass == 2)) {
    // the originals must lie in one window half: LowRate k <= 64 (half 0); HighRate chunk 64
    // (half 1).  Both passes of a decode come from the same kernel family.
    if (p.rows_w != 128 || (p.low_rate ? p.k > 64 : p.chunk != 64)) return hipErrorInvalidValue;
    if (pl) {
      // LowRate: outputs (originals < 32 when k <= 32) in half 0; HighRate: half 1
      if (p.low_rate && p.k <= 32) {
        if (pass == 1) AG_H8(0, 1, 64, 0);
        else AG_H8(0, 2, 0, 0);
      } else if (p.low_rate) {
        if (pass == 1) AG_H8(-1, 1, 64, 0);
        else AG_H8(-1, 2, 0, 0);
      } else {
        if (pass == 1) AG_H8(-1, 1, 0, 64);
        else AG_H8(-1, 2, 64, 64);
      }
    } else if (p.low_rate) {  // outputs in half 0
      if (pass == 1) AG_X16(1, 64, 0);
      else AG_X16(2, 0, 0);
    } else {                  // outputs in half 1
      if (pass == 1) AG_X16(1, 0, 64);
      else AG_X16(2, 64, 64);
    }
  } else {
    return hipErrorInvalidValue;
  }
#undef AG_H8
#undef AG_H8T
#undef AG_X16
  return x16 != hipSuccess ? x16 : hipGetLastError();
}

// W = 128 windows: m6[pat] = {erased lo, hi, present lo, hi, restored lo, hi} (position bits
// 0..63, 64..127); rows [pat][128] polynomial-basis constants (decode_rows poly form).
__global__ __launch_bounds__(256) void decode_rows128_kernel(const uint64_t* __restrict__ m6, uint32_t npat,
                                                            const uint16_t* __restrict__ log_t,
                                                            const uint16_t* __restrict__ exp_t, uint32_t* rows) {
  const uint64_t pat = static_cast<uint64_t>(blockIdx.x) * 4 + (threadIdx.x >> 6);
  if (pat >= npat) return;  // wave-uniform
  const int lane = threadIdx.x & 63;
  const uint64_t* m = m6 + 6 * pat;
  // decode_rows' Walsh route at N = 128: positions lane (v0) and lane + 64 (v1)
  uint32_t l0 = lane ? log_t[lane] : 0u, l1 = log_t[lane + 64];
  walsh128(l0, l1, lane);
  l0 = m65535_mul(l0, 512u);  // 128^-1 = 512
  l1 = m65535_mul(l1, 512u);
  uint32_t i0 = static_cast<uint32_t>((m[0] >> lane) & 1), i1 = static_cast<uint32_t>((m[1] >> lane) & 1);
  walsh128(i0, i1, lane);
  uint32_t a0 = m65535_mul(l0, i0), a1 = m65535_mul(l1, i1);
  walsh128(a0, a1, lane);
  static_for<2>([&](auto H) {
    constexpr int h = decltype(H)::value;
    const bool is_in = (m[2 + h] >> lane) & 1, is_out = (m[4 + h] >> lane) & 1;
    if (is_in || is_out) rows[pat * 128 + h * 64 + lane] = dev::to_poly(exp_t[locator_log(h ? a1 : a0, is_in)]);
  });
}

hipError_t launch_decode_rows128(const uint64_t* m6, uint32_t npat, const GfDeviceTables& t, uint32_t* rows,
                                 hipStream_t stream) {
  if (npat == 0) return hipSuccess;
  hipLaunchKernelGGL(decode_rows128_kernel, dim3((npat + 3) / 4), dim3(256), 0, stream, m6, npat, t.log, t.exp, rows);
  return hipGetLastError();
}

hipError_t launch_decode_rows(const uint64_t* emask, const uint64_t* pmask, uint32_t npat, uint32_t W,
                              const GfDeviceTables& t, uint32_t* rows, bool poly, hipStream_t stream) {
  if (npat == 0) return hipSuccess;
  if (W > 64) return hipErrorInvalidValue;
  hipLaunchKernelGGL(decode_rows_kernel, dim3((npat + 3) / 4), dim3(256), 0, stream, emask, pmask, npat, W, t.log, t.exp,
                     rows, poly ? 1u : 0u);
  return hipGetLastError();
}

}  // namespace ag
