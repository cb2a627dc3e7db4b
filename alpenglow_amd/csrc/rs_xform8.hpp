// xform8's tile body: the 32-point transform of one 64-column tile on 8 waves x 4 slots
// (layouts and swaps in rs_xform.hpp).  Shared by xform8_kernel's grid and the per-call
// server's transform jobs (both in rs_tile64.hip); xform8_stream_tile is the same transform
// behind the streamed intake (xform8_stream_kernel).  gfx950 / CDNA4 only.
#pragma once
#include <hip/hip_runtime.h>

#include <type_traits>

#include "rs_device.hpp"
#include "rs_launch.hpp"
#include "rs_xform.hpp"

namespace ag {
namespace {

using dev::static_for;

// HALF: every stored output has position bit 4 clear (a decode whose erased originals all
// lie in shards 0..15).  After FFT layer 4 only the x halves are needed (no y update),
// and the remaining 16-point FFT runs on the two live slots per wave (slot bit 0 = p4 = 0)
// with one slot moved per exchange; the stores are two shards per wave:
//   H3 slots p4 p3 | waves p0 p1 p2   FFT b4 (x only), b3
//   H2 slots p4 p2 | waves p0 p1 p3   FFT b2
//   H1 slots p4 p1 | waves p0 p2 p3   FFT b1
//   H0 slots p4 p0 | waves p1 p2 p3   FFT b0, store shards 2w, 2w + 1
// One tile (flags zeroed by the caller, every wave of the 512-thread workgroup calls it):
// xform8_kernel's grid and the per-call server's jobs (latency_server_kernel).
template <int DIN, int DOUT, bool HALF = false, int TAIL = 0>
__device__ __forceinline__ void xform8_tile(const XformParams& p, uint32_t tile, uint4* lds, X8Flags* fl) {
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const TileIO io = tile_io<TAIL>(p, tile, lane, p.in_block_stride);
  Regs4 r;
  // a tile past the batch's last column (one slice per call: 16 of 64 columns) loads only
  // its existing pieces -- over PCIe from mapped host memory, the idle re-reads were 3/4 of
  // the per-call server's input traffic
  const bool whole = p.total_columns >= (static_cast<uint64_t>(tile) + 1) * kXfLanes;
  static_for<4>([&](auto T) {
    constexpr int t = decltype(T)::value;
    const uint32_t sh = 4 * wave + t;  // LA: wave-uniform
    if (sh < p.n_in) {
      const uint8_t* base = p.in + sh * p.in_shard_stride;
      static_for<4>([&](auto Q) {
        constexpr int q = decltype(Q)::value;
        uint4 x = make_uint4(0, 0, 0, 0);
        if (whole || ((io.valid >> q) & 1)) x = ld_piece_io<TAIL>(base, io, q);
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
    tail_fix_all<TAIL>(io, r[decltype(T)::value]);
    swap_halves(r[decltype(T)::value]);
    dev::planes_from_raw(r[decltype(T)::value]);
  });
  x8_layer<0, 0, true, DIN>(wave, r);
  x8_layer<0, 1, true, DIN>(wave, r);
  x8_swap<0, 0, 1>(wave, lane, lds, fl, r);
  x8_layer<1, 2, true, DIN>(wave, r);
  x8_swap<1, 1, 2>(wave, lane, lds, fl, r);
  x8_layer<2, 3, true, DIN>(wave, r);
  x8_swap<0, 2, 3>(wave, lane, lds, fl, r);
  if constexpr (HALF) {
    using H3 = X8Lay<4, 3, 0, 1, 2>;
    using H2 = X8Lay<4, 2, 0, 1, 3>;
    using H1 = X8Lay<4, 1, 0, 2, 3>;
    using H0 = X8Lay<4, 0, 1, 2, 3>;
    static_assert(std::is_same_v<H3, X8Layout<3>>, "H3 is layout L3");
    x8_layer<3, 4, true, DIN>(wave, r);
    x8_layer<3, 4, false, DOUT, 0x5, false>(wave, r);
    x8_layer_lay<H3, 3, DOUT, 0x5>(wave, r);
    x8_swap<1, 2, 4, 0x5>(wave, lane, lds, fl, r);
    x8_layer_lay<H2, 2, DOUT, 0x5>(wave, r);
    x8_swap<1, 1, 5, 0x5>(wave, lane, lds, fl, r);
    x8_layer_lay<H1, 1, DOUT, 0x5>(wave, r);
    x8_swap<1, 0, 6, 0x5>(wave, lane, lds, fl, r);
    const TileIO out_io = tile_io<TAIL>(p, tile, lane, p.out_block_stride);
    uint64_t mask[4] = {~0ull, ~0ull, ~0ull, ~0ull};
    if (p.out_mask) {
      if (!p.pattern_per_block) {
        const uint64_t m = p.out_mask[0];
        mask[0] = mask[1] = mask[2] = mask[3] = m;
      } else {
        static_for<4>([&](auto Q) { mask[decltype(Q)::value] = p.out_mask[out_io.blk[decltype(Q)::value]]; });
      }
    }
    // store predicates packed before the first store (bits 4 u + q; see qmask_all)
    const uint32_t qall = qmask_all<2>(out_io, mask, 2 * wave, p.n_out);
    if (__builtin_amdgcn_ballot_w64(qall != 0) == 0) return;
    x8_layer_lay<H0, 0, DOUT, 0x5>(wave, r);
    static_for<2>([&](auto U) {
      constexpr int t = 2 * decltype(U)::value;
      const uint32_t sh = 2 * wave + (t >> 1);  // H0 position of live slot t
      if (sh < p.n_out) store_shard<false, TAIL>(p.out + sh * p.out_shard_stride, out_io, (qall >> (4 * (t >> 1))) & 15u, r[t]);
    });
    return;
  }
  x8_layer<3, 4, true, DIN>(wave, r);
  x8_layer<3, 4, false, DOUT>(wave, r);
  x8_layer<3, 3, false, DOUT>(wave, r);
  x8_swap<0, 2, 4>(wave, lane, lds, fl, r);
  x8_layer<2, 2, false, DOUT>(wave, r);
  x8_swap<1, 1, 5>(wave, lane, lds, fl, r);
  x8_layer<1, 1, false, DOUT>(wave, r);
  x8_swap<0, 0, 6>(wave, lane, lds, fl, r);
  // store masks fetched only now: live across the transform they cost registers (spills)
  const TileIO out_io = tile_io<TAIL>(p, tile, lane, p.out_block_stride);
  uint64_t mask[4] = {~0ull, ~0ull, ~0ull, ~0ull};
  if (p.out_mask) {
    if (!p.pattern_per_block) {
      const uint64_t m = p.out_mask[0];
      mask[0] = mask[1] = mask[2] = mask[3] = m;
    } else {
      static_for<4>([&](auto Q) { mask[decltype(Q)::value] = p.out_mask[out_io.blk[decltype(Q)::value]]; });
    }
  }
  const uint32_t qall = qmask_all<4>(out_io, mask, 4 * wave, p.n_out);
  // slots some lane stores (wave-uniform): a decode restores only the erased originals, so
  // the last FFT layer skips butterflies with no stored output (y not updated where only x is
  // stored) and unstored slots skip their planes -> bytes conversion
  uint32_t need = 0;
  static_for<4>([&](auto T) {
    constexpr int t = decltype(T)::value;
    if (__builtin_amdgcn_ballot_w64(((qall >> (4 * t)) & 15u) != 0) != 0) need |= 1u << t;
  });
  if (need == 0) return;
  {
    using L0 = X8Layout<0>;
    const int v = x8_compress<L0::rel(0)>(wave);
    if (need & 3u) x8_bfly_w<L0, 0, false, DOUT, 0>(v, r[0], r[1], (need & 2u) != 0);
    if (need & 12u) x8_bfly_w<L0, 0, false, DOUT, 2>(v, r[2], r[3], (need & 8u) != 0);
  }
  static_for<4>([&](auto T) {
    constexpr int t = decltype(T)::value;
    const uint32_t sh = 4 * wave + t;  // wave-uniform
    if (((need >> t) & 1u) && sh < p.n_out)
      store_shard<false, TAIL>(p.out + sh * p.out_shard_stride, out_io, (qall >> (4 * t)) & 15u, r[t]);
  });
}

// xform8_tile with the streamed intake, for launches where every input shard exists, shards are
// whole chunks and store masks are given (launch_xform: the 32:32 full-recovery reconstruct):
//   - the tile's 16 loads per lane are issued with no control flow between them and slot t is
//     converted behind s_waitcnt vmcnt(4 (3 - t)), a layer-0 butterfly behind its two slots
//     (load_slots_stream; xform8_tile's first conversion waits for the whole tile);
//   - the store-mask words are loaded ahead of the pieces and folded into the store predicates
//     while the pieces are in flight: one VGPR lives across the transform, and no load sits
//     between the last swap and the stores (xform8_tile fetches the words there: a dependent
//     round trip per wave with nothing in flight to hide it).
// The transform is xform8_tile's, written out again: shared through one template, the tiles
// that keep the old intake (and the server's) compile to different instructions.
template <int DIN, int DOUT, bool HALF>
__device__ __forceinline__ void xform8_stream_tile(const XformParams& p, uint32_t tile, uint4* lds, X8Flags* fl) {
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const TileIO io = tile_io<0>(p, tile, lane, p.in_block_stride);
  Regs4 r;
  // One pattern for the batch reads word 0 through the same four loads (index masked, not
  // branched: after a branch the words merge in a phi, and its copies wait for them before the
  // first piece is requested).  A chunk's block and validity do not depend on the block stride:
  // the input io's are the output's.
  uint64_t mask[4];
  const uint64_t per_block = p.pattern_per_block ? ~0ull : 0ull;
  static_for<4>([&](auto Q) { mask[decltype(Q)::value] = p.out_mask[io.blk[decltype(Q)::value] & per_block]; });
  load_slots_stream<4>(p, io, 4 * wave, r);
  // store predicates packed before the first store (see qmask_all): here, before the transform
  uint32_t qall;
  if constexpr (HALF) qall = qmask_all<2>(io, mask, 2 * wave, p.n_out);
  else qall = qmask_all<4>(io, mask, 4 * wave, p.n_out);
  {
    using L0 = X8Layout<0>;
    const int v = x8_compress<L0::rel(0)>(wave);
    static_for<2>([&](auto I) {
      constexpr int t = 2 * decltype(I)::value;
      static_for<2>([&](auto U) {
        swap_halves(r[t + decltype(U)::value]);
        dev::planes_from_raw(r[t + decltype(U)::value]);
      });
      x8_bfly_w<L0, 0, true, DIN, t>(v, r[t], r[t + 1]);
    });
  }
  x8_layer<0, 1, true, DIN>(wave, r);
  x8_swap<0, 0, 1>(wave, lane, lds, fl, r);
  x8_layer<1, 2, true, DIN>(wave, r);
  x8_swap<1, 1, 2>(wave, lane, lds, fl, r);
  x8_layer<2, 3, true, DIN>(wave, r);
  x8_swap<0, 2, 3>(wave, lane, lds, fl, r);
  if constexpr (HALF) {
    using H3 = X8Lay<4, 3, 0, 1, 2>;
    using H2 = X8Lay<4, 2, 0, 1, 3>;
    using H1 = X8Lay<4, 1, 0, 2, 3>;
    using H0 = X8Lay<4, 0, 1, 2, 3>;
    x8_layer<3, 4, true, DIN>(wave, r);
    x8_layer<3, 4, false, DOUT, 0x5, false>(wave, r);
    x8_layer_lay<H3, 3, DOUT, 0x5>(wave, r);
    x8_swap<1, 2, 4, 0x5>(wave, lane, lds, fl, r);
    x8_layer_lay<H2, 2, DOUT, 0x5>(wave, r);
    x8_swap<1, 1, 5, 0x5>(wave, lane, lds, fl, r);
    x8_layer_lay<H1, 1, DOUT, 0x5>(wave, r);
    x8_swap<1, 0, 6, 0x5>(wave, lane, lds, fl, r);
    const TileIO out_io = tile_io<0>(p, tile, lane, p.out_block_stride);
    if (__builtin_amdgcn_ballot_w64(qall != 0) == 0) return;
    x8_layer_lay<H0, 0, DOUT, 0x5>(wave, r);
    static_for<2>([&](auto U) {
      constexpr int t = 2 * decltype(U)::value;
      const uint32_t sh = 2 * wave + (t >> 1);  // H0 position of live slot t
      if (sh < p.n_out) store_shard(p.out + sh * p.out_shard_stride, out_io, (qall >> (4 * (t >> 1))) & 15u, r[t]);
    });
    return;
  }
  x8_layer<3, 4, true, DIN>(wave, r);
  x8_layer<3, 4, false, DOUT>(wave, r);
  x8_layer<3, 3, false, DOUT>(wave, r);
  x8_swap<0, 2, 4>(wave, lane, lds, fl, r);
  x8_layer<2, 2, false, DOUT>(wave, r);
  x8_swap<1, 1, 5>(wave, lane, lds, fl, r);
  x8_layer<1, 1, false, DOUT>(wave, r);
  x8_swap<0, 0, 6>(wave, lane, lds, fl, r);
  const TileIO out_io = tile_io<0>(p, tile, lane, p.out_block_stride);
  // slots some lane stores (wave-uniform), as in xform8_tile
  uint32_t need = 0;
  static_for<4>([&](auto T) {
    constexpr int t = decltype(T)::value;
    if (__builtin_amdgcn_ballot_w64(((qall >> (4 * t)) & 15u) != 0) != 0) need |= 1u << t;
  });
  if (need == 0) return;
  {
    using L0 = X8Layout<0>;
    const int v = x8_compress<L0::rel(0)>(wave);
    if (need & 3u) x8_bfly_w<L0, 0, false, DOUT, 0>(v, r[0], r[1], (need & 2u) != 0);
    if (need & 12u) x8_bfly_w<L0, 0, false, DOUT, 2>(v, r[2], r[3], (need & 8u) != 0);
  }
  static_for<4>([&](auto T) {
    constexpr int t = decltype(T)::value;
    const uint32_t sh = 4 * wave + t;  // wave-uniform
    if (((need >> t) & 1u) && sh < p.n_out)
      store_shard(p.out + sh * p.out_shard_stride, out_io, (qall >> (4 * t)) & 15u, r[t]);
  });
}

}  // namespace

}  // namespace ag
