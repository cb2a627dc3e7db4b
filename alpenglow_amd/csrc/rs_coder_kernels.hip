// Byte movers around the coder (gfx950 / CDNA4): ReedSolomonCoder's shred padding and strip,
// the restride between packed and 64-byte-padded shard layouts, and the synthetic input fill.
//
// Kernels
//   coder_pad_kernel, coder_strip_kernel   payload || 0x80 || 0... padding, marker search
//   restride_kernel, unpack_tail_kernel    shard layouts for sizes that are no multiple of 64
//   fill_splitmix_kernel                   input blocks for bench / tests, generated on the device
#include <hip/hip_runtime.h>

#include <algorithm>

#include "rs_device.hpp"
#include "rs_launch.hpp"
#include "unaligned.hpp"

namespace ag {
namespace {

// =====================================================================================
// ReedSolomonCoder batch helpers (reed_solomon.rs:88-128 shred padding, :190-203 strip)
// =====================================================================================
// Data region of slice b (32 * S bytes at cw + b * cw_stride) := payload || 0x80 || 0...
// (payload == null: the payload already sits in the data region; only the padding is
// written).  One thread per 16 output bytes.
// One workgroup per slice, its threads striding over the slice's 16-byte pieces: with a
// payload source every piece is copied (the tail piece merged with 0x80 00..); in place
// (payload null) only the pieces from the one holding byte `len` are written -- a maximum
// slice's padding is one piece, where the earlier one-thread-per-piece grid read every
// piece's length word and divided for it (0.3 ms per 65 536 slices for one byte each).
__global__ __launch_bounds__(256) void coder_pad_kernel(const uint8_t* __restrict__ payload, uint64_t payload_stride,
                                                        const uint32_t* __restrict__ lens, uint8_t* cw,
                                                        uint64_t cw_stride, uint32_t data_bytes, uint64_t nslices) {
  // with a payload one workgroup copies one slice; in place (payload null) only the pieces
  // from byte len on change, so a wave serves one slice and a workgroup four (dispatch-bound
  // otherwise: 65 536 one-wave workgroups took 25 us for one piece each)
  const uint64_t b = payload ? blockIdx.x : static_cast<uint64_t>(blockIdx.x) * 4 + (threadIdx.x >> 6);
  if (b >= nslices) return;
  const uint32_t tid = payload ? threadIdx.x : (threadIdx.x & 63), nt = payload ? blockDim.x : 64;
  const uint32_t per = data_bytes / 16;
  const uint32_t len = lens[b];
  uint8_t* base = cw + b * cw_stride;
  const uint8_t* src = payload ? payload + b * payload_stride : nullptr;
  const bool a16 = src && (reinterpret_cast<uintptr_t>(src) & 15) == 0;
  for (uint32_t piece = (src ? 0u : len / 16) + tid; piece < per; piece += nt) {
    const uint32_t j = piece * 16;
    uint8_t* dst = base + j;
    if (j + 16 <= len) {  // whole payload piece (only with a source)
      if (a16) {
        *reinterpret_cast<uint4*>(dst) = *reinterpret_cast<const uint4*>(src + j);
      } else {
        for (int i = 0; i < 16; ++i) dst[i] = src[j + i];
      }
      continue;
    }
    if (j >= len + 1) {  // padding zeros only
      *reinterpret_cast<uint4*>(dst) = make_uint4(0, 0, 0, 0);
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

// Shard restride for shard sizes that are not whole 64-byte chunks (the
// crate stores the last T = S mod 64 bytes as T/2 low bytes then T/2 high bytes of T/2
// symbols).  pack: shard (S bytes, any alignment) -> padded shard of Sp = ceil(S/64)*64
// bytes whose last chunk holds the tail symbols in whole-chunk layout (low bytes at 0..,
// high bytes at 32..) with zero symbols after them; unpack is the inverse and writes only
// the shards selected by the store mask.  A pack mask skips shards (the decoders never read
// an absent shard, so its padded slot may keep stale bytes).  Zero symbols are zero columns of every linear
// transform, so the bitsliced kernels run on the padded shards unchanged.
struct RestrideParams {
  const uint8_t* src;
  uint64_t src_block_stride, src_shard_stride;
  uint8_t* dst;
  uint64_t dst_block_stride, dst_shard_stride;
  uint32_t S, Sp, nshards, unpack;
  uint64_t nblocks;
  const uint64_t* mask;  // unpack: store shard s of block b iff bit s of mask[per_block ? b : 0]
  uint32_t mask_per_block;
};
// padded offset q -> offset in the crate-layout shard, or -1 (a zero symbol's byte)
__device__ __forceinline__ int64_t restride_src(uint32_t q, uint32_t S) {
  const uint32_t whole = S >> 6, h = (S & 63) >> 1;
  if (q < 64 * whole) return q;
  const uint32_t w = q - 64 * whole;
  if (w < 32) return w < h ? static_cast<int64_t>(64 * whole + w) : -1;
  return w - 32 < h ? static_cast<int64_t>(64 * whole + h + (w - 32)) : -1;
}
// 16 bytes at a 2-byte-aligned (or better) address as 4 little-endian dwords
__device__ __forceinline__ uint4 load16_a2(const uint8_t* src) {
  const uintptr_t a = reinterpret_cast<uintptr_t>(src);
  if ((a & 15) == 0) return *reinterpret_cast<const uint4*>(src);
  if ((a & 7) == 0) {
    const uint2 lo = reinterpret_cast<const uint2*>(src)[0], hi = reinterpret_cast<const uint2*>(src)[1];
    return make_uint4(lo.x, lo.y, hi.x, hi.y);
  }
  if ((a & 3) == 0) {
    const uint32_t* d = reinterpret_cast<const uint32_t*>(src);
    return make_uint4(d[0], d[1], d[2], d[3]);
  }
  // a % 4 == 2: the middle three dwords are aligned; the outer half-dwords are read as
  // 16-bit loads so that nothing outside [a, a + 16) is touched
  const uint32_t* d = reinterpret_cast<const uint32_t*>(a + 2);
  const uint32_t d0 = static_cast<uint32_t>(*reinterpret_cast<const uint16_t*>(src)) << 16;
  const uint32_t d1 = d[0], d2 = d[1], d3 = d[2];
  const uint32_t d4 = *reinterpret_cast<const uint16_t*>(src + 14);
  return make_uint4(__builtin_amdgcn_alignbyte(d1, d0, 2), __builtin_amdgcn_alignbyte(d2, d1, 2),
                    __builtin_amdgcn_alignbyte(d3, d2, 2), __builtin_amdgcn_alignbyte(d4, d3, 2));
}
__device__ __forceinline__ void store16_a2(uint8_t* dst, uint4 v) {
  const uintptr_t a = reinterpret_cast<uintptr_t>(dst);
  if ((a & 15) == 0) {
    *reinterpret_cast<uint4*>(dst) = v;
  } else if ((a & 7) == 0) {
    reinterpret_cast<uint2*>(dst)[0] = make_uint2(v.x, v.y);
    reinterpret_cast<uint2*>(dst)[1] = make_uint2(v.z, v.w);
  } else if ((a & 3) == 0) {
    uint32_t* d = reinterpret_cast<uint32_t*>(dst);
    d[0] = v.x;
    d[1] = v.y;
    d[2] = v.z;
    d[3] = v.w;
  } else {  // a % 4 == 2: a half-dword, three dwords, a half-dword
    uint16_t* h = reinterpret_cast<uint16_t*>(dst);
    uint32_t* d = reinterpret_cast<uint32_t*>(dst + 2);
    h[0] = static_cast<uint16_t>(v.x);
    d[0] = __builtin_amdgcn_alignbyte(v.y, v.x, 2);
    d[1] = __builtin_amdgcn_alignbyte(v.z, v.y, 2);
    d[2] = __builtin_amdgcn_alignbyte(v.w, v.z, 2);
    h[7] = static_cast<uint16_t>(v.w >> 16);
  }
}

// One thread per 16 bytes of the padded shard.  Whole chunks move as 16-byte pieces (shard
// sizes are even, so the crate-layout side is at least 2-byte aligned when its strides
// are even); the tail chunk and odd strides go byte by byte.
__global__ __launch_bounds__(256) void restride_kernel(const RestrideParams p) {
  // one thread per 16-byte piece of the padded layout, flattened over (block, shard, piece):
  // small tails (4 pieces per shard) fill whole workgroups
  const uint32_t per_shard = p.Sp / 16, per_block = per_shard * p.nshards;
  const uint64_t gid = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  const uint64_t b = gid / per_block;
  if (b >= p.nblocks) return;
  const uint32_t r = static_cast<uint32_t>(gid - b * per_block);
  const uint32_t sh = r / per_shard, u = r - sh * per_shard;
  const uint32_t q = 16 * u;
  const bool whole = q + 16 <= 64 * (p.S >> 6);
  if (p.mask && !((p.mask[p.mask_per_block ? b : 0] >> sh) & 1)) return;  // shard not selected
  if (!p.unpack) {
    const uint8_t* src = p.src + b * p.src_block_stride + sh * p.src_shard_stride;
    uint4* dst = reinterpret_cast<uint4*>(p.dst + b * p.dst_block_stride + sh * p.dst_shard_stride + q);
    if (whole && (reinterpret_cast<uintptr_t>(src) & 1) == 0) {
      *dst = load16_a2(src + q);
    } else if (!whole && (reinterpret_cast<uintptr_t>(src) & 1) == 0) {
      // a tail piece: L <= 16 contiguous source bytes (low or high half of the tail
      // symbols), read as the aligned dwords holding them (never past a dword with a valid
      // byte, so never across a page), funnel-shifted, bytes past L zeroed
      const uint32_t tb = 64 * (p.S >> 6), h = (p.S & 63) >> 1, w = q - tb;
      const uint32_t off = w & 31, start = tb + (w < 32 ? 0 : h) + off;
      const uint32_t L = off < h ? min(16u, h - off) : 0u;
      uint32_t v[4] = {0, 0, 0, 0};
      if (L) {
        const uintptr_t a = reinterpret_cast<uintptr_t>(src + start);
        const uint32_t* base = reinterpret_cast<const uint32_t*>(a & ~uintptr_t{3});
        const uint32_t sh = static_cast<uint32_t>(a & 3), nd = (sh + L + 3) >> 2;
        uint32_t d[5];
#pragma unroll
        for (uint32_t j = 0; j < 5; ++j) d[j] = base[min(j, nd - 1)];
#pragma unroll
        for (uint32_t j = 0; j < 4; ++j) {
          const uint32_t x = __builtin_amdgcn_alignbyte(d[j + 1], d[j], sh);
          const uint32_t nb = L > 4 * j ? min(4u, L - 4 * j) : 0u;
          v[j] = nb >= 4 ? x : x & ((1u << (8 * nb)) - 1);
        }
      }
      *dst = make_uint4(v[0], v[1], v[2], v[3]);
    } else {
      // 16 independent byte loads (a zero symbol's byte reads the tail's first byte and is
      // masked): a conditional load per byte serialised 16 memory latencies per wave
      const int64_t tb = 64 * (p.S >> 6);
      uint32_t v[4] = {0, 0, 0, 0};
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const int64_t o = restride_src(q + i, p.S);
        const uint32_t x = src[o >= 0 ? o : tb];
        v[i >> 2] |= (o >= 0 ? x : 0u) << (8 * (i & 3));
      }
      *dst = make_uint4(v[0], v[1], v[2], v[3]);
    }
  } else {
    const uint4 v = *reinterpret_cast<const uint4*>(p.src + b * p.src_block_stride + sh * p.src_shard_stride + q);
    uint8_t* dst = p.dst + b * p.dst_block_stride + sh * p.dst_shard_stride;
    if (whole && (reinterpret_cast<uintptr_t>(dst) & 1) == 0) {
      store16_a2(dst + q, v);
    } else {
      // a tail piece is one run of L <= 16 contiguous destination bytes (the low or high
      // half of the tail symbols): dword stores when the run is dword-aligned and whole
      const uint32_t w[4] = {v.x, v.y, v.z, v.w};
      const uint32_t tb = 64 * (p.S >> 6), h = (p.S & 63) >> 1, wq = q - tb;
      const uint32_t off = wq & 31, start = tb + (wq < 32 ? 0 : h) + off;
      const uint32_t L = whole ? 16u : (off < h ? min(16u, h - off) : 0u);
      if (!whole && ((reinterpret_cast<uintptr_t>(dst + start) | L) & 3) == 0) {
        uint32_t* d4 = reinterpret_cast<uint32_t*>(dst + start);
#pragma unroll
        for (uint32_t j = 0; j < 4; ++j)
          if (4 * j < L) d4[j] = w[j];
      } else {
        for (int i = 0; i < 16; ++i) {
          const int64_t o = restride_src(q + i, p.S);
          if (o >= 0) dst[o] = static_cast<uint8_t>(w[i >> 2] >> (8 * (i & 3)));
        }
      }
    }
  }
}

// Unpack of tail-only shards (0 < S < 64: one padded chunk per shard) to an even destination.
// The workgroup stages its 64 chunks in LDS; then the four threads of a shard write the S
// destination bytes as aligned dwords, with half-dwords at the two ends.  The per-piece path
// above falls back to byte stores for every run that starts off a dword: 3 of the 4 runs of
// a 62-byte tail.
__global__ __launch_bounds__(256) void unpack_tail_kernel(const RestrideParams p) {
  __shared__ uint4 chunk[256];
  const uint32_t t = threadIdx.x, u = t & 3;
  const uint64_t g = (static_cast<uint64_t>(blockIdx.x) * 256 + t) >> 2;  // (block, shard)
  const uint64_t b = g / p.nshards;
  const uint32_t sh = static_cast<uint32_t>(g - b * p.nshards);
  const bool sel = b < p.nblocks && (!p.mask || ((p.mask[p.mask_per_block ? b : 0] >> sh) & 1));
  if (sel)
    chunk[t] = *reinterpret_cast<const uint4*>(p.src + b * p.src_block_stride + sh * p.src_shard_stride + 16 * u);
  __syncthreads();
  if (!sel) return;
  const uint8_t* c = reinterpret_cast<const uint8_t*>(chunk + (t & ~3u));
  const int32_t T = static_cast<int32_t>(p.S), h = T >> 1;
  uint8_t* a = p.dst + b * p.dst_block_stride + sh * p.dst_shard_stride;
  const int32_t lead = static_cast<int32_t>(reinterpret_cast<uintptr_t>(a) & 3);  // 0 or 2
  uint8_t* a0 = a - lead;
  const int32_t nd = (lead + T + 3) >> 2;
  for (int32_t j = static_cast<int32_t>(u); j < nd; j += 4) {
    const int32_t i0 = 4 * j - lead;  // destination byte of the dword's first byte
    uint32_t x = 0;
#pragma unroll
    for (int32_t s = 0; s < 4; ++s) {
      // destination byte i: the low symbol bytes (padded 0..h-1), then the high (32..)
      const int32_t i = i0 + s;
      if (i >= 0 && i < T) x |= static_cast<uint32_t>(c[i < h ? i : 32 + i - h]) << (8 * s);
    }
    if (i0 >= 0 && i0 + 4 <= T) *reinterpret_cast<uint32_t*>(a0 + 4 * j) = x;
    else if (i0 < 0) *reinterpret_cast<uint16_t*>(a0 + 4 * j + 2) = static_cast<uint16_t>(x >> 16);
    else *reinterpret_cast<uint16_t*>(a0 + 4 * j) = static_cast<uint16_t>(x);
  }
}

// Per slice: payload length after stripping the bit padding (trailing zeros, then a 0x80
// marker), or -1 when the padding is invalid.  One workgroup per slice.
// Padding strip (reed_solomon.rs:191-203): the last non-zero byte of the data region must
// be 0x80.  The padding sits at the end, so the workgroup scans 4 KiB windows backwards
// with 16-byte loads and stops at the first window holding a non-zero byte.
// Padding strip (reed_solomon.rs:189-202): the last nonzero byte of the slice's data region
// must be the 0x80 marker.  One wave per slice scans back from the end in 1 KiB windows (one
// 16-byte piece per lane, a ballot picks the highest lane with a nonzero byte): a maximum
// slice's marker lies in its last shred, so the wave reads 1 KiB and never synchronises.
__global__ __launch_bounds__(256) void coder_strip_kernel(const uint8_t* __restrict__ cw, uint64_t cw_stride,
                                                          uint32_t data_bytes, uint64_t nslices, int64_t* out) {
  const uint64_t b = static_cast<uint64_t>(blockIdx.x) * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (b >= nslices) return;  // wave-uniform
  const uint8_t* d = cw + b * cw_stride;
  const bool a16 = ((reinterpret_cast<uintptr_t>(cw) | cw_stride) & 15) == 0;
  int64_t found = -1;
  for (int64_t hi = data_bytes; hi > 0 && found < 0; hi -= 1024) {  // data_bytes % 16 == 0
    const int64_t i0 = hi - 1024 + 16 * static_cast<int64_t>(lane);
    int32_t last = -1;  // highest nonzero byte of this lane's piece
    if (i0 >= 0) {
      uint32_t w[4];
      if (a16) {
        const uint4 x = *reinterpret_cast<const uint4*>(d + i0);
        w[0] = x.x;
        w[1] = x.y;
        w[2] = x.z;
        w[3] = x.w;
      } else {
        for (int q = 0; q < 4; ++q)
          w[q] = d[i0 + 4 * q] | d[i0 + 4 * q + 1] << 8 | d[i0 + 4 * q + 2] << 16 | static_cast<uint32_t>(d[i0 + 4 * q + 3]) << 24;
      }
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

// =====================================================================================
// splitmix64 fill (same generator as oracle/rs_oracle.py splitmix64_bytes)
// =====================================================================================
__global__ __launch_bounds__(256) void fill_splitmix_kernel(uint8_t* dst, uint64_t nblocks, uint64_t words_per_block,
                                                            uint64_t dst_block_stride, uint64_t seed_base) {
  const uint64_t tid = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  const uint64_t pairs = (words_per_block + 1) / 2;
  if (tid >= nblocks * pairs) return;
  const uint64_t b = tid / pairs;
  const uint64_t w0 = (tid - b * pairs) * 2;
  uint64_t out[2];
  for (int q = 0; q < 2; ++q) {
    uint64_t z = seed_base + b + (w0 + q + 1) * 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    out[q] = z ^ (z >> 31);
  }
  uint64_t* d = reinterpret_cast<uint64_t*>(dst + b * dst_block_stride) + w0;
  d[0] = out[0];
  if (w0 + 1 < words_per_block) d[1] = out[1];
}

}  // namespace

// ---- launchers ----------------------------------------------------------------------
hipError_t launch_coder_pad(const uint8_t* payload, uint64_t payload_stride, const uint32_t* lens, uint8_t* cw,
                            uint64_t cw_stride, uint32_t data_bytes, uint64_t nslices, hipStream_t stream) {
  if (data_bytes % 16) return hipErrorInvalidValue;
  if (nslices == 0 || data_bytes == 0) return hipSuccess;
  if (nslices > 0x7FFFFFFFull) return hipErrorInvalidValue;
  const uint64_t groups = payload ? nslices : (nslices + 3) / 4;
  hipLaunchKernelGGL(coder_pad_kernel, dim3(static_cast<unsigned>(groups)), dim3(256), 0, stream, payload,
                     payload_stride, lens, cw, cw_stride, data_bytes, nslices);
  return hipGetLastError();
}

hipError_t launch_restride(const uint8_t* src, uint64_t src_block_stride, uint64_t src_shard_stride, uint8_t* dst,
                           uint64_t dst_block_stride, uint64_t dst_shard_stride, uint32_t S, uint32_t nshards,
                           uint64_t nblocks, bool unpack, const uint64_t* mask, bool mask_per_block,
                           hipStream_t stream) {
  RestrideParams p{};
  p.src = src;
  p.src_block_stride = src_block_stride;
  p.src_shard_stride = src_shard_stride;
  p.dst = dst;
  p.dst_block_stride = dst_block_stride;
  p.dst_shard_stride = dst_shard_stride;
  p.S = S;
  p.Sp = (S + 63) / 64 * 64;
  p.nshards = nshards;
  p.unpack = unpack ? 1u : 0u;
  p.nblocks = nblocks;
  p.mask = mask;
  p.mask_per_block = mask_per_block ? 1u : 0u;
  const uint64_t per_block = static_cast<uint64_t>(nshards) * (p.Sp / 16);
  if (per_block == 0 || nblocks == 0) return hipSuccess;
  const uint64_t groups = (per_block * nblocks + 255) / 256;
  if (per_block > 0x7FFFFFFFull || groups > 0x7FFFFFFFull) return hipErrorInvalidValue;
  // tail-only unpack to an even destination (S even: the sizes are whole symbols)
  if (unpack && S > 0 && S < 64 && S % 2 == 0 &&
      ((reinterpret_cast<uintptr_t>(dst) | dst_block_stride | dst_shard_stride) & 1) == 0) {
    hipLaunchKernelGGL(unpack_tail_kernel, dim3(static_cast<unsigned>(groups)), dim3(256), 0, stream, p);
    return hipGetLastError();
  }
  hipLaunchKernelGGL(restride_kernel, dim3(static_cast<unsigned>(groups)), dim3(256), 0, stream, p);
  return hipGetLastError();
}

hipError_t launch_coder_strip(const uint8_t* cw, uint64_t cw_stride, uint32_t data_bytes, uint64_t nslices,
                              int64_t* out, hipStream_t stream) {
  if (nslices == 0) return hipSuccess;
  if (data_bytes % 16) return hipErrorInvalidValue;
  const uint64_t groups = (nslices + 3) / 4;  // one wave per slice
  if (groups > 0x7FFFFFFFull) return hipErrorInvalidValue;
  hipLaunchKernelGGL(coder_strip_kernel, dim3(static_cast<unsigned>(groups)), dim3(256), 0, stream, cw, cw_stride,
                     data_bytes, nslices, out);
  return hipGetLastError();
}

hipError_t launch_fill_splitmix(uint8_t* dst, uint64_t nblocks, uint64_t block_bytes, uint64_t dst_block_stride,
                                uint64_t seed_base, hipStream_t stream) {
  if (block_bytes % 8) return hipErrorInvalidValue;
  const uint64_t words = block_bytes / 8, pairs = (words + 1) / 2;
  if (nblocks == 0 || pairs == 0) return hipSuccess;
  if (pairs > (uint64_t{1} << 30)) return hipErrorInvalidValue;
  // a dispatch's grid is at most 2^32 - 1 work-items (HSA packet): launches of at most 2^30
  // threads' worth of whole blocks (BASELINE configs[4]'s 64 GiB stream at N = 1 is 2^32 pairs)
  const uint64_t per = std::max<uint64_t>(1, (uint64_t{1} << 30) / pairs);
  for (uint64_t b0 = 0; b0 < nblocks; b0 += per) {
    const uint64_t nb = std::min(per, nblocks - b0), n = nb * pairs;
    hipLaunchKernelGGL(fill_splitmix_kernel, dim3(static_cast<unsigned>((n + 255) / 256)), dim3(256), 0, stream,
                       dst + b0 * dst_block_stride, nb, words, dst_block_stride, seed_base + b0);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

}  // namespace ag
