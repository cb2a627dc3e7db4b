// The table-driven path of the Reed-Solomon shredder (gfx950 / CDNA4): the crate's algorithm
// with log/exp tables for every geometry (correctness path: multi-chunk HighRate, LowRate,
// exact decode with any erasures).
// What they replace: the reed-solomon-simd 3.1.0 calls inside ReedSolomonCoder (encode,
// decode, re-encode).  Arithmetic: GF(2^16) Leopard additive FFT.
//
// Kernels
//   generic_encode_kernel, generic_decode_kernel   one thread per (block, symbol position)
//   locator_kernel   erasure-locator logs (crate eval_poly: FWHT over 65536 in LDS)
#include <hip/hip_runtime.h>

#include "rs_device.hpp"
#include "rs_launch.hpp"

namespace ag {
namespace {

// =====================================================================================
// Generic kernels: one thread per (block, symbol position); the crate's algorithm with
// log/exp tables, work rows in a global scratch column (stride nsym).
// =====================================================================================

struct SymAddr {
  uint32_t lo, hi;
};
__device__ __forceinline__ SymAddr sym_addr(uint32_t j, uint32_t shard_bytes) {
  const uint32_t c = j >> 5, jj = j & 31, whole = shard_bytes >> 6;
  if (c < whole) return {64 * c + jj, 64 * c + 32 + jj};
  const uint32_t h = (shard_bytes & 63) >> 1;
  return {64 * whole + jj, 64 * whole + h + jj};
}

struct Col {
  uint16_t* w;
  uint64_t st;
  __device__ uint16_t& operator[](uint32_t i) const { return w[i * st]; }
};

__device__ void g_fft(const Col& w, const GfDeviceTables& t, uint32_t pos, uint32_t size, uint32_t trunc,
                      uint32_t delta) {
  for (uint32_t dist = size >> 1; dist >= 1; dist >>= 1) {
    for (uint32_t r = 0; r < trunc; r += 2 * dist) {
      const uint16_t lm = t.skew[r + dist + delta - 1];
      for (uint32_t i = r; i < r + dist; ++i) {
        uint16_t x = w[pos + i], y = w[pos + i + dist];
        if (lm != 65535) x ^= dev::gmul(t.exp, t.log, y, lm);
        y ^= x;
        w[pos + i] = x;
        w[pos + i + dist] = y;
      }
    }
  }
}

__device__ void g_ifft(const Col& w, const GfDeviceTables& t, uint32_t pos, uint32_t size, uint32_t trunc,
                       uint32_t delta) {
  for (uint32_t dist = 1; dist < size; dist <<= 1) {
    for (uint32_t r = 0; r < trunc; r += 2 * dist) {
      const uint16_t lm = t.skew[r + dist + delta - 1];
      for (uint32_t i = r; i < r + dist; ++i) {
        uint16_t x = w[pos + i], y = w[pos + i + dist];
        y ^= x;
        if (lm != 65535) x ^= dev::gmul(t.exp, t.log, y, lm);
        w[pos + i] = x;
        w[pos + i + dist] = y;
      }
    }
  }
}

__global__ __launch_bounds__(256) void generic_encode_kernel(const GenericEncodeParams p) {
  const uint64_t tid = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (tid >= p.nblocks * p.nsym) return;
  const uint64_t b = tid / p.nsym;
  const uint32_t j = static_cast<uint32_t>(tid - b * p.nsym);
  const SymAddr a = sym_addr(j, p.shard_bytes);
  const Col w{p.scratch + b * p.rows * p.nsym + j, p.nsym};
  const uint8_t* ob = p.orig + b * p.orig_block_stride;
  for (uint32_t i = 0; i < p.rows; ++i) {
    uint16_t v = 0;
    if (i < p.k) {
      const uint8_t* s = ob + i * p.orig_shard_stride;
      v = static_cast<uint16_t>(s[a.lo] | (s[a.hi] << 8));
    }
    w[i] = v;
  }
  const uint32_t chunk = p.chunk, k = p.k, m = p.m;
  if (p.high_rate) {
    g_ifft(w, p.t, 0, chunk, k < chunk ? k : chunk, chunk);
    if (k > chunk) {
      uint32_t cs = chunk;
      for (; cs + chunk <= k; cs += chunk) {
        g_ifft(w, p.t, cs, chunk, chunk, cs + chunk);
        for (uint32_t i = 0; i < chunk; ++i) w[i] ^= w[cs + i];
      }
      const uint32_t last = k % chunk;
      if (last) {
        g_ifft(w, p.t, cs, chunk, last, cs + chunk);
        for (uint32_t i = 0; i < chunk; ++i) w[i] ^= w[cs + i];
      }
    }
    g_fft(w, p.t, 0, chunk, m, 0);
  } else {
    g_ifft(w, p.t, 0, chunk, k, 0);
    for (uint32_t cs = chunk; cs < m; cs += chunk)
      for (uint32_t i = 0; i < chunk; ++i) w[cs + i] = w[i];
    uint32_t cs = 0;
    for (; cs + chunk <= m; cs += chunk) g_fft(w, p.t, cs, chunk, chunk, cs + chunk);
    if (m % chunk) g_fft(w, p.t, cs, chunk, m % chunk, cs + chunk);
  }
  uint8_t* rb = p.rec + b * p.rec_block_stride;
  for (uint32_t i = 0; i < m; ++i) {
    uint8_t* s = rb + i * p.rec_shard_stride;
    const uint16_t v = w[i];
    s[a.lo] = static_cast<uint8_t>(v);
    s[a.hi] = static_cast<uint8_t>(v >> 8);
  }
}

__global__ __launch_bounds__(256) void generic_decode_kernel(const GenericDecodeParams p) {
  const uint64_t tid = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (tid >= p.nblocks * p.nsym) return;
  const uint64_t bi = tid / p.nsym;
  const uint32_t j = static_cast<uint32_t>(tid - bi * p.nsym);
  const uint64_t b = p.block_ids ? p.block_ids[bi] : p.block_base + bi;
  const uint64_t pat = p.pattern_per_block ? b : 0;
  const uint8_t* op = p.orig_present + pat * p.k;
  const uint8_t* rp = p.rec_present + pat * p.m;
  const uint16_t* loc = p.loc + pat * p.W;
  const SymAddr a = sym_addr(j, p.shard_bytes);
  const Col w{p.scratch + bi * p.W * p.nsym + j, p.nsym};
  const uint32_t opos = p.high_rate ? p.chunk : 0, rpos = p.high_rate ? 0 : p.chunk;
  for (uint32_t i = 0; i < p.W; ++i) w[i] = 0;
  uint8_t* ob = p.orig + b * p.orig_block_stride;
  const uint8_t* rbk = p.rec + b * p.rec_block_stride;
  for (uint32_t i = 0; i < p.k; ++i)
    if (op[i]) {
      const uint8_t* s = ob + i * p.orig_shard_stride;
      w[opos + i] = dev::gmul(p.t.exp, p.t.log, static_cast<uint16_t>(s[a.lo] | (s[a.hi] << 8)), loc[opos + i]);
    }
  for (uint32_t i = 0; i < p.m; ++i)
    if (rp[i]) {
      const uint8_t* s = rbk + i * p.rec_shard_stride;
      w[rpos + i] = dev::gmul(p.t.exp, p.t.log, static_cast<uint16_t>(s[a.lo] | (s[a.hi] << 8)), loc[rpos + i]);
    }
  g_ifft(w, p.t, 0, p.W, p.end, 0);
  for (uint32_t i = 1; i < p.W; ++i) {  // formal derivative
    const uint32_t width = i & (~i + 1);
    for (uint32_t q = 0; q < width; ++q) w[i - width + q] ^= w[i + q];
  }
  g_fft(w, p.t, 0, p.W, p.high_rate ? p.end : p.k, 0);
  for (uint32_t i = 0; i < p.k; ++i)
    if (!op[i]) {
      const uint16_t v = dev::gmul(p.t.exp, p.t.log, w[opos + i], static_cast<uint16_t>(65535 - loc[opos + i]));
      uint8_t* s = ob + i * p.orig_shard_stride;
      s[a.lo] = static_cast<uint8_t>(v);
      s[a.hi] = static_cast<uint8_t>(v >> 8);
    }
}

// =====================================================================================
// Erasure locator: the crate's eval_poly (FWHT, pointwise x log_walsh, FWHT), mod 65535,
// one 1024-thread workgroup per pattern with the 65536-entry vector in LDS (128 KiB).
// =====================================================================================
__device__ __forceinline__ void fwht_lds(uint16_t* buf) {
  for (uint32_t dist = 1; dist < 65536; dist <<= 1) {
    for (uint32_t idx = threadIdx.x; idx < 32768; idx += blockDim.x) {
      const uint32_t i = (idx / dist) * 2 * dist + (idx % dist);
      const uint16_t a = buf[i], b = buf[i + dist];
      buf[i] = dev::add_mod(a, b);
      buf[i + dist] = dev::sub_mod(a, b);
    }
    __syncthreads();
  }
}

__global__ __launch_bounds__(1024) void locator_kernel(const uint8_t* erased, uint32_t W, uint32_t fill_from,
                                                       const uint16_t* log_walsh, uint16_t* loc) {
  __shared__ uint16_t buf[65536];
  const uint64_t pat = blockIdx.x;
  for (uint32_t x = threadIdx.x; x < 65536; x += blockDim.x)
    buf[x] = x < W ? (erased[pat * W + x] ? 1 : 0) : (x >= fill_from ? 1 : 0);
  __syncthreads();
  fwht_lds(buf);
  for (uint32_t x = threadIdx.x; x < 65536; x += blockDim.x) {
    const uint32_t prod = static_cast<uint32_t>(buf[x]) * log_walsh[x];
    buf[x] = dev::add_mod(prod & 0xFFFF, prod >> 16);
  }
  __syncthreads();
  fwht_lds(buf);
  for (uint32_t x = threadIdx.x; x < W; x += blockDim.x) loc[pat * W + x] = buf[x];
}

}  // namespace

// ---- launchers ----------------------------------------------------------------------
hipError_t launch_generic_encode(const GenericEncodeParams& p, hipStream_t stream) {
  const uint64_t n = p.nblocks * p.nsym;
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(generic_encode_kernel, dim3(static_cast<unsigned>((n + 255) / 256)), dim3(256), 0, stream, p);
  return hipGetLastError();
}

hipError_t launch_generic_decode(const GenericDecodeParams& p, hipStream_t stream) {
  const uint64_t n = p.nblocks * p.nsym;
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(generic_decode_kernel, dim3(static_cast<unsigned>((n + 255) / 256)), dim3(256), 0, stream, p);
  return hipGetLastError();
}

hipError_t launch_locator(const uint8_t* erased, uint32_t npatterns, uint32_t W, uint32_t fill_from,
                          const uint16_t* log_walsh, uint16_t* loc, hipStream_t stream) {
  if (npatterns == 0) return hipSuccess;
  hipLaunchKernelGGL(locator_kernel, dim3(npatterns), dim3(1024), 0, stream, erased, W, fill_from, log_walsh, loc);
  return hipGetLastError();
}

}  // namespace ag
