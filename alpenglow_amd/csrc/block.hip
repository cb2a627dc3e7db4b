// Block assembly: BlockData::try_reconstruct_block (slot_block_data.rs:376-454) over the rows the
// deshred left in the codeword buffer (include/alpenglow_rs.h section 12).  Per block the verdict
// is a pure function of its rows, and the only thing that crosses blocks is the prefix of the
// transaction counts, so the chain is per-block workgroups and per-row lanes with kernel
// boundaries between them (block.hpp); no kernel waits on another workgroup.
//
// The transaction walk reads only the u64 length prefixes: a lane chases them through its row,
// one dependent load per transaction.  It consumes at least 8 bytes per step, so it is bounded by
// the row's data length (at most 4 094 steps), never by the count the slice claims.  Every read
// is inside [data, data + data_len), which the host has checked to lie inside the row.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/alpenglow_rs.h"
#include "block.hpp"
#include "unaligned.hpp"

namespace ag {

namespace {

constexpr uint32_t kThreads = 256;
constexpr uint32_t kMaxSlices = AG_BLOCK_MAX_SLICES;

__device__ __forceinline__ uint64_t ld_u64(const uint8_t* q) {
  const uint2 v = ld8u(q);
  return v.x | (static_cast<uint64_t>(v.y) << 32);
}

// the rows' parent ids are 8-byte aligned (40-byte rows of an aligned upload)
__device__ __forceinline__ bool same_parent(const uint8_t* a, const uint8_t* b) {
  const uint64_t* x = reinterpret_cast<const uint64_t*>(a);
  const uint64_t* y = reinterpret_cast<const uint64_t*>(b);
  uint64_t d = 0;
#pragma unroll
  for (int q = 0; q < 5; ++q) d |= x[q] ^ y[q];
  return d == 0;
}

// The index of the k-th (k = 0, 1) set bit of the 1024-bit set `m`, or kBlockNone.
__device__ uint32_t nth_set(const uint64_t* m, uint32_t k) {
  for (uint32_t w = 0; w < kMaxSlices / 64; ++w) {
    uint64_t v = m[w];
    const uint32_t c = __popcll(v);
    if (k >= c) {
      k -= c;
      continue;
    }
    if (k) v &= v - 1;
    return 64 * w + (__ffsll(static_cast<long long>(v)) - 1);
  }
  return kBlockNone;
}

// Rules 1 and 3, and the tree's input.  The parent rule needs only the first two slices i > 0
// that carry a parent: the first either repeats slice 0's parent (PARENT_SAME) or switches, the
// second either repeats the switched parent (PARENT_SAME) or is a second switch (PARENT_TWICE);
// whatever comes later is behind the first failure.
__global__ __launch_bounds__(kThreads) void block_scan_kernel(const BlockParams p) {
  __shared__ uint64_t carries[kMaxSlices / 64];  // bit i: slice 0 < i <= l carries a parent
  __shared__ uint32_t s_count;
  const uint32_t b = blockIdx.x, tid = threadIdx.x;
  const uint64_t r0 = static_cast<uint64_t>(b) * p.spb;
  const int32_t l = p.last_slice[b];
  const bool has_last = l >= 0 && static_cast<uint32_t>(l) < p.spb;
  const uint32_t n = has_last ? static_cast<uint32_t>(l) + 1 : 0;
  int ok = 1;
  for (uint32_t base = 0; base < kMaxSlices; base += kThreads) {  // uniform: every lane ballots
    const uint32_t i = base + tid;
    const bool in = i < n;
    if (in && p.row_ok[r0 + i] == 0) ok = 0;
    const uint64_t m = __ballot(in && i > 0 && p.parent_flags[r0 + i] != 0);
    if ((tid & 63) == 0) carries[i / 64] = m;
  }
  ok = __syncthreads_and(ok);  // (also publishes carries)
  if (tid == 0) {
    // a row 0 without a parent was never inserted (slot_block_data.rs:361-364)
    const bool complete = n != 0 && ok && p.parent_flags[r0] != 0;
    uint32_t err = kBlockNone;
    uint8_t code = 0;
    const uint8_t* parent = p.parent_ids + kBlockParentBytes * r0;
    if (complete) {
      const uint32_t i1 = nth_set(carries, 0);
      if (i1 != kBlockNone) {
        const uint8_t* p1 = p.parent_ids + kBlockParentBytes * (r0 + i1);
        if (same_parent(p1, parent)) {
          err = i1;
          code = AG_BLOCK_PARENT_SAME;
        } else {
          parent = p1;
          const uint32_t i2 = nth_set(carries, 1);
          if (i2 != kBlockNone) {
            err = i2;
            code = same_parent(p.parent_ids + kBlockParentBytes * (r0 + i2), p1) ? AG_BLOCK_PARENT_SAME
                                                                                   : AG_BLOCK_PARENT_TWICE;
          }
        }
      }
      const uint64_t* src = reinterpret_cast<const uint64_t*>(parent);
      uint64_t* dst = reinterpret_cast<uint64_t*>(p.cand_parent + kBlockParentBytes * b);
#pragma unroll
      for (int q = 0; q < 5; ++q) dst[q] = src[q];
    }
    p.first[b] = r0;
    p.count[b] = complete ? n : 0;
    p.perr_slice[b] = err;
    p.perr_code[b] = code;
    s_count = complete ? n : 0;
  }
  __syncthreads();
  // the block's roots (stride 49 inside the stores' commitments: no alignment) as 32-byte digests
  const uint32_t words = s_count * 8;
  for (uint32_t w = tid; w < words; w += kThreads) {
    const uint64_t r = r0 + w / 8;
    const uint8_t* src = p.slice_roots + r * p.roots_stride + 4 * (w % 8);
    const uint32_t v = src[0] | (src[1] << 8) | (src[2] << 16) | (static_cast<uint32_t>(src[3]) << 24);
    reinterpret_cast<uint32_t*>(p.roots)[r * 8 + w % 8] = v;
  }
}

// Rule 4 over `len` bytes at `data`: u64 count n, then n times (u64 length, that many bytes),
// exactly len bytes consumed.  With kEmit the entries go to offs / lens (offset of the payload
// from the codeword buffer: data_off is data's), at most emit_cap of them -- the count the first
// walk found, so a buffer the caller changed under the call cannot push a write past the row's
// share of the table.  Returns false where the reference's decode fails.
template <bool kEmit>
__device__ __forceinline__ bool walk(const uint8_t* data, uint32_t len, uint64_t max_txs, uint32_t* cnt_out,
                                     uint32_t* bytes_out, uint64_t data_off, uint64_t* offs, uint32_t* lens,
                                     uint32_t emit_cap) {
  *cnt_out = 0;
  *bytes_out = 0;
  if (len < 8) return false;
  const uint64_t n = ld_u64(data);
  if (max_txs && n > max_txs) return false;
  uint32_t pos = 8, cnt = 0, bytes = 0;
  while (cnt < n) {  // each step consumes >= 8 bytes: at most len / 8 steps
    if (len - pos < 8) return false;
    const uint64_t tx = ld_u64(data + pos);
    pos += 8;
    if (tx > len - pos) return false;  // (u64 against the bytes left: 2^64 - 1 cannot wrap)
    if (kEmit) {
      if (cnt >= emit_cap) return false;
      offs[cnt] = data_off + pos;
      lens[cnt] = static_cast<uint32_t>(tx);
    }
    pos += static_cast<uint32_t>(tx);
    bytes += static_cast<uint32_t>(tx);
    ++cnt;
  }
  if (pos != len) return false;
  *cnt_out = cnt;
  *bytes_out = bytes;
  return true;
}

__device__ __forceinline__ uint32_t data_offset(uint8_t flag) { return flag ? 9 + kBlockParentBytes : 9; }

__global__ __launch_bounds__(kThreads) void block_walk_kernel(const BlockParams p) {
  const uint32_t r = blockIdx.x * kThreads + threadIdx.x;
  if (r >= p.nblocks * p.spb) return;
  const uint32_t b = r / p.spb, i = r - b * p.spb;
  uint32_t cnt = 0, bytes = 0;
  bool good = true;
  if (i < p.count[b]) {  // a candidate block's row: row_ok is set, so offset and length were checked
    const uint32_t off = data_offset(p.parent_flags[r]);
    good = walk<false>(p.codewords + r * p.codeword_stride + off, p.data_lens[r], p.max_txs, &cnt, &bytes, 0,
                       nullptr, nullptr, 0);
  }
  p.row_cnt[r] = cnt;
  p.row_bytes[r] = bytes;
  p.row_bad[r] = good ? 0 : 1;
}

// Exclusive prefix of v over the workgroup's kThreads lanes; *total = the sum.  s: kThreads words.
template <typename T>
__device__ T scan_exclusive(T v, T* s, T* total) {
  const uint32_t tid = threadIdx.x;
  s[tid] = v;
  __syncthreads();
  for (uint32_t d = 1; d < kThreads; d <<= 1) {
    const T add = tid >= d ? s[tid - d] : 0;
    __syncthreads();
    s[tid] += add;
    __syncthreads();
  }
  const T incl = s[tid];
  *total = s[kThreads - 1];
  __syncthreads();
  return incl - v;
}

// The verdict: the first failing slice, the parent rule before the decode within a slice.  Lane
// t owns slices 4t .. 4t + 3.
__global__ __launch_bounds__(kThreads) void block_finish_kernel(const BlockParams p) {
  static_assert(4 * kThreads == kMaxSlices);
  __shared__ uint32_t s_bad;
  __shared__ uint32_t s_scan[kThreads];
  const uint32_t b = blockIdx.x, tid = threadIdx.x;
  const uint64_t r0 = static_cast<uint64_t>(b) * p.spb;
  const uint32_t n = p.count[b];
  if (tid == 0) s_bad = kBlockNone;
  __syncthreads();
  uint32_t cnt[4], csum = 0, bsum = 0;
#pragma unroll
  for (uint32_t q = 0; q < 4; ++q) {
    const uint32_t i = 4 * tid + q;
    cnt[q] = 0;
    if (i < n) {
      if (p.row_bad[r0 + i]) atomicMin(&s_bad, i);  // (LDS, within the workgroup)
      cnt[q] = p.row_cnt[r0 + i];
      bsum += p.row_bytes[r0 + i];
    }
    csum += cnt[q];
  }
  __syncthreads();
  const uint32_t bad = s_bad, perr = p.perr_slice[b];
  uint8_t verdict = AG_BLOCK_COMPLETE;
  uint32_t where = 0;
  if (n == 0) {
    verdict = AG_BLOCK_INCOMPLETE;
  } else if (perr != kBlockNone && perr <= bad) {
    verdict = p.perr_code[b];
    where = perr;
  } else if (bad != kBlockNone) {
    verdict = AG_BLOCK_BAD_TRANSACTIONS;
    where = bad;
  }
  uint32_t ctotal, btotal;
  uint32_t before = scan_exclusive(csum, s_scan, &ctotal);
  (void)scan_exclusive(bsum, s_scan, &btotal);
  const bool complete = verdict == AG_BLOCK_COMPLETE;
#pragma unroll
  for (uint32_t q = 0; q < 4; ++q) {
    const uint32_t i = 4 * tid + q;
    if (i < p.spb) p.row_first[r0 + i] = before;
    before += cnt[q];
  }
  if (tid < kBlockParentBytes)
    p.parents[kBlockParentBytes * b + tid] = complete ? p.cand_parent[kBlockParentBytes * b + tid] : 0;
  if (p.hashes && n != 0 && tid < 2)
    reinterpret_cast<uint4*>(p.hashes)[2 * b + tid] = reinterpret_cast<const uint4*>(p.block_hashes)[2 * b + tid];
  if (tid == 0) {
    p.verdict[b] = verdict;
    p.error_slice[b] = where;
    p.tx_counts[b] = complete ? ctotal : 0;
    p.tx_bytes[b] = complete ? btotal : 0;
  }
}

// tx_first = the exclusive prefix of tx_counts over the blocks, the total, and whether the table
// may be written: one workgroup, 256 blocks a round with a carry.
__global__ __launch_bounds__(kThreads) void block_total_kernel(const BlockParams p) {
  __shared__ uint64_t s_scan[kThreads];
  uint64_t carry = 0;
  for (uint32_t base = 0; base < p.nblocks; base += kThreads) {  // uniform
    const uint32_t b = base + threadIdx.x;
    const uint64_t v = b < p.nblocks ? p.tx_counts[b] : 0;
    uint64_t round;
    const uint64_t before = scan_exclusive(v, s_scan, &round);
    if (b < p.nblocks) p.tx_first[b] = carry + before;
    carry += round;
  }
  if (threadIdx.x == 0) {
    *p.tx_total = carry;
    *p.fit = p.tx_offsets != nullptr && carry <= p.tx_capacity;
  }
}

// The table: the rows of COMPLETE blocks walk again (every one decodes) and write their entries
// at tx_first[b] + row_first[r] ..; nothing when the total does not fit.
__global__ __launch_bounds__(kThreads) void block_index_kernel(const BlockParams p) {
  if (*p.fit == 0) return;
  const uint32_t r = blockIdx.x * kThreads + threadIdx.x;
  if (r >= p.nblocks * p.spb) return;
  const uint32_t b = r / p.spb, i = r - b * p.spb;
  if (p.verdict[b] != AG_BLOCK_COMPLETE || i >= p.count[b]) return;
  const uint64_t e = p.tx_first[b] + p.row_first[r];
  const uint64_t off = r * p.codeword_stride + data_offset(p.parent_flags[r]);
  uint32_t cnt, bytes;
  (void)walk<true>(p.codewords + off, p.data_lens[r], p.max_txs, &cnt, &bytes, off, p.tx_offsets + e, p.tx_lens + e,
                   p.row_cnt[r]);
}

dim3 per_item(uint64_t n) { return dim3(static_cast<unsigned>((n + kThreads - 1) / kThreads)); }

}  // namespace

hipError_t launch_block_scan(const BlockParams& p, hipStream_t stream) {
  hipLaunchKernelGGL(block_scan_kernel, dim3(p.nblocks), dim3(kThreads), 0, stream, p);
  return hipGetLastError();
}
hipError_t launch_block_walk(const BlockParams& p, hipStream_t stream) {
  hipLaunchKernelGGL(block_walk_kernel, per_item(static_cast<uint64_t>(p.nblocks) * p.spb), dim3(kThreads), 0, stream, p);
  return hipGetLastError();
}
hipError_t launch_block_finish(const BlockParams& p, hipStream_t stream) {
  hipLaunchKernelGGL(block_finish_kernel, dim3(p.nblocks), dim3(kThreads), 0, stream, p);
  return hipGetLastError();
}
hipError_t launch_block_total(const BlockParams& p, hipStream_t stream) {
  hipLaunchKernelGGL(block_total_kernel, dim3(1), dim3(kThreads), 0, stream, p);
  return hipGetLastError();
}
hipError_t launch_block_index(const BlockParams& p, hipStream_t stream) {
  hipLaunchKernelGGL(block_index_kernel, per_item(static_cast<uint64_t>(p.nblocks) * p.spb), dim3(kThreads), 0, stream, p);
  return hipGetLastError();
}

}  // namespace ag
