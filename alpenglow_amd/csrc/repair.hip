// Repair intake: the parallel form of "process the repair replies one at a time in arrival
// order" (include/alpenglow_rs.h section 11).  As in intake.hip every sequential rule depends on
// the past only through "the earliest reply that ...", one atomicMin of the arrival index t per
// word, completed by a kernel boundary before the next kernel reads it; no kernel waits on
// another workgroup.  What repair.rs:410-445 changes against the dissemination path:
//   - the row is the request's (block, slice), not the header's: the header only has to agree;
//   - the root proved for the row stands in front of the signature, so a row's pick can only be
//     chosen once the roots are derived;
//   - try_new runs without a cache: every reply's own signature counts.  A reply whose
//     commitment AND signature bytes equal a pair already known valid is the same verification,
//     so it inherits the verdict; an honest block still costs one verification per row;
//   - the leader key belongs to the block: each reply gets a copy of its block's key in a
//     scratch row, which is what the verify launches index.
// Setter, claim, route and finalize are intake's kernels over the same words (repair.hpp).
#include <hip/hip_runtime.h>

#include <cstdint>

#include "intake_device.hpp"
#include "repair.hpp"
#include "wire.hpp"

namespace ag {

namespace {

__device__ __forceinline__ bool same16(uint4 a, uint4 b) {
  return ((a.x ^ b.x) | (a.y ^ b.y) | (a.z ^ b.z) | (a.w ^ b.w)) == 0;
}
// 64 signature bytes at any alignment (the store's rows are the caller's).
__device__ __forceinline__ bool same_sig(const uint8_t* a, const uint8_t* b) {
  bool same = true;
#pragma unroll
  for (int q = 0; q < 4; ++q) same &= same16(ld16u(a + 16 * q), ld16u(b + 16 * q));
  return same;
}

__global__ __launch_bounds__(256) void repair_key_kernel(const RepairParams p) {
  const IntakeParams& in = p.in;
  const uint64_t t = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (t >= in.n) return;
  in.row[t] = kIntakeNone;
  in.plausible[t] = 0;
  const uint32_t len = in.rx_lens[t];
  const uint8_t st = in.wire[t];
  if (len > in.rx_stride || st == kWireMalformed) {  // as intake: no shred at all
    in.verdict[t] = kMalformed;
    return;
  }
  const uint32_t b = p.req_block[t], s = p.req_slice[t], want_j = p.req_index[t];
  if (b >= in.nslots || s >= in.spp || want_j >= kTotalShreds) {
    in.verdict[t] = kOutOfWindow;
    return;
  }
  // the header, as intake_key reads it (the wire check bounded slice index, shred index and data
  // length to their low bytes)
  const uint4* h = reinterpret_cast<const uint4*>(in.rx + t * in.rx_stride);
  const uint4 x = h[0], y = h[1];
  const uint32_t kind = x.x;
  const uint64_t slot = x.y | (static_cast<uint64_t>(x.z) << 32);
  const uint32_t si = x.w;
  const uint32_t is_last = y.y & 0xFFu, j = (y.y >> 8) & 0xFFu, dlen = (y.w >> 8) & 0xFFFFu;
  if (slot != p.block_slots[b] || si != s || j != want_j) {  // repair.rs:417-423
    in.verdict[t] = kRequestMismatch;
    return;
  }
  if (st != kWireOk || kind != (j >= 32 ? 1u : 0u) || dlen == 0 || (dlen & 1u) || dlen > 1024 || in.height[t] != 6) {
    in.verdict[t] = kImplausible;
    return;
  }
  in.row[t] = b * in.spp + s;
  in.meta[t] = j | (is_last << 8) | (dlen << 16);
  in.plausible[t] = 1;
}

__global__ __launch_bounds__(256) void repair_root_kernel(const RepairParams p) {
  const IntakeParams& in = p.in;
  const uint64_t t = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (t >= in.n) return;
  const uint32_t r = in.row[t];
  if (r == kIntakeNone) return;
  if (!p.have_root[r]) {  // repair.rs:424-426: the reference never asks before the root is proved
    in.verdict[t] = kNoRoot;
    in.row[t] = kIntakeNone;
    return;
  }
  const uint4 x = *reinterpret_cast<const uint4*>(in.roots + 32 * t);
  const uint4 y = *reinterpret_cast<const uint4*>(in.roots + 32 * t + 16);
  if (!same16(x, ld16u(p.slice_roots + 32ull * r)) || !same16(y, ld16u(p.slice_roots + 32ull * r + 16))) {
    in.verdict[t] = kWrongRoot;  // repair.rs:428-432: no signature check
    in.row[t] = kIntakeNone;
    return;
  }
  const uint32_t root[8] = {x.x, x.y, x.z, x.w, y.x, y.y, y.z, y.w};
  store_commit(in.commit + kIntakeCommitStride * t,
               make_commit(in.slot[t], in.slice_index[t], meta_last(in.meta[t]), root));
  const uint8_t* pk = p.pks + 32ull * (r / in.spp);
  uint4* key = reinterpret_cast<uint4*>(p.keys + 32 * t);
  key[0] = ld16u(pk);
  key[1] = ld16u(pk + 16);
  if (in.shred_bytes[r] == 0) min_index(in.pick + r, static_cast<uint32_t>(t));
}

__global__ __launch_bounds__(256) void repair_picks_kernel(const RepairParams p) {
  const IntakeParams& in = p.in;
  const uint64_t t = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (t >= in.n) return;
  const uint32_t r = in.row[t];
  if (r != kIntakeNone && in.pick[r] == t) in.list1[atomicAdd(in.counts, 1u)] = static_cast<uint32_t>(t);
}

__global__ __launch_bounds__(256) void repair_classify_kernel(const RepairParams p) {
  const IntakeParams& in = p.in;
  const uint64_t t = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (t >= in.n) return;
  const uint32_t r = in.row[t];
  if (r == kIntakeNone || in.pick[r] == t) return;  // (a pick: verified already)
  // the pair known valid for the row: the store's, or the pick's if it verified.  ok[] of the
  // picks is complete (the first verify launch); this kernel writes ok[] of non-picks only.
  const uint8_t *commit = nullptr, *sig = nullptr;
  const uint32_t pick = in.pick[r];
  if (in.shred_bytes[r] != 0) {
    commit = in.commitments + 49ull * r;
    sig = p.signatures + 64ull * r;
  } else if (pick != kIntakeNone && p.ok[pick]) {
    commit = in.commit + uint64_t{kIntakeCommitStride} * pick;
    sig = p.sig + 64ull * pick;
  }
  if (commit && same_commit(load_commit(commit), load_commit(in.commit + kIntakeCommitStride * t)) &&
      same_sig(sig, p.sig + 64 * t)) {
    p.ok[t] = 1;  // the same (key, commitment, signature): the same verification
    return;
  }
  in.list2[atomicAdd(in.counts + 1, 1u)] = static_cast<uint32_t>(t);
}

__global__ __launch_bounds__(256) void repair_accept_kernel(const RepairParams p) {
  const IntakeParams& in = p.in;
  const uint64_t t = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (t >= in.n) return;
  const uint32_t r = in.row[t];
  if (r == kIntakeNone) return;
  if (!p.ok[t]) {  // repair.rs:433-437: try_new(shred, None, pk), wherever the row's cache stands
    in.verdict[t] = kInvalidSignature;
    return;
  }
  const uint32_t m = in.meta[t];
  uint32_t size = in.shred_bytes[r];
  const uint8_t* cache = in.commitments + 49ull * r;
  if (size == 0) {  // the setter's: it is not after t, which is valid itself
    const uint32_t s = in.setter[r];
    if (s == kIntakeNone) {  // (unreachable: launch_intake_setter saw ok[t])
      in.verdict[t] = kInvalidSignature;
      return;
    }
    size = meta_len(in.meta[s]);
    cache = in.commit + uint64_t{kIntakeCommitStride} * s;
  }
  if (!same_commit(load_commit(cache), load_commit(in.commit + kIntakeCommitStride * t))) {
    in.verdict[t] = kEquivocation;  // slot_block_data.rs:214-217
    return;
  }
  if (meta_len(m) != size) {
    in.verdict[t] = kSizeMismatch;
    return;
  }
  in.verdict[t] = kIntakeAccepted;
  const uint32_t b = r / in.spp;
  if (meta_last(m) && in.last_slice[b] < 0) min_index(in.tstar + b, static_cast<uint32_t>(t));
}

__global__ __launch_bounds__(256) void repair_signatures_kernel(const RepairParams p) {
  const IntakeParams& in = p.in;
  const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= in.nrows || in.shred_bytes[r] != 0) return;
  const uint32_t s = in.setter[r];
  if (s == kIntakeNone) return;
#pragma unroll
  for (int q = 0; q < 4; ++q) st16u(p.signatures + 64ull * r + 16 * q, ld16u(p.sig + 64ull * s + 16 * q));
}

dim3 per_item(uint64_t n) { return dim3(static_cast<unsigned>((n + 255) / 256)); }

}  // namespace

#define AG_REPAIR_LAUNCH(name, kernel)                                       \
  hipError_t name(const RepairParams& p, hipStream_t stream) {               \
    if (p.in.n == 0) return hipSuccess;                                      \
    hipLaunchKernelGGL(kernel, per_item(p.in.n), dim3(256), 0, stream, p);   \
    return hipGetLastError();                                                \
  }
AG_REPAIR_LAUNCH(launch_repair_key, repair_key_kernel)
AG_REPAIR_LAUNCH(launch_repair_root, repair_root_kernel)
AG_REPAIR_LAUNCH(launch_repair_picks, repair_picks_kernel)
AG_REPAIR_LAUNCH(launch_repair_classify, repair_classify_kernel)
AG_REPAIR_LAUNCH(launch_repair_accept, repair_accept_kernel)
#undef AG_REPAIR_LAUNCH

hipError_t launch_repair_signatures(const RepairParams& p, hipStream_t stream) {
  if (p.in.nrows == 0) return hipSuccess;
  hipLaunchKernelGGL(repair_signatures_kernel, per_item(p.in.nrows), dim3(256), 0, stream, p);
  return hipGetLastError();
}

}  // namespace ag
