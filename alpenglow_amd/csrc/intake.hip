// Shred intake: the parallel form of "process the datagrams one at a time in arrival order"
// (include/alpenglow_rs.h section 10).  Every sequential rule of ValidatedShred::try_new
// (validated_shred.rs:52-79) and BlockData::add_shred (slot_block_data.rs:202-248) depends on
// the past only through "the earliest datagram that ...": the row's cache is set by its
// earliest datagram with a valid signature, the slot's last slice by its earliest accepted
// is_last datagram, a datagram slot is taken by the earliest datagram that reaches it.  Each
// of those is an atomicMin of the arrival index t into one word, completed by a kernel
// boundary before the next kernel reads it; no kernel waits on another workgroup.
//
// Contention (the rows' words take one atomic per datagram of the row): an atomicMin is
// skipped when a plain load already shows a smaller index -- the word only ever decreases, so
// a stale read can only fail to skip.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "intake.hpp"
#include "intake_device.hpp"
#include "wire.hpp"

namespace ag {

namespace {

// Is slice index i with flag is_last consistent with the last slice l (slot_block_data.rs:228)?
__device__ __forceinline__ bool last_consistent(uint32_t i, bool is_last, uint32_t l) {
  return (i < l && !is_last) || (i == l && is_last);
}

__global__ __launch_bounds__(256) void intake_key_kernel(const IntakeParams p) {
  const uint64_t t = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (t >= p.n) return;
  p.row[t] = kIntakeNone;
  p.plausible[t] = 0;
  const uint32_t len = p.rx_lens[t];
  const uint8_t st = p.wire[t];
  // network::deserialize rejects it (a zero length too); a length the caller's row cannot hold
  // is no datagram at all
  if (len > p.rx_stride || st == kWireMalformed) {
    p.verdict[t] = kMalformed;
    return;
  }
  // the header (37 bytes; the row is 16-byte aligned and longer): the wire check bounded every
  // field, so slice index, shred index and data length fit their low bytes
  const uint4* h = reinterpret_cast<const uint4*>(p.rx + t * p.rx_stride);
  const uint4 a = h[0], b = h[1];
  const uint32_t kind = a.x;
  const uint64_t slot = a.y | (static_cast<uint64_t>(a.z) << 32);
  const uint32_t si = a.w;
  const uint32_t is_last = b.y & 0xFFu, j = (b.y >> 8) & 0xFFu, dlen = (b.w >> 8) & 0xFFFFu;
  // the window: binary search of the ascending slot ids
  uint32_t lo = 0, hi = p.nslots;
  while (lo < hi) {
    const uint32_t mid = (lo + hi) / 2;
    if (p.win_ids[mid] < slot) lo = mid + 1; else hi = mid;
  }
  if (lo >= p.nslots || p.win_ids[lo] != slot || si >= p.spp) {
    p.verdict[t] = kOutOfWindow;
    return;
  }
  if (st != kWireOk || kind != (j >= 32 ? 1u : 0u) || dlen == 0 || (dlen & 1u) || dlen > 1024 || p.height[t] != 6) {
    p.verdict[t] = kImplausible;
    return;
  }
  const uint32_t r = p.win_w[lo] * p.spp + si;
  p.row[t] = r;
  p.meta[t] = j | (is_last << 8) | (dlen << 16);
  p.plausible[t] = 1;
  if (p.shred_bytes[r] == 0) min_index(p.pick + r, static_cast<uint32_t>(t));
}

__global__ __launch_bounds__(256) void intake_commit_kernel(const IntakeParams p) {
  const uint64_t t = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (t >= p.n) return;
  const uint32_t r = p.row[t];
  if (r == kIntakeNone) return;
  const uint64_t slot = p.slot[t], si = p.slice_index[t];
  const uint4 x = *reinterpret_cast<const uint4*>(p.roots + 32 * t);
  const uint4 y = *reinterpret_cast<const uint4*>(p.roots + 32 * t + 16);
  const uint32_t root[8] = {x.x, x.y, x.z, x.w, y.x, y.y, y.z, y.w};
  store_commit(p.commit + kIntakeCommitStride * t, make_commit(slot, si, meta_last(p.meta[t]), root));
  if (p.pick[r] == t) p.list1[atomicAdd(p.counts, 1u)] = static_cast<uint32_t>(t);
}

// The row's cache as far as the first verify launch settled it: the store's, or a valid pick's.
__device__ __forceinline__ bool early_cache(const IntakeParams& p, uint32_t r, Commit* c) {
  if (p.shred_bytes[r] != 0) {
    *c = load_commit(p.commitments + 49ull * r);
    return true;
  }
  const uint32_t pk = p.pick[r];
  if (pk == kIntakeNone || !p.ok[pk]) return false;
  *c = load_commit(p.commit + uint64_t{kIntakeCommitStride} * pk);
  return true;
}

__global__ __launch_bounds__(256) void intake_classify_kernel(const IntakeParams p) {
  const uint64_t t = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (t >= p.n) return;
  const uint32_t r = p.row[t];
  if (r == kIntakeNone) return;
  if (p.shred_bytes[r] == 0 && p.pick[r] == t) return;  // verified already
  Commit cache;
  if (early_cache(p, r, &cache) && same_commit(cache, load_commit(p.commit + kIntakeCommitStride * t))) return;
  p.list2[atomicAdd(p.counts + 1, 1u)] = static_cast<uint32_t>(t);
}

__global__ __launch_bounds__(256) void intake_setter_kernel(const IntakeParams p) {
  const uint64_t t = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (t >= p.n) return;
  const uint32_t r = p.row[t];
  if (r == kIntakeNone || p.shred_bytes[r] != 0 || !p.ok[t]) return;
  min_index(p.setter + r, static_cast<uint32_t>(t));
}

__global__ __launch_bounds__(256) void intake_accept_kernel(const IntakeParams p) {
  const uint64_t t = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (t >= p.n) return;
  const uint32_t r = p.row[t];
  if (r == kIntakeNone) return;
  const uint32_t m = p.meta[t];
  uint32_t size = p.shred_bytes[r];
  bool is_setter = false;
  Commit cache;
  if (size != 0) {
    cache = load_commit(p.commitments + 49ull * r);
  } else {
    // no cache before the setter: the signature decides, and every datagram before the
    // earliest valid one has an invalid one (validated_shred.rs:71-77)
    const uint32_t s = p.setter[r];
    if (s == kIntakeNone || t < s) {
      p.verdict[t] = kInvalidSignature;
      return;
    }
    is_setter = s == t;
    size = meta_len(p.meta[s]);
    if (!is_setter) cache = load_commit(p.commit + uint64_t{kIntakeCommitStride} * s);
  }
  if (!is_setter && !same_commit(cache, load_commit(p.commit + kIntakeCommitStride * t))) {
    p.verdict[t] = p.ok[t] ? kEquivocation : kInvalidSignature;  // validated_shred.rs:65-69
    return;
  }
  if (meta_len(m) != size) {
    p.verdict[t] = kSizeMismatch;
    return;
  }
  p.verdict[t] = kIntakeAccepted;
  const uint32_t w = r / p.spp;
  if (meta_last(m) && p.last_slice[w] < 0) min_index(p.tstar + w, static_cast<uint32_t>(t));
}

// The last slice of row r's slot as datagram t meets it (slot_block_data.rs:224-233): the
// store's, or the one the slot's earliest accepted is_last datagram marks -- for the datagrams
// after it.  *marked_now: this call marks it.  False: none yet at t.
__device__ __forceinline__ bool last_slice_at(const IntakeParams& p, uint32_t w, uint64_t t, uint32_t* l,
                                              bool* marked_now) {
  const int32_t l0 = p.last_slice[w];
  *marked_now = false;
  if (l0 >= 0) {
    *l = static_cast<uint32_t>(l0);
    return true;
  }
  const uint32_t ts = p.tstar[w];
  if (ts == kIntakeNone) return false;
  *marked_now = true;
  *l = p.row[ts] % p.spp;
  return t > ts;
}

__global__ __launch_bounds__(256) void intake_claim_kernel(const IntakeParams p) {
  const uint64_t t = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (t >= p.n || p.verdict[t] != kIntakeAccepted) return;
  const uint32_t r = p.row[t], m = p.meta[t];
  uint32_t l = 0;
  bool now;
  if (last_slice_at(p, r / p.spp, t, &l, &now) && !last_consistent(r % p.spp, meta_last(m), l)) {
    p.verdict[t] = kEquivocation;
    return;
  }
  min_index(p.claim + (64ull * r + meta_index(m)), static_cast<uint32_t>(t));
}

// One wave per datagram, grid-stride.  Source and destination rows are 16-byte aligned: whole
// 16-byte pieces, then the last len % 16 bytes singly, so no byte past the length is written.
__global__ __launch_bounds__(256) void intake_route_kernel(const IntakeParams p) {
  const int lane = threadIdx.x & 63;
  const uint64_t waves = static_cast<uint64_t>(gridDim.x) * 4;
  for (uint64_t t = static_cast<uint64_t>(blockIdx.x) * 4 + (threadIdx.x >> 6); t < p.n; t += waves) {
    if (p.verdict[t] != kIntakeAccepted) continue;
    const uint32_t r = p.row[t], m = p.meta[t];
    const uint64_t slot = 64ull * r + meta_index(m);
    uint8_t v = kStored;
    uint32_t l = 0;
    bool now;
    if (p.claim[slot] != t || p.packet_lens[slot] != 0) {
      v = kDuplicate;  // slot_block_data.rs:241-247
    } else if (!last_slice_at(p, r / p.spp, t, &l, &now) && now && r % p.spp > l) {
      v = kPruned;  // stored before the slot's last slice was marked, beyond it (mark_last_slice)
    }
    if (v == kStored) {
      const uint32_t len = p.rx_lens[t];
      const uint8_t* src = p.rx + t * p.rx_stride;
      uint8_t* dst = p.packets + slot * p.packet_stride;
      const uint32_t n16 = len >> 4;
      for (uint32_t i = lane; i < n16; i += 64)
        reinterpret_cast<uint4*>(dst)[i] = reinterpret_cast<const uint4*>(src)[i];
      for (uint32_t i = 16 * n16 + lane; i < len; i += 64) dst[i] = src[i];
      if (lane == 0) p.packet_lens[slot] = len;
    }
    if (lane == 0) p.verdict[t] = v;
  }
}

__global__ __launch_bounds__(256) void intake_rows_kernel(const IntakeParams p) {
  const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= p.nrows) return;
  uint32_t size = p.shred_bytes[r];
  if (size == 0) {
    const uint32_t s = p.setter[r];
    if (s != kIntakeNone) {  // slot_block_data.rs:219-221: the vacant cache takes the commitment
      size = meta_len(p.meta[s]);
      p.shred_bytes[r] = size;
      store_commit(p.commitments + 49ull * r, load_commit(p.commit + uint64_t{kIntakeCommitStride} * s));
    }
  }
  const uint32_t w = r / p.spp;
  uint32_t* lens = p.packet_lens + 64ull * r;
  uint32_t count = 0;
  const uint32_t ts = p.tstar[w];
  if (p.last_slice[w] < 0 && ts != kIntakeNone && r % p.spp > p.row[ts] % p.spp) {
    for (int j = 0; j < 64; ++j) lens[j] = 0;  // mark_last_slice: shreds.retain(ind <= slice_index)
  } else {
    for (int j = 0; j < 64; ++j) count += lens[j] != 0;
  }
  p.out[r] = size;
  p.out[p.nrows + r] = count;
}

__global__ __launch_bounds__(256) void intake_last_kernel(const IntakeParams p) {
  const uint32_t w = blockIdx.x * blockDim.x + threadIdx.x;
  if (w >= p.nslots) return;
  const uint32_t ts = p.tstar[w];
  if (p.last_slice[w] < 0 && ts != kIntakeNone) p.last_slice[w] = static_cast<int32_t>(p.row[ts] % p.spp);
}

dim3 per_item(uint64_t n) { return dim3(static_cast<unsigned>((n + 255) / 256)); }

}  // namespace

#define AG_INTAKE_LAUNCH(name, kernel)                                     \
  hipError_t name(const IntakeParams& p, hipStream_t stream) {             \
    if (p.n == 0) return hipSuccess;                                       \
    hipLaunchKernelGGL(kernel, per_item(p.n), dim3(256), 0, stream, p);    \
    return hipGetLastError();                                              \
  }
AG_INTAKE_LAUNCH(launch_intake_key, intake_key_kernel)
AG_INTAKE_LAUNCH(launch_intake_commit, intake_commit_kernel)
AG_INTAKE_LAUNCH(launch_intake_classify, intake_classify_kernel)
AG_INTAKE_LAUNCH(launch_intake_setter, intake_setter_kernel)
AG_INTAKE_LAUNCH(launch_intake_accept, intake_accept_kernel)
AG_INTAKE_LAUNCH(launch_intake_claim, intake_claim_kernel)
#undef AG_INTAKE_LAUNCH

hipError_t launch_intake_route(const IntakeParams& p, hipStream_t stream) {
  if (p.n == 0) return hipSuccess;
  // four datagrams per workgroup; at most eight workgroups per CU's worth of grid (256 CUs)
  const uint64_t groups = (p.n + 3) / 4;
  hipLaunchKernelGGL(intake_route_kernel, dim3(static_cast<unsigned>(groups < 2048 ? groups : 2048)), dim3(256), 0,
                     stream, p);
  return hipGetLastError();
}

hipError_t launch_intake_finalize(const IntakeParams& p, hipStream_t stream) {
  if (p.nrows == 0) return hipSuccess;
  hipLaunchKernelGGL(intake_rows_kernel, per_item(p.nrows), dim3(256), 0, stream, p);
  hipLaunchKernelGGL(intake_last_kernel, per_item(p.nslots), dim3(256), 0, stream, p);
  return hipGetLastError();
}

}  // namespace ag
