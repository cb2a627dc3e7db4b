// Device helpers shared by the intake kernels (intake.hip) and the repair intake kernels
// (repair.hip): the verdict codes, the arrival-index atomicMin, the 49-byte commitment in
// registers and the packed per-datagram meta word.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "unaligned.hpp"

namespace ag {

enum : uint8_t {  // AG_INTAKE_* (include/alpenglow_rs.h)
  kStored = 0, kMalformed = 1, kOutOfWindow = 2, kImplausible = 3, kInvalidSignature = 4, kEquivocation = 5,
  kSizeMismatch = 6, kDuplicate = 7, kPruned = 8, kRequestMismatch = 9, kNoRoot = 10, kWrongRoot = 11
};

// The word only ever decreases, so a stale read can only fail to skip the atomic.
__device__ __forceinline__ void min_index(uint32_t* word, uint32_t t) {
  if (*static_cast<volatile uint32_t*>(word) > t) atomicMin(word, t);
}

// SliceCommitment (shredder.rs:206-215): 49 bytes as 12 little-endian words and one byte.
struct Commit {
  uint32_t w[12];
  uint32_t last;
};
__device__ __forceinline__ Commit load_commit(const uint8_t* p) {
  Commit c;
#pragma unroll
  for (int q = 0; q < 3; ++q) {
    const uint4 x = ld16u(p + 16 * q);
    c.w[4 * q] = x.x;
    c.w[4 * q + 1] = x.y;
    c.w[4 * q + 2] = x.z;
    c.w[4 * q + 3] = x.w;
  }
  c.last = p[48];
  return c;
}
__device__ __forceinline__ void store_commit(uint8_t* p, const Commit& c) {
#pragma unroll
  for (int q = 0; q < 3; ++q) st16u(p + 16 * q, make_uint4(c.w[4 * q], c.w[4 * q + 1], c.w[4 * q + 2], c.w[4 * q + 3]));
  p[48] = static_cast<uint8_t>(c.last);
}
__device__ __forceinline__ bool same_commit(const Commit& a, const Commit& b) {
  uint32_t diff = a.last ^ b.last;
#pragma unroll
  for (int i = 0; i < 12; ++i) diff |= a.w[i] ^ b.w[i];
  return diff == 0;
}
// The commitment of (slot, slice index, is_last, root): the root shifted up one byte.
__device__ __forceinline__ Commit make_commit(uint64_t slot, uint64_t si, bool is_last, const uint32_t (&root)[8]) {
  Commit c;
  c.w[0] = static_cast<uint32_t>(slot);
  c.w[1] = static_cast<uint32_t>(slot >> 32);
  c.w[2] = static_cast<uint32_t>(si);
  c.w[3] = static_cast<uint32_t>(si >> 32);
  c.w[4] = (is_last ? 1u : 0u) | (root[0] << 8);
#pragma unroll
  for (int k = 1; k < 8; ++k) c.w[4 + k] = __builtin_amdgcn_alignbyte(root[k], root[k - 1], 3);
  c.last = root[7] >> 24;
  return c;
}

// meta: shred index | is_last << 8 | data_len << 16
__device__ __forceinline__ uint32_t meta_index(uint32_t m) { return m & 0xFFu; }
__device__ __forceinline__ bool meta_last(uint32_t m) { return (m >> 8) & 1u; }
__device__ __forceinline__ uint32_t meta_len(uint32_t m) { return m >> 16; }

}  // namespace ag
