// Slice Merkle trees on the GPU.
//
// What it replaces: the reference builds one SHA-256 Merkle tree per slice over its 64
// shreds (data shreds, then coding shreds; shredder.rs:628-632 build_merkle_tree) with
// MerkleTree::new (crypto/merkle.rs:281-333), takes the root (:337) and one proof per shred
// (create_proof, :351-370); receivers check proofs (check_proof / derive_root, :374-425)
// and rebuild the tree after decoding (check_merkle_tree, shredder.rs:616-626).
//   leaf  = SHA-256(LEAF_LABEL || shred bytes)                      (merkle.rs:457-460)
//   inner = SHA-256(LEFT_LABEL || left || RIGHT_LABEL || right)     (merkle.rs:466-468)
//   an odd node at height h pairs with EMPTY_ROOTS[h]               (merkle.rs:312-315)
// SHA-256 is the sha2 crate's (crypto/hash.rs:64-79); here it is a plain FIPS 180-4
// implementation shared by host and device.
//
// Kernels
//   merkle_leaf_kernel    one thread per leaf (all slices): SHA-256 of label || shred.
//                         Integer VALU-bound (~1.2k VALU per 64-byte SHA-256 block and
//                         lane: v_alignbit rotations, v_bitop3 sigma XORs / ch / maj, v_add3)
//   merkle_leaf_var_kernel  the same with one leaf size per slice: one wave per slice
//   merkle_level_kernel   one launch per tree level, one thread per (slice, pair)
//   merkle_proof_kernel   one thread per leaf: its create_proof siblings
//   merkle_verify_kernel  one thread per (leaf, index, root, proof): derive_root == root;
//                         optionally a proof length and the check_proof_last rule per item
//   block_tree_kernel     one workgroup per block: the double-Merkle tree over its slice roots
//                         (DoubleMerkleTree, merkle.rs:263), all levels in LDS, one launch
//   block_proof_kernel    every slice's create_proof of a block tree, from its nodes
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>

#include "merkle.hpp"
#include "sha256.hpp"
#include "unaligned.hpp"

namespace ag {

namespace {

using sha::hash_pair;

// How leaf_hash loads the leaf bytes.
enum LeafLoad : int {
  kLeafByte = 0,  // any address: four byte loads per SHA word
  kLeafA16 = 1,   // data is 16-byte aligned: vector loads
  kLeafU16 = 2,   // any address: the same vector loads through types of alignment 1 (unaligned.hpp);
                  // the hardware splits an access that straddles, no byte loads for whole words
};

// SHA-256(LEAF_LABEL || data[0..len)).  A4 = a LeafLoad (true / false: kLeafA16 / kLeafByte).
// The blocks made only of data bytes (b = 1 .. T/64 - 1, T = 32 + len) are software-pipelined:
// block b + 1's four 16-byte loads are issued before block b's compression, so each lane's
// HBM latency (its leaf is 1 KiB away from its neighbours', one cache line per lane and
// instruction) hides under ~1.2k VALU of rounds instead of stalling every block.
template <int A4>
__device__ __forceinline__ void leaf_hash(const uint8_t* __restrict__ data, uint32_t len, uint32_t out[8]) {
  uint32_t st[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) st[i] = sha::kIv[i];
  const uint32_t T = 32 + len, nblk = (T + 9 + 63) / 64;
  auto word = [&](uint32_t j) -> uint32_t {
    if constexpr (A4 == kLeafA16) {
      return reinterpret_cast<const uint32_t*>(data)[j];
    } else if constexpr (A4 == kLeafU16) {
      return ld4u(data + 4 * j);
    } else {
      return uint32_t(data[4 * j]) | (uint32_t(data[4 * j + 1]) << 8) | (uint32_t(data[4 * j + 2]) << 16) |
             (uint32_t(data[4 * j + 3]) << 24);
    }
  };
  auto byte = [&](uint32_t i) -> uint32_t { return data[i]; };
  auto generic = [&](uint32_t b) __attribute__((always_inline)) {
    uint32_t w[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) w[i] = sha::leaf_msg_word(16 * b + i, len, nblk, word, byte);
    sha::compress(st, w);
  };
  if constexpr (A4 != kLeafByte) {
    const uint32_t nd = T / 64;  // blocks 1 .. nd - 1 are data only (words 16 b - 8 ..)
    uint4 nx[4];
    auto fetch = [&](uint32_t b) __attribute__((always_inline)) {
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        if constexpr (A4 == kLeafU16) nx[q] = ld16u(data + 64 * b - 32 + 16 * q);
        else nx[q] = *reinterpret_cast<const uint4*>(data + 64 * b - 32 + 16 * q);
      }
    };
    if (nd > 1) fetch(1);
    generic(0);
    for (uint32_t b = 1; b < nd; ++b) {
      uint32_t w[16];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        w[4 * q] = sha::bswap(nx[q].x);
        w[4 * q + 1] = sha::bswap(nx[q].y);
        w[4 * q + 2] = sha::bswap(nx[q].z);
        w[4 * q + 3] = sha::bswap(nx[q].w);
      }
      if (b + 1 < nd) fetch(b + 1);
      sha::compress(st, w);
    }
    for (uint32_t b = nd > 1 ? nd : 1; b < nblk; ++b) generic(b);
  } else {
    for (uint32_t b = 0; b < nblk; ++b) {
      uint32_t w[16];
      const uint32_t o0 = 64 * b;
      if (b > 0 && o0 + 64 <= T) {  // a block of data only: words j0 .. j0 + 15
        const uint32_t j0 = (o0 - 32) >> 2;
#pragma unroll
        for (int i = 0; i < 16; ++i) w[i] = sha::bswap(word(j0 + i));
        sha::compress(st, w);
      } else {
        generic(b);
      }
    }
  }
#pragma unroll
  for (int i = 0; i < 8; ++i) out[i] = st[i];
}

// Digests are stored as 8 big-endian words -> 32 bytes in the crate's byte order.
__device__ __forceinline__ void store_digest(uint8_t* dst, const uint32_t h[8]) {
  uint4* d = reinterpret_cast<uint4*>(dst);
  d[0] = make_uint4(sha::bswap(h[0]), sha::bswap(h[1]), sha::bswap(h[2]), sha::bswap(h[3]));
  d[1] = make_uint4(sha::bswap(h[4]), sha::bswap(h[5]), sha::bswap(h[6]), sha::bswap(h[7]));
}
__device__ __forceinline__ void load_digest(const uint8_t* src, uint32_t h[8]) {
  const uint4* s = reinterpret_cast<const uint4*>(src);
  const uint4 a = s[0], b = s[1];
  h[0] = sha::bswap(a.x);
  h[1] = sha::bswap(a.y);
  h[2] = sha::bswap(a.z);
  h[3] = sha::bswap(a.w);
  h[4] = sha::bswap(b.x);
  h[5] = sha::bswap(b.y);
  h[6] = sha::bswap(b.z);
  h[7] = sha::bswap(b.w);
}

// Build = one kernel per tree level, every launch fully parallel over all slices (a fused
// one-wave-per-slice build left 50..98% of the lanes idle in its 6 dependent levels of 3
// compressions each: as long as the 17-block leaf phase).
//   level 0: thread (slice, leaf) hashes the leaf into nodes[slice][leaf]
//   level h: thread (slice, j) hashes nodes[off + 2j], nodes[off + 2j + 1] (or EMPTY_ROOTS[h]
//            past the end) into nodes[off + len + j]; the last level also writes the root
//   proofs:  thread (slice, leaf) copies its siblings (create_proof)
// LIST: thread i hashes leaf list[i] for i < list[nslices * n_leaves] (hash_leaf compacted)
template <bool A4, bool LIST = false>
__global__ __launch_bounds__(256) void merkle_leaf_kernel(const MerkleBuildParams p, uint8_t* nodes,
                                                          uint64_t nodes_stride) {
  uint64_t t = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if constexpr (LIST) {
    if (t >= p.list[p.nslices * p.n_leaves]) return;
    t = p.list[t];
  } else {
    if (t >= p.nslices * p.n_leaves) return;
  }
  const uint64_t s = t / p.n_leaves, j = t - s * p.n_leaves;
  uint32_t h[8];
  const uint64_t jr = j + (p.skip_leaf && j >= p.skip_leaf ? 1u : 0u);
  leaf_hash<A4>(p.leaves + s * p.slice_stride + jr * p.leaf_stride, p.leaf_bytes, h);
  store_digest(nodes + s * nodes_stride + 32 * j, h);
  if (p.n_leaves == 1) store_digest(p.roots + 32 * s, h);  // a one-leaf tree's root is the leaf
}

// Level 0 with one leaf size per slice (p.leaf_sizes): one wave per slice, a lane per leaf, so
// the size is wave-uniform (a scalar: the block loops of leaf_hash branch on it without
// divergence) and a wave's 64 rows are one contiguous run of 64 * size bytes.  Rows sit at
// j * size: 16-byte aligned for every j only when size % 16 == 0, 2-byte aligned otherwise.
// One loader serves both: kLeafU16 issues the aligned path's global_load_dwordx4 / _dword at
// whatever address the row has (an aligned row costs what it costs in merkle_leaf_kernel<true>;
// a straddling access is split by the memory pipeline, not by byte loads in the shader).
// FLAGGED: only the leaves with p.hash_leaf[64 s + j] != 0 (a deshred's rebuild: the other leaves'
// digests are already in nodes).  Still one wave per slice, so the size stays wave-uniform; the
// lanes of kept leaves idle.
template <bool FLAGGED>
__device__ __forceinline__ void merkle_leaf_var_body(const MerkleBuildParams& p, uint8_t* nodes,
                                                     uint64_t nodes_stride) {
  const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const uint64_t s = static_cast<uint64_t>(blockIdx.x) * 4 + wave;
  if (s >= p.nslices) return;
  const uint32_t j = threadIdx.x & 63;
  const uint32_t len = __builtin_amdgcn_readfirstlane(p.leaf_sizes[s]);
  if constexpr (FLAGGED) {
    if (!p.hash_leaf[s * kMerkleMaxLeaves + j]) return;
  }
  uint32_t h[8];
  leaf_hash<kLeafU16>(p.leaves + s * p.slice_stride + static_cast<uint64_t>(j) * len, len, h);
  store_digest(nodes + s * nodes_stride + 32 * j, h);
}
__global__ __launch_bounds__(256) void merkle_leaf_var_kernel(const MerkleBuildParams p, uint8_t* nodes,
                                                              uint64_t nodes_stride) {
  merkle_leaf_var_body<false>(p, nodes, nodes_stride);
}
__global__ __launch_bounds__(256) void merkle_leaf_var_flagged_kernel(const MerkleBuildParams p, uint8_t* nodes,
                                                                      uint64_t nodes_stride) {
  merkle_leaf_var_body<true>(p, nodes, nodes_stride);
}

__global__ __launch_bounds__(256) void merkle_level_kernel(const MerkleBuildParams p, uint8_t* nodes,
                                                           uint64_t nodes_stride, uint32_t off, uint32_t len,
                                                           uint32_t height) {
  const uint32_t nlen = (len + 1) / 2;
  const uint64_t t = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (t >= p.nslices * nlen) return;
  const uint64_t s = t / nlen, j = t - s * nlen;
  uint8_t* nd = nodes + s * nodes_stride;
  uint32_t l[8], r[8], h[8];
  load_digest(nd + 32 * (off + 2 * j), l);
  if (2 * j + 1 < len) {
    load_digest(nd + 32 * (off + 2 * j + 1), r);
  } else {
#pragma unroll
    for (int i = 0; i < 8; ++i) r[i] = p.empty_roots[8 * height + i];
  }
  hash_pair(l, r, h);
  store_digest(nd + 32 * (off + len + j), h);
  if (nlen == 1) store_digest(p.roots + 32 * s, h);
}

// One wave per slice: the slice's proofs are one contiguous run of n_leaves * height digests, so
// lane-consecutive 16-byte pieces make every store instruction one contiguous 1 KiB (a thread
// per leaf wrote 16 bytes per lane at a 32 * height-byte stride: 1.1 TB/s of proof bytes)
__global__ __launch_bounds__(256) void merkle_proof_kernel(const MerkleBuildParams p, const uint8_t* nodes,
                                                           uint64_t nodes_stride, uint32_t height) {
  const uint64_t s = static_cast<uint64_t>(blockIdx.x) * 4 + (threadIdx.x >> 6);
  if (s >= p.nslices) return;
  const uint32_t lane = threadIdx.x & 63;
  const uint8_t* nd = nodes + s * nodes_stride;
  uint8_t* dst = p.proofs + s * p.proofs_stride;
  const uint32_t pieces = p.n_leaves * height * 2;  // 16-byte halves of the digests
  for (uint32_t i = lane; i < pieces; i += 64) {
    const uint32_t j = i / (2 * height), r = i - j * 2 * height, h = r >> 1, half = r & 1;
    // level h starts at node offset off_h; its length l_h
    uint32_t off = 0, l = p.n_leaves;
    for (uint32_t g = 0; g < h; ++g) {
      off += l;
      l = (l + 1) / 2;
    }
    const uint32_t sib = (j >> h) ^ 1;
    uint4 v;
    if (sib >= l) {
      const uint32_t* e = p.empty_roots + 8 * h + 4 * half;
      v = make_uint4(sha::bswap(e[0]), sha::bswap(e[1]), sha::bswap(e[2]), sha::bswap(e[3]));
    } else {
      v = *reinterpret_cast<const uint4*>(nd + 32 * (off + sib) + 16 * half);
    }
    *reinterpret_cast<uint4*>(dst + 16 * static_cast<uint64_t>(i)) = v;
  }
}

// check_proof (merkle.rs:374-387, 417-428) for one leaf per thread; derive_root (:411-428)
// when roots_out is set.
// LIST: thread i verifies leaf list[i] for i < list[n] (the compacted active leaves).
// ITEM: per-item proof length and the check_proof_last rule (proof_len / last; check mode only).
// VAR (p.leaf_sizes set; derive-root mode): leaf t is leaf_sizes[t / size_group] bytes -- size_group
// 1: at t * leaf_stride (gathered rows); 64: row t % 64 of slice t / 64, packed at that size from
// the slice's group_stride.  Rows are 2-byte aligned: the kLeafU16 loader.
template <bool A4, bool LIST, bool ITEM, bool VAR>
__device__ __forceinline__ void merkle_verify_body(const MerkleVerifyParams& p) {
  uint64_t t = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if constexpr (LIST) {
    if (t >= p.list[p.n]) return;
    t = p.list[t];
  } else {
    if (t >= p.n || (p.active && !p.active[t])) return;
  }
  uint32_t node[8];
  if constexpr (VAR) {
    const uint64_t g = t / p.size_group;
    const uint32_t len = p.leaf_sizes[g];
    const uint64_t off = p.size_group == 1 ? t * p.leaf_stride : g * p.group_stride + (t - g * p.size_group) * len;
    leaf_hash<kLeafU16>(p.leaves + off, len, node);
  } else {
    leaf_hash<A4>(p.leaves + grouped_row_offset(t, p.leaf_stride, p.group_stride, p.skip_row), p.leaf_bytes, node);
  }
  if (p.leaf_nodes)
    store_digest(p.leaf_nodes + (t / p.leaves_per_tree) * p.leaf_nodes_stride + 32 * (t % p.leaves_per_tree), node);
  uint32_t idx = p.index[t];
  const uint8_t* pr = p.proofs + t * p.proofs_stride;
  uint32_t height = p.height;
  bool last = false, canonical = true;
  if constexpr (ITEM) {
    height = p.proof_len[t];
    // merkle.rs:381-383 / :398-400 (a proof longer than EMPTY_ROOTS), and a proof the item's
    // stride cannot hold: rejected before any of it is read
    if (height > static_cast<uint32_t>(kMerkleMaxHeight) || 32ull * height > p.proofs_stride) {
      p.ok[t] = 0;
      return;
    }
    last = p.last && p.last[t];
  }
  for (uint32_t h = 0; h < height; ++h) {
    uint32_t s[8], nn[8];
    load_digest(pr + 32 * h, s);
    if constexpr (ITEM) {
      // derive_hash_root_last (merkle.rs:436-452): a right-hand sibling must be EMPTY_ROOTS[h]
      if (last && !(idx & 1)) {
#pragma unroll
        for (int i = 0; i < 8; ++i) canonical = canonical && s[i] == p.empty_roots[8 * h + i];
      }
    }
    if (idx & 1) hash_pair(s, node, nn); else hash_pair(node, s, nn);
#pragma unroll
    for (int i = 0; i < 8; ++i) node[i] = nn[i];
    idx >>= 1;
  }
  if (p.roots_out) {  // derive_root: the root digest bytes (big-endian words)
    uint32_t* o = reinterpret_cast<uint32_t*>(p.roots_out + 32 * t);
#pragma unroll
    for (int i = 0; i < 8; ++i) o[i] = sha::bswap(node[i]);
    return;
  }
  uint32_t root[8];
  load_digest(p.roots + t * p.roots_stride, root);
  bool ok = canonical;
#pragma unroll
  for (int i = 0; i < 8; ++i) ok = ok && node[i] == root[i];
  p.ok[t] = ok ? 1 : 0;
}
template <bool A4, bool LIST, bool ITEM = false>
__global__ __launch_bounds__(256) void merkle_verify_kernel(const MerkleVerifyParams p) {
  merkle_verify_body<A4, LIST, ITEM, false>(p);
}
template <bool LIST>
__global__ __launch_bounds__(256) void merkle_verify_var_kernel(const MerkleVerifyParams p) {
  merkle_verify_body<false, LIST, false, true>(p);
}

// list[0 .. *count) = the t < n with active[t] != 0 (in no particular order): per 1024-thread
// workgroup one atomic on the counter (a per-wave atomic serialises 65 536 of them, 0.75 ms).
__global__ __launch_bounds__(1024) void compact_active_kernel(const uint8_t* __restrict__ active, uint64_t n,
                                                              uint32_t* count, uint32_t* __restrict__ list) {
  __shared__ uint32_t wcnt[16];
  __shared__ uint32_t base;
  const uint64_t t = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const bool a = t < n && active[t] != 0;
  const uint64_t m = __builtin_amdgcn_ballot_w64(a);
  if (lane == 0) wcnt[wave] = static_cast<uint32_t>(__builtin_popcountll(m));
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t tot = 0;
    for (int w = 0; w < 16; ++w) {
      const uint32_t c = wcnt[w];
      wcnt[w] = tot;
      tot += c;
    }
    base = tot ? atomicAdd(count, tot) : 0;
  }
  __syncthreads();
  if (a) list[base + wcnt[wave] + __builtin_popcountll(m & ((uint64_t{1} << lane) - 1))] = static_cast<uint32_t>(t);
}

// ---- block trees: the double-Merkle tree over a block's slice roots -----------------------
//
// One workgroup per block, the whole tree in one launch: a block hash is wanted the moment the
// block's last slice lands, usually for one block, and the tree is a chain of up to 10
// dependent levels over at most 1024 leaves of 2 compressions each -- per-level launches (the
// slice trees' shape above) would put 10 kernel boundaries into a chain of ~5 100 compressions
// (not built, so not measured).  The
// current level lives in LDS as native state words, ping-ponged between a 1024- and a
// 512-digest buffer (48 KiB); bytes are swapped only at the global loads and stores.  Each
// level: hash pairs from one buffer into the other, barrier.  (The fused one-wave-per-slice
// build that lost for the slice trees had 17-block leaves and 65 536 trees; here the leaves
// are short and the trees few.)
// Measured on an MI355X (profiles/block_tree_bench.jsonl, kernel trace): one 1024-slice block
// 102 us, 64 such blocks 113 us -- the time is the chain, not the work: a level is one
// hash_pair, ~3 600 VALU that a lone wave issues at ~4 cycles each, 8-9 us, times 10 levels,
// plus the leaves.  Workgroup size, kernel time for 1 / 64 blocks: 256 threads 105 / 115 us,
// 512 threads 102 / 113 us, 1024 threads 110 / 122 us (128 VGPRs: 11 spilled); 512 it is.
__device__ __forceinline__ void lds_put(uint4* lv, uint32_t j, const uint32_t h[8]) {
  lv[2 * j] = make_uint4(h[0], h[1], h[2], h[3]);
  lv[2 * j + 1] = make_uint4(h[4], h[5], h[6], h[7]);
}
__device__ __forceinline__ void lds_get(const uint4* lv, uint32_t j, uint32_t h[8]) {
  const uint4 a = lv[2 * j], b = lv[2 * j + 1];
  h[0] = a.x;
  h[1] = a.y;
  h[2] = a.z;
  h[3] = a.w;
  h[4] = b.x;
  h[5] = b.y;
  h[6] = b.z;
  h[7] = b.w;
}

constexpr uint32_t kBlockTreeThreads = 512;
__global__ __launch_bounds__(kBlockTreeThreads) void block_tree_kernel(const BlockTreeParams p) {
  __shared__ uint4 lv_a[2 * kBlockMaxSlices];  // levels 0, 2, 4, ..: at most 1024 digests
  __shared__ uint4 lv_b[kBlockMaxSlices];      // levels 1, 3, 5, ..: at most 512 digests
  const uint64_t b = blockIdx.x;
  const uint32_t n = p.count[b];
  if (n > kBlockMaxSlices) return;  // the launcher's caller validates the counts; never past the LDS
  const uint8_t* in = p.slice_roots + 32 * p.first[b];
  uint8_t* nd = p.nodes ? p.nodes + b * p.nodes_stride : nullptr;
  uint8_t* out = p.block_hashes + 32 * b;
  // leaves: SHA-256(LEAF_LABEL || root) = one data block and the constant padding block
  for (uint32_t j = threadIdx.x; j < n; j += kBlockTreeThreads) {
    uint32_t st[8], w[16];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      st[i] = sha::kIv[i];
      w[i] = sha::kLeafLabel.w[i];
    }
    load_digest(in + 32 * static_cast<uint64_t>(j), w + 8);
    sha::compress(st, w);
    w[0] = 0x80000000u;
#pragma unroll
    for (int i = 1; i < 15; ++i) w[i] = 0;
    w[15] = 64 * 8;
    sha::compress(st, w);
    lds_put(lv_a, j, st);
    if (nd) store_digest(nd + 32 * j, st);
    if (n == 1) store_digest(out, st);  // a one-slice block: height 0, the hash is the leaf
  }
  __syncthreads();
  uint4* src = lv_a;
  uint4* dst = lv_b;
  uint32_t off = 0, len = n;  // n is uniform in the workgroup: so is every barrier below
  for (uint32_t h = 0; len > 1; ++h) {
    const uint32_t nlen = (len + 1) / 2;
    for (uint32_t j = threadIdx.x; j < nlen; j += kBlockTreeThreads) {
      uint32_t l[8], r[8], o[8];
      lds_get(src, 2 * j, l);
      if (2 * j + 1 < len) {
        lds_get(src, 2 * j + 1, r);
      } else {
#pragma unroll
        for (int i = 0; i < 8; ++i) r[i] = p.empty_roots[8 * h + i];
      }
      hash_pair(l, r, o);
      lds_put(dst, j, o);
      if (nd) store_digest(nd + 32 * (off + len + j), o);
      if (nlen == 1) store_digest(out, o);
    }
    __syncthreads();
    uint4* t = src;
    src = dst;
    dst = t;
    off += len;
    len = nlen;
  }
}

// create_proof for every slice of a block from its nodes: blockIdx.x = the block, blockIdx.y
// splits its 16-byte pieces (one block's 1024 x 10 digests are 20 480 of them).  Lane-consecutive
// pieces as in merkle_proof_kernel; the height is the block's own.
constexpr unsigned kBlockProofSplit = 8;
__global__ __launch_bounds__(256) void block_proof_kernel(const BlockTreeParams p) {
  const uint64_t b = blockIdx.x;
  const uint32_t n = p.count[b];
  if (n > kBlockMaxSlices) return;
  uint32_t height = 0;
  for (uint32_t l = n; l > 1; l = (l + 1) / 2) ++height;
  const uint8_t* nd = p.nodes + b * p.nodes_stride;
  uint8_t* dst = p.proofs + b * p.proofs_stride;
  const uint32_t pieces = n * height * 2;
  for (uint32_t i = blockIdx.y * 256 + threadIdx.x; i < pieces; i += kBlockProofSplit * 256) {
    const uint32_t j = i / (2 * height), r = i - j * 2 * height, h = r >> 1, half = r & 1;
    uint32_t off = 0, l = n;
    for (uint32_t g = 0; g < h; ++g) {
      off += l;
      l = (l + 1) / 2;
    }
    const uint32_t sib = (j >> h) ^ 1;
    uint4 v;
    if (sib >= l) {
      const uint32_t* e = p.empty_roots + 8 * h + 4 * half;
      v = make_uint4(sha::bswap(e[0]), sha::bswap(e[1]), sha::bswap(e[2]), sha::bswap(e[3]));
    } else {
      v = *reinterpret_cast<const uint4*>(nd + 32 * (off + sib) + 16 * half);
    }
    *reinterpret_cast<uint4*>(dst + 16 * static_cast<uint64_t>(i)) = v;
  }
}

}  // namespace

hipError_t launch_block_tree(const BlockTreeParams& p, hipStream_t stream) {
  if (p.nblocks == 0) return hipSuccess;
  if (p.nblocks > 0x7FFFFFFFull || !p.first || !p.count || !p.slice_roots || !p.empty_roots || !p.block_hashes ||
      (p.proofs && !p.nodes) ||
      (reinterpret_cast<uintptr_t>(p.slice_roots) | reinterpret_cast<uintptr_t>(p.block_hashes) |
       reinterpret_cast<uintptr_t>(p.nodes) | reinterpret_cast<uintptr_t>(p.proofs) | p.nodes_stride |
       p.proofs_stride) % 16)
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(block_tree_kernel, dim3(static_cast<unsigned>(p.nblocks)), dim3(kBlockTreeThreads), 0, stream,
                     p);
  if (p.proofs)
    hipLaunchKernelGGL(block_proof_kernel, dim3(static_cast<unsigned>(p.nblocks), kBlockProofSplit), dim3(256), 0,
                       stream, p);
  return hipGetLastError();
}

hipError_t launch_merkle_build(const MerkleBuildParams& p, uint8_t* nodes, uint64_t nodes_stride,
                               hipStream_t stream, uint32_t* leaf_kernels) {
  if (p.nslices == 0) return hipSuccess;
  if (p.n_leaves == 0 || p.n_leaves > kMerkleMaxLeaves || !nodes || nodes_stride % 16) return hipErrorInvalidValue;
  if (p.leaf_sizes && (p.n_leaves != kMerkleMaxLeaves || p.skip_leaf)) return hipErrorInvalidValue;
  auto grid_of = [](uint64_t threads) { return dim3(static_cast<unsigned>((threads + 255) / 256)); };
  if ((p.nslices * p.n_leaves + 255) / 256 > 0x7FFFFFFFull) return hipErrorInvalidValue;
  const bool a16 = (reinterpret_cast<uintptr_t>(p.leaves) | p.leaf_stride | p.slice_stride) % 16 == 0;
  const dim3 g0 = grid_of(p.nslices * p.n_leaves);
  if (leaf_kernels)
    *leaf_kernels |= p.leaf_sizes ? (p.hash_leaf ? kMkLeafVarFlagged : kMkLeafVar) : a16 ? kMkLeafAligned : kMkLeafByte;
  if (p.leaf_sizes && p.hash_leaf) {  // (no compaction: one wave per slice keeps the size wave-uniform)
    hipLaunchKernelGGL(merkle_leaf_var_flagged_kernel, g0, dim3(256), 0, stream, p, nodes, nodes_stride);
  } else if (p.leaf_sizes) {  // (g0: four waves, four slices, per workgroup)
    hipLaunchKernelGGL(merkle_leaf_var_kernel, g0, dim3(256), 0, stream, p, nodes, nodes_stride);
  } else if (p.hash_leaf && p.list) {  // only the flagged leaves: compacted, so no lane idles on a known one
    const uint64_t nl = p.nslices * p.n_leaves;
    if (nl >= 0xFFFFFFFFull || hipMemsetAsync(p.list + nl, 0, 4, stream) != hipSuccess) return hipErrorInvalidValue;
    hipLaunchKernelGGL(compact_active_kernel, dim3(static_cast<unsigned>((nl + 1023) / 1024)), dim3(1024), 0, stream,
                       p.hash_leaf, nl, p.list + nl, p.list);
    if (a16) hipLaunchKernelGGL((merkle_leaf_kernel<true, true>), g0, dim3(256), 0, stream, p, nodes, nodes_stride);
    else hipLaunchKernelGGL((merkle_leaf_kernel<false, true>), g0, dim3(256), 0, stream, p, nodes, nodes_stride);
  } else if (a16) {
    hipLaunchKernelGGL((merkle_leaf_kernel<true>), g0, dim3(256), 0, stream, p, nodes, nodes_stride);
  } else {
    hipLaunchKernelGGL((merkle_leaf_kernel<false>), g0, dim3(256), 0, stream, p, nodes, nodes_stride);
  }
  uint32_t off = 0, len = p.n_leaves, height = 0;
  while (len > 1) {
    const uint32_t nlen = (len + 1) / 2;
    hipLaunchKernelGGL(merkle_level_kernel, grid_of(p.nslices * nlen), dim3(256), 0, stream, p, nodes, nodes_stride,
                       off, len, height);
    off += len;
    len = nlen;
    ++height;
  }
  if (p.proofs && height)
    hipLaunchKernelGGL(merkle_proof_kernel, grid_of(p.nslices * 64) , dim3(256), 0, stream, p, nodes, nodes_stride,
                       height);
  return hipGetLastError();
}

hipError_t launch_merkle_verify(const MerkleVerifyParams& p, hipStream_t stream) {
  if (p.n == 0) return hipSuccess;
  const uint64_t groups = (p.n + 255) / 256;
  if (groups > 0x7FFFFFFFull) return hipErrorInvalidValue;
  const bool a16 = (reinterpret_cast<uintptr_t>(p.leaves) | p.leaf_stride | p.group_stride) % 16 == 0;
  const dim3 grid(static_cast<unsigned>(groups));
  if (p.proof_len) {  // per-item lengths: plain check mode only
    if (p.roots_out || p.active || !p.empty_roots) return hipErrorInvalidValue;
    if (a16) hipLaunchKernelGGL((merkle_verify_kernel<true, false, true>), grid, dim3(256), 0, stream, p);
    else hipLaunchKernelGGL((merkle_verify_kernel<false, false, true>), grid, dim3(256), 0, stream, p);
    return hipGetLastError();
  }
  if (p.last) return hipErrorInvalidValue;
  if (p.leaf_sizes) {  // one leaf size per group of items: derive-root mode only
    if (!p.roots_out || p.skip_row ||
        (p.size_group != 1 && (p.size_group != kMerkleMaxLeaves || !p.group_stride || p.n % kMerkleMaxLeaves)))
      return hipErrorInvalidValue;
    if (p.active && p.list && p.n < 0xFFFFFFFFull) {
      if (hipMemsetAsync(p.list + p.n, 0, 4, stream) != hipSuccess) return hipErrorInvalidValue;
      hipLaunchKernelGGL(compact_active_kernel, dim3(static_cast<unsigned>((p.n + 1023) / 1024)), dim3(1024), 0,
                         stream, p.active, p.n, p.list + p.n, p.list);
      hipLaunchKernelGGL(merkle_verify_var_kernel<true>, grid, dim3(256), 0, stream, p);
    } else {
      hipLaunchKernelGGL(merkle_verify_var_kernel<false>, grid, dim3(256), 0, stream, p);
    }
    return hipGetLastError();
  }
  if (p.active && p.list && p.n < 0xFFFFFFFFull) {
    if (hipMemsetAsync(p.list + p.n, 0, 4, stream) != hipSuccess) return hipErrorInvalidValue;
    hipLaunchKernelGGL(compact_active_kernel, dim3(static_cast<unsigned>((p.n + 1023) / 1024)), dim3(1024), 0, stream,
                       p.active, p.n, p.list + p.n, p.list);
    if (a16) hipLaunchKernelGGL((merkle_verify_kernel<true, true>), grid, dim3(256), 0, stream, p);
    else hipLaunchKernelGGL((merkle_verify_kernel<false, true>), grid, dim3(256), 0, stream, p);
  } else if (a16) {
    hipLaunchKernelGGL((merkle_verify_kernel<true, false>), grid, dim3(256), 0, stream, p);
  } else {
    hipLaunchKernelGGL((merkle_verify_kernel<false, false>), grid, dim3(256), 0, stream, p);
  }
  return hipGetLastError();
}

// EMPTY_ROOTS (merkle.rs:62-157): hash_leaf([]) then hash_pair(node, node) per height.
void merkle_empty_roots(uint32_t out[kMerkleMaxHeight][8]) {
  uint32_t st[8], w[16];
  for (int i = 0; i < 8; ++i) st[i] = sha::kIv[i];
  for (int i = 0; i < 8; ++i) w[i] = sha::kLeafLabel.w[i];
  w[8] = 0x80000000u;
  for (int i = 9; i < 15; ++i) w[i] = 0;
  w[15] = 32 * 8;
  sha::compress(st, w);
  for (int i = 0; i < 8; ++i) out[0][i] = st[i];
  for (int h = 1; h < kMerkleMaxHeight; ++h) sha::hash_pair(out[h - 1], out[h - 1], out[h]);
}

}  // namespace ag
