// Slice Merkle trees (merkle.hip): parameter blocks and launchers.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace ag {

// TOTAL_SHREDS (shredder.rs:47): every shredder's slice tree has 64 leaves.
constexpr uint32_t kMerkleMaxLeaves = 64;

// Row t of a per-shred table (data rows, leaves): t * stride, or -- with group_stride set --
// grouped by slice: row j of slice g = t / 64 at g * group_stride + (j + (j >= skip)) * stride
// (skip 0: none).  The composed shredders address their output shreds in the caller's codeword
// buffer this way (CodingOnly: the coding rows; PETS: every row but the withheld data shard).
__host__ __device__ inline uint64_t grouped_row_offset(uint64_t t, uint64_t stride, uint64_t group_stride,
                                                       uint32_t skip) {
  if (!group_stride) return t * stride;
  const uint64_t j = t & (kMerkleMaxLeaves - 1);
  return (t / kMerkleMaxLeaves) * group_stride + (j + (skip && j >= skip ? 1u : 0u)) * stride;
}
// MAX_MERKLE_TREE_HEIGHT (merkle.rs:33)
constexpr int kMerkleMaxHeight = 32;

// nslices trees of n_leaves leaves; leaf j of slice s: leaves + s*slice_stride + j*leaf_stride,
// leaf_bytes long.  Outputs (device): roots[s] (32 B); nodes (optional) = the reference's
// `nodes` vector (leaf hashes, then each level); proofs (optional) = create_proof(j) for
// every leaf, height digests each.
struct MerkleBuildParams {
  const uint8_t* leaves;
  uint64_t leaf_stride;
  uint64_t slice_stride;
  uint32_t leaf_bytes;
  uint32_t n_leaves;
  uint64_t nslices;
  const uint32_t* empty_roots;  // device [32][8] big-endian words (EMPTY_ROOTS)
  uint8_t* roots;
  uint8_t* proofs;  // may be null
  uint64_t proofs_stride;
  // nullable pair: hash only the leaves t (slice-major, t = slice * n_leaves + j) with
  // hash_leaf[t] != 0, compacted into list (nslices * n_leaves + 1 words of scratch); the other
  // leaves' digests must already be in nodes (a proof check's leaf_nodes, same bytes)
  const uint8_t* hash_leaf;
  uint32_t* list;
  uint32_t skip_leaf;  // > 0: leaf j >= skip_leaf sits at (j + 1) * leaf_stride (a withheld row)
  // nullable: one leaf size per slice (device [nslices], each even, 2 .. 1024).  Needs n_leaves =
  // 64 and no skip_leaf; leaf j of slice s is then leaf_sizes[s] bytes at leaves +
  // s*slice_stride + j*leaf_sizes[s] (the var coder's packed codewords); leaf_stride and
  // leaf_bytes are unused.  One leaf kernel for the whole batch, whatever the mix of sizes.
  // With hash_leaf: only the flagged leaves, one wave per slice (list unused: no compaction, the
  // size stays wave-uniform).
  const uint32_t* leaf_sizes;
};
// The leaf kernel classes a build launches (leaf_kernels below; a test aid).
enum MerkleLeafKernelBit : uint32_t {
  kMkLeafAligned = 1u << 0,  // uniform size, every row 16-byte aligned: vector loads
  kMkLeafByte = 1u << 1,     // uniform size, any alignment: the per-byte loader
  kMkLeafVar = 1u << 2,      // one size per slice (leaf_sizes)
  kMkLeafVarFlagged = 1u << 3,  // one size per slice, only the flagged leaves (leaf_sizes + hash_leaf)
};
// nodes: the node digests (reference order, nodes_stride per slice; the caller's buffer or
// scratch) -- the levels are built there.  leaf_kernels (nullable): |= the MerkleLeafKernelBit of
// the leaf kernel launched.
hipError_t launch_merkle_build(const MerkleBuildParams& p, uint8_t* nodes, uint64_t nodes_stride,
                               hipStream_t stream, uint32_t* leaf_kernels = nullptr);

// check_proof for n leaves (or, with roots_out set, derive_root: the root each proof yields): leaf t at leaves + t*leaf_stride, its index index[t], the root
// roots + t*roots_stride, height proof digests at proofs + t*proofs_stride; ok[t] = 0/1.
struct MerkleVerifyParams {
  const uint8_t* leaves;
  uint64_t leaf_stride;
  uint32_t leaf_bytes;
  uint32_t height;
  const uint32_t* index;
  const uint8_t* roots;
  uint64_t roots_stride;
  const uint8_t* proofs;
  uint64_t proofs_stride;
  uint64_t n;
  uint8_t* ok;
  uint8_t* roots_out;  // derive_root mode (merkle.rs:411-428): root digests out, 32 B each; ok unused
  const uint8_t* active;  // nullable: leaves with active[t] == 0 are skipped (nothing written)
  uint32_t* list;         // nullable, n + 1 words of device scratch: with `active`, the active
                          // leaves are compacted first so that no lane idles on a skipped one
  uint8_t* leaf_nodes;    // nullable: leaf t's digest also to leaf_nodes + (t / leaves_per_tree) *
  uint64_t leaf_nodes_stride;  // leaf_nodes_stride + 32 (t % leaves_per_tree) (a later build's
  uint32_t leaves_per_tree;    // level 0, launch_merkle_build's nodes layout)
  uint64_t group_stride;       // leaf t at leaves + grouped_row_offset(t, leaf_stride, group_stride,
  uint32_t skip_row;           // skip_row) (group_stride 0: t * leaf_stride)
  // nullable pair (check mode only; needs empty_roots): item t's proof is proof_len[t] digests
  // instead of `height` (> 32, or more than proofs_stride holds: ok = 0, its proof is not read),
  // and with last[t] != 0 the check is check_proof_last (merkle.rs:394-407, 436-452): every
  // sibling on the right must be EMPTY_ROOTS[its height].  last null = all 0.
  const uint32_t* proof_len;
  const uint8_t* last;
  const uint32_t* empty_roots;  // device [32][8] big-endian words
  // nullable (derive-root mode with active + list): one leaf size per size_group consecutive items
  // (device [n / size_group], each even, 2 .. 1024) instead of leaf_bytes.  size_group 1: leaf t
  // at leaves + t*leaf_stride; size_group 64: leaf t is row t % 64 of slice t / 64, at leaves +
  // (t / 64)*group_stride + (t % 64)*size (rows packed at the slice's size; no skip_row)
  const uint32_t* leaf_sizes;
  uint32_t size_group;
};
hipError_t launch_merkle_verify(const MerkleVerifyParams& p, hipStream_t stream);

// MAX_SLICES_PER_BLOCK (slice_index.rs:15): a block's double-Merkle tree has at most 1024 leaves.
constexpr uint32_t kBlockMaxSlices = 1024;

// DoubleMerkleTree::new (merkle.rs:263, 281-333) for nblocks blocks: block b's leaves are the
// count[b] slice roots (32 B each, 1 <= count[b] <= 1024) from slice_roots + 32 * first[b].
// Outputs (device): block_hashes[b] (32 B, the BlockHash); nodes (optional) = the reference's
// `nodes` vector per block at nodes_stride; proofs (optional, needs nodes) = create_proof(j) for
// every slice j, height(count[b]) digests each, at proofs + b * proofs_stride.
struct BlockTreeParams {
  const uint64_t* first;  // device [nblocks]
  const uint32_t* count;  // device [nblocks]
  uint64_t nblocks;
  const uint8_t* slice_roots;
  const uint32_t* empty_roots;  // device [32][8] big-endian words (EMPTY_ROOTS)
  uint8_t* block_hashes;
  uint8_t* nodes;  // may be null (unless proofs is set)
  uint64_t nodes_stride;
  uint8_t* proofs;  // may be null
  uint64_t proofs_stride;
};
hipError_t launch_block_tree(const BlockTreeParams& p, hipStream_t stream);

// EMPTY_ROOTS[h] as big-endian words (host; the same SHA-256 code as the kernels).
void merkle_empty_roots(uint32_t out[kMerkleMaxHeight][8]);

}  // namespace ag
