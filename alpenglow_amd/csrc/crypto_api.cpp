// The C ABI of what surrounds the coder (include/alpenglow_rs.h): slice Merkle trees, block
// trees, the all-or-nothing payload transforms, Ed25519 signatures and shred validation --
// argument checks and scratch in front of the kernels of merkle.hip, cipher.hip, ed25519.hip and
// shredder.hip.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../include/alpenglow_rs.h"
#include "cipher.hpp"
#include "ed25519.hpp"
#include "merkle.hpp"
#include "rs_ctx.hpp"
#include "shredder.hpp"

using namespace ag::host;

namespace {
constexpr size_t kMerkleVarMaxSlices = size_t{1} << 27;  // (the var coder's limit)

// ag_merkle_build_batch_var's host-side checks (sizes on the host): 0 or the status
int merkle_var_check(size_t nslices, const uint32_t* leaf_bytes, const uint8_t* leaves, size_t slice_stride,
                     const uint8_t* roots, const uint8_t* nodes, size_t nodes_stride, const uint8_t* proofs,
                     size_t proofs_stride) {
  if (!leaf_bytes || !leaves || !roots || nslices > kMerkleVarMaxSlices) return AG_RS_ERR_INVALID_ARGUMENT;
  size_t max_s = 0;
  for (size_t b = 0; b < nslices; ++b) {
    if (leaf_bytes[b] == 0 || leaf_bytes[b] % 2) return AG_RS_ERR_INVALID_SHARD_SIZE;
    if (leaf_bytes[b] > AG_RS_MAX_DATA_PER_SHRED) return AG_RS_ERR_TOO_MUCH_DATA;
    max_s = std::max<size_t>(max_s, leaf_bytes[b]);
  }
  constexpr size_t n = AG_MERKLE_MAX_LEAVES;
  if (slice_stride < n * max_s ||
      (nodes && (nodes_stride % 16 || nodes_stride < 32 * ag_merkle_node_count(n))) ||
      (proofs && (proofs_stride % 16 || proofs_stride < 32 * ag_merkle_height(n) * n)) ||
      reinterpret_cast<uintptr_t>(roots) % 16 || reinterpret_cast<uintptr_t>(nodes) % 16 ||
      reinterpret_cast<uintptr_t>(proofs) % 16)
    return AG_RS_ERR_INVALID_ARGUMENT;
  return AG_RS_OK;
}

}  // namespace

namespace ag::host {
int ensure_ed_base(ag_rs_ctx* c) {
  if (c->d_ed_base.ptr) return AG_RS_OK;
  int st = c->d_ed_base.ensure(ag::kEdBaseTableBytes, c->stream);
  if (st) return st;
  return ag::launch_ed25519_init(c->d_ed_base.as<int32_t>(), c->stream) == hipSuccess ? AG_RS_OK : AG_RS_ERR_DEVICE;
}
int ensure_empty_roots(ag_rs_ctx* c) {
  if (c->d_empty_roots.ptr) return AG_RS_OK;
  uint32_t er[ag::kMerkleMaxHeight][8];
  ag::merkle_empty_roots(er);
  int st = c->d_empty_roots.ensure(sizeof er, c->stream);
  if (st) return st;
  AG_HIP(hipMemcpy(c->d_empty_roots.ptr, er, sizeof er, hipMemcpyHostToDevice));
  return AG_RS_OK;
}

// The launches of ag_merkle_build_batch_var over sizes already on the device (d_sizes; checked by
// the caller on the host): the composed shred hands over the table its coder stage uploaded.
int merkle_var_launch(ag_rs_ctx* c, size_t nslices, const uint32_t* d_sizes, const uint8_t* leaves,
                      size_t slice_stride, uint8_t* roots, uint8_t* nodes, size_t nodes_stride, uint8_t* proofs,
                      size_t proofs_stride) {
  int st = ensure_empty_roots(c);
  if (st) return st;
  ag::MerkleBuildParams p{};
  p.leaves = leaves;
  p.slice_stride = slice_stride;
  p.n_leaves = AG_MERKLE_MAX_LEAVES;
  p.nslices = nslices;
  p.empty_roots = c->d_empty_roots.as<uint32_t>();
  p.roots = roots;
  p.proofs = proofs;
  p.proofs_stride = proofs_stride;
  p.leaf_sizes = d_sizes;
  if (!nodes) {
    nodes_stride = (32 * ag_merkle_node_count(AG_MERKLE_MAX_LEAVES) + 255) / 256 * 256;
    if ((st = c->d_merkle_nodes.ensure(nslices * nodes_stride, c->stream))) return st;
    nodes = c->d_merkle_nodes.as<uint8_t>();
  }
  c->last_merkle_kernels = 0;
  return ag::launch_merkle_build(p, nodes, nodes_stride, c->stream, &c->last_merkle_kernels) == hipSuccess
             ? AG_RS_OK
             : AG_RS_ERR_DEVICE;
}

// lengths (host) -> device; the batch descriptor
int aon_batch(ag_rs_ctx* c, size_t n, uint8_t* buffers, size_t stride, const uint32_t* lens, uint32_t extra,
              ag::BufferBatch* bb) {
  uint32_t mx = 0;
  for (size_t b = 0; b < n; ++b) {
    if (lens[b] > (1u << 28)) return AG_RS_ERR_INVALID_ARGUMENT;
    mx = std::max(mx, lens[b]);
  }
  if (n > 1 && stride < static_cast<size_t>(mx) + extra) return AG_RS_ERR_INVALID_ARGUMENT;
  int st = c->d_aon_lens.ensure(n * 4, c->stream);
  if (st) return st;
  AG_HIP(hipStreamSynchronize(c->stream));  // a previous call's upload may still be pending
  AG_HIP(hipMemcpy(c->d_aon_lens.ptr, lens, n * 4, hipMemcpyHostToDevice));
  bb->base = buffers;
  bb->stride = stride;
  bb->lens = c->d_aon_lens.as<uint32_t>();
  bb->n = n;
  bb->max_len = mx;
  return AG_RS_OK;
}

// ag_shred_validate_batch with the cache entries shared by cached_group consecutive shreds
// (the composed deshred: one cached commitment per slice).
// `merkle`: the shreds and their Merkle paths (step 1's launch; n shreds, `active` nullable);
// its roots_out and list are filled in here.  The caller has checked its arguments.
// roots_ready: step 1 already ran (launch_merkle_verify over `merkle`, e.g. on another stream):
// roots_out holds every active shred's derived root.
int shred_validate_impl(ag_rs_ctx* c, const ag::MerkleVerifyParams& merkle, const uint64_t* slots,
                        const uint64_t* slice_indices, const uint8_t* is_last, const uint8_t* sigs, size_t sig_stride,
                        const uint8_t* pk, const uint8_t* cached, const uint8_t* has_cached, uint32_t cached_group,
                        uint8_t* status, uint8_t* roots_out, uint8_t* commitments_out, bool roots_ready) {
  if (roots_ready && !roots_out) return AG_RS_ERR_INVALID_ARGUMENT;
  const size_t n = merkle.n;
  if (c->enter()) return AG_RS_ERR_DEVICE;
  int st = ensure_ed_base(c);
  if (st) return st;
  uint8_t* roots = roots_out;
  if (!roots) {
    if ((st = c->d_sh_roots.ensure(32 * n, c->stream))) return st;
    roots = c->d_sh_roots.as<uint8_t>();
  }
  uint8_t* commits = commitments_out;
  if (!commits) {
    if ((st = c->d_sh_commit.ensure(ag::kSliceCommitmentLen * n, c->stream))) return st;
    commits = c->d_sh_commit.as<uint8_t>();
  }
  if ((st = c->d_sh_onvalid.ensure(n, c->stream)) || (st = c->d_sh_list.ensure(4 * (n + 1), c->stream))) return st;
  uint32_t* list = c->d_sh_list.as<uint32_t>();
  uint32_t* count = list + n;
  // 1. Shred::slice_root (shredder.rs:168-175): derive_root from the Merkle path
  ag::MerkleVerifyParams mp = merkle;
  mp.roots_out = roots;
  mp.list = list;  // scratch until the signature list below reuses it (stream order)
  if (!roots_ready && ag::launch_merkle_verify(mp, c->stream) != hipSuccess) return AG_RS_ERR_DEVICE;
  // 2. SliceCommitment + cached-commitment rule (validated_shred.rs:57-64)
  AG_HIP(hipMemsetAsync(count, 0, 4, c->stream));
  ag::ShredCommitParams cp{};
  cp.slots = slots;
  cp.slice_indices = slice_indices;
  cp.is_last = is_last;
  cp.roots = roots;
  cp.cached = cached;
  cp.has_cached = has_cached;
  cp.cached_group = cached_group;
  cp.active = merkle.active;
  cp.n = n;
  cp.commitments = commits;
  cp.status = status;
  cp.on_valid = c->d_sh_onvalid.as<uint8_t>();
  cp.list = list;
  cp.list_count = count;
  if (ag::launch_shred_commit(cp, c->stream) != hipSuccess) return AG_RS_ERR_DEVICE;
  // 3. signature checks for the listed shreds (validated_shred.rs:65-77)
  ag::EdVerifyParams vp{};
  vp.pks = pk;
  vp.pk_stride = 0;
  vp.msgs = commits;
  vp.msg_stride = ag::kSliceCommitmentLen;
  vp.msg_len = ag::kSliceCommitmentLen;
  vp.sigs = sigs;
  vp.sig_stride = sig_stride;
  vp.n = n;
  vp.list = list;
  vp.list_count = count;
  vp.status = status;
  vp.on_valid = c->d_sh_onvalid.as<uint8_t>();
  vp.base_table = c->d_ed_base.as<int32_t>();
  return ag::launch_ed25519_verify(vp, c->stream) == hipSuccess ? AG_RS_OK : AG_RS_ERR_DEVICE;
}

// ag_slice_sign_batch in two pieces, so that a caller can sign on another stream than c->stream.
// The first: the argument checks, the Ed25519 table and the scratch, everything that may launch,
// wait or free on c->stream (the validation above shares that scratch on that stream).
int slice_sign_prepare(ag_rs_ctx* c, size_t nslices, const uint8_t* seed, const uint8_t* pk, const uint64_t* slots,
                       const uint64_t* slice_indices, const uint8_t* is_last, const uint8_t* roots,
                       const uint8_t* sigs, const uint8_t* commitments_out) {
  if (!c || nslices >= kMaxSigBatch ||
      (nslices && (!seed || !pk || !slots || !slice_indices || !is_last || !roots || !sigs)))
    return AG_RS_ERR_INVALID_ARGUMENT;
  if (nslices == 0) return AG_RS_OK;
  if (c->enter()) return AG_RS_ERR_DEVICE;
  int st = ensure_ed_base(c);
  if (st) return st;
  if (!commitments_out && (st = c->d_sh_commit.ensure(ag::kSliceCommitmentLen * nslices, c->stream))) return st;
  if ((st = c->d_sh_onvalid.ensure(2 * nslices, c->stream))) return st;
  return c->d_sh_list.ensure(4 * (nslices + 1), c->stream);
}

// The second (nslices > 0, prepared): only enqueues, on `stream`.
int slice_sign_enqueue(ag_rs_ctx* c, size_t nslices, const uint8_t* seed, const uint8_t* pk, const uint64_t* slots,
                       const uint64_t* slice_indices, const uint8_t* is_last, const uint8_t* roots, uint8_t* sigs,
                       uint8_t* commitments_out, hipStream_t stream) {
  const size_t n = nslices;
  uint8_t* commits = commitments_out ? commitments_out : c->d_sh_commit.as<uint8_t>();
  uint32_t* list = c->d_sh_list.as<uint32_t>();
  AG_HIP(hipMemsetAsync(list + n, 0, 4, stream));
  // SliceCommitment::new (shredder.rs:206-215); no cache, so every slice is listed
  ag::ShredCommitParams cp{};
  cp.slots = slots;
  cp.slice_indices = slice_indices;
  cp.is_last = is_last;
  cp.roots = roots;
  cp.n = n;
  cp.commitments = commits;
  cp.status = c->d_sh_onvalid.as<uint8_t>() + n;
  cp.on_valid = c->d_sh_onvalid.as<uint8_t>();
  cp.list = list;
  cp.list_count = list + n;
  if (ag::launch_shred_commit(cp, stream) != hipSuccess) return AG_RS_ERR_DEVICE;
  // sk.sign_bytes(commitment) (shredder.rs:540)
  ag::EdSignParams p{};
  p.seeds = seed;
  p.seed_stride = 0;
  p.pks = pk;
  p.pk_stride = 0;
  p.msgs = commits;
  p.msg_stride = ag::kSliceCommitmentLen;
  p.msg_len = ag::kSliceCommitmentLen;
  p.sigs = sigs;
  p.n = n;
  p.base_table = c->d_ed_base.as<int32_t>();
  return ag::launch_ed25519_sign(p, stream) == hipSuccess ? AG_RS_OK : AG_RS_ERR_DEVICE;
}
}  // namespace ag::host

extern "C" {

// ---- slice Merkle trees --------------------------------------------------------------

size_t ag_merkle_height(size_t n) {
  size_t h = 0;
  for (size_t len = n; len > 1; len = (len + 1) / 2) ++h;
  return h;
}

size_t ag_merkle_node_count(size_t n) {
  size_t total = n;
  for (size_t len = n; len > 1;) {
    len = (len + 1) / 2;
    total += len;
  }
  return total;
}

int ag_merkle_empty_root(size_t height, uint8_t out[32]) {
  if (!out || height >= static_cast<size_t>(ag::kMerkleMaxHeight)) return AG_RS_ERR_INVALID_ARGUMENT;
  uint32_t er[ag::kMerkleMaxHeight][8];
  ag::merkle_empty_roots(er);
  for (int i = 0; i < 8; ++i)
    for (int b = 0; b < 4; ++b) out[4 * i + b] = static_cast<uint8_t>(er[height][i] >> (24 - 8 * b));
  return AG_RS_OK;
}

int ag_merkle_build_batch(ag_rs_ctx* c, size_t n_leaves, size_t leaf_bytes, size_t nslices, const uint8_t* leaves,
                          size_t leaf_stride, size_t slice_stride, uint8_t* roots, uint8_t* nodes,
                          size_t nodes_stride, uint8_t* proofs, size_t proofs_stride) {
  if (!c || n_leaves == 0 || n_leaves > AG_MERKLE_MAX_LEAVES || leaf_bytes >= (size_t{1} << 28))
    return AG_RS_ERR_INVALID_ARGUMENT;
  if (nslices == 0) return AG_RS_OK;
  if ((leaf_bytes && !leaves) || !roots || (n_leaves > 1 && leaf_stride < leaf_bytes) ||
      (nslices > 1 && slice_stride < (n_leaves - 1) * leaf_stride + leaf_bytes))
    return AG_RS_ERR_INVALID_ARGUMENT;
  const size_t h = ag_merkle_height(n_leaves);
  if ((nodes && (nodes_stride % 16 || (nslices > 1 && nodes_stride < 32 * ag_merkle_node_count(n_leaves)))) ||
      (proofs && (proofs_stride % 16 || (nslices > 1 && proofs_stride < 32 * h * n_leaves))) ||
      reinterpret_cast<uintptr_t>(roots) % 16 || reinterpret_cast<uintptr_t>(nodes) % 16 ||
      reinterpret_cast<uintptr_t>(proofs) % 16)
    return AG_RS_ERR_INVALID_ARGUMENT;
  if (c->enter()) return AG_RS_ERR_DEVICE;
  int st = ensure_empty_roots(c);
  if (st) return st;
  ag::MerkleBuildParams p{};
  p.leaves = leaves;
  p.leaf_stride = leaf_stride;
  p.slice_stride = slice_stride;
  p.leaf_bytes = static_cast<uint32_t>(leaf_bytes);
  p.n_leaves = static_cast<uint32_t>(n_leaves);
  p.nslices = nslices;
  p.empty_roots = c->d_empty_roots.as<uint32_t>();
  p.roots = roots;
  p.proofs = proofs;
  p.proofs_stride = proofs_stride;
  if (!nodes) {  // the levels are built in memory: scratch when the caller wants no nodes
    nodes_stride = (32 * ag_merkle_node_count(n_leaves) + 255) / 256 * 256;
    if ((st = c->d_merkle_nodes.ensure(nslices * nodes_stride, c->stream))) return st;
    nodes = c->d_merkle_nodes.as<uint8_t>();
  }
  c->last_merkle_kernels = 0;
  return ag::launch_merkle_build(p, nodes, nodes_stride, c->stream, &c->last_merkle_kernels) == hipSuccess
             ? AG_RS_OK
             : AG_RS_ERR_DEVICE;
}

int ag_merkle_build_batch_var(ag_rs_ctx* c, size_t nslices, const uint32_t* leaf_bytes, const uint8_t* leaves,
                              size_t slice_stride, uint8_t* roots, uint8_t* nodes, size_t nodes_stride,
                              uint8_t* proofs, size_t proofs_stride) {
  if (!c) return AG_RS_ERR_INVALID_ARGUMENT;
  if (nslices == 0) return AG_RS_OK;
  int st = merkle_var_check(nslices, leaf_bytes, leaves, slice_stride, roots, nodes, nodes_stride, proofs,
                            proofs_stride);
  if (st) return st;
  if ((st = c->enter())) return st;
  // the sizes go up through pinned staging of their own (the coder's payload lengths keep theirs)
  uint32_t* h;
  if ((st = c->leaf_sizes.host(4 * nslices, &h))) return st;
  std::memcpy(h, leaf_bytes, 4 * nslices);
  if ((st = c->leaf_sizes.send(4 * nslices, c->stream))) return st;
  return merkle_var_launch(c, nslices, c->leaf_sizes.dev.as<uint32_t>(), leaves, slice_stride, roots, nodes,
                           nodes_stride, proofs, proofs_stride);
}

int ag_merkle_verify_batch(ag_rs_ctx* c, size_t n, size_t leaf_bytes, const uint8_t* leaves, size_t leaf_stride,
                           const uint32_t* index, const uint8_t* roots, size_t roots_stride, const uint8_t* proofs,
                           size_t proofs_stride, size_t height, uint8_t* ok) {
  if (!c || leaf_bytes >= (size_t{1} << 28) || height > static_cast<size_t>(ag::kMerkleMaxHeight))
    return AG_RS_ERR_INVALID_ARGUMENT;
  if (n == 0) return AG_RS_OK;
  if ((leaf_bytes && !leaves) || !index || !roots || !ok || (height && !proofs) || roots_stride % 16 ||
      proofs_stride % 16 || reinterpret_cast<uintptr_t>(roots) % 16 || reinterpret_cast<uintptr_t>(proofs) % 16 ||
      (n > 1 && leaf_stride < leaf_bytes))
    return AG_RS_ERR_INVALID_ARGUMENT;
  if (c->enter()) return AG_RS_ERR_DEVICE;
  ag::MerkleVerifyParams p{};
  p.leaves = leaves;
  p.leaf_stride = leaf_stride;
  p.leaf_bytes = static_cast<uint32_t>(leaf_bytes);
  p.height = static_cast<uint32_t>(height);
  p.index = index;
  p.roots = roots;
  p.roots_stride = roots_stride;
  p.proofs = proofs;
  p.proofs_stride = proofs_stride;
  p.n = n;
  p.ok = ok;
  return ag::launch_merkle_verify(p, c->stream) == hipSuccess ? AG_RS_OK : AG_RS_ERR_DEVICE;
}

// ---- block trees: the double-Merkle tree over a block's slice roots -----------------------

int ag_block_tree_batch(ag_rs_ctx* c, size_t nblocks, const uint32_t* count, const uint8_t* slice_roots,
                        uint8_t* block_hashes, uint8_t* nodes, size_t nodes_stride, uint8_t* proofs,
                        size_t proofs_stride) {
  static_assert(AG_BLOCK_MAX_SLICES == ag::kBlockMaxSlices);
  if (!c) return AG_RS_ERR_INVALID_ARGUMENT;
  if (nblocks == 0) return AG_RS_OK;
  if (!count || !slice_roots || !block_hashes || nblocks > 0x7FFFFFFFull) return AG_RS_ERR_INVALID_ARGUMENT;
  uint32_t mx = 0;
  for (size_t b = 0; b < nblocks; ++b) {
    if (count[b] == 0 || count[b] > AG_BLOCK_MAX_SLICES) return AG_RS_ERR_INVALID_ARGUMENT;
    mx = std::max(mx, count[b]);
  }
  // node count and height * count both grow with the count: the largest block sets the strides
  if ((reinterpret_cast<uintptr_t>(slice_roots) | reinterpret_cast<uintptr_t>(block_hashes) |
       reinterpret_cast<uintptr_t>(nodes) | reinterpret_cast<uintptr_t>(proofs)) % 16 ||
      (nodes && (nodes_stride % 16 || (nblocks > 1 && nodes_stride < 32 * ag_merkle_node_count(mx)))) ||
      (proofs && (proofs_stride % 16 || (nblocks > 1 && proofs_stride < 32 * ag_merkle_height(mx) * mx))))
    return AG_RS_ERR_INVALID_ARGUMENT;
  int st = c->enter();
  if (st || (st = ensure_empty_roots(c))) return st;
  // offsets and counts go up through pinned staging on the context stream, as the coder's
  // payload lengths do
  uint64_t* first;
  if ((st = c->block_meta.host(12 * nblocks, &first))) return st;
  uint32_t* cnt = reinterpret_cast<uint32_t*>(first + nblocks);
  uint64_t at = 0;
  for (size_t b = 0; b < nblocks; ++b) {
    first[b] = at;
    cnt[b] = count[b];
    at += count[b];
  }
  if ((st = c->block_meta.send(12 * nblocks, c->stream))) return st;
  ag::BlockTreeParams p{};
  p.first = c->block_meta.dev.as<uint64_t>();
  p.count = reinterpret_cast<const uint32_t*>(p.first + nblocks);
  p.nblocks = nblocks;
  p.slice_roots = slice_roots;
  p.empty_roots = c->d_empty_roots.as<uint32_t>();
  p.block_hashes = block_hashes;
  p.nodes = nodes;
  p.nodes_stride = nodes_stride;
  p.proofs = proofs;
  p.proofs_stride = proofs_stride;
  if (proofs && !nodes) {  // the proofs are gathered from the nodes: scratch when the caller wants none
    p.nodes_stride = (32 * ag_merkle_node_count(mx) + 255) / 256 * 256;
    if ((st = c->d_merkle_nodes.ensure(nblocks * p.nodes_stride, c->stream))) return st;
    p.nodes = c->d_merkle_nodes.as<uint8_t>();
  }
  return ag::launch_block_tree(p, c->stream) == hipSuccess ? AG_RS_OK : AG_RS_ERR_DEVICE;
}

int ag_block_proof_check_batch(ag_rs_ctx* c, size_t n, const uint8_t* slice_roots, size_t roots_stride,
                               const uint32_t* index, const uint8_t* block_hashes, size_t hashes_stride,
                               const uint8_t* proofs, size_t proofs_stride, const uint32_t* proof_len,
                               const uint8_t* last, uint8_t* ok) {
  if (!c) return AG_RS_ERR_INVALID_ARGUMENT;
  if (n == 0) return AG_RS_OK;
  // proofs may be null only with a zero stride, which holds no digest: any proof_len > 0 is then ok = 0
  if (!slice_roots || !index || !block_hashes || !proof_len || !ok || (!proofs && proofs_stride) ||
      hashes_stride % 16 || proofs_stride % 16 || reinterpret_cast<uintptr_t>(block_hashes) % 16 ||
      reinterpret_cast<uintptr_t>(proofs) % 16 || (n > 1 && roots_stride < 32))
    return AG_RS_ERR_INVALID_ARGUMENT;
  int st = c->enter();
  if (st || (st = ensure_empty_roots(c))) return st;
  ag::MerkleVerifyParams p{};
  p.leaves = slice_roots;
  p.leaf_stride = roots_stride;
  p.leaf_bytes = 32;
  p.index = index;
  p.roots = block_hashes;
  p.roots_stride = hashes_stride;
  p.proofs = proofs;
  p.proofs_stride = proofs_stride;
  p.n = n;
  p.ok = ok;
  p.proof_len = proof_len;
  p.last = last;
  p.empty_roots = c->d_empty_roots.as<uint32_t>();
  return ag::launch_merkle_verify(p, c->stream) == hipSuccess ? AG_RS_OK : AG_RS_ERR_DEVICE;
}

// ---- all-or-nothing payload transforms ------------------------------------------------

int ag_aes128_encrypt_block(const uint8_t key[16], const uint8_t in[16], uint8_t out[16]) {
  if (!key || !in || !out) return AG_RS_ERR_INVALID_ARGUMENT;
  ag::aes128_encrypt_block(key, in, out);
  return AG_RS_OK;
}

int ag_cipher_apply_keystream_batch(ag_rs_ctx* c, size_t n, const uint8_t* keys, uint8_t* buffers, size_t stride,
                                    const uint32_t* lens) {
  if (!c || (n && (!keys || !buffers || !lens))) return AG_RS_ERR_INVALID_ARGUMENT;
  if (n == 0) return AG_RS_OK;
  if (c->enter()) return AG_RS_ERR_DEVICE;
  ag::BufferBatch bb;
  int st = aon_batch(c, n, buffers, stride, lens, 0, &bb);
  if (st) return st;
  return ag::launch_apply_keystream(bb, keys, 0, c->stream) == hipSuccess ? AG_RS_OK : AG_RS_ERR_DEVICE;
}

int ag_sha256_batch(ag_rs_ctx* c, size_t n, const uint8_t* buffers, size_t stride, const uint32_t* lens,
                    uint8_t* digests) {
  if (!c || (n && (!buffers || !lens || !digests))) return AG_RS_ERR_INVALID_ARGUMENT;
  if (n == 0) return AG_RS_OK;
  if (c->enter()) return AG_RS_ERR_DEVICE;
  ag::BufferBatch bb;
  int st = aon_batch(c, n, const_cast<uint8_t*>(buffers), stride, lens, 0, &bb);
  if (st) return st;
  return ag::launch_sha256(bb, 0, digests, c->stream) == hipSuccess ? AG_RS_OK : AG_RS_ERR_DEVICE;
}

int ag_aon_encrypt_batch(ag_rs_ctx* c, int scheme, size_t n, const uint8_t* keys, uint8_t* buffers, size_t stride,
                         const uint32_t* lens) {
  if (!c || (scheme != AG_AON_AONT && scheme != AG_AON_PETS) || (n && (!keys || !buffers || !lens)))
    return AG_RS_ERR_INVALID_ARGUMENT;
  if (n == 0) return AG_RS_OK;
  if (c->enter()) return AG_RS_ERR_DEVICE;
  ag::BufferBatch bb;
  int st = aon_batch(c, n, buffers, stride, lens, ag::kCipherKeyBytes, &bb);
  if (st) return st;
  const bool aont = scheme == AG_AON_AONT;
  if (aont && (st = c->d_aon_digests.ensure(n * 32, c->stream))) return st;
  if (ag::launch_apply_keystream(bb, keys, 0, c->stream) != hipSuccess) return AG_RS_ERR_DEVICE;
  if (aont && ag::launch_sha256(bb, 0, c->d_aon_digests.as<uint8_t>(), c->stream) != hipSuccess)
    return AG_RS_ERR_DEVICE;
  return ag::launch_write_key_tail(bb, aont, keys, aont ? c->d_aon_digests.as<uint8_t>() : nullptr, c->stream) ==
                 hipSuccess
             ? AG_RS_OK
             : AG_RS_ERR_DEVICE;
}

int ag_aon_decrypt_batch(ag_rs_ctx* c, int scheme, size_t n, uint8_t* buffers, size_t stride, const uint32_t* lens,
                         int64_t* plain_len_out) {
  if (!c || (scheme != AG_AON_AONT && scheme != AG_AON_PETS) || (n && (!buffers || !lens || !plain_len_out)))
    return AG_RS_ERR_INVALID_ARGUMENT;
  if (n == 0) return AG_RS_OK;
  if (c->enter()) return AG_RS_ERR_DEVICE;
  // buffers too short for a key: BadEncoding, left untouched (length 16 => empty payload)
  std::vector<uint32_t> lv(lens, lens + n);
  for (size_t b = 0; b < n; ++b) {
    plain_len_out[b] = lens[b] < ag::kCipherKeyBytes ? -AG_RS_ERR_BAD_ENCODING
                                                      : static_cast<int64_t>(lens[b]) - ag::kCipherKeyBytes;
    if (lens[b] < ag::kCipherKeyBytes) lv[b] = ag::kCipherKeyBytes;  // no-op (empty ciphertext, key unused)
  }
  ag::BufferBatch bb;
  int st = aon_batch(c, n, buffers, stride, lv.data(), 0, &bb);
  if (st) return st;
  const bool aont = scheme == AG_AON_AONT;
  if ((st = c->d_aon_keys.ensure(n * 16, c->stream))) return st;
  if (aont) {
    if ((st = c->d_aon_digests.ensure(n * 32, c->stream))) return st;
    if (ag::launch_sha256(bb, ag::kCipherKeyBytes, c->d_aon_digests.as<uint8_t>(), c->stream) != hipSuccess)
      return AG_RS_ERR_DEVICE;
  }
  if (ag::launch_derive_keys(bb, aont, aont ? c->d_aon_digests.as<uint8_t>() : nullptr, c->d_aon_keys.as<uint8_t>(),
                             c->stream) != hipSuccess ||
      ag::launch_apply_keystream(bb, c->d_aon_keys.as<uint8_t>(), ag::kCipherKeyBytes, c->stream) != hipSuccess)
    return AG_RS_ERR_DEVICE;
  AG_HIP(hipStreamSynchronize(c->stream));
  return AG_RS_OK;
}

// ---- Ed25519 shred signatures ------------------------------------------------------------

int ag_ed25519_public_key_batch(ag_rs_ctx* c, size_t n, const uint8_t* seeds, uint8_t* pks) {
  if (!c || n >= kMaxSigBatch || (n && (!seeds || !pks))) return AG_RS_ERR_INVALID_ARGUMENT;
  if (n == 0) return AG_RS_OK;
  if (c->enter()) return AG_RS_ERR_DEVICE;
  int st = ensure_ed_base(c);
  if (st) return st;
  return ag::launch_ed25519_public_key(seeds, pks, n, c->d_ed_base.as<int32_t>(), c->stream) == hipSuccess
             ? AG_RS_OK
             : AG_RS_ERR_DEVICE;
}

int ag_ed25519_sign_batch(ag_rs_ctx* c, size_t n, const uint8_t* seeds, size_t seed_stride, const uint8_t* pks,
                          size_t pk_stride, const uint8_t* msgs, size_t msg_stride, size_t msg_len, uint8_t* sigs) {
  if (!c || n >= kMaxSigBatch || msg_len >= (size_t{1} << 28) ||
      (n && (!seeds || !pks || !sigs || (msg_len && !msgs))))
    return AG_RS_ERR_INVALID_ARGUMENT;
  if (n == 0) return AG_RS_OK;
  if (c->enter()) return AG_RS_ERR_DEVICE;
  int st = ensure_ed_base(c);
  if (st) return st;
  ag::EdSignParams p{};
  p.seeds = seeds;
  p.seed_stride = seed_stride;
  p.pks = pks;
  p.pk_stride = pk_stride;
  p.msgs = msgs;
  p.msg_stride = msg_stride;
  p.msg_len = static_cast<uint32_t>(msg_len);
  p.sigs = sigs;
  p.n = n;
  p.base_table = c->d_ed_base.as<int32_t>();
  return ag::launch_ed25519_sign(p, c->stream) == hipSuccess ? AG_RS_OK : AG_RS_ERR_DEVICE;
}

int ag_ed25519_verify_batch(ag_rs_ctx* c, size_t n, const uint8_t* pks, size_t pk_stride, const uint8_t* msgs,
                            size_t msg_stride, const uint32_t* msg_lens, size_t msg_len, const uint8_t* sigs,
                            size_t sig_stride, uint8_t* ok) {
  if (!c || n >= kMaxSigBatch || msg_len >= (size_t{1} << 28) || (n && (!pks || !sigs || !ok)) ||
      (n && !msgs && (msg_lens || msg_len)))
    return AG_RS_ERR_INVALID_ARGUMENT;
  if (n == 0) return AG_RS_OK;
  if (c->enter()) return AG_RS_ERR_DEVICE;
  int st = ensure_ed_base(c);
  if (st) return st;
  ag::EdVerifyParams p{};
  p.pks = pks;
  p.pk_stride = pk_stride;
  p.msgs = msgs;
  p.msg_stride = msg_stride;
  p.msg_lens = msg_lens;
  p.msg_len = static_cast<uint32_t>(msg_len);
  p.sigs = sigs;
  p.sig_stride = sig_stride;
  p.n = n;
  p.ok = ok;
  p.base_table = c->d_ed_base.as<int32_t>();
  return ag::launch_ed25519_verify(p, c->stream) == hipSuccess ? AG_RS_OK : AG_RS_ERR_DEVICE;
}

int ag_shred_validate_batch(ag_rs_ctx* c, size_t n, const uint8_t* data, size_t data_stride, size_t data_bytes,
                            const uint32_t* shred_index, const uint8_t* proofs, size_t proofs_stride, size_t height,
                            const uint64_t* slots, const uint64_t* slice_indices, const uint8_t* is_last,
                            const uint8_t* sigs, size_t sig_stride, const uint8_t* pk, const uint8_t* cached,
                            const uint8_t* has_cached, uint8_t* status, uint8_t* roots_out, uint8_t* commitments_out) {
  if (!c || n >= kMaxSigBatch || data_bytes >= (size_t{1} << 28) ||
      height > static_cast<size_t>(ag::kMerkleMaxHeight) ||
      (n && (!shred_index || !slots || !slice_indices || !is_last || !sigs || !pk || !status ||
             (data_bytes && !data) || (height && !proofs))) ||
      (cached == nullptr) != (has_cached == nullptr) || proofs_stride % 16 ||
      reinterpret_cast<uintptr_t>(proofs) % 16 || (n > 1 && data_stride < data_bytes))
    return AG_RS_ERR_INVALID_ARGUMENT;
  if (n == 0) return AG_RS_OK;
  ag::MerkleVerifyParams mp{};
  mp.leaves = data;
  mp.leaf_stride = data_stride;
  mp.leaf_bytes = static_cast<uint32_t>(data_bytes);
  mp.height = static_cast<uint32_t>(height);
  mp.index = shred_index;
  mp.proofs = proofs;
  mp.proofs_stride = proofs_stride;
  mp.n = n;
  return shred_validate_impl(c, mp, slots, slice_indices, is_last, sigs, sig_stride, pk, cached, has_cached, 1, status,
                             roots_out, commitments_out, false);
}

int ag_slice_sign_batch(ag_rs_ctx* c, size_t nslices, const uint8_t* seed, const uint8_t* pk, const uint64_t* slots,
                        const uint64_t* slice_indices, const uint8_t* is_last, const uint8_t* roots, uint8_t* sigs,
                        uint8_t* commitments_out) {
  const int st = slice_sign_prepare(c, nslices, seed, pk, slots, slice_indices, is_last, roots, sigs, commitments_out);
  if (st || nslices == 0) return st;
  return slice_sign_enqueue(c, nslices, seed, pk, slots, slice_indices, is_last, roots, sigs, commitments_out,
                            c->stream);
}

}  // extern "C"
