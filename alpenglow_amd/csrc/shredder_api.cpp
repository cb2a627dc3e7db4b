// Host side of the composed shredders: ag_shredder_shred_batch[_var|_kind] and
// ag_shredder_deshred_batch[_var|_kind] (include/alpenglow_rs.h), the four shredders of shredder.rs
// (Regular, CodingOnly, PETS, AONT) chained on the device from the batched stages of
// rs_coder_api.cpp, crypto_api.cpp and wire_api.cpp (slice framing, ReedSolomonCoder, Merkle trees,
// signatures, all-or-nothing transforms; the coder's encode / decode dispatch is rs_dispatch.cpp)
// and the glue kernels of shredder.hip / wire.hip.
//
// The entry points keep what is their own (argument checks, framing, the coder call, how a
// failed slice is decoded again) and share the stages around it: the row layout as data
// (ShredderKind), shred_tail, deshred_front, pipe_statuses, fill_missing.  Work on the context's side
// stream goes through SideScope (rs_ctx.hpp), which states and keeps the side-stream rule.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <vector>

#include "../../include/alpenglow_rs.h"
#include "cipher.hpp"
#include "ed25519.hpp"
#include "merkle.hpp"
#include "rs_ctx.hpp"
#include "rs_launch.hpp"
#include "shredder.hpp"
#include "wire.hpp"

using namespace ag::host;

namespace {

constexpr size_t kPipeProofBytes = 32 * ag::kPipeHeight;  // one Merkle path of a slice tree

// The composed shredders' scratch: two buffers of the context, each carved into a typed layout
// (Carver, rs_ctx.hpp).  d_pipe holds one call's scratch -- every size follows from the slice
// count, the row capacity and the kind, so an entry point grows it once, before its first launch,
// and carves ShredScratch or DeshredScratch out of it; calls on a context are ordered on its
// stream, so the two layouts share the bytes.  d_pipe_rerun holds the EXACT re-run's (RerunScratch):
// sized by the listed slices and so grown in mid-call, which must not move d_pipe under the
// kernels already queued.

// The shred side: the per-shred columns shred_tail writes (N = 64 n rows), and the per-slice roots
// and signatures of callers that pass no roots_out / sigs_out.
struct ShredScratch {
  uint8_t *kind, *proof, *roots, *sigs;
  uint32_t *shred_index, *data_len, *height;
};
size_t carve(uint8_t* base, size_t n, ShredScratch* s) {
  const size_t N = n * ag::kPipeShreds;
  Carver c{base};
  s->roots = c.take<uint8_t>(32 * n);
  s->sigs = c.take<uint8_t>(64 * n);
  s->kind = c.take<uint8_t>(N);
  s->shred_index = c.take<uint32_t>(N);
  s->data_len = c.take<uint32_t>(N);
  s->height = c.take<uint32_t>(N);
  s->proof = c.take<uint8_t>(kPipeProofBytes * N);
  return c.used;
}
int shred_scratch(ag_rs_ctx* c, size_t n, ShredScratch* s) {
  const int st = c->d_pipe.ensure(carve(nullptr, n, s), c->stream);
  if (st) return st;
  carve(c->d_pipe.as<uint8_t>(), n, s);
  return AG_RS_OK;
}

// The per-slice columns pipe_check writes, as read_pipe_meta brings them to the host in one copy
// (pinned staging: valid until the next call on the context)
struct PipeMeta {
  const uint64_t *present, *slot, *sidx;
  const uint8_t* last;
};

// The deshred side: what steps 1-3 (deshred_front) leave for the later ones, and the later
// steps' own columns.
struct DeshredScratch {
  // per shred (N = 64 n rows): the parsed columns (payload rows go straight into their codeword
  // rows: deshred_front sets cols.data and the row addressing)
  ag::ShredColumns cols{};
  uint8_t* wire;          // deserialize status
  uint8_t* val_status;    // the full validation's status
  uint8_t* roots;         // [N][32] every plausible shred's derived root
  uint8_t* plausible;     // the datagram parsed and fits its slot
  // [N + 1] list scratch of the Merkle kernels.  Two users in the Regular deshred: the compaction
  // list of the proof verify (side stream) and then of the Merkle rebuild (main stream) -- safe
  // because the main stream joins the side stream before the second validation, long before the
  // rebuild is enqueued.
  uint32_t* merkle_list;
  uint8_t* leaf_flags;    // Regular: leaves the rebuild hashes again
  uint32_t* fresh_lens;   // lengths of the datagrams fill_missing serialized
  // per slice: the picked shred (pipe_pick) and its validation
  uint8_t *pick, *g_data, *g_proof, *g_is_last, *g_sig, *pick_status, *commits, *has_cached;
  uint64_t *g_slot, *g_slice_index;
  uint32_t* g_shred_index;
  // per slice: pipe_check's outputs and the rebuilt roots
  uint8_t* sroot;         // [n][32] the kept shreds' signed root
  uint8_t* roots2;        // [n][32] for the rebuilt tree's root
  uint8_t* ssig;          // [n][64]
  // present | slot | slice index | is_last: ONE section split by hand, 25 n contiguous bytes from
  // d_present (read_pipe_meta's single copy)
  uint64_t *d_present, *d_slot, *d_slice_index;
  uint8_t* d_is_last;
  uint64_t* coder_words;  // CodingOnly / PETS: the kept shreds as codeword-row present words (two per slice)
  uint8_t* same;          // rebuilt root == signed root
  uint8_t* slice_ok;      // the slices fill_missing serves
  PipeMeta h;             // present | slot | slice index | is_last on the host
};
// row: the capacity of a picked row (S, or 1024 with mixed sizes); coder_words: per slice
size_t carve(uint8_t* base, size_t n, size_t row, size_t coder_words, DeshredScratch* s) {
  const size_t N = n * ag::kPipeShreds;
  Carver c{base};
  s->cols.kind = c.take<uint8_t>(N);
  s->cols.slot = c.take<uint64_t>(N);
  s->cols.slice_index = c.take<uint64_t>(N);
  s->cols.is_last = c.take<uint8_t>(N);
  s->cols.shred_index = c.take<uint32_t>(N);
  s->cols.data_len = c.take<uint32_t>(N);
  s->cols.sig = c.take<uint8_t>(64 * N);
  s->cols.proof = c.take<uint8_t>(kPipeProofBytes * N);
  s->cols.proof_stride = kPipeProofBytes;
  s->cols.height = c.take<uint32_t>(N);
  s->wire = c.take<uint8_t>(N);
  s->val_status = c.take<uint8_t>(N);
  s->roots = c.take<uint8_t>(32 * N);
  s->plausible = c.take<uint8_t>(N);
  s->merkle_list = c.take<uint32_t>(N + 1);
  s->leaf_flags = c.take<uint8_t>(N);
  s->fresh_lens = c.take<uint32_t>(N);
  s->pick = c.take<uint8_t>(n);
  s->g_data = c.take<uint8_t>(n * row);
  s->g_proof = c.take<uint8_t>(kPipeProofBytes * n);
  s->g_slot = c.take<uint64_t>(n);
  s->g_slice_index = c.take<uint64_t>(n);
  s->g_is_last = c.take<uint8_t>(n);
  s->g_shred_index = c.take<uint32_t>(n);
  s->g_sig = c.take<uint8_t>(64 * n);
  s->pick_status = c.take<uint8_t>(n);
  s->commits = c.take<uint8_t>(ag::kSliceCommitmentLen * n);
  s->has_cached = c.take<uint8_t>(n);
  s->sroot = c.take<uint8_t>(32 * n);
  s->roots2 = c.take<uint8_t>(32 * n);
  s->ssig = c.take<uint8_t>(64 * n);
  if (uint8_t* meta = c.take<uint8_t>(25 * n)) {
    s->d_present = reinterpret_cast<uint64_t*>(meta);
    s->d_slot = s->d_present + n;
    s->d_slice_index = s->d_slot + n;
    s->d_is_last = meta + 24 * n;
  }
  s->coder_words = c.take<uint64_t>(coder_words * n);
  s->same = c.take<uint8_t>(n);
  s->slice_ok = c.take<uint8_t>(n);
  return c.used;
}

// The EXACT re-run, per listed slice (R of them, compact codewords of cstride bytes).
struct RerunScratch {
  uint32_t *list, *sizes, *col_base;  // ONE section, list | sizes | column prefix: one upload
  uint8_t* codewords;                 // the compact codewords
  uint8_t *sroot, *roots;             // [R][32] signed roots, rebuilt roots
  uint64_t* present;                  // kept-shred words
  uint8_t* same;                      // the root comparison
  uint8_t* proofs;                    // the rebuilt trees' 64 paths
};
size_t carve(uint8_t* base, size_t R, size_t cstride, RerunScratch* s) {
  Carver c{base};
  if ((s->list = c.take<uint32_t>(3 * R + 1))) {
    s->sizes = s->list + R;
    s->col_base = s->list + 2 * R;
  }
  s->codewords = c.take<uint8_t>(R * cstride);
  s->sroot = c.take<uint8_t>(32 * R);
  s->roots = c.take<uint8_t>(32 * R);
  s->present = c.take<uint64_t>(R);
  s->same = c.take<uint8_t>(R);
  s->proofs = c.take<uint8_t>(R * ag::kPipeShreds * kPipeProofBytes);
  return c.used;
}

int read_pipe_meta(ag_rs_ctx* c, size_t n, DeshredScratch* v) {
  const int st = c->h_pipe_meta.ensure(25 * n);
  if (st) return st;
  AG_HIP(hipMemcpyAsync(c->h_pipe_meta.ptr, v->d_present, 25 * n, hipMemcpyDeviceToHost, c->stream));
  AG_HIP(hipStreamSynchronize(c->stream));
  v->h.present = c->h_pipe_meta.as<uint64_t>();
  v->h.slot = v->h.present + n;
  v->h.sidx = v->h.slot + n;
  v->h.last = c->h_pipe_meta.as<uint8_t>() + 24 * n;
  return AG_RS_OK;
}

bool pipe_args_ok(size_t nslices, size_t S, const uint8_t* codewords, const uint8_t* packets,
                  const uint32_t* packet_lens) {
  return S != 0 && S % 2 == 0 && S <= 1024 && nslices < (size_t{1} << 24) &&
         (nslices == 0 || (codewords && packets && packet_lens)) && reinterpret_cast<uintptr_t>(codewords) % 16 == 0;
}

// Output shred j of a slice <-> codeword row (data rows 0..31, coding rows 32..32+m-1):
// Regular / AONT: j; CodingOnly: 32 + j (the 64 coding shreds, no data shreds: shredder.rs:
// 367-376); PETS: j for j < 31, j + 1 after (the data shred holding the key withheld,
// :414-422).  The pipeline addresses the output rows in the caller's codeword buffer itself
// (grouped_row_offset: base row row0, slice stride cw_stride, row `skip` and later one shard
// further), so no row is copied between the coder's layout and the datagrams'.
struct ShredderKind {
  uint32_t m;         // coding shreds of the coder (ReedSolomonCoder::new(CODING_OUTPUT_SHREDS))
  uint32_t num_data;  // DATA_OUTPUT_SHREDS
  int aon;            // AG_AON_* or -1
  uint32_t row0;      // codeword row of output shred 0
  uint32_t skip;      // output shreds >= skip sit one row further (0: none)
  // the kernels' group stride: rows addressed per slice (the slice stride), or 0 for flat
  // addressing, row 64 s + j of the whole buffer (Regular: its slices are exactly 64 rows)
  size_t group_stride;
};
bool shredder_kind(int kind, size_t cw_stride, ShredderKind* k) {
  switch (kind) {
    case AG_SHREDDER_REGULAR: *k = {32, 32, -1, 0, 0, 0}; return true;
    case AG_SHREDDER_CODING_ONLY: *k = {64, 0, -1, kDataShreds, 0, cw_stride}; return true;
    case AG_SHREDDER_PETS: *k = {33, 31, AG_AON_PETS, 0, 31, cw_stride}; return true;
    case AG_SHREDDER_AONT: *k = {32, 32, AG_AON_AONT, 0, 0, cw_stride}; return true;
    default: return false;
  }
}
// One deshred's scratch, grown and carved at entry.  row: S, or 1024 with mixed sizes.
int deshred_scratch(ag_rs_ctx* c, const ShredderKind& k, size_t n, size_t row, DeshredScratch* v) {
  const size_t coder_words = k.m > kDataShreds ? 2 : 0;  // CodingOnly / PETS
  const int st = c->d_pipe.ensure(carve(nullptr, n, row, coder_words, v), c->stream);
  if (st) return st;
  carve(c->d_pipe.as<uint8_t>(), n, row, coder_words, v);
  return AG_RS_OK;
}
uint32_t kind_row(const ShredderKind& k, uint32_t j) { return k.row0 + j + (k.skip && j >= k.skip ? 1u : 0u); }
// the kept output shreds of one slice (present bit j) as ag_rs_coder_deshred_batch's flags of its
// data rows (dp[32]) and coding rows (cp[m]); rows that are no output shred keep their flag
void coder_flags(const ShredderKind& k, uint64_t present, uint8_t* dp, uint8_t* cp) {
  for (uint32_t j = 0; j < ag::kPipeShreds; ++j) {
    const uint32_t r = kind_row(k, j);
    const uint8_t bit = static_cast<uint8_t>((present >> j) & 1);
    if (r < kDataShreds) dp[r] = bit;
    else cp[r - kDataShreds] = bit;
  }
}
// the Merkle tree over the 64 output rows of each slice: roots, proofs (nodes in context scratch)
int kind_merkle(ag_rs_ctx* c, const ShredderKind& k, size_t n, size_t S, const uint8_t* codewords, size_t cw_stride,
                uint8_t* roots, uint8_t* proofs) {
  const size_t nodes_stride = (32 * ag_merkle_node_count(ag::kPipeShreds) + 255) / 256 * 256;
  int st;
  if ((st = c->d_merkle_nodes.ensure(n * nodes_stride, c->stream)) || (st = ensure_empty_roots(c))) return st;
  ag::MerkleBuildParams mb{};
  mb.leaves = codewords + k.row0 * S;
  mb.leaf_stride = S;
  mb.slice_stride = cw_stride;
  mb.skip_leaf = k.skip;
  mb.leaf_bytes = static_cast<uint32_t>(S);
  mb.n_leaves = ag::kPipeShreds;
  mb.nslices = n;
  mb.empty_roots = c->d_empty_roots.as<uint32_t>();
  mb.roots = roots;
  mb.proofs = proofs;
  mb.proofs_stride = ag::kPipeShreds * kPipeProofBytes;
  c->last_merkle_kernels = 0;
  return ag::launch_merkle_build(mb, c->d_merkle_nodes.as<uint8_t>(), nodes_stride, c->stream,
                                 &c->last_merkle_kernels) == hipSuccess
             ? AG_RS_OK
             : AG_RS_ERR_DEVICE;
}

// The shred side from the encoded codewords on: the slice Merkle trees (roots and every shred's
// path), slice_sig = sign(SliceCommitment(header, root)) on the side stream, forked behind the
// roots (one signature per lane: latency-bound), while the main stream serializes the 64
// datagrams per slice (header and signature shared by the slice's rows), then the signatures
// patched in.  The sign's table and scratch are made ready on the main stream, before the fork:
// the validation uses the same scratch there.  roots_out / sigs_out null: the scratch's (sc).
// d_sizes (device, nullable): one shred size per slice -- the var Merkle build, rows packed at
// the slice's own size (S is 0 then); null: shreds of S bytes in the rows of `k`.
// nblocks > 0: the block hashes over the roots, a chain of dependent levels a few workgroups
// wide, placed where the main stream would otherwise only wait for the signatures.
int shred_tail(ag_rs_ctx* c, const ShredderKind& k, const ShredScratch& sc, size_t n, size_t S,
               const uint32_t* d_sizes, uint8_t* codewords, size_t cw_stride, const uint64_t* slots, const uint64_t* slice_indices, const uint8_t* is_last,
               const uint8_t* seed, const uint8_t* pk, uint8_t* roots_out, uint8_t* sigs_out, uint8_t* packets,
               size_t packet_stride, uint32_t* packet_lens, size_t nblocks, const uint32_t* block_counts,
               uint8_t* block_hashes_out) {
  const size_t N = n * ag::kPipeShreds;
  int st;
  uint8_t *roots = roots_out ? roots_out : sc.roots, *sigs = sigs_out ? sigs_out : sc.sigs, *proofs = sc.proof;
  if (reinterpret_cast<uintptr_t>(roots) % 16) return AG_RS_ERR_INVALID_ARGUMENT;  // (the Merkle build's stores)
  if ((st = d_sizes ? merkle_var_launch(c, n, d_sizes, codewords, cw_stride, roots, nullptr, 0, proofs,
                                        ag::kPipeShreds * kPipeProofBytes)
                    : kind_merkle(c, k, n, S, codewords, cw_stride, roots, proofs)))
    return st;
  if ((st = slice_sign_prepare(c, n, seed, pk, slots, slice_indices, is_last, roots, sigs, nullptr))) return st;
  SideScope side(c);
  if ((st = side.open()) ||
      (st = slice_sign_enqueue(c, n, seed, pk, slots, slice_indices, is_last, roots, sigs, nullptr, side.stream())) ||
      (st = side.close()))
    return st;
  ag::PipeExpandParams ep{};
  ep.nslices = n;
  ep.shred_bytes = static_cast<uint32_t>(S);
  ep.num_data = k.num_data;
  ep.kind = sc.kind;
  ep.shred_index = sc.shred_index;
  ep.data_len = sc.data_len;
  ep.height = sc.height;
  ep.slice_bytes = d_sizes;
  AG_HIP(ag::launch_pipe_expand(ep, c->stream));
  ag::ShredColumns cols{};
  cols.kind = sc.kind;
  cols.slot = const_cast<uint64_t*>(slots);
  cols.slice_index = const_cast<uint64_t*>(slice_indices);
  cols.is_last = const_cast<uint8_t*>(is_last);
  cols.shred_index = ep.shred_index;
  cols.data = codewords + k.row0 * S;
  cols.data_stride = d_sizes ? AG_RS_MAX_DATA_PER_SHRED : S;
  cols.group_stride = k.group_stride;
  cols.skip_row = k.skip;
  cols.row_sizes = d_sizes;
  cols.data_len = ep.data_len;
  cols.sig = sigs;
  cols.proof = proofs;
  cols.proof_stride = kPipeProofBytes;
  cols.height = ep.height;
  cols.hdr_group = ag::kPipeShreds;
  cols.skip_sig = 1;
  AG_HIP(ag::launch_shred_serialize(cols, N, packets, packet_stride, packet_lens, c->stream));
  if (nblocks && (st = ag_block_tree_batch(c, nblocks, block_counts, roots, block_hashes_out, nullptr, 0, nullptr, 0)))
    return st;
  if ((st = side.join())) return st;
  AG_HIP(ag::launch_shred_sig_patch(cols, N, packets, packet_stride, packet_lens, c->stream));
  return AG_RS_OK;
}

// Steps 1-3 of a deshred in the row layout `k`:
// 1. network::deserialize (absent slots have length 0: malformed, never written);
// 2. ValidatedShred::try_new: one signature per slice (its first plausible shred), then every
//    shred against its slice's commitment (the blockstore's cached commitment; signature only
//    without a cache);
// 3. per slice: the shreds kept, the root, header and signature, read back to the host.
// Every plausible shred's root (derive_root) is computed on the side stream: it needs only the
// parse and the pick's plausibility flags, so it overlaps the picked shreds' signature checks
// (one signature per lane: a latency-bound kernel).  leaf_nodes (nullable; with its stride and
// leaves_per_tree): that verify also keeps each shred's leaf digest there, at (slice, index),
// for a Merkle rebuild's level 0.
// d_sizes (device, nullable; Regular only): one shred size per slice, rows packed at the slice's
// own size from k.group_stride (the slice stride; S is 0 then) -- every stage reads the slice's
// size where it reads S: the parse (row capacity), the slot check of pick / check, the leaf size
// of both verifies.  The picked rows are gathered at a fixed stride of 1024 bytes.
// v: the call's carved scratch (deshred_scratch, same row capacity); the codeword addressing of
// its columns and the host copy of pipe_check's outputs are filled in here.
int deshred_front(ag_rs_ctx* c, const ShredderKind& k, size_t n, size_t S, const uint32_t* d_sizes,
                  const uint8_t* packets, size_t packet_stride, const uint32_t* packet_lens, const uint8_t* pk,
                  uint8_t* codewords, uint8_t* leaf_nodes, size_t leaf_nodes_stride, uint32_t leaves_per_tree,
                  DeshredScratch* v) {
  const size_t N = n * ag::kPipeShreds;
  const size_t row = d_sizes ? size_t{AG_RS_MAX_DATA_PER_SHRED} : S;  // row capacity; stride of the picked rows
  int st;
  ag::ShredColumns& cols = v->cols;
  cols.data = codewords + k.row0 * S;
  cols.data_stride = row;
  cols.group_stride = k.group_stride;
  cols.skip_row = k.skip;
  cols.row_sizes = d_sizes;
  if (ag::launch_shred_deserialize(packets, packet_stride, packet_lens, N, cols, v->wire, c->stream) != hipSuccess)
    return AG_RS_ERR_DEVICE;
  ag::PipePickParams pp{};
  pp.nslices = n;
  pp.shred_bytes = static_cast<uint32_t>(S);
  pp.num_data = k.num_data;
  pp.wire_status = v->wire;
  pp.cols = cols;
  pp.pick = v->pick;
  pp.g_data = v->g_data;
  pp.g_proof = v->g_proof;
  pp.g_slot = v->g_slot;
  pp.g_slice_index = v->g_slice_index;
  pp.g_is_last = v->g_is_last;
  pp.g_shred_index = v->g_shred_index;
  pp.g_sig = v->g_sig;
  pp.plausible = v->plausible;  // per shred: the datagram parsed and fits its slot
  pp.slice_bytes = d_sizes;
  AG_HIP(hipMemsetAsync(v->g_data, 0, n * row, c->stream));  // slices without a pick: defined bytes
  AG_HIP(hipMemsetAsync(v->g_shred_index, 0, 4 * n, c->stream));
  if (ag::launch_pipe_pick(pp, c->stream) != hipSuccess) return AG_RS_ERR_DEVICE;
  ag::MerkleVerifyParams mp{};
  mp.leaves = cols.data;
  mp.leaf_stride = S;
  mp.leaf_bytes = static_cast<uint32_t>(S);
  mp.height = ag::kPipeHeight;
  mp.index = cols.shred_index;
  mp.proofs = cols.proof;
  mp.proofs_stride = kPipeProofBytes;
  mp.n = N;
  mp.roots_out = v->roots;
  mp.active = v->plausible;
  mp.list = v->merkle_list;
  mp.leaf_nodes = leaf_nodes;
  mp.leaf_nodes_stride = leaf_nodes_stride;
  mp.leaves_per_tree = leaves_per_tree;
  mp.group_stride = k.group_stride;
  mp.skip_row = k.skip;
  mp.leaf_sizes = d_sizes;  // (the full pass: one size per 64 rows, the leaf address follows the packed rows)
  mp.size_group = d_sizes ? ag::kPipeShreds : 0;
  SideScope side(c);
  if ((st = side.open())) return st;
  AG_HIP(ag::launch_merkle_verify(mp, side.stream()));
  if ((st = side.close())) return st;
  ag::MerkleVerifyParams gp{};  // the picked rows: one per slice, at a slice's own size when the sizes are mixed
  gp.leaves = v->g_data;
  gp.leaf_stride = row;
  gp.leaf_bytes = static_cast<uint32_t>(row);
  gp.height = ag::kPipeHeight;
  gp.index = v->g_shred_index;
  gp.proofs = v->g_proof;
  gp.proofs_stride = kPipeProofBytes;
  gp.n = n;
  gp.leaf_sizes = d_sizes;
  gp.size_group = d_sizes ? 1 : 0;
  if ((st = shred_validate_impl(c, gp, v->g_slot, v->g_slice_index, v->g_is_last, v->g_sig, 64, pk, nullptr, nullptr, 1,
                                v->pick_status, nullptr, v->commits, false)))
    return st;
  AG_HIP(ag::launch_pipe_cache_flags(v->pick, v->pick_status, n, v->has_cached, c->stream));
  if ((st = side.join())) return st;
  // the side stream derived every plausible shred's root from `mp`: roots_ready
  if ((st = shred_validate_impl(c, mp, cols.slot, cols.slice_index, cols.is_last, cols.sig, 64, pk, v->commits,
                                v->has_cached, ag::kPipeShreds, v->val_status, v->roots, nullptr,
                                /*roots_ready=*/true)))
    return st;
  ag::PipeCheckParams kp{};
  kp.nslices = n;
  kp.shred_bytes = static_cast<uint32_t>(S);
  kp.num_data = k.num_data;
  kp.wire_status = v->wire;
  kp.val_status = v->val_status;
  kp.roots = v->roots;
  kp.cols = cols;
  kp.present = v->d_present;
  kp.root = v->sroot;
  kp.slot = v->d_slot;
  kp.slice_index = v->d_slice_index;
  kp.is_last = v->d_is_last;
  kp.sig = v->ssig;
  kp.slice_bytes = d_sizes;
  if (ag::launch_pipe_check(kp, c->stream) != hipSuccess) return AG_RS_ERR_DEVICE;
  return read_pipe_meta(c, n, v);
}

// Shredder::deshred's result per slice from the coder's (plen: payload length or -error), the
// Merkle check's (h_same) and SlicePayload::try_from's (sstat): status, ok, and the slice's
// header for the slices that succeeded (zero for the others).
// key_bytes (PETS / AONT: the key tail, else 0): decrypt_payload runs inside
// deshred_validated_shreds, before check_merkle_tree (shredder.rs:293, :303), so a decoded buffer
// shorter than the key is BadEncoding whatever the root comparison says.  A slice whose tree
// differs was never decrypted (pass 0's and the EXACT re-run's alike), so its plen is still the
// coder's buffer length: this is the one place both kinds of entries go through.
void pipe_statuses(size_t n, const int64_t* plen, const uint8_t* h_same, const uint8_t* sstat, const PipeMeta& h,
                   size_t key_bytes, int32_t* status, uint8_t* ok, uint64_t* slots_out, uint64_t* slice_indices_out,
                   uint8_t* is_last_out) {
  for (size_t s = 0; s < n; ++s) {
    int32_t r = AG_RS_OK;
    if (plen[s] < 0) {
      r = -plen[s] == AG_RS_ERR_INVALID_PADDING ? AG_RS_ERR_BAD_ENCODING : static_cast<int32_t>(-plen[s]);
    } else if (!h_same[s]) {
      r = plen[s] < static_cast<int64_t>(key_bytes) ? AG_RS_ERR_BAD_ENCODING : AG_RS_ERR_INVALID_MERKLE_TREE;
    } else if (sstat[s] == AG_SLICE_TOO_LARGE) {
      r = AG_RS_ERR_TOO_MUCH_DATA;
    } else if (sstat[s] != AG_SLICE_OK) {
      r = AG_RS_ERR_BAD_ENCODING;
    }
    status[s] = r;
    ok[s] = r == AG_RS_OK;
    slots_out[s] = ok[s] ? h.slot[s] : 0;
    slice_indices_out[s] = ok[s] ? h.sidx[s] : 0;
    is_last_out[s] = ok[s] ? h.last[s] : 0;
  }
}

// fill_missing_shreds: the datagrams of the absent slots of the slices with ok[s], serialized
// into their packets; their lengths go to v.fresh_lens (pipe_merge_lens moves the final slices'
// lengths into packet_lens), the uploaded flags to v.slice_ok.  Enqueued only: `ok` is host memory
// the upload reads, so the caller synchronizes before it changes.  Slices of mixed sizes
// (v.cols.row_sizes, deshred_front's d_sizes): each datagram at its slice's own size.
int fill_missing(ag_rs_ctx* c, const ShredderKind& k, size_t n, size_t S, const DeshredScratch& v, const uint8_t* ok,
                 uint8_t* packets, size_t packet_stride) {
  const size_t N = n * ag::kPipeShreds;
  AG_HIP(hipMemcpyAsync(v.slice_ok, ok, n, hipMemcpyHostToDevice, c->stream));
  ag::PipeExpandParams ep{};
  ep.nslices = n;
  ep.shred_bytes = static_cast<uint32_t>(S);
  ep.num_data = k.num_data;
  ep.skip = v.d_present;
  ep.slice_ok = v.slice_ok;
  ep.kind = v.cols.kind;
  ep.shred_index = v.cols.shred_index;
  ep.data_len = v.cols.data_len;
  ep.height = v.cols.height;
  ep.slice_bytes = v.cols.row_sizes;
  if (ag::launch_pipe_expand(ep, c->stream) != hipSuccess) return AG_RS_ERR_DEVICE;
  ag::ShredColumns fc = v.cols;
  fc.slot = v.d_slot;
  fc.slice_index = v.d_slice_index;
  fc.is_last = v.d_is_last;
  fc.sig = v.ssig;
  fc.hdr_group = ag::kPipeShreds;
  if (ag::launch_shred_serialize(fc, N, packets, packet_stride, v.fresh_lens, c->stream) != hipSuccess)
    return AG_RS_ERR_DEVICE;
  return AG_RS_OK;
}

// What rerun_exact hands back for the listed slices, entry r for slice list[r]: the coder's
// result, the root comparison and SlicePayload::try_from's outputs.
struct RerunResult {
  std::vector<int64_t> plen;
  std::vector<uint8_t> same, sstat, parent_flag, parent_id;
  std::vector<uint32_t> data_offset, data_len;
};

// Step 6b of the composed deshreds: the listed slices (ascending; each failed the padding or the
// Merkle check of the ANY_K pass with more than 32 kept shreds) decoded again with the crate's
// decoder over every kept shred, all of them in one pass over a compact batch.
//   gather   the kept shreds' payloads out of their datagram slots (the pass before rewrote the
//            restored and re-encoded rows, and PETS / AONT decrypted in place), every other row
//            as the codeword holds it, the kept-shred words and the signed roots;
//   coder    Regular: the mixed-size device stages with EXACT masks (pipe_coder_deshred_var),
//            whatever the sizes -- a uniform call is the mix of one size, tails under 16 bytes
//            included; the other shredders: ag_rs_coder_deshred_batch(EXACT), batched on its
//            host-pattern route;
//   checks   the Merkle rebuild over the raw output shreds (every leaf hashed), the root
//            comparison, SlicePayload::try_from;
//   scatter  the codeword rows (nothing past them), proof rows and rebuilt roots back to the
//            slices' places.  The caller copies *out into the slices' entries.
// S: the uniform shred size, or sizes (HOST, per slice of the whole batch; Regular only).
// passed (nullable): set when some listed slice decoded and matches its signed root -- nothing is
// scattered then, the caller redoes its batch.  (It does not happen: kept shreds that no decode
// of 32 of them reproduces are no codeword, and no codeword's tree has their signed root.)
int rerun_exact(ag_rs_ctx* c, const ShredderKind& k, const std::vector<uint32_t>& list, size_t S,
                const uint32_t* sizes, const uint8_t* packets, size_t packet_stride, const DeshredScratch& v,
                uint8_t* codewords, size_t cw_stride, RerunResult* out, bool* passed) {
  const size_t R = list.size(), rows = kDataShreds + k.m;
  const bool regular = k.aon < 0 && k.m == kDataShreds;
  int st;
  // list | sizes | column prefix through pinned staging, rewritten once its last upload completed
  const size_t words = 3 * R + 1;
  uint32_t* h;
  if ((st = c->rerun.host(4 * words, &h))) return st;
  size_t max_s = 0;
  uint32_t cols = 0;
  for (size_t r = 0; r < R; ++r) {
    const uint32_t Ss = sizes ? sizes[list[r]] : static_cast<uint32_t>(S);
    h[r] = list[r];
    h[R + r] = Ss;
    h[2 * R + r] = cols;
    cols += (Ss + 63) / 64;
    max_s = std::max<size_t>(max_s, Ss);
  }
  h[3 * R] = cols;
  const size_t cstride = (rows * max_s + 15) / 16 * 16;
  // a buffer of its own: growing it here leaves d_pipe (`v`, read by the queued kernels) in place
  RerunScratch rs;
  if ((st = c->d_pipe_rerun.ensure(carve(nullptr, R, cstride, &rs), c->stream))) return st;
  carve(c->d_pipe_rerun.as<uint8_t>(), R, cstride, &rs);
  if ((st = c->rerun.send(4 * words, c->stream, rs.list))) return st;
  uint8_t *const ccw = rs.codewords, *const c_roots = rs.roots, *const c_proofs = rs.proofs;
  const uint32_t* d_sizes = rs.sizes;
  ag::PipeRerunParams rp{};
  rp.list = rs.list;
  rp.sizes = d_sizes;
  rp.nlist = static_cast<uint32_t>(R);
  rp.rows = static_cast<uint32_t>(rows);
  rp.row0 = k.row0;
  rp.skip = k.skip;
  rp.codewords = codewords;
  rp.cw_stride = cw_stride;
  rp.compact = ccw;
  rp.compact_stride = cstride;
  rp.packets = packets;
  rp.packet_stride = packet_stride;
  rp.present = v.d_present;
  rp.sroot = v.sroot;
  rp.c_sroot = rs.sroot;
  rp.c_roots = c_roots;
  rp.c_present = rs.present;
  rp.roots = v.roots2;
  rp.c_proofs = c_proofs;
  rp.proofs = v.cols.proof;
  rp.proof_stride = kPipeProofBytes;
  if (ag::launch_pipe_rerun_gather(rp, c->stream) != hipSuccess) return AG_RS_ERR_DEVICE;
  out->plen.assign(R, 0);
  if (regular) {
    c->last_encode_kernels = 0;
    c->last_window_kernels = 0;
    if ((st = pipe_coder_deshred_var(c, R, ccw, cstride, rp.c_present, d_sizes, rs.col_base, cols, true,
                                     out->plen.data(), true)) ||
        (st = merkle_var_launch(c, R, d_sizes, ccw, cstride, c_roots, nullptr, 0, c_proofs,
                                ag::kPipeShreds * kPipeProofBytes)))
      return st;
  } else {
    std::vector<uint8_t> dp(R * kDataShreds, 0), cp(R * k.m, 0);
    for (size_t r = 0; r < R; ++r) coder_flags(k, v.h.present[list[r]], &dp[r * kDataShreds], &cp[r * k.m]);
    if ((st = ag_rs_coder_deshred_batch(c, k.m, R, S, ccw, cstride, dp.data(), cp.data(), AG_RS_DECODE_EXACT,
                                        out->plen.data())) ||
        (st = kind_merkle(c, k, R, S, ccw, cstride, c_roots, c_proofs)))
      return st;
  }
  c->last_rerun_slices = R;
  c->last_rerun_passes = 1;
  if (ag::launch_pipe_root_cmp(c_roots, rp.c_sroot, R, rs.same, c->stream) != hipSuccess) return AG_RS_ERR_DEVICE;
  out->same.assign(R, 0);
  AG_HIP(hipMemcpyAsync(out->same.data(), rs.same, R, hipMemcpyDeviceToHost, c->stream));
  out->sstat.assign(R, 0);
  out->parent_flag.assign(R, 0);
  out->parent_id.assign(R * AG_SLICE_BLOCK_ID_BYTES, 0);
  out->data_offset.assign(R, 0);
  out->data_len.assign(R, 0);
  if ((st = ag_slice_parse_batch(c, R, ccw, cstride, out->plen.data(), out->sstat.data(), out->parent_flag.data(),
                                 out->parent_id.data(), out->data_offset.data(), out->data_len.data())))
    return st;  // synchronous: the comparison has landed
  for (size_t r = 0; r < R; ++r) {
    if (out->plen[r] < 0) out->same[r] = 0;
    if (passed && out->same[r]) *passed = true;
  }
  if (passed && *passed) return AG_RS_OK;
  return ag::launch_pipe_rerun_scatter(rp, c->stream) == hipSuccess ? AG_RS_OK : AG_RS_ERR_DEVICE;
}

// RegularShredder's deshred, the body of ag_shredder_deshred_batch (sizes null: every shred S
// bytes, cw_stride = 64 S) and of ag_shredder_deshred_batch_var (sizes: HOST, one checked shred
// size per slice, S = 0; slice s's rows packed at sizes[s] from codewords + s * cw_stride).  The
// sizes go up once (upload_var_sizes) and every kernel reads them from the device; the stages
// and their order are the same, so the number of launches does not depend on the mix.
int regular_deshred(ag_rs_ctx* c, size_t n, size_t S, const uint32_t* sizes, uint8_t* packets, size_t packet_stride,
                    uint32_t* packet_lens, const uint8_t* pk, uint8_t* codewords, size_t cw_stride, int32_t* status,
                    uint64_t* slots_out, uint64_t* slice_indices_out, uint8_t* is_last_out,
                    uint8_t* parent_flags_out, uint8_t* parent_ids_out, uint32_t* data_offsets_out,
                    uint32_t* data_lens_out) {
  int st;
  ShredderKind k;
  shredder_kind(AG_SHREDDER_REGULAR, cw_stride, &k);
  c->last_rerun_slices = c->last_rerun_passes = 0;
  DeshredScratch v;
  if ((st = deshred_scratch(c, k, n, sizes ? size_t{AG_RS_MAX_DATA_PER_SHRED} : S, &v))) return st;
  const uint32_t *d_sizes = nullptr, *d_col_base = nullptr;
  uint32_t total_columns = 0;
  if (sizes) {
    if ((st = upload_var_sizes(c, n, sizes, &d_sizes, &d_col_base, &total_columns))) return st;
    k.group_stride = cw_stride;  // rows packed at each slice's own size: addressed per slice
  }
  // 1-3. the kept shreds of every slice (payload rows straight into the codewords: row 64 s + j
  //      is shard j of slice s), with every plausible shred's leaf digest kept for the Merkle
  //      rebuild's level 0: step 5 hashes only the rows the coder restores or may rewrite
  const size_t nodes_stride = (32 * ag_merkle_node_count(ag::kPipeShreds) + 255) / 256 * 256;
  if ((st = c->d_merkle_nodes.ensure(n * nodes_stride, c->stream))) return st;
  uint8_t* nodes = c->d_merkle_nodes.as<uint8_t>();
  if ((st = deshred_front(c, k, n, S, d_sizes, packets, packet_stride, packet_lens, pk, codewords, nodes, nodes_stride,
                          ag::kPipeShreds, &v)))
    return st;
  const uint64_t* h_present = v.h.present;
  // 4. ReedSolomonCoder::deshred over the kept shreds (restores the data shreds, re-encodes
  //    all coding shreds, strips the padding); on the device for whole-chunk shreds
  std::vector<int64_t> plen(n);
  bool no_reencode = true;  // no surplus shreds and no slice with every data shred
  for (size_t s = 0; s < n && no_reencode; ++s)
    no_reencode = __builtin_popcountll(h_present[s]) <= static_cast<int>(ag::kPipeData) &&
                  (h_present[s] & 0xFFFFFFFFull) != 0xFFFFFFFFull;
  const bool device_coder = sizes || pipe_tail_ok(S, kDataShreds, no_reencode);
  if (sizes) {
    // the var coder's device stages (every even size; exactly-32 slices get their absent coding
    // shreds from the decode, surplus slices the re-encode under their store masks)
    c->last_encode_kernels = 0;
    c->last_window_kernels = 0;
    if ((st = pipe_coder_deshred_var(c, n, codewords, cw_stride, v.d_present, d_sizes, d_col_base, total_columns,
                                     !no_reencode, plen.data())))
      return st;
  } else if (device_coder) {
    if ((st = pipe_coder_deshred(c, n, S, codewords, cw_stride, v.d_present, plen.data(), kDataShreds, no_reencode)))
      return st;
  } else {
    std::vector<uint8_t> dp(n * ag::kPipeData), cp(n * k.m);
    for (size_t s = 0; s < n; ++s) coder_flags(k, h_present[s], &dp[s * ag::kPipeData], &cp[s * k.m]);
    if ((st = ag_rs_coder_deshred_batch(c, k.m, n, S, codewords, cw_stride, dp.data(), cp.data(), AG_RS_DECODE_ANY_K,
                                        plen.data())))
      return st;
  }
  // 5. check_merkle_tree: the rebuilt tree's root must be the signed one; its paths serve
  //    the reconstructed datagrams.  Kept shreds the coder left as received reuse the digests
  //    their proof check computed (same bytes); restored rows, and coding rows the re-encode
  //    may have rewritten, are hashed again.
  //    Mixed sizes: the same, verbatim -- the var verify wrote the kept rows' digests from the
  //    same packed bytes the var leaf kernel would read, the var coder stage obeys the same store
  //    masks, and only the flagged leaves are hashed again.
  //    Invariant the reuse depends on: present ⊆ active ∧ proof-ok.  Every kept
  //    shred (a bit of d_present, set by pipe_check only for shreds that were active in the
  //    step-3 verify and whose derived root matched) had its leaf digest written to
  //    d_merkle_nodes at (slice, index) by that verify; nothing between step 3 and here writes
  //    those rows of the codeword or those nodes (the coder stage touches only absent rows
  //    and, per the store masks, coding rows the leaf flags mark for re-hashing).  The verify
  //    also stores digests of rows it then rejects: those rows are not in d_present, so the
  //    flags below re-hash or ignore them.  A new step in between that writes kept rows or
  //    d_merkle_nodes must clear the matching present bits or re-hash.
  {
    if ((st = ensure_empty_roots(c))) return st;
    // the host coder path (shreds not whole 64-byte chunks) re-encodes every coding shred; the
    // var coder never does: its decode restores the absent coding shreds of exactly-32 slices,
    // and the kernel flags the surplus slices' coding rows itself
    if (ag::launch_pipe_leaf_flags(v.d_present, n, !device_coder, v.leaf_flags, c->stream) != hipSuccess)
      return AG_RS_ERR_DEVICE;
    ag::MerkleBuildParams mb{};
    mb.leaves = codewords;
    mb.leaf_stride = S;
    mb.slice_stride = cw_stride;
    mb.leaf_bytes = static_cast<uint32_t>(S);
    mb.n_leaves = ag::kPipeShreds;
    mb.nslices = n;
    mb.empty_roots = c->d_empty_roots.as<uint32_t>();
    mb.roots = v.roots2;
    mb.proofs = v.cols.proof;
    mb.proofs_stride = ag::kPipeShreds * kPipeProofBytes;
    mb.hash_leaf = v.leaf_flags;
    mb.list = v.merkle_list;  // (its second user: see DeshredScratch)
    mb.leaf_sizes = d_sizes;  // (leaf_stride / leaf_bytes unused then: rows at the slice's own size)
    c->last_merkle_kernels = 0;
    if (ag::launch_merkle_build(mb, nodes, nodes_stride, c->stream, &c->last_merkle_kernels) != hipSuccess)
      return AG_RS_ERR_DEVICE;
  }
  if (ag::launch_pipe_root_cmp(v.roots2, v.sroot, n, v.same, c->stream) != hipSuccess) return AG_RS_ERR_DEVICE;
  std::vector<uint8_t> h_same(n);
  AG_HIP(hipMemcpyAsync(h_same.data(), v.same, n, hipMemcpyDeviceToHost, c->stream));
  // 6. SlicePayload::try_from
  std::vector<uint8_t> sstat(n);
  if ((st = ag_slice_parse_batch(c, n, codewords, cw_stride, plen.data(), sstat.data(), parent_flags_out,
                                 parent_ids_out, data_offsets_out, data_lens_out)))
    return st;  // synchronous: h_same has landed
  // 6b. The crate's decoder reads every kept shred (reed_solomon.rs:154-166); the pass above
  //     reads 32 of them (ANY_K).  On a consistent slice both restore the same bytes (MDS), and
  //     a slice that passed check_merkle_tree is consistent: the rebuilt codeword matches the
  //     signed root that commits every kept shred.  A slice that failed the padding or the
  //     Merkle check with more than 32 kept shreds may hold an inconsistent shred the ANY_K
  //     pass did not read (a leader signing a non-codeword), and the crate's bytes -- hence
  //     the error, BadEncoding vs InvalidMerkleTree -- can differ.  Such slices are decoded
  //     again from their received bytes with EXACT and re-checked, all of them in one batched
  //     pass (rerun_exact; honest leaders never produce them: nothing is launched then).
  std::vector<uint32_t> rerun;
  for (size_t s = 0; s < n; ++s) {
    const bool failed = plen[s] == -AG_RS_ERR_INVALID_PADDING || (plen[s] >= 0 && !h_same[s]);
    if (failed && __builtin_popcountll(h_present[s]) > static_cast<int>(ag::kPipeData))
      rerun.push_back(static_cast<uint32_t>(s));
  }
  if (!rerun.empty()) {
    RerunResult rr;
    if ((st = rerun_exact(c, k, rerun, S, sizes, packets, packet_stride, v, codewords, cw_stride, &rr, nullptr)))
      return st;
    for (size_t r = 0; r < rerun.size(); ++r) {
      const size_t s = rerun[r];
      plen[s] = rr.plen[r];
      h_same[s] = rr.same[r];
      sstat[s] = rr.sstat[r];
      parent_flags_out[s] = rr.parent_flag[r];
      std::copy_n(&rr.parent_id[AG_SLICE_BLOCK_ID_BYTES * r], AG_SLICE_BLOCK_ID_BYTES,
                  parent_ids_out + AG_SLICE_BLOCK_ID_BYTES * s);
      data_offsets_out[s] = rr.data_offset[r];
      data_lens_out[s] = rr.data_len[r];
    }
  }
  std::vector<uint8_t> ok(n);
  pipe_statuses(n, plen.data(), h_same.data(), sstat.data(), v.h, 0, status, ok.data(), slots_out, slice_indices_out,
                is_last_out);
  // 7. fill_missing_shreds: datagrams for the absent slots of the slices that succeeded
  if ((st = fill_missing(c, k, n, S, v, ok.data(), packets, packet_stride))) return st;
  if (ag::launch_pipe_merge_lens(v.fresh_lens, v.d_present, v.slice_ok, n, packet_lens, c->stream) != hipSuccess)
    return AG_RS_ERR_DEVICE;
  AG_HIP(hipStreamSynchronize(c->stream));  // host vectors read by async copies
  return AG_RS_OK;
}

}  // namespace

extern "C" {

int ag_shredder_shred_batch(ag_rs_ctx* c, size_t nslices, size_t S, const uint8_t* parent_flags,
                            const uint8_t* parent_ids, const uint8_t* data, size_t data_stride,
                            const uint32_t* data_lens, const uint64_t* slots, const uint64_t* slice_indices,
                            const uint8_t* is_last, const uint8_t* seed, const uint8_t* pk, uint8_t* codewords,
                            uint8_t* roots_out, uint8_t* sigs_out, uint8_t* packets, size_t packet_stride,
                            uint32_t* packet_lens) {
  if (!c || !pipe_args_ok(nslices, S, codewords, packets, packet_lens) ||
      (nslices && (!parent_flags || !parent_ids || !data_lens || !slots || !slice_indices || !is_last || !seed ||
                   !pk)))
    return AG_RS_ERR_INVALID_ARGUMENT;
  if (nslices == 0) return AG_RS_OK;
  if (c->enter()) return AG_RS_ERR_DEVICE;
  const size_t n = nslices, cw_stride = ag::kPipeShreds * S;
  ShredderKind k;
  shredder_kind(AG_SHREDDER_REGULAR, cw_stride, &k);
  ShredScratch sc;
  int st = shred_scratch(c, n, &sc);
  if (st) return st;
  // 1. Slice::payload_bytes into the data regions, 2. ReedSolomonCoder::shred in place
  std::vector<uint32_t> lens(n);
  if ((st = ag_slice_frame_batch(c, n, S, parent_flags, parent_ids, data, data_stride, data_lens, codewords, cw_stride,
                                 lens.data())))
    return st;
  if ((st = ag_rs_coder_shred_batch(c, k.m, n, S, nullptr, 0, lens.data(), codewords, cw_stride))) return st;
  // 3. slice Merkle trees, 4. slice signatures, 5. the 64 datagrams per slice
  return shred_tail(c, k, sc, n, S, nullptr, codewords, cw_stride, slots, slice_indices, is_last, seed, pk, roots_out,
                    sigs_out, packets, packet_stride, packet_lens, 0, nullptr, nullptr);
}

// RegularShredder::shred over slices of mixed shred sizes: the stages of ag_shredder_shred_batch,
// each taking one size per slice -- the var coder (one launch set for the whole mix), the var
// Merkle build over the size table the coder uploaded (lens.dev: lens | sizes | column prefix; it
// stays valid on the stream until the next coder call), the serializer with a row size per slice.
int ag_shredder_shred_batch_var(ag_rs_ctx* c, size_t nslices, const uint8_t* parent_flags, const uint8_t* parent_ids,
                                const uint8_t* data, size_t data_stride, const uint32_t* data_lens,
                                const uint64_t* slots, const uint64_t* slice_indices, const uint8_t* is_last,
                                const uint8_t* seed, const uint8_t* pk, uint8_t* codewords, size_t codeword_stride,
                                uint32_t* shred_bytes_out, uint8_t* roots_out, uint8_t* sigs_out, uint8_t* packets,
                                size_t packet_stride, uint32_t* packet_lens, size_t nblocks,
                                const uint32_t* block_counts, uint8_t* block_hashes_out) {
  if (!c || nslices >= (size_t{1} << 24)) return AG_RS_ERR_INVALID_ARGUMENT;
  if (nslices == 0) return nblocks ? AG_RS_ERR_INVALID_ARGUMENT : AG_RS_OK;
  if (!parent_flags || !parent_ids || !data_lens || !slots || !slice_indices || !is_last || !seed || !pk ||
      !codewords || !packets || !packet_lens || reinterpret_cast<uintptr_t>(codewords) % 16 || codeword_stride % 16)
    return AG_RS_ERR_INVALID_ARGUMENT;
  const size_t n = nslices;
  // every check on the host, before the first launch: the framing's, the strides', the blocks'
  std::vector<uint32_t> lens(n);
  size_t max_s = 0, max_len = 0;
  for (size_t b = 0; b < n; ++b) {
    if (parent_flags[b] > 1) return AG_RS_ERR_INVALID_ARGUMENT;
    const size_t framed = 1 + (parent_flags[b] ? AG_SLICE_BLOCK_ID_BYTES : 0) + 8 + size_t{data_lens[b]};
    if (framed > AG_SLICE_MAX_DATA) return AG_RS_ERR_TOO_MUCH_DATA;
    size_t S = 0;
    if (ag_rs_coder_shred_bytes(framed, &S)) return AG_RS_ERR_TOO_MUCH_DATA;
    max_s = std::max(max_s, S);
    max_len = std::max<size_t>(max_len, data_lens[b]);
  }
  size_t need = 0;
  if (ag_shred_datagram_bytes(max_s, ag::kPipeHeight, &need) || packet_stride < need ||
      codeword_stride < ag::kPipeShreds * max_s || (max_len && (!data || (n > 1 && data_stride < max_len))))
    return AG_RS_ERR_INVALID_ARGUMENT;
  if (nblocks) {
    if (!block_counts || !block_hashes_out || reinterpret_cast<uintptr_t>(block_hashes_out) % 16 || nblocks > n)
      return AG_RS_ERR_INVALID_ARGUMENT;
    size_t sum = 0;
    for (size_t b = 0; b < nblocks; ++b) {
      if (block_counts[b] == 0 || block_counts[b] > AG_BLOCK_MAX_SLICES) return AG_RS_ERR_INVALID_ARGUMENT;
      sum += block_counts[b];
    }
    if (sum != n) return AG_RS_ERR_INVALID_ARGUMENT;
  }
  if (c->enter()) return AG_RS_ERR_DEVICE;
  ShredderKind k;
  shredder_kind(AG_SHREDDER_REGULAR, codeword_stride, &k);
  k.group_stride = codeword_stride;  // rows packed at each slice's own size: addressed per slice
  ShredScratch sc;
  int st = shred_scratch(c, n, &sc);
  if (st) return st;
  // 1. Slice::payload_bytes into the data regions (a framed payload is shorter than 32 * S_s, so
  //    it stays inside its own slice's data shreds), 2. ReedSolomonCoder::shred in place
  if ((st = ag_slice_frame_batch(c, n, max_s, parent_flags, parent_ids, data, data_stride, data_lens, codewords,
                                 codeword_stride, lens.data())))
    return st;
  if ((st = ag_rs_coder_shred_batch_var(c, k.m, n, nullptr, 0, lens.data(), codewords, codeword_stride,
                                        shred_bytes_out)))
    return st;
  if (!(c->last_encode_kernels & ag::kEkVar)) return AG_RS_ERR_DEVICE;  // (16-byte-aligned codewords: always var)
  const uint32_t* d_sizes = c->lens.dev.as<uint32_t>() + n;
  // 3. slice Merkle trees, 4. slice signatures, 5. the 64 datagrams per slice (rows and data
  //    lengths at the slice's own size), 6. the block hashes over the roots
  return shred_tail(c, k, sc, n, 0, d_sizes, codewords, codeword_stride, slots, slice_indices, is_last, seed, pk,
                    roots_out, sigs_out, packets, packet_stride, packet_lens, nblocks, block_counts,
                    block_hashes_out);
}

int ag_shredder_deshred_batch(ag_rs_ctx* c, size_t nslices, size_t S, uint8_t* packets, size_t packet_stride,
                              uint32_t* packet_lens, const uint8_t* pk, uint8_t* codewords, int32_t* status,
                              uint64_t* slots_out, uint64_t* slice_indices_out, uint8_t* is_last_out,
                              uint8_t* parent_flags_out, uint8_t* parent_ids_out, uint32_t* data_offsets_out,
                              uint32_t* data_lens_out) {
  if (!c || !pipe_args_ok(nslices, S, codewords, packets, packet_lens) ||
      (nslices && (!pk || !status || !slots_out || !slice_indices_out || !is_last_out || !parent_flags_out ||
                   !parent_ids_out || !data_offsets_out || !data_lens_out)))
    return AG_RS_ERR_INVALID_ARGUMENT;
  if (nslices == 0) return AG_RS_OK;
  if (c->enter()) return AG_RS_ERR_DEVICE;
  return regular_deshred(c, nslices, S, nullptr, packets, packet_stride, packet_lens, pk, codewords,
                         ag::kPipeShreds * S, status, slots_out, slice_indices_out, is_last_out, parent_flags_out,
                         parent_ids_out, data_offsets_out, data_lens_out);
}

// Shredder::deshred over slices of mixed shred sizes (the layout of ag_shredder_shred_batch_var):
// every check on the host before the first launch, then regular_deshred with the size table.
int ag_shredder_deshred_batch_var(ag_rs_ctx* c, size_t nslices, const uint32_t* shred_bytes, uint8_t* packets,
                                  size_t packet_stride, uint32_t* packet_lens, const uint8_t* pk, uint8_t* codewords,
                                  size_t codeword_stride, int32_t* status, uint64_t* slots_out,
                                  uint64_t* slice_indices_out, uint8_t* is_last_out, uint8_t* parent_flags_out,
                                  uint8_t* parent_ids_out, uint32_t* data_offsets_out, uint32_t* data_lens_out) {
  if (!c || nslices >= (size_t{1} << 24)) return AG_RS_ERR_INVALID_ARGUMENT;
  if (nslices == 0) return AG_RS_OK;
  if (!shred_bytes || !packets || !packet_lens || !pk || !codewords || !status || !slots_out || !slice_indices_out ||
      !is_last_out || !parent_flags_out || !parent_ids_out || !data_offsets_out || !data_lens_out ||
      reinterpret_cast<uintptr_t>(codewords) % 16 || codeword_stride % 16)
    return AG_RS_ERR_INVALID_ARGUMENT;
  size_t max_s = 0, need = 0;
  for (size_t s = 0; s < nslices; ++s) {
    if (shred_bytes[s] == 0 || shred_bytes[s] % 2 || shred_bytes[s] > AG_RS_MAX_DATA_PER_SHRED)
      return AG_RS_ERR_INVALID_ARGUMENT;
    max_s = std::max<size_t>(max_s, shred_bytes[s]);
  }
  // the kernels' bounds: no row past its slice's stride, no datagram past its slot
  if (codeword_stride < ag::kPipeShreds * max_s || ag_shred_datagram_bytes(max_s, ag::kPipeHeight, &need) ||
      packet_stride < need)
    return AG_RS_ERR_INVALID_ARGUMENT;
  if (c->enter()) return AG_RS_ERR_DEVICE;
  return regular_deshred(c, nslices, 0, shred_bytes, packets, packet_stride, packet_lens, pk, codewords,
                         codeword_stride, status, slots_out, slice_indices_out, is_last_out, parent_flags_out,
                         parent_ids_out, data_offsets_out, data_lens_out);
}

// ---- the other three shredders of shredder.rs composed (CodingOnly, PETS, AONT) -------------

int ag_shredder_shred_batch_kind(ag_rs_ctx* c, int kind, size_t nslices, size_t S, const uint8_t* parent_flags,
                                 const uint8_t* parent_ids, const uint8_t* data, size_t data_stride,
                                 const uint32_t* data_lens, const uint64_t* slots, const uint64_t* slice_indices,
                                 const uint8_t* is_last, const uint8_t* seed, const uint8_t* pk, const uint8_t* keys,
                                 uint8_t* codewords, size_t cw_stride, uint8_t* roots_out, uint8_t* sigs_out,
                                 uint8_t* packets, size_t packet_stride, uint32_t* packet_lens) {
  if (kind == AG_SHREDDER_REGULAR) {
    if (cw_stride != ag::kPipeShreds * S) return AG_RS_ERR_INVALID_ARGUMENT;
    return ag_shredder_shred_batch(c, nslices, S, parent_flags, parent_ids, data, data_stride, data_lens, slots,
                                   slice_indices, is_last, seed, pk, codewords, roots_out, sigs_out, packets,
                                   packet_stride, packet_lens);
  }
  ShredderKind k;
  if (!c || !shredder_kind(kind, cw_stride, &k) || !pipe_args_ok(nslices, S, codewords, packets, packet_lens) ||
      cw_stride < (kDataShreds + k.m) * S || cw_stride % 4 ||
      (nslices && (!parent_flags || !parent_ids || !data_lens || !slots || !slice_indices || !is_last || !seed ||
                   !pk || (k.aon >= 0 && !keys))))
    return AG_RS_ERR_INVALID_ARGUMENT;
  if (nslices == 0) return AG_RS_OK;
  if (c->enter()) return AG_RS_ERR_DEVICE;
  const size_t n = nslices;
  // MAX_DATA_SIZE: the key tail of PETS / AONT must fit the slice as well (shredder.rs:409, 457)
  const size_t extra = k.aon >= 0 ? ag::kCipherKeyBytes : 0;
  for (size_t b = 0; b < n; ++b) {
    const size_t framed = 1 + (parent_flags[b] ? AG_SLICE_BLOCK_ID_BYTES : 0) + 8 + size_t{data_lens[b]};
    if (framed + extra > kMaxPayload) return AG_RS_ERR_TOO_MUCH_DATA;
  }
  ShredScratch sc;
  int st = shred_scratch(c, n, &sc);
  if (st) return st;
  // 1. Slice::payload_bytes into the data regions; 2. PETS / AONT: encrypt_with_random_key with
  //    the caller's key + the key tail; 3. ReedSolomonCoder::shred in place
  std::vector<uint32_t> lens(n);
  if ((st = ag_slice_frame_batch(c, n, S, parent_flags, parent_ids, data, data_stride, data_lens, codewords, cw_stride,
                                 lens.data())))
    return st;
  if (k.aon >= 0) {
    if ((st = ag_aon_encrypt_batch(c, k.aon, n, keys, codewords, cw_stride, lens.data()))) return st;
    for (uint32_t& l : lens) l += static_cast<uint32_t>(ag::kCipherKeyBytes);
  }
  if ((st = ag_rs_coder_shred_batch(c, k.m, n, S, nullptr, 0, lens.data(), codewords, cw_stride))) return st;
  // 4. the 64 output shreds (data first) in place: Merkle tree, signature, datagrams over them
  return shred_tail(c, k, sc, n, S, nullptr, codewords, cw_stride, slots, slice_indices, is_last, seed, pk, roots_out,
                    sigs_out, packets, packet_stride, packet_lens, 0, nullptr, nullptr);
}

int ag_shredder_deshred_batch_kind(ag_rs_ctx* c, int kind, size_t nslices, size_t S, uint8_t* packets,
                                   size_t packet_stride, uint32_t* packet_lens, const uint8_t* pk, uint8_t* codewords,
                                   size_t cw_stride, int32_t* status, uint64_t* slots_out, uint64_t* slice_indices_out,
                                   uint8_t* is_last_out, uint8_t* parent_flags_out, uint8_t* parent_ids_out,
                                   uint32_t* data_offsets_out, uint32_t* data_lens_out) {
  if (kind == AG_SHREDDER_REGULAR) {
    if (cw_stride != ag::kPipeShreds * S) return AG_RS_ERR_INVALID_ARGUMENT;
    return ag_shredder_deshred_batch(c, nslices, S, packets, packet_stride, packet_lens, pk, codewords, status,
                                     slots_out, slice_indices_out, is_last_out, parent_flags_out, parent_ids_out,
                                     data_offsets_out, data_lens_out);
  }
  ShredderKind k;
  if (!c || !shredder_kind(kind, cw_stride, &k) || !pipe_args_ok(nslices, S, codewords, packets, packet_lens) ||
      cw_stride < (kDataShreds + k.m) * S || cw_stride % 4 ||
      (nslices && (!pk || !status || !slots_out || !slice_indices_out || !is_last_out || !parent_flags_out ||
                   !parent_ids_out || !data_offsets_out || !data_lens_out)))
    return AG_RS_ERR_INVALID_ARGUMENT;
  if (nslices == 0) return AG_RS_OK;
  if (c->enter()) return AG_RS_ERR_DEVICE;
  const size_t n = nslices;
  int st;
  // Pass 0 decodes with ANY_K on the device (per-slice window patterns, no host per-slice work);
  // a slice with surplus kept shreds that then fails the padding or the Merkle check could decode
  // differently under the crate's decoder over every kept shred, so those slices -- and only
  // those -- are decoded again with EXACT in one batched pass (rerun_exact), as the Regular
  // deshred does.  A slice that decoded and matches its signed root decoded the codeword that
  // root commits, which every kept shred matches: EXACT agrees there, whatever
  // its decryption or its parse then say.  The re-run slices were not among the slices whose
  // absent datagrams PETS / AONT serialized, nor among the decrypted ones, and they still fail
  // (rerun_exact), so their statuses follow from the coder's result and the root comparison.
  // Pass 1, the whole batch with EXACT on the coder's host-pattern route, is what shred sizes
  // and batches outside the device-pattern path run instead of pass 0 (!fast_ok).  The packets'
  // lengths change only in step 7 (PETS / AONT serialize the absent datagrams before decrypting,
  // into length-0 slots that a redo parses as absent), so a redo starts from the same datagrams.
  c->last_rerun_slices = c->last_rerun_passes = 0;
  // (test aids: the device-pattern pass only adds to them, the coder's host-pattern route resets them)
  c->last_encode_kernels = c->last_window_kernels = 0;
  const size_t key_bytes = k.aon >= 0 ? ag::kCipherKeyBytes : 0;
  DeshredScratch v;  // one layout for both passes: a redo writes the same sections again
  if ((st = deshred_scratch(c, k, n, S, &v))) return st;
  std::vector<uint8_t> ok(n), pre_ok(n), h_same(n), sstat(n);
  std::vector<int64_t> plen(n);
  std::vector<uint32_t> rerun;
  const bool fast_ok = pipe_tail_ok(S, k.m, true) && n > 1 && k.m >= kDataShreds && k.m <= 2 * kDataShreds;
  auto run_pass = [&](int pass) -> int {
    // 1-3. the kept shreds of every slice (the Regular pipeline's steps with this shredder's data
    //      / coding layout), payloads parsed straight into their codeword rows
    if ((st = deshred_front(c, k, n, S, nullptr, packets, packet_stride, packet_lens, pk, codewords, nullptr, 0, 0, &v)))
      return st;
    const uint64_t* h_present = v.h.present;
    // 4. deshred_validated_shreds: ReedSolomonCoder::deshred over the kept shreds (in their
    //    codeword rows already), then decrypt_payload (PETS / AONT) after the raw shreds are
    //    taken.  Pass 0: ANY_K with the window patterns built on the device from the kept
    //    shreds' codeword-row words; pass 1: the crate's decoder over every kept shred (EXACT)
    bool any_k = false;
    bool surplus = false;
    for (size_t s = 0; s < n; ++s) surplus |= __builtin_popcountll(h_present[s]) > static_cast<int>(kDataShreds);
    bool full_data = false;
    if (kind == AG_SHREDDER_AONT)
      for (size_t s = 0; s < n; ++s) full_data |= (h_present[s] & 0xFFFFFFFFull) == 0xFFFFFFFFull;
    if (pass == 0 && pipe_tail_ok(S, k.m, !surplus && !full_data)) {
      any_k = true;
      // codeword-row present words (pipe_coder_deshred: data | coding 0..31 << 32, coding
      // 32..63 in word 1 when m > 32); AONT's rows are the codeword rows
      const size_t wps = k.m > kDataShreds ? 2 : 1;
      const uint64_t* words = v.d_present;
      if (kind != AG_SHREDDER_AONT) {
        if ((st = c->h_strip.ensure(8 * wps * n))) return st;
        uint64_t* hw = c->h_strip.as<uint64_t>();
        for (size_t s = 0; s < n; ++s) {
          const uint64_t o = h_present[s];
          if (kind == AG_SHREDDER_CODING_ONLY) {  // output j = coding j
            hw[2 * s] = (o & 0xFFFFFFFFull) << 32;
            hw[2 * s + 1] = o >> 32;
          } else {  // PETS: output j < 31 = data j, output 31 + i = coding i
            hw[2 * s] = (o & 0x7FFFFFFFull) | (((o >> 31) & 0xFFFFFFFFull) << 32);
            hw[2 * s + 1] = o >> 63;
          }
        }
        AG_HIP(hipMemcpyAsync(v.coder_words, hw, 8 * wps * n, hipMemcpyHostToDevice, c->stream));
        words = v.coder_words;
      }
      // (pipe_coder_deshred reads its results back through h_strip after the upload completed)
      if ((st = pipe_coder_deshred(c, n, S, codewords, cw_stride, words, plen.data(), k.m, !surplus && !full_data)))
        return st;
    } else {
      std::vector<uint8_t> dp(n * kDataShreds, 0), cp(n * k.m, 0);
      for (size_t s = 0; s < n; ++s) coder_flags(k, h_present[s], &dp[s * kDataShreds], &cp[s * k.m]);
      if ((st = ag_rs_coder_deshred_batch(c, k.m, n, S, codewords, cw_stride, dp.data(), cp.data(), AG_RS_DECODE_EXACT,
                                          plen.data())))
        return st;
    }
    // AONT: the SHA-256 of every decoded ciphertext (decrypt_payload's key mask) runs on the side
    // stream, overlapping the Merkle rebuild, the root comparison and the absent datagrams'
    // serialization below (all of them only read the rows); one SHA-256 chain per slice leaves
    // most of the chip's issue slots to them.  Forked here, joined in step 5's decrypt.
    SideScope sha(c);
    if (k.aon == AG_AON_AONT) {
      std::vector<uint32_t> shl(n);
      uint32_t mx = ag::kCipherKeyBytes;
      for (size_t s = 0; s < n; ++s) {
        shl[s] = plen[s] >= static_cast<int64_t>(ag::kCipherKeyBytes) ? static_cast<uint32_t>(plen[s])
                                                                      : static_cast<uint32_t>(ag::kCipherKeyBytes);
        mx = std::max(mx, shl[s]);
      }
      if ((st = c->d_aon_lens2.ensure(n * 4, c->stream)) || (st = c->d_aon_digests.ensure(n * 32, c->stream)))
        return st;
      AG_HIP(hipStreamSynchronize(c->stream));
      AG_HIP(hipMemcpy(c->d_aon_lens2.ptr, shl.data(), n * 4, hipMemcpyHostToDevice));
      ag::BufferBatch sb;
      sb.base = codewords;
      sb.stride = cw_stride;
      sb.lens = c->d_aon_lens2.as<uint32_t>();
      sb.n = n;
      sb.max_len = mx;
      if ((st = sha.open())) return st;
      AG_HIP(ag::launch_sha256(sb, ag::kCipherKeyBytes, c->d_aon_digests.as<uint8_t>(), sha.stream()));
      if ((st = sha.close())) return st;
    }
    // 5. check_merkle_tree over the raw output shreds (before any decryption: they are the
    //    codeword rows)
    if ((st = kind_merkle(c, k, n, S, codewords, cw_stride, v.roots2, v.cols.proof))) return st;
    if (ag::launch_pipe_root_cmp(v.roots2, v.sroot, n, v.same, c->stream) != hipSuccess) return AG_RS_ERR_DEVICE;
    AG_HIP(hipMemcpyAsync(h_same.data(), v.same, n, hipMemcpyDeviceToHost, c->stream));
    AG_HIP(hipStreamSynchronize(c->stream));
    // the slices the ANY_K decode may have wronged (regular_deshred's step 6b)
    rerun.clear();
    for (size_t s = 0; any_k && s < n; ++s) {
      const bool failed = plen[s] == -AG_RS_ERR_INVALID_PADDING || (plen[s] >= 0 && !h_same[s]);
      if (failed && __builtin_popcountll(h_present[s]) > static_cast<int>(kDataShreds))
        rerun.push_back(static_cast<uint32_t>(s));
    }
    if (k.aon >= 0) {
      // the absent datagrams of the slices that decoded and match their root, serialized from
      // the encrypted rows; then decrypt_payload (BadEncoding for a buffer shorter than the key)
      for (size_t s = 0; s < n; ++s) pre_ok[s] = plen[s] >= 0 && h_same[s];
      if ((st = fill_missing(c, k, n, S, v, pre_ok.data(), packets, packet_stride))) return st;
      AG_HIP(hipStreamSynchronize(c->stream));
      std::vector<uint32_t> cl(n);
      for (size_t s = 0; s < n; ++s) cl[s] = pre_ok[s] ? static_cast<uint32_t>(plen[s]) : 0;
      std::vector<int64_t> pl(n);
      if (sha.is_open()) {
        // decrypt_payload with the side stream's digests (ag_aon_decrypt_batch's key and
        // length rules; the digests of the slices decrypted here hash the same lengths)
        for (size_t s = 0; s < n; ++s) {
          pl[s] = cl[s] < ag::kCipherKeyBytes ? -AG_RS_ERR_BAD_ENCODING
                                              : static_cast<int64_t>(cl[s]) - ag::kCipherKeyBytes;
          // a failed slice (cl 0) or a buffer shorter than the key: a keystream of zero bytes
          if (cl[s] < ag::kCipherKeyBytes) cl[s] = ag::kCipherKeyBytes;
        }
        ag::BufferBatch bb;
        if ((st = aon_batch(c, n, codewords, cw_stride, cl.data(), 0, &bb)) ||
            (st = c->d_aon_keys.ensure(n * 16, c->stream)))
          return st;
        if ((st = sha.join())) return st;
        if (ag::launch_derive_keys(bb, 1, c->d_aon_digests.as<uint8_t>(), c->d_aon_keys.as<uint8_t>(), c->stream) !=
                hipSuccess ||
            ag::launch_apply_keystream(bb, c->d_aon_keys.as<uint8_t>(), ag::kCipherKeyBytes, c->stream) != hipSuccess)
          return AG_RS_ERR_DEVICE;
        AG_HIP(hipStreamSynchronize(c->stream));
      } else if ((st = ag_aon_decrypt_batch(c, k.aon, n, codewords, cw_stride, cl.data(), pl.data()))) {
        return st;
      }
      for (size_t s = 0; s < n; ++s)
        if (pre_ok[s]) plen[s] = pl[s];
    }
    // 6. SlicePayload::try_from on the (decrypted) payload
    if ((st = ag_slice_parse_batch(c, n, codewords, cw_stride, plen.data(), sstat.data(), parent_flags_out,
                                   parent_ids_out, data_offsets_out, data_lens_out)))
      return st;
    pipe_statuses(n, plen.data(), h_same.data(), sstat.data(), v.h, key_bytes, status, ok.data(), slots_out,
                  slice_indices_out, is_last_out);
    return AG_RS_OK;
  };
  if ((st = run_pass(fast_ok ? 0 : 1))) return st;
  if (!rerun.empty()) {
    // 6b. the batched EXACT pass over the listed slices; their entries replace pass 0's
    RerunResult rr;
    bool passed = false;
    if ((st = rerun_exact(c, k, rerun, S, nullptr, packets, packet_stride, v, codewords, cw_stride, &rr, &passed)))
      return st;
    if (passed) {
      // A listed slice that decodes and matches its root after all (a SHA-256 collision, or two
      // decoders of this library disagreeing) cannot be finished here as Regular finishes it:
      // PETS / AONT would still have to serialize its absent datagrams from the encrypted rows
      // and decrypt it, stages that run over the whole batch inside a pass and have run already.
      // Correct before cheap: the batch is redone with EXACT, which does exactly that.
      if ((st = run_pass(1))) return st;
    } else {
      for (size_t r = 0; r < rerun.size(); ++r) {
        const size_t s = rerun[r];
        plen[s] = rr.plen[r];
        h_same[s] = rr.same[r];
        sstat[s] = rr.sstat[r];
        parent_flags_out[s] = rr.parent_flag[r];
        std::copy_n(&rr.parent_id[AG_SLICE_BLOCK_ID_BYTES * r], AG_SLICE_BLOCK_ID_BYTES,
                    parent_ids_out + AG_SLICE_BLOCK_ID_BYTES * s);
        data_offsets_out[s] = rr.data_offset[r];
        data_lens_out[s] = rr.data_len[r];
      }
      pipe_statuses(n, plen.data(), h_same.data(), sstat.data(), v.h, key_bytes, status, ok.data(), slots_out,
                    slice_indices_out, is_last_out);
    }
  }
  // 7. fill_missing_shreds: every absent slot of a successful slice gets its datagram (PETS /
  //    AONT serialized theirs from the encrypted rows, before the decrypt)
  if (k.aon < 0) {
    if ((st = fill_missing(c, k, n, S, v, ok.data(), packets, packet_stride))) return st;
    AG_HIP(hipStreamSynchronize(c->stream));
  }
  AG_HIP(hipMemcpyAsync(v.slice_ok, ok.data(), n, hipMemcpyHostToDevice, c->stream));
  if (ag::launch_pipe_merge_lens(v.fresh_lens, v.d_present, v.slice_ok, n, packet_lens, c->stream) != hipSuccess)
    return AG_RS_ERR_DEVICE;
  AG_HIP(hipStreamSynchronize(c->stream));
  return AG_RS_OK;
}

}  // extern "C"
