// Host side of ag_block_assemble_batch (include/alpenglow_rs.h section 12): the argument checks
// (the per-row offset / length check is what keeps the walk inside a row), the upload of the
// caller's host columns, the carve-up of the context's block scratch and the fixed chain of
// launches -- scan, the block tree (merkle.hip, unchanged) with the walk beside it on the side
// stream, finish, total and, when a table was passed, index (block.hip).  Every launch is made whatever the slices hold; whether the
// table fits is decided on the device.  One copy brings the host outputs back.
#include <hip/hip_runtime.h>

#include <cstring>

#include "../../include/alpenglow_rs.h"
#include "block.hpp"
#include "merkle.hpp"
#include "rs_ctx.hpp"

using namespace ag::host;

namespace {

constexpr size_t kMaxRows = size_t{1} << 24;
constexpr size_t kMinCodewordStride = 32768;  // a framed payload is at most 32 767 bytes

bool aligned16(const void* p) { return reinterpret_cast<uintptr_t>(p) % 16 == 0; }

// The scratch, then the staged host outputs (contiguous: one copy).  Returns the total; *out_at /
// *out_bytes: where the staged outputs lie.
size_t carve(uint8_t* base, size_t nblocks, size_t nrows, bool want_hashes, ag::BlockParams* p, size_t* out_at,
             size_t* out_bytes) {
  Carver c{base};
  p->roots = c.take<uint8_t>(32 * nrows);
  p->first = c.take<uint64_t>(nblocks);
  p->count = c.take<uint32_t>(nblocks);
  p->perr_slice = c.take<uint32_t>(nblocks);
  p->perr_code = c.take<uint8_t>(nblocks);
  p->cand_parent = c.take<uint8_t>(ag::kBlockParentBytes * nblocks);
  p->row_cnt = c.take<uint32_t>(nrows);
  p->row_bytes = c.take<uint32_t>(nrows);
  p->row_bad = c.take<uint8_t>(nrows);
  p->row_first = c.take<uint32_t>(nrows);
  p->fit = c.take<uint32_t>(1);
  *out_at = c.used;
  p->tx_first = c.take<uint64_t>(nblocks);
  p->tx_bytes = c.take<uint64_t>(nblocks);
  p->tx_total = c.take<uint64_t>(1);
  p->error_slice = c.take<uint32_t>(nblocks);
  p->tx_counts = c.take<uint32_t>(nblocks);
  p->hashes = c.take<uint8_t>(want_hashes ? 32 * nblocks : 0);
  if (!want_hashes) p->hashes = nullptr;
  p->parents = c.take<uint8_t>(ag::kBlockParentBytes * nblocks);
  p->verdict = c.take<uint8_t>(nblocks);
  *out_bytes = c.used - *out_at;
  return c.used;
}

}  // namespace

int ag_block_assemble_batch(ag_rs_ctx* c, size_t nblocks, size_t slices_per_block, const uint8_t* row_ok,
                            const uint8_t* parent_flags, const uint8_t* parent_ids, const uint32_t* data_offsets,
                            const uint32_t* data_lens, const uint8_t* codewords, size_t codeword_stride,
                            const uint8_t* slice_roots, size_t roots_stride, const int32_t* last_slice,
                            size_t max_txs_per_slice, uint8_t* verdict_out, uint32_t* error_slice_out,
                            uint8_t* parents_out, uint32_t* tx_counts_out, uint64_t* tx_bytes_out,
                            uint8_t* block_hashes, uint8_t* block_hashes_host, uint8_t* nodes, size_t nodes_stride,
                            uint8_t* proofs, size_t proofs_stride, uint64_t* tx_offsets, uint32_t* tx_lens,
                            size_t tx_capacity, uint64_t* tx_first_out, uint64_t* tx_total_out) {
  static_assert(AG_BLOCK_MAX_SLICES == ag::kBlockMaxSlices && AG_SLICE_BLOCK_ID_BYTES == ag::kBlockParentBytes);
  if (!c) return AG_RS_ERR_INVALID_ARGUMENT;
  if (nblocks == 0) {
    if (tx_total_out) *tx_total_out = 0;
    return AG_RS_OK;
  }
  if (slices_per_block == 0 || slices_per_block > AG_BLOCK_MAX_SLICES || nblocks >= kMaxRows ||
      nblocks * slices_per_block >= kMaxRows || !row_ok || !parent_flags || !parent_ids || !data_offsets ||
      !data_lens || !codewords || !slice_roots || !last_slice || !verdict_out || !error_slice_out || !parents_out ||
      !tx_counts_out || !tx_bytes_out || !block_hashes || !tx_first_out || !tx_total_out || !aligned16(codewords) ||
      codeword_stride % 16 || codeword_stride < kMinCodewordStride || roots_stride < 32 || !aligned16(block_hashes) ||
      !aligned16(nodes) || !aligned16(proofs) || (proofs && !nodes) || (!tx_offsets) != (!tx_lens) ||
      (nodes && (nodes_stride % 16 || nodes_stride < 32 * ag_merkle_node_count(slices_per_block))) ||
      (proofs &&
       (proofs_stride % 16 || proofs_stride < 32 * ag_merkle_height(slices_per_block) * slices_per_block)))
    return AG_RS_ERR_INVALID_ARGUMENT;
  const size_t nrows = nblocks * slices_per_block;
  for (size_t r = 0; r < nrows; ++r) {
    if (!row_ok[r]) continue;
    const uint32_t want = parent_flags[r] == 0 ? 9u : 9u + AG_SLICE_BLOCK_ID_BYTES;
    if (parent_flags[r] > 1 || data_offsets[r] != want || data_lens[r] > AG_SLICE_MAX_DATA - want)
      return AG_RS_ERR_INVALID_ARGUMENT;
  }
  int st = c->enter();
  if (st || (st = ensure_empty_roots(c))) return st;

  // the columns: lengths, parent ids (8-byte aligned rows), then the two flag columns
  const size_t ids_at = (4 * nrows + 255) / 256 * 256, ok_at = ids_at + ag::kBlockParentBytes * nrows,
               flags_at = ok_at + nrows, cols_bytes = flags_at + nrows;
  uint8_t* cols = nullptr;
  if ((st = c->block_cols.host(cols_bytes, &cols))) return st;
  std::memcpy(cols, data_lens, 4 * nrows);
  std::memcpy(cols + ids_at, parent_ids, ag::kBlockParentBytes * nrows);
  std::memcpy(cols + ok_at, row_ok, nrows);
  std::memcpy(cols + flags_at, parent_flags, nrows);
  if ((st = c->block_cols.send(cols_bytes, c->stream))) return st;

  ag::BlockParams p{};
  size_t out_at = 0, out_bytes = 0;
  const size_t need = carve(nullptr, nblocks, nrows, block_hashes_host != nullptr, &p, &out_at, &out_bytes);
  if ((st = c->d_block.ensure(need, c->stream)) || (st = c->h_block.ensure(out_bytes))) return st;
  carve(c->d_block.as<uint8_t>(), nblocks, nrows, block_hashes_host != nullptr, &p, &out_at, &out_bytes);
  const uint8_t* dcols = c->block_cols.dev.as<uint8_t>();
  p.nblocks = static_cast<uint32_t>(nblocks);
  p.spb = static_cast<uint32_t>(slices_per_block);
  p.data_lens = reinterpret_cast<const uint32_t*>(dcols);
  p.parent_ids = dcols + ids_at;
  p.row_ok = dcols + ok_at;
  p.parent_flags = dcols + flags_at;
  p.codewords = codewords;
  p.codeword_stride = codeword_stride;
  p.slice_roots = slice_roots;
  p.roots_stride = roots_stride;
  p.last_slice = last_slice;
  p.block_hashes = block_hashes;
  p.max_txs = max_txs_per_slice;
  p.tx_capacity = tx_capacity;
  p.tx_offsets = tx_offsets;
  p.tx_lens = tx_lens;

  ag::BlockTreeParams t{};
  t.first = p.first;
  t.count = p.count;
  t.nblocks = nblocks;
  t.slice_roots = p.roots;
  t.empty_roots = c->d_empty_roots.as<uint32_t>();
  t.block_hashes = block_hashes;
  t.nodes = nodes;
  t.nodes_stride = nodes_stride;
  t.proofs = proofs;
  t.proofs_stride = proofs_stride;

  // The tree (a chain of up to 10 dependent levels per block) and the walk (a chain of dependent
  // loads per row) read only what the scan wrote: the walk runs on the side stream beside the
  // tree.
  hipStream_t q = c->stream;
  AG_HIP(ag::launch_block_scan(p, q));
  SideScope side(c);
  if ((st = side.open())) return st;
  AG_HIP(ag::launch_block_walk(p, side.stream()));
  if ((st = side.close())) return st;
  AG_HIP(ag::launch_block_tree(t, q));
  if ((st = side.join())) return st;
  AG_HIP(ag::launch_block_finish(p, q));
  AG_HIP(ag::launch_block_total(p, q));
  if (tx_offsets) AG_HIP(ag::launch_block_index(p, q));
  uint8_t* h = c->h_block.as<uint8_t>();
  const uint8_t* d = c->d_block.as<uint8_t>();
  AG_HIP(hipMemcpyAsync(h, d + out_at, out_bytes, hipMemcpyDeviceToHost, q));
  AG_HIP(hipStreamSynchronize(q));

  auto staged = [&](const void* dev) { return h + (static_cast<const uint8_t*>(dev) - d - out_at); };
  std::memcpy(tx_first_out, staged(p.tx_first), 8 * nblocks);
  std::memcpy(tx_bytes_out, staged(p.tx_bytes), 8 * nblocks);
  std::memcpy(tx_total_out, staged(p.tx_total), 8);
  std::memcpy(error_slice_out, staged(p.error_slice), 4 * nblocks);
  std::memcpy(tx_counts_out, staged(p.tx_counts), 4 * nblocks);
  std::memcpy(parents_out, staged(p.parents), ag::kBlockParentBytes * nblocks);
  std::memcpy(verdict_out, staged(p.verdict), nblocks);
  if (block_hashes_host) {  // like the device hashes: an INCOMPLETE block's 32 bytes are not written
    const uint8_t* hs = staged(p.hashes);
    for (size_t b = 0; b < nblocks; ++b)
      if (verdict_out[b] != AG_BLOCK_INCOMPLETE) std::memcpy(block_hashes_host + 32 * b, hs + 32 * b, 32);
  }
  return AG_RS_OK;
}
