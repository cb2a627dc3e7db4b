// Block assembly (block.hip): the reconstructed slices of a block -> the verdict of
// BlockData::try_reconstruct_block (slot_block_data.rs:376-454), the block hash, the parent after
// the optimistic-handover rule and an index of the block's transactions.  Parameter block and
// launchers; the host composition is block_api.cpp, the sequential definition is
// include/alpenglow_rs.h section 12 (tests/block_model.py restates it and is the checker).
//
// The chain, the same launches whatever the slices hold (walk on the context's side stream beside
// the tree, everything else on its stream):
//   scan    one workgroup per block: completeness, the parent rule, the tree's (first, count),
//           the block's slice roots gathered into contiguous digests
//   tree    launch_block_tree (merkle.hip) unchanged; a block with count 0 writes nothing there
//   walk    one lane per row of a candidate block: deserialize_exact::<Vec<Transaction>> over the
//           row's data, reading only the length prefixes
//   finish  one workgroup per block: the first failing slice, the sums, each row's prefix
//   total   one workgroup: the blocks' prefix, the total, "the table fits"
//   index   (only with a table) one lane per row: walks again and writes the entries
// Kernel boundaries are the only synchronisation between workgroups.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace ag {

constexpr uint32_t kBlockNone = 0xFFFFFFFFu;
constexpr uint32_t kBlockParentBytes = 40;  // BlockId = (Slot u64, BlockHash [u8; 32])

struct BlockParams {
  uint32_t nblocks, spb;  // row r = b * spb + i, nrows = nblocks * spb < 2^24
  // the caller's columns, uploaded (device copies; parent_ids 8-byte aligned rows of 40)
  const uint8_t* row_ok;
  const uint8_t* parent_flags;
  const uint8_t* parent_ids;
  const uint32_t* data_lens;
  // the caller's device buffers
  const uint8_t* codewords;  // row r's framed payload at codewords + r * codeword_stride
  uint64_t codeword_stride;
  const uint8_t* slice_roots;  // row r's root at slice_roots + r * roots_stride, any alignment
  uint64_t roots_stride;
  const int32_t* last_slice;  // [nblocks]
  const uint8_t* block_hashes;  // what the tree wrote (finish copies it for the host)
  uint64_t max_txs;      // 0 = no limit
  uint64_t tx_capacity;  // entries tx_offsets / tx_lens hold
  uint64_t* tx_offsets;  // nullable together
  uint32_t* tx_lens;
  // scratch
  uint8_t* roots;        // [nrows][32] gathered roots: the tree's leaves
  uint64_t* first;       // [nblocks] = b * spb
  uint32_t* count;       // [nblocks] last_slice + 1, or 0 for an INCOMPLETE block
  uint32_t* perr_slice;  // [nblocks] the slice the parent rule fails at, or kBlockNone
  uint8_t* perr_code;    // [nblocks] AG_BLOCK_PARENT_SAME / _TWICE there
  uint8_t* cand_parent;  // [nblocks][40] the parent if nothing fails
  uint32_t* row_cnt;     // [nrows] transactions of the row (0 outside candidate blocks)
  uint32_t* row_bytes;   // [nrows] their payload bytes
  uint8_t* row_bad;      // [nrows] rule 4 failed
  uint32_t* row_first;   // [nrows] transactions of the block's earlier rows
  uint32_t* fit;         // [1] a table was passed and the total fits
  // the host outputs, staged on the device for one copy
  uint64_t* tx_first;     // [nblocks]
  uint64_t* tx_bytes;     // [nblocks]
  uint64_t* tx_total;     // [1]
  uint32_t* error_slice;  // [nblocks]
  uint32_t* tx_counts;    // [nblocks]
  uint8_t* hashes;        // [nblocks][32], 16-byte aligned; null when the caller wants no host copy
  uint8_t* parents;       // [nblocks][40]
  uint8_t* verdict;       // [nblocks]
};

hipError_t launch_block_scan(const BlockParams& p, hipStream_t stream);
hipError_t launch_block_walk(const BlockParams& p, hipStream_t stream);
hipError_t launch_block_finish(const BlockParams& p, hipStream_t stream);
hipError_t launch_block_total(const BlockParams& p, hipStream_t stream);
hipError_t launch_block_index(const BlockParams& p, hipStream_t stream);

}  // namespace ag
