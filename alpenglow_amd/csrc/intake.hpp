// Shred intake (intake.hip): received datagrams in arrival order -> the slice slots of
// ag_shredder_deshred_batch_var, with the reference's per-datagram verdicts
// (ValidatedShred::try_new, validated_shred.rs:52-79; BlockData::add_shred,
// slot_block_data.rs:202-248).  Parameter block and launchers; the host composition is
// intake_api.cpp, the sequential definition is include/alpenglow_rs.h section 10.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace ag {

constexpr uint32_t kIntakeNone = 0xFFFFFFFFu;  // no datagram (arrival-index tables), no row
constexpr uint32_t kIntakeCommitStride = 64;   // scratch rows of the 49-byte commitments
// verdict of a datagram try_new accepted, until the route kernel settles it (internal: never
// left in the caller's verdict array)
constexpr uint8_t kIntakeAccepted = 0xF0;

// One block for every kernel: each reads what it needs.  n datagrams, nrows = nslots * spp rows.
struct IntakeParams {
  uint64_t n;
  uint32_t nslots, spp, nrows;
  // the window: slot ids ascending and the caller's index w of each (device)
  const uint64_t* win_ids;
  const uint32_t* win_w;
  // input
  const uint8_t* rx;
  uint64_t rx_stride;
  const uint32_t* rx_lens;
  // the caller's store
  uint8_t* packets;
  uint64_t packet_stride;
  uint32_t* packet_lens;  // [64 * nrows]
  uint8_t* commitments;   // [nrows][49]
  uint32_t* shred_bytes;  // [nrows]
  int32_t* last_slice;    // [nslots]
  uint8_t* verdict;       // [n]
  // per datagram scratch
  const uint8_t* wire;    // launch_shred_deserialize's status
  const uint64_t* slot;   // its slot / slice_index / height columns
  const uint64_t* slice_index;
  const uint32_t* height;
  uint32_t* row;          // window row, kIntakeNone = not plausible
  uint32_t* meta;         // shred index | is_last << 8 | data_len << 16
  uint8_t* plausible;     // the Merkle stage's `active`
  const uint8_t* roots;   // [n][32] derived roots
  uint8_t* commit;        // [n][kIntakeCommitStride]
  const uint8_t* ok;      // signature verdicts of the datagrams verified (zeroed per call)
  uint32_t* list1;        // first verify launch: the rows' picks
  uint32_t* list2;        // second: everything not equal to a valid cache
  uint32_t* counts;       // [2] their lengths (zeroed per call)
  // per row / slot scratch, all kIntakeNone per call
  uint32_t* pick;         // [nrows] earliest plausible datagram of a row without a cache
  uint32_t* setter;       // [nrows] earliest datagram with a valid signature of such a row
  uint32_t* tstar;        // [nslots] earliest accepted is_last datagram of a slot without a last slice
  uint32_t* claim;        // [64 * nrows] earliest datagram that reached the slot
  uint32_t* out;          // [2 * nrows]: S_s | occupied slots, for the host
};

// 1-3 of the definition: MALFORMED / OUT_OF_WINDOW / IMPLAUSIBLE, else row, meta and the pick.
hipError_t launch_intake_key(const IntakeParams& p, hipStream_t stream);
// commitments of the plausible datagrams; list1 = the picks.
hipError_t launch_intake_commit(const IntakeParams& p, hipStream_t stream);
// list2 = plausible datagrams that are neither a pick nor equal to a valid cache.
hipError_t launch_intake_classify(const IntakeParams& p, hipStream_t stream);
// setter[r] = min t over the datagrams with a valid signature.
hipError_t launch_intake_setter(const IntakeParams& p, hipStream_t stream);
// 4-5: INVALID_SIGNATURE / EQUIVOCATION / SIZE_MISMATCH or kIntakeAccepted; tstar.
hipError_t launch_intake_accept(const IntakeParams& p, hipStream_t stream);
// 6.2: the last-slice rule (EQUIVOCATION), then the claim of the slot.
hipError_t launch_intake_claim(const IntakeParams& p, hipStream_t stream);
// 6.3-6.4: DUPLICATE / PRUNED / STORED and the copy, one wave per datagram.
hipError_t launch_intake_route(const IntakeParams& p, hipStream_t stream);
// per row: new caches into the store, pruned lengths zeroed, S_s and the occupied count to
// `out`; then (a launch of its own: the rows read last_slice) the slots' new last slices.
hipError_t launch_intake_finalize(const IntakeParams& p, hipStream_t stream);

}  // namespace ag
