// Repair intake (repair.hip): repaired shreds in arrival order, each with the coordinates of the
// request it answers -> the slice slots of ag_shredder_deshred_batch_var, with the verdicts of the
// reference's RepairResponse::Shred handling (repair.rs:410-445, ValidatedShred::try_new without
// a cache, BlockData::add_shred per repaired block).  Parameter block and launchers; the host
// composition is repair_api.cpp, the sequential definition is include/alpenglow_rs.h section 11.
//
// The chain shares the dissemination intake's last stages unchanged (launch_intake_setter,
// _claim, _route, _finalize read `in` with nslots = the blocks under repair); what differs --
// the row from the request, the proved root in front of the signature, a signature per reply
// with inheritance by (commitment, signature), a key per block -- is the kernels here.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "intake.hpp"

namespace ag {

struct RepairParams {
  // store, verdicts and scratch as intake names them.  in.nslots = blocks, in.spp = slices per
  // block, in.win_ids / win_w unused; in.pick: earliest reply that matches the proved root, in
  // a row without a cache; in.setter: earliest such reply with a valid signature.
  IntakeParams in;
  const uint64_t* block_slots;  // [blocks] slot of each block under repair (device copy)
  const uint32_t* req_block;    // [n] the request of reply t: block, slice, shred index
  const uint32_t* req_slice;
  const uint32_t* req_index;
  const uint8_t* pks;           // [blocks][32] leader keys
  const uint8_t* slice_roots;   // [nrows][32] proved roots, valid where have_root[r] != 0
  const uint8_t* have_root;     // [nrows]
  uint8_t* signatures;          // [nrows][64] the store's signature beside each cached commitment
  const uint8_t* sig;           // [n][64] the parsed signatures (scratch)
  uint8_t* keys;                // [n][32] the block's key per reply: the verify launches' pks (scratch)
  uint8_t* ok;                  // = in.ok: classify marks the replies that inherit "valid"
};

// 1-4 of the definition: MALFORMED / OUT_OF_WINDOW / REQUEST_MISMATCH / IMPLAUSIBLE, else row
// and meta.
hipError_t launch_repair_key(const RepairParams& p, hipStream_t stream);
// 5: NO_ROOT / WRONG_ROOT (the reply leaves the chain), else commitment, key row and the pick.
hipError_t launch_repair_root(const RepairParams& p, hipStream_t stream);
// list1 = the picks.
hipError_t launch_repair_picks(const RepairParams& p, hipStream_t stream);
// list2 = root-matching replies that are no pick and whose (commitment, signature) is not the
// store's pair or a valid pick's; those that are inherit ok = 1.
hipError_t launch_repair_classify(const RepairParams& p, hipStream_t stream);
// 6-7: INVALID_SIGNATURE / EQUIVOCATION / SIZE_MISMATCH or kIntakeAccepted; tstar per block.
hipError_t launch_repair_accept(const RepairParams& p, hipStream_t stream);
// the new setters' signatures into the store (before launch_intake_finalize sets shred_bytes).
hipError_t launch_repair_signatures(const RepairParams& p, hipStream_t stream);

}  // namespace ag
