"""The sequential definition of ag_repair_intake_batch (include/alpenglow_rs.h section 11) --
TEST INFRASTRUCTURE ONLY: the checker of tests/test_repair_intake.py, never the product path.

Repair replies are processed one at a time in arrival order, each through the reference's
RepairResponse::Shred handling, composed from the existing oracles (shred_wire_oracle.deserialize,
merkle_oracle.derive_root, ed25519_oracle.slice_commitment / validate_shred, the signature
verdicts memoised by intake_model):

  repair.rs:410-423           the reply's header against the request it answers
  repair.rs:424-432           the proved slice root of (block, slice) in front of the signature
  repair.rs:433-437           ValidatedShred::try_new(shred, None, leader_pk): always verified
  slot_block_data.rs:101-113  add_shred_from_repair: one BlockData per (slot, block hash)
  slot_block_data.rs:202-248  BlockData::add_shred: commitment cache, last-slice rule, duplicates
  slot_block_data.rs:269-274  mark_last_slice: shreds.retain(ind <= slice_index), cache kept

with the two documented deviations of the dissemination intake (intake_model.py): the
plausibility check, and a shred of another size than the row's counting as absent.
"""

from __future__ import annotations

import ed25519_oracle as ed
import intake_model as im
import merkle_oracle as mk
import shred_wire_oracle as wire
from intake_model import (DATA_SHREDS, DUPLICATE, EQUIVOCATION, HEIGHT, IMPLAUSIBLE,  # noqa: F401
                          INVALID_SIGNATURE, MALFORMED, MAX_DATA_PER_SHRED, OUT_OF_WINDOW, PRUNED, SIZE_MISMATCH,
                          STORED, TOTAL_SHREDS)

REQUEST_MISMATCH, NO_ROOT, WRONG_ROOT = 9, 10, 11


class Store:
    """The caller-owned store: per row (block b, slice i: r = b * spb + i) the 64 datagram slots,
    the cached commitment, the signature that verified for it and the shred size that came with
    it; per block the last slice.  Blocks may share a slot id: they are kept apart by index."""

    def __init__(self, block_slots, pks, slices_per_block: int):
        assert len(block_slots) == len(pks)
        self.block_slots, self.pks, self.spb = list(block_slots), list(pks), slices_per_block
        self.nrows = len(self.block_slots) * slices_per_block
        self.slots = [[None] * TOTAL_SHREDS for _ in range(self.nrows)]
        self.commitment = [None] * self.nrows   # BlockData::commitment_cache
        self.signature = [None] * self.nrows
        self.shred_bytes = [0] * self.nrows
        self.last_slice = [None] * len(self.block_slots)  # BlockData::last_slice
        self.roots = [None] * self.nrows        # Repair::slice_roots: None = not proved

    def counts(self):
        return [sum(x is not None for x in row) for row in self.slots]


def intake(store: Store, replies) -> list:
    """Feeds the replies ((shred bytes, req_block, req_slice, req_index) each) in order; returns
    their verdicts.  `store` is updated."""
    verdicts = [None] * len(replies)
    placed = {}  # (row, shred index) -> t of the reply this call stored there
    for t, (buf, b, s, i) in enumerate(replies):
        verdicts[t] = _one(store, t, bytes(buf), b, s, i, placed, verdicts)
    return verdicts


def _one(st: Store, t: int, buf: bytes, b: int, s: int, i: int, placed: dict, verdicts: list) -> int:
    # 1. network::deserialize; an empty datagram is no shred
    parsed = wire.deserialize(buf) if len(buf) else None
    if parsed is None:
        return MALFORMED
    kind, slot, si, is_last, j, data, sig, proof = parsed
    # 2. the request names no row of the store
    if b >= len(st.block_slots) or s >= st.spb or i >= TOTAL_SHREDS:
        return OUT_OF_WINDOW
    # 3. repair.rs:417-423
    if slot != st.block_slots[b] or si != s or j != i:
        return REQUEST_MISMATCH
    r = b * st.spb + s
    # 4. plausibility (the deviation ag_shredder_deshred_batch documents)
    if (kind != (wire.DATA if j < DATA_SHREDS else wire.CODING) or len(data) == 0 or len(data) % 2 or
            len(data) > MAX_DATA_PER_SHRED or len(proof) != HEIGHT):
        return IMPLAUSIBLE
    # 5. repair.rs:424-432: the proved root, before any signature work
    if st.roots[r] is None:
        return NO_ROOT
    root = mk.derive_root(data, j, proof)
    if root != st.roots[r]:
        return WRONG_ROOT
    # 6. repair.rs:433-437: try_new(shred, None, leader_pk) -- no equal-commitment shortcut
    msg = ed.slice_commitment(slot, si, is_last, root)
    if im._validate(msg, sig, st.pks[b], None) != ed.OK:
        return INVALID_SIGNATURE
    # 7. BlockData::add_shred of the block's own BlockData (slot_block_data.rs:202-248)
    if st.commitment[r] is not None:
        if st.commitment[r] != msg:                           # :215-217
            return EQUIVOCATION
        if len(data) != st.shred_bytes[r]:                    # deshred_batch_var's receive model
            return SIZE_MISMATCH
    else:                                                     # :219-221 Entry::Vacant
        st.commitment[r], st.signature[r], st.shred_bytes[r] = msg, sig, len(data)
    l = st.last_slice[b]
    if l is None:
        if is_last:                                           # :225 mark_last_slice (:269-274)
            st.last_slice[b] = si
            for k in range(si + 1, st.spb):                   # shreds.retain(ind <= slice_index)
                q = b * st.spb + k
                for jj in range(TOTAL_SHREDS):
                    if (q, jj) in placed:
                        verdicts[placed.pop((q, jj))] = PRUNED
                    st.slots[q][jj] = None
    else:
        consistent = (si < l and not is_last) or (si == l and is_last)  # :228
        if not consistent:
            return EQUIVOCATION                               # :229-231
    if st.slots[r][j] is not None:                            # :241-247
        return DUPLICATE
    st.slots[r][j] = buf                                      # :248
    placed[(r, j)] = t
    return STORED
