"""The sequential definition of ag_shredder_intake_batch (include/alpenglow_rs.h section 10) --
TEST INFRASTRUCTURE ONLY: the checker of tests/test_shredder_intake.py, never the product path.

Datagrams are processed one at a time in arrival order, each through the reference's receive
path, composed from the existing oracles (shred_wire_oracle.deserialize, merkle_oracle.derive_root,
ed25519_oracle.slice_commitment / validate_shred):

  consensus.rs:376-416        network::deserialize, then Blockstore::add_shred_from_disseminator
  validated_shred.rs:52-79    ValidatedShred::try_new with the cached commitment of the slice
  slot_block_data.rs:202-248  BlockData::add_shred: commitment cache, last-slice rule, duplicates
  slot_block_data.rs:269-274  mark_last_slice: shreds.retain(ind <= slice_index), cache kept

Two checks stand in front that the reference does not make (the documented deviation of
ag_shredder_deshred_batch: such shreds are never stored), and one behind try_new that is the
receive model of ag_shredder_deshred_batch_var (a datagram of another size than the row's counts
as absent).
"""

from __future__ import annotations

import ed25519_oracle as ed
import merkle_oracle as mk
import shred_wire_oracle as wire

(STORED, MALFORMED, OUT_OF_WINDOW, IMPLAUSIBLE, INVALID_SIGNATURE, EQUIVOCATION, SIZE_MISMATCH, DUPLICATE,
 PRUNED) = range(9)

TOTAL_SHREDS, DATA_SHREDS, HEIGHT, MAX_DATA_PER_SHRED = 64, 32, 6, 1024

_verified: dict = {}  # (pk, commitment, sig) -> validate_shred's signature verdict (pure Python: slow)


def _validate(commitment: bytes, sig: bytes, pk: bytes, cached):
    """ed25519_oracle.validate_shred, its signature checks memoised."""
    if cached is not None and cached == commitment:
        return ed.OK  # validated_shred.rs:62-64: no signature check
    key = (pk, commitment, sig)
    if key not in _verified:
        _verified[key] = ed.validate_shred(commitment, sig, pk, None) == ed.OK
    if cached is not None:
        return ed.EQUIVOCATION if _verified[key] else ed.INVALID_SIGNATURE  # :65-69
    return ed.OK if _verified[key] else ed.INVALID_SIGNATURE  # :71-77


class Store:
    """The caller-owned store: per row the 64 datagram slots (bytes or None), the cached
    commitment and the shred size that came with it; per slot of the window the last slice."""

    def __init__(self, slot_ids, slices_per_slot: int):
        assert len(set(slot_ids)) == len(slot_ids)
        self.slot_ids, self.spp = list(slot_ids), slices_per_slot
        self.nrows = len(self.slot_ids) * slices_per_slot
        self.slots = [[None] * TOTAL_SHREDS for _ in range(self.nrows)]
        self.commitment = [None] * self.nrows   # BlockData::commitment_cache
        self.shred_bytes = [0] * self.nrows
        self.last_slice = [None] * len(self.slot_ids)  # BlockData::last_slice

    def counts(self):
        return [sum(x is not None for x in row) for row in self.slots]


def intake(store: Store, datagrams, pk: bytes) -> list:
    """Feeds the datagrams (bytes each) in order; returns their verdicts.  `store` is updated."""
    verdicts = [None] * len(datagrams)
    placed = {}  # (row, shred index) -> t of the datagram this call stored there
    for t, buf in enumerate(datagrams):
        verdicts[t] = _one(store, t, bytes(buf), pk, placed, verdicts)
    return verdicts


def _one(st: Store, t: int, buf: bytes, pk: bytes, placed: dict, verdicts: list) -> int:
    # 1. consensus.rs: network::deserialize; an empty datagram is no shred
    parsed = wire.deserialize(buf) if len(buf) else None
    if parsed is None:
        return MALFORMED
    kind, slot, si, is_last, j, data, sig, proof = parsed
    # 2. the window
    if slot not in st.slot_ids or si >= st.spp:
        return OUT_OF_WINDOW
    w = st.slot_ids.index(slot)
    r = w * st.spp + si
    # 3. plausibility (the deviation ag_shredder_deshred_batch documents)
    if (kind != (wire.DATA if j < DATA_SHREDS else wire.CODING) or len(data) == 0 or len(data) % 2 or
            len(data) > MAX_DATA_PER_SHRED or len(proof) != HEIGHT):
        return IMPLAUSIBLE
    # 4. ValidatedShred::try_new (validated_shred.rs:52-79)
    root = mk.derive_root(data, j, proof)                     # :57 shred.slice_root()
    msg = ed.slice_commitment(slot, si, is_last, root)        # :58
    v = _validate(msg, sig, pk, st.commitment[r])             # :60-78
    if v == ed.INVALID_SIGNATURE:
        return INVALID_SIGNATURE
    if v == ed.EQUIVOCATION:
        return EQUIVOCATION
    # 5. the receive model of deshred_batch_var: another size than the row's counts as absent
    if st.commitment[r] is not None and len(data) != st.shred_bytes[r]:
        return SIZE_MISMATCH
    # 6. BlockData::add_shred (slot_block_data.rs:202-248)
    if st.commitment[r] is None:                              # :219-221 Entry::Vacant
        st.commitment[r] = msg
        st.shred_bytes[r] = len(data)
    else:
        assert st.commitment[r] == msg                        # :215-217 cannot fire after try_new
    l = st.last_slice[w]
    if l is None:
        if is_last:                                           # :225 mark_last_slice (:269-274)
            st.last_slice[w] = si
            for i in range(si + 1, st.spp):                   # shreds.retain(ind <= slice_index)
                q = w * st.spp + i
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
