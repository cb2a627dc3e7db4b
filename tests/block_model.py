"""The sequential definition of ag_block_assemble_batch (include/alpenglow_rs.h section 12) --
TEST INFRASTRUCTURE ONLY: the checker of tests/test_block_assemble.py, never the product path.

BlockData::try_reconstruct_block (slot_block_data.rs:376-454), one block at a time over its
reconstructed slices, composed from the existing oracles (slice_oracle for the framing,
merkle_oracle.MerkleTree for the double-Merkle tree):

  slot_block_data.rs:382-388  last slice known and every slice up to it present, else NoAction
  slot_block_data.rs:361-364  a first slice without a parent was never inserted
  slot_block_data.rs:390-394  DoubleMerkleTree::new(slice roots).get_root(), before anything fails
  slot_block_data.rs:401-423  the optimistic handover: one switch, to another parent
  slot_block_data.rs:426-435  deserialize_exact::<Vec<Transaction>> per slice

wincode's encoding of Vec<Transaction(Vec<u8>)> (fixed-width little-endian u64 lengths) and its
preallocation limit are recalled, as slice_oracle recalls the framing: the crate is not vendored.
"""

from __future__ import annotations

import struct
from dataclasses import dataclass, field

import merkle_oracle as mk
import slice_oracle as so

INCOMPLETE, COMPLETE, PARENT_SAME, PARENT_TWICE, BAD_TRANSACTIONS = range(5)
MAX_TXS_PER_SLICE = so.MAX_DATA_PER_SLICE // 24  # n * size_of::<Transaction>() <= MAX_DATA_PER_SLICE
assert MAX_TXS_PER_SLICE == 1365
U64_MAX = (1 << 64) - 1


def tx_encode(txs, count=None) -> bytes:
    """wincode::serialize(&Vec<Transaction>): u64 count, then (u64 length, bytes) per transaction.
    count overrides the prefix (malformed inputs)."""
    out = [struct.pack("<Q", len(txs) if count is None else count)]
    for t in txs:
        out.append(struct.pack("<Q", len(t)))
        out.append(bytes(t))
    return b"".join(out)


def tx_decode(data: bytes, max_txs: int = MAX_TXS_PER_SLICE):
    """deserialize_exact::<Vec<Transaction>>: the list of (offset, length) of the transactions'
    payloads inside data, or None where the decode fails.  max_txs = 0: no limit."""
    if len(data) < 8:
        return None
    n = struct.unpack_from("<Q", data, 0)[0]
    if max_txs and n > max_txs:
        return None
    pos, out = 8, []
    while len(out) < n:
        if len(data) - pos < 8:
            return None
        length = struct.unpack_from("<Q", data, pos)[0]
        pos += 8
        if length > len(data) - pos:
            return None
        out.append((pos, length))
        pos += length
    return out if pos == len(data) else None


@dataclass
class Slice:
    """One row: ok = the slice is in BlockData::slices; parent None or (slot, 32-byte hash)."""
    ok: bool = True
    parent: object = None
    data: bytes = b""
    root: bytes = bytes(32)


@dataclass
class Result:
    verdict: int
    error_slice: int = 0
    parent: object = None          # COMPLETE only
    block_hash: object = None      # every verdict but INCOMPLETE
    tree: object = None            # likewise: the MerkleTree over the slice roots
    txs: list = field(default_factory=list)  # COMPLETE only: (slice, offset in its data, length)

    @property
    def tx_bytes(self) -> int:
        return sum(t[2] for t in self.txs)


def parent_bytes(parent) -> bytes:
    return struct.pack("<Q", parent[0]) + bytes(parent[1])


def assemble(slices, last_slice: int, max_txs: int = MAX_TXS_PER_SLICE) -> Result:
    """One block: `slices` are its slices_per_block rows, last_slice the store's (-1 = none)."""
    if last_slice < 0 or last_slice >= len(slices):
        return Result(INCOMPLETE)
    mine = slices[: last_slice + 1]  # mark_last_slice pruned the rest
    if not all(s.ok for s in mine) or mine[0].parent is None:
        return Result(INCOMPLETE)
    tree = mk.MerkleTree([s.root for s in mine])
    failed = lambda verdict, i: Result(verdict, i, block_hash=tree.root(), tree=tree)  # noqa: E731
    parent, switched, txs = mine[0].parent, False, []
    for i, s in enumerate(mine):
        if i > 0 and s.parent is not None:
            if parent_bytes(s.parent) == parent_bytes(parent):
                return failed(PARENT_SAME, i)
            if switched:
                return failed(PARENT_TWICE, i)
            switched, parent = True, s.parent
        found = tx_decode(s.data, max_txs)
        if found is None:
            return failed(BAD_TRANSACTIONS, i)
        txs += [(i, off, length) for off, length in found]
    return Result(COMPLETE, 0, parent, tree.root(), tree, txs)


def assemble_batch(blocks, last_slices, max_txs: int = MAX_TXS_PER_SLICE):
    """Every block, then the table's layout: (results, tx_first per block, total)."""
    results = [assemble(b, l, max_txs) for b, l in zip(blocks, last_slices)]
    first, at = [], 0
    for r in results:
        first.append(at)
        at += len(r.txs)
    return results, first, at
