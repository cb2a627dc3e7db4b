"""Block assembly on the device: ag_block_assemble_batch (include/alpenglow_rs.h section 12)
against its sequential definition, tests/block_model.py, which restates
BlockData::try_reconstruct_block (slot_block_data.rs:376-454) over slice_oracle and
merkle_oracle.MerkleTree.

CPU: the symbol and the constants, hand-worked model cases for the decode rule and the block rule
(the reference's own tests, slot_block_data.rs:522-646, re-expressed).  GPU: every verdict in one
call with payloads written straight into a codeword buffer, the table's capacity rule, the decode
edges, the tree at capacity, two blocks end to end through shred, repair intake and deshred, the
argument errors.  Every output buffer starts at 0xA5 so stray writes show; the model is the only
checker.
"""

import os
import random
import re
import struct

import numpy as np
import pytest

import block_model as bm
import ed25519_oracle as ed
import merkle_oracle as mk
import shredder_oracle as so
import slice_oracle as sl
from alpenglow_amd import build, rs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "alpenglow_rs.h")

FILL = 0xA5
STRIDE = 32768        # one row of the codeword buffer: the least the call takes
NAMES = ("INCOMPLETE", "COMPLETE", "PARENT_SAME", "PARENT_TWICE", "BAD_TRANSACTIONS")
U64_MAX = (1 << 64) - 1
P0, P1, P2 = (11, bytes(range(32))), (12, bytes(range(1, 33))), (11, bytes(range(2, 34)))
GOOD = bm.tx_encode([b"abc", b"", b"0123456789"])
BAD = bm.tx_encode([b"abc"]) + b"\x00"


# ------------------------------------------------------------------------------ CPU

def test_symbol_declared_exported_and_callable():
    build.build()
    lib = rs.load()
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = set(re.findall(r"\b(ag_\w+)\s*\(", text))
    name = "ag_block_assemble_batch"
    assert name in declared and name in rs.EXPORTS and hasattr(lib, name)
    assert callable(rs.block_assemble_batch)
    for i, v in enumerate(NAMES):
        assert getattr(rs, "BLOCK_" + v) == i == getattr(bm, v)
        assert re.search(r"\bAG_BLOCK_%s = %d\b" % (v, i), text)
    assert re.search(r"#define\s+AG_BLOCK_MAX_TXS_PER_SLICE\s+1365\b", text)
    assert rs.BLOCK_MAX_TXS_PER_SLICE == bm.MAX_TXS_PER_SLICE == 1365


def u64(x):
    return struct.pack("<Q", x)


# (name, data, decodes under the limit 1365, decodes without a limit)
DECODE_CASES = [
    ("count 0 in exactly 8 bytes", u64(0), True, True),
    ("count 0 and one more byte", u64(0) + b"\x00", False, False),
    *[("data_len %d" % n, bytes(n), False, False) for n in range(8)],
    ("count 1, len 0", u64(1) + u64(0), True, True),
    ("count 2 with one transaction", u64(2) + u64(3) + b"abc", False, False),
    ("a transaction ending at the end", u64(1) + u64(5) + b"abcde", True, True),
    ("one byte short", u64(1) + u64(5) + b"abcd", False, False),
    ("len 2^64 - 1", u64(1) + u64(U64_MAX) + bytes(24), False, False),
    ("count 2^64 - 1", u64(U64_MAX) + u64(0) + u64(0), False, False),
    ("a length prefix cut short", u64(2) + u64(1) + b"a" + bytes(7), False, False),
    ("1365 empty transactions", u64(1365) + u64(0) * 1365, True, True),
    ("1366 empty transactions", u64(1366) + u64(0) * 1366, False, True),
]


@pytest.mark.parametrize("name,data,limited,unlimited", DECODE_CASES, ids=[c[0] for c in DECODE_CASES])
def test_model_decode_rule_by_hand(name, data, limited, unlimited):
    assert (bm.tx_decode(data, 1365) is not None) == limited
    assert (bm.tx_decode(data, 0) is not None) == unlimited


def test_model_decode_positions_by_hand():
    assert bm.tx_decode(GOOD) == [(16, 3), (27, 0), (35, 10)] and len(GOOD) == 45
    assert bm.tx_decode(bm.tx_encode([])) == []


def S(parent=None, data=GOOD, ok=True, root=None):
    return bm.Slice(ok, parent, data, root if root is not None else bytes(32))


def test_model_handover_at_slice_1_gives_the_new_parent():
    r = bm.assemble([S(P0), S(P1), S()], 2)
    assert (r.verdict, r.parent) == (bm.COMPLETE, P1)
    assert [t[0] for t in r.txs] == [0, 0, 0, 1, 1, 1, 2, 2, 2] and r.tx_bytes == 39
    assert bm.assemble([S(P0), S(), S()], 2).parent == P0


def test_model_slice_2_repeating_slice_0s_parent_is_parent_same():
    r = bm.assemble([S(P0), S(), S(P0)], 2)
    assert (r.verdict, r.error_slice, r.parent) == (bm.PARENT_SAME, 2, None)
    assert r.block_hash == mk.MerkleTree([bytes(32)] * 3).root()


def test_model_two_switches_are_parent_twice():
    r = bm.assemble([S(P0), S(P1), S(P2), S()], 3)
    assert (r.verdict, r.error_slice) == (bm.PARENT_TWICE, 2)
    # back to the original parent after a switch: still a second switch
    r = bm.assemble([S(P0), S(P1), S(), S(P0)], 3)
    assert (r.verdict, r.error_slice) == (bm.PARENT_TWICE, 3)


def test_model_second_some_equal_to_the_current_parent_is_parent_same():
    r = bm.assemble([S(P0), S(P1), S(P1)], 2)
    assert (r.verdict, r.error_slice) == (bm.PARENT_SAME, 2)
    # the slot alone differs: another parent
    assert bm.assemble([S(P0), S((P0[0] + 1, P0[1]))], 1).verdict == bm.COMPLETE


def test_model_row_0_without_a_parent_is_incomplete():
    r = bm.assemble([S(), S(P1)], 1)
    assert (r.verdict, r.block_hash) == (bm.INCOMPLETE, None)


def test_model_first_failing_slice_decides():
    r = bm.assemble([S(P0), S(data=BAD), S(P0)], 2)
    assert (r.verdict, r.error_slice) == (bm.BAD_TRANSACTIONS, 1)
    r = bm.assemble([S(P0), S(), S(P0, data=BAD)], 2)   # both in slice 2: the parent rule first
    assert (r.verdict, r.error_slice) == (bm.PARENT_SAME, 2)
    r = bm.assemble([S(P0, data=BAD), S(P0)], 1)        # slice 0 decodes too
    assert (r.verdict, r.error_slice) == (bm.BAD_TRANSACTIONS, 0)


def test_model_completeness():
    assert bm.assemble([S(P0), S()], -1).verdict == bm.INCOMPLETE
    assert bm.assemble([S(P0), S()], 2).verdict == bm.INCOMPLETE
    assert bm.assemble([S(P0), S(ok=False), S()], 2).verdict == bm.INCOMPLETE
    # rows above the last slice are ignored, whatever they hold
    r = bm.assemble([S(P0), S(), S(P0, data=BAD), S(ok=False)], 1)
    assert (r.verdict, len(r.txs)) == (bm.COMPLETE, 6)
    assert r.block_hash == mk.MerkleTree([bytes(32)] * 2).root()


def test_model_table_layout():
    res, first, total = bm.assemble_batch([[S(P0), S()], [S(), S()], [S(P0), S(P1)]], [1, 1, 0])
    assert [r.verdict for r in res] == [bm.COMPLETE, bm.INCOMPLETE, bm.COMPLETE]
    assert first == [0, 6, 6] and total == 9


# ------------------------------------------------------------------------------ GPU

torch = None


@pytest.fixture(scope="module")
def dev(ctx):
    """All torch work and every library launch go to one explicit (non-null) stream."""
    global torch
    import torch as _torch

    torch = _torch
    d = torch.device("cuda:0")
    s = torch.cuda.Stream(d)
    torch.cuda.set_stream(s)
    ctx.set_stream(s.cuda_stream)
    return d


def to_dev(a, dev):
    return torch.from_numpy(np.array(a, copy=True)).to(dev)


def filled(n, dev):
    return torch.full((n,), FILL, dtype=torch.uint8, device=dev)


def root_of(seed, r):
    return random.Random(seed * 100003 + r).randbytes(32)


class Case:
    """Blocks of model slices laid out as the deshred leaves them: the framed payload at the start
    of row r of a 0xA5 codeword buffer, the roots at offset 17 of fake 49-byte commitments.  Rows
    that are not ok carry garbage columns: the call must not look at them."""

    def __init__(self, blocks, last_slices, seed=1):
        self.blocks, self.last, self.nb, self.spb = blocks, list(last_slices), len(blocks), len(blocks[0])
        assert all(len(b) == self.spb for b in blocks)
        self.nrows = n = self.nb * self.spb
        self.cw = np.full((n, STRIDE), FILL, np.uint8)
        self.com = np.full((n, 49), FILL, np.uint8)
        self.ok = np.zeros(n, np.uint8)
        self.flags = np.zeros(n, np.uint8)
        self.ids = np.zeros((n, 40), np.uint8)
        self.offs = np.full(n, 0xA5A5A5A5, np.uint32)
        self.lens = np.full(n, 0xA5A5A5A5, np.uint32)
        for r, s in enumerate(x for b in blocks for x in b):
            s.root = root_of(seed, r)
            self.com[r, 17:] = np.frombuffer(s.root, np.uint8)
            if not s.ok:
                self.flags[r] = 0xA5
                continue
            framed = sl.payload_bytes(s.parent, s.data)
            self.cw[r, :len(framed)] = np.frombuffer(framed, np.uint8)
            self.ok[r] = 1
            self.offs[r], self.lens[r] = sl.header_len(s.parent), len(s.data)
            if s.parent is not None:
                self.flags[r] = 1
                self.ids[r] = np.frombuffer(bm.parent_bytes(s.parent), np.uint8)

    def expect(self, max_txs):
        return bm.assemble_batch(self.blocks, self.last, max_txs)


class Call:
    """One raw call of the C entry point over a Case, every output buffer 0xA5 before it.  `over`
    replaces arguments by name (the argument-error cases)."""

    ARGS = ("nblocks", "spb", "row_ok", "parent_flags", "parent_ids", "data_offsets", "data_lens", "codewords",
            "codeword_stride", "slice_roots", "roots_stride", "last_slice", "max_txs", "verdict", "error_slice",
            "parents", "tx_counts", "tx_bytes", "block_hashes", "hashes_host", "nodes", "nodes_stride", "proofs",
            "proofs_stride", "tx_offsets", "tx_lens", "tx_capacity", "tx_first", "tx_total")

    def __init__(self, ctx, dev, case, max_txs=1365, capacity=64, **over):
        nb, spb = case.nb, case.spb
        self.case, self.capacity = case, capacity
        self.nstride = 32 * rs.merkle_node_count(spb)
        self.pstride = max(32 * rs.merkle_height(spb) * spb, 16)
        self.d_cw, self.d_com = to_dev(case.cw.reshape(-1), dev), to_dev(case.com.reshape(-1), dev)
        self.d_last = to_dev(np.array(case.last, np.int32), dev)
        self.d = {"block_hashes": filled(32 * nb, dev), "nodes": filled(nb * self.nstride, dev),
                  "proofs": filled(nb * self.pstride, dev), "tx_offsets": filled(8 * max(capacity, 1), dev),
                  "tx_lens": filled(4 * max(capacity, 1), dev)}
        self.h = {"verdict": np.full(nb, FILL, np.uint8), "error_slice": np.full(nb, 0xA5A5A5A5, np.uint32),
                  "parents": np.full((nb, 40), FILL, np.uint8), "tx_counts": np.full(nb, 0xA5A5A5A5, np.uint32),
                  "tx_bytes": np.full(nb, 0xA5A5A5A5A5A5A5A5, np.uint64),
                  "hashes_host": np.full((nb, 32), FILL, np.uint8),
                  "tx_first": np.full(nb, 0xA5A5A5A5A5A5A5A5, np.uint64),
                  "tx_total": np.full(1, 0xA5A5A5A5A5A5A5A5, np.uint64)}
        a = {"nblocks": nb, "spb": spb, "row_ok": case.ok.ctypes.data, "parent_flags": case.flags.ctypes.data,
             "parent_ids": case.ids.ctypes.data, "data_offsets": case.offs.ctypes.data,
             "data_lens": case.lens.ctypes.data, "codewords": self.d_cw.data_ptr(), "codeword_stride": STRIDE,
             "slice_roots": self.d_com.data_ptr() + 17, "roots_stride": 49, "last_slice": self.d_last.data_ptr(),
             "max_txs": max_txs, "nodes_stride": self.nstride, "proofs_stride": self.pstride,
             "tx_capacity": capacity}
        a.update({k: v.data_ptr() for k, v in self.d.items()})
        a.update({k: v.ctypes.data for k, v in self.h.items()})
        for k, v in over.items():   # "+8" / "-16": relative to this call's own argument
            a[k] = a[k] + int(v) if isinstance(v, str) else v
        self.args = a
        self.status = rs.load().ag_block_assemble_batch(ctx.handle, *(a[k] for k in self.ARGS))
        torch.cuda.synchronize()
        self.out = {k: v.cpu().numpy() for k, v in self.d.items()}
        assert np.array_equal(self.d_cw.cpu().numpy().reshape(case.cw.shape), case.cw), "codewords were written"

    def untouched(self):
        return all((v.view(np.uint8) == FILL).all() for v in list(self.out.values()) + list(self.h.values()))

    def snapshot(self, table=True):
        """Every output but (table = False) the transaction table."""
        keep = {k: v for k, v in self.out.items() if table or not k.startswith("tx_")}
        return {**{k: v.copy() for k, v in keep.items()}, **{k: v.copy() for k, v in self.h.items()}}

    def check(self, max_txs=1365, table=True):
        """Every output against the model."""
        case, h, out = self.case, self.h, self.out
        res, first, total = case.expect(max_txs)
        assert self.status == 0
        assert [NAMES[v] for v in h["verdict"]] == [NAMES[r.verdict] for r in res]
        assert h["error_slice"].tolist() == [r.error_slice for r in res]
        assert h["tx_counts"].tolist() == [len(r.txs) for r in res]
        assert h["tx_bytes"].tolist() == [r.tx_bytes for r in res]
        assert h["tx_first"].tolist() == first and int(h["tx_total"][0]) == total
        hashes = out["block_hashes"].reshape(-1, 32)
        nodes, proofs = out["nodes"].reshape(case.nb, -1), out["proofs"].reshape(case.nb, -1)
        for b, r in enumerate(res):
            want = bm.parent_bytes(r.parent) if r.verdict == bm.COMPLETE else bytes(40)
            assert h["parents"][b].tobytes() == want, b
            if r.verdict == bm.INCOMPLETE:
                assert (hashes[b] == FILL).all() and (h["hashes_host"][b] == FILL).all(), b
                assert (nodes[b] == FILL).all() and (proofs[b] == FILL).all(), b
                continue
            t = r.tree
            assert hashes[b].tobytes() == r.block_hash == h["hashes_host"][b].tobytes() == t.root(), b
            want = b"".join(t.nodes)
            assert nodes[b, :len(want)].tobytes() == want and (nodes[b, len(want):] == FILL).all(), b
            want = b"".join(b"".join(t.create_proof(j)) for j in range(len(t.nodes[:t.levels[0][1]])))
            assert proofs[b, :len(want)].tobytes() == want and (proofs[b, len(want):] == FILL).all(), b
        offs, lens = out["tx_offsets"].view(np.uint64), out["tx_lens"].view(np.uint32)
        if not table or total > self.capacity:
            assert (out["tx_offsets"] == FILL).all() and (out["tx_lens"] == FILL).all()
            return
        want_offs, want_lens = [], []
        for b, r in enumerate(res):
            for i, off, length in r.txs:
                row = b * case.spb + i
                want_offs.append(row * STRIDE + int(case.offs[row]) + off)
                want_lens.append(length)
        assert offs[:total].tolist() == want_offs and lens[:total].tolist() == want_lens
        assert (out["tx_offsets"][8 * total:] == FILL).all() and (out["tx_lens"][4 * total:] == FILL).all()
        flat = case.cw.reshape(-1)   # and the entries lead to the transactions
        at = 0
        for b, r in enumerate(res):
            for i, off, length in r.txs:
                assert flat[want_offs[at]:want_offs[at] + length].tobytes() == case.blocks[b][i].data[off:off + length]
                at += 1


def direct_case():
    """Six blocks of four rows: every verdict, a one-slice block, rows above the last slice."""
    txs = lambda *sizes: bm.tx_encode([bytes([(7 + n) % 256]) * n for n in sizes])  # noqa: E731
    blocks = [
        [S(P0, txs(1, 0, 300)), S(P1, txs()), S(None, txs(512, 2)), S(None, txs(5))],       # COMPLETE, handed over
        [S(P0), S(None), S(P0), S(P1)],                                                        # PARENT_SAME at 2
        [S(P0), S(P1), S(None, BAD), S(P0)],                                                   # BAD at 2 before TWICE at 3
        [S(P0, txs(9)), S(P2, BAD, ok=False), S(P0, BAD), S(ok=False)],                         # one slice; rest ignored
        [S(P0), S(ok=False), S(), S()],                                                        # a hole: INCOMPLETE
        [S(P0), S(P1), S(P2), S(P2, BAD)],                                                     # PARENT_TWICE at 2
    ]
    return Case(blocks, [3, 3, 3, 0, 2, 3], seed=2)


@pytest.fixture(scope="module")
def direct(ctx, dev):
    case = direct_case()
    return case, Call(ctx, dev, case)


@pytest.mark.gpu
def test_direct_every_verdict(direct):
    case, call = direct
    res, first, total = case.expect(1365)
    assert [r.verdict for r in res] == [bm.COMPLETE, bm.PARENT_SAME, bm.BAD_TRANSACTIONS, bm.COMPLETE,
                                        bm.INCOMPLETE, bm.PARENT_TWICE]
    assert [r.error_slice for r in res] == [0, 2, 2, 0, 0, 2] and res[0].parent == P1
    assert first == [0, 6, 6, 6, 7, 7] and total == 7
    call.check()


@pytest.mark.gpu
def test_direct_other_shapes_of_incomplete(ctx, dev):
    """No last slice, a last slice past the rows, row 0 without a parent; hashes only."""
    blocks = [[S(P0), S()], [S(P0), S()], [S(), S(P1)], [S(P0), S(P1)]]
    case = Case(blocks, [-1, 2, 1, 1], seed=3)
    call = Call(ctx, dev, case, nodes=None, proofs=None, tx_offsets=None, tx_lens=None, hashes_host=None)
    res, _, total = case.expect(1365)
    assert [r.verdict for r in res] == [bm.INCOMPLETE] * 3 + [bm.COMPLETE] and total == 6
    assert call.status == 0 and call.h["verdict"].tolist() == [0, 0, 0, 1]
    assert call.h["tx_first"].tolist() == [0, 0, 0, 0] and int(call.h["tx_total"][0]) == 6
    hashes = call.out["block_hashes"].reshape(-1, 32)
    assert (hashes[:3] == FILL).all() and hashes[3].tobytes() == res[3].block_hash
    assert all((call.out[k] == FILL).all() for k in ("nodes", "proofs", "tx_offsets", "tx_lens"))
    assert (call.h["hashes_host"] == FILL).all()


@pytest.mark.gpu
def test_capacity_one_short_writes_no_entry(ctx, dev, direct):
    case, full = direct
    short = Call(ctx, dev, case, capacity=7 - 1)
    short.check()   # (the table all 0xA5: check() knows the capacity)
    a, b = full.snapshot(table=False), short.snapshot(table=False)
    assert a.keys() == b.keys() and all(np.array_equal(a[k], b[k]) for k in a)
    exact = Call(ctx, dev, case, capacity=7)
    exact.check()
    # a pure function of its inputs: again on the same context
    again = Call(ctx, dev, case)
    a, b = full.snapshot(), again.snapshot()
    assert all(np.array_equal(a[k], b[k]) for k in a)


@pytest.mark.gpu
@pytest.mark.parametrize("max_txs", [1365, 0])
def test_decode_edges_on_the_device(ctx, dev, max_txs):
    """Block 0: the CPU list as its slices (the first failing one decides); then one block per
    case, the case behind a good slice 0."""
    datas = [c[1] for c in DECODE_CASES]
    n = len(datas)
    blocks = [[S(P0 if i == 0 else None, d) for i, d in enumerate(datas)]]
    last = [n - 1]
    for d in datas:
        blocks.append([S(P0), S(None, d)] + [S(ok=False) for _ in range(n - 2)])
        last.append(1)
    case = Case(blocks, last, seed=4)
    res, _, total = case.expect(max_txs)
    want = [c[2] if max_txs else c[3] for c in DECODE_CASES]
    assert [r.verdict == bm.COMPLETE for r in res[1:]] == want
    assert (res[0].verdict, res[0].error_slice) == (bm.BAD_TRANSACTIONS, 1)
    call = Call(ctx, dev, case, max_txs=max_txs, capacity=total + 3)
    call.check(max_txs)


@pytest.mark.gpu
def test_tree_at_capacity(ctx, dev):
    """1024 slices of one empty transaction each, and 513 (odd at every level) of 1024 rows."""
    one = bm.tx_encode([b""])
    assert len(one) == 16
    blocks = [[S(P0 if i == 0 else None, one) for i in range(1024)] for _ in range(2)]
    case = Case(blocks, [1023, 512], seed=5)
    call = Call(ctx, dev, case, capacity=1024 + 513)
    res, first, total = case.expect(1365)
    assert [r.tree.height() for r in res] == [10, 10] and (first, total) == ([0, 1024], 1537)
    call.check()


@pytest.mark.gpu
def test_end_to_end_small(ctx, dev):
    """Two blocks of three slices through shred, repair intake, deshred and the assembly; slice 1
    of block 0 hands over."""
    rng = random.Random(0xB10C)
    seed = bytes(range(7, 39))
    pk = ed.secret_to_public(seed)
    slots, sizes, spb, pkt = [41, 42], [2, 24, 1000, 1000, 2, 24], 3, 1536
    parents = [P0, P1, None, P2, None, None]

    def data_for(S_, parent):
        """Transaction framing whose framed slice pads to shred size S_."""
        lo, hi = max(32 * S_ - 64, sl.header_len(parent) + 8), min(32 * S_ - 1, sl.MAX_DATA_PER_SLICE)
        left, txs = rng.randrange(lo, hi + 1) - sl.header_len(parent) - 8, []
        if left < 8:
            left = 0   # (only the smallest size: no room for a prefix)
        while left >= 8:
            n = min(rng.randrange(0, 200), left - 8)
            if left - 8 - n < 8:
                n = left - 8
            txs.append(rng.randbytes(n))
            left -= 8 + n
        assert left == 0
        return bm.tx_encode(txs)

    slices, stream, roots = [], [], []
    for r, S_ in enumerate(sizes):
        b, si = divmod(r, spb)
        data = data_for(S_, parents[r])
        pkts, _, root, _ = so.shred(parents[r], data, slots[b], si, si == spb - 1, seed)
        slices.append(bm.Slice(True, parents[r], data, root))
        roots.append(root)
        stream += [(pkts[j], b, si, j) for j in sorted(rng.sample(range(64), 40))]
    rng.shuffle(stream)
    n, nrows = len(stream), 6
    rx, ln = np.full((n, pkt), FILL, np.uint8), np.zeros(n, np.int32)
    for t, (p, *_) in enumerate(stream):
        rx[t, :len(p)], ln[t] = np.frombuffer(p, np.uint8), len(p)
    req = [to_dev(np.array([x[k] for x in stream], np.uint32), dev) for k in (1, 2, 3)]
    packets, lens = torch.zeros((64 * nrows, pkt), dtype=torch.uint8, device=dev), torch.zeros(
        64 * nrows, dtype=torch.int32, device=dev)
    commitments, signatures = filled(49 * nrows, dev), filled(64 * nrows, dev)
    shred_bytes = torch.zeros(nrows, dtype=torch.int32, device=dev)
    last_slice = torch.full((2,), -1, dtype=torch.int32, device=dev)
    d_pk = to_dev(np.frombuffer(pk, np.uint8), dev)
    sb, counts = rs.repair_intake_batch(ctx, slots, to_dev(np.frombuffer(pk * 2, np.uint8), dev), spb, n,
                                        to_dev(rx, dev), pkt, to_dev(ln, dev), *req,
                                        to_dev(np.frombuffer(b"".join(roots), np.uint8), dev),
                                        to_dev(np.ones(nrows, np.uint8), dev), packets, pkt, lens, commitments,
                                        signatures, shred_bytes, last_slice, filled(n, dev))
    assert sb.tolist() == sizes and counts.tolist() == [40] * nrows
    stride = 64 * 1024
    cw = filled(nrows * stride, dev)
    de = rs.shredder_deshred_batch_var(ctx, nrows, sb, packets, pkt, lens, d_pk, cw, stride)
    assert de.status.tolist() == [0] * nrows
    cap = 4096
    hashes, tx_offsets, tx_lens = filled(64, dev), filled(8 * cap, dev), filled(4 * cap, dev)
    got = rs.block_assemble_batch(ctx, 2, spb, de.status == 0, de.parents, de.data_offsets, de.data_lens, cw, stride,
                                  commitments[17:], 49, last_slice, hashes, tx_offsets=tx_offsets, tx_lens=tx_lens,
                                  tx_capacity=cap)
    torch.cuda.synchronize()
    res, first, total = bm.assemble_batch([slices[:3], slices[3:]], [2, 2])
    assert [r.verdict for r in res] == [bm.COMPLETE] * 2 and res[0].parent == P1 and res[1].parent == P2
    assert got.verdict.tolist() == [rs.BLOCK_COMPLETE] * 2 and got.parents == [P1, P2]
    assert got.tx_counts.tolist() == [len(r.txs) for r in res] and got.tx_bytes.tolist() == [r.tx_bytes for r in res]
    assert got.tx_first.tolist() == first and got.tx_total == total <= cap
    tree = filled(64, dev)
    rs.block_tree_batch(ctx, 2, [3, 3], to_dev(np.frombuffer(b"".join(roots), np.uint8), dev), tree)
    torch.cuda.synchronize()
    for b, r in enumerate(res):
        assert got.hashes[b].tobytes() == r.block_hash == hashes.cpu().numpy()[32 * b:32 * b + 32].tobytes()
        assert tree.cpu().numpy()[32 * b:32 * b + 32].tobytes() == r.block_hash
    flat = cw.cpu().numpy()
    offs, tl = tx_offsets.cpu().numpy().view(np.uint64), tx_lens.cpu().numpy().view(np.uint32)
    at = 0
    for b, r in enumerate(res):
        for i, off, length in r.txs:
            assert tl[at] == length
            assert flat[int(offs[at]):int(offs[at]) + length].tobytes() == slices[3 * b + i].data[off:off + length]
            at += 1
    assert (offs[total:].view(np.uint8) == FILL).all()


def _errors(case):
    """(label, overrides): each alone makes the call an INVALID_ARGUMENT."""
    bad_off, bad_len, bad_flag = case.offs.copy(), case.lens.copy(), case.flags.copy()
    bad_off[0] = 9                               # row 0 carries a parent: 49
    bad_len[1] = sl.MAX_DATA_PER_SLICE - 9 + 1   # offset 9: one byte past the payload limit
    bad_flag[1] = 2
    out = [("%s null" % k, {k: None}) for k in ("row_ok", "parent_flags", "parent_ids", "data_offsets", "data_lens",
                                                "codewords", "slice_roots", "last_slice", "verdict", "error_slice",
                                                "parents", "tx_counts", "tx_bytes", "block_hashes", "tx_first",
                                                "tx_total")]
    out += [("spb 0", {"spb": 0}), ("spb 1025", {"spb": 1025}), ("nrows 2^24", {"nblocks": 1 << 22}),
            ("codewords + 8", {"codewords": "+8"}), ("codeword_stride + 8", {"codeword_stride": STRIDE + 8}),
            ("codeword_stride 16384", {"codeword_stride": 16384}), ("roots_stride 31", {"roots_stride": 31}),
            ("block_hashes + 8", {"block_hashes": "+8"}), ("nodes + 8", {"nodes": "+8"}),
            ("proofs + 8", {"proofs": "+8"}), ("nodes_stride + 8", {"nodes_stride": "+8"}),
            ("proofs_stride + 8", {"proofs_stride": "+8"}), ("nodes_stride short", {"nodes_stride": "-16"}),
            ("proofs_stride short", {"proofs_stride": "-16"}), ("proofs without nodes", {"nodes": None}),
            ("tx_lens alone", {"tx_offsets": None}), ("tx_offsets alone", {"tx_lens": None}),
            ("offset 9 with a parent", {"data_offsets": bad_off.ctypes.data}),
            ("data past the payload limit", {"data_lens": bad_len.ctypes.data}),
            ("parent flag 2", {"parent_flags": bad_flag.ctypes.data})]
    return out, (bad_off, bad_len, bad_flag)


@pytest.mark.gpu
def test_argument_errors(ctx, dev, direct):
    case, good = direct
    cases, keep = _errors(case)
    for label, over in cases:
        call = Call(ctx, dev, case, **over)
        assert call.status == 100, label
        assert call.untouched(), label
    lib = rs.load()
    assert lib.ag_block_assemble_batch(None, *(good.args[k] for k in Call.ARGS)) == 100
    # no blocks: nothing to do
    call = Call(ctx, dev, case, nblocks=0)
    assert call.status == 0 and int(call.h["tx_total"][0]) == 0
    call.h["tx_total"][0] = 0xA5A5A5A5A5A5A5A5
    assert call.untouched()
    del keep
