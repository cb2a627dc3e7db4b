"""Repair intake on the device: ag_repair_intake_batch (include/alpenglow_rs.h section 11) against
its sequential definition, tests/repair_model.py, which restates the reference's
RepairResponse::Shred handling (repair.rs:410-445, slot_block_data.rs:101-113, :202-274) over
the existing oracles.

CPU: the symbol, hand-worked model cases for every rule that differs from the dissemination
intake.  GPU: an honest catch-up over three blocks (two of one slot, one of another leader) with
the deshred and the block hashes behind it, the same stream in chunks, an adversarial stream in
one call and cut in two, the argument errors.  Buffers start at 0xA5 so stray writes show.
"""

import os
import random
import re

import numpy as np
import pytest

import ed25519_oracle as ed
import intake_model as im
import merkle_oracle as mk
import repair_model as rm
import rs_oracle as o
import shred_wire_oracle as wire
import shredder_oracle as so
import slice_oracle as sl
from alpenglow_amd import build, rs
from test_shredder_intake import make_slice, resign, tamper

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "alpenglow_rs.h")

FILL = 0xA5
PKT = 1536            # stride of the store's slots and of the receive rows
STRIDE = 64 * 1024    # one slice's codeword region (the deshred behind the intake)
SEED_A, SEED_B = bytes(range(7, 39)), bytes(range(60, 92))
OTHER_SEED = bytes(range(100, 132))   # nobody's leader

SLOT_X, SLOT_Y = 7_000_001, 12
BLOCK_SLOTS = [SLOT_X, SLOT_X, SLOT_Y]     # blocks 0 and 1: one slot, two hashes
SEEDS = [SEED_A, SEED_A, SEED_B]
PKS = [ed.secret_to_public(s) for s in SEEDS]
SPB = 3
SIZES = [2, 24, 1000, 1010, 1024, 1000, 2, 1024, 24]   # row r's shred size
NAMES = ("STORED", "MALFORMED", "OUT_OF_WINDOW", "IMPLAUSIBLE", "INVALID_SIGNATURE", "EQUIVOCATION", "SIZE_MISMATCH",
         "DUPLICATE", "PRUNED", "REQUEST_MISMATCH", "NO_ROOT", "WRONG_ROOT")


def relast(pkt, seed):
    """The datagram with is_last flipped and the signature `seed`'s over that commitment: the
    same slice root, another commitment."""
    kind, slot, si, last, j, data, _, proof = wire.deserialize(pkt)
    sig = ed.sign(seed, ed.slice_commitment(slot, si, not last, mk.derive_root(data, j, proof)))
    return wire.serialize(kind, slot, si, not last, j, data, sig, proof)


def root_of(pkt):
    _, _, _, _, j, data, _, proof = wire.deserialize(pkt)
    return mk.derive_root(data, j, proof)


def mixed_slice(rng, slot, si, seed):
    """The 64 datagrams of a slice whose leader signed a tree over leaves of 24 and (leaf 3) 26 bytes."""
    raw = o.coder_shred(sl.payload_bytes(None, rng.randbytes(700)), 32)
    shards = list(raw.data) + list(raw.coding)
    assert len(shards[0]) == 24
    shards[3] += b"\x11\x22"
    return so.datagrams(shards[:32], shards[32:], slot, si, False, seed)[0]


# ------------------------------------------------------------------------------ CPU

def test_symbol_declared_exported_and_callable():
    build.build()
    lib = rs.load()
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = set(re.findall(r"\b(ag_\w+)\s*\(", text))
    name = "ag_repair_intake_batch"
    assert name in declared and name in rs.EXPORTS and hasattr(lib, name)
    assert callable(rs.repair_intake_batch)
    for i, v in enumerate(NAMES):
        assert getattr(rs, "INTAKE_" + v) == i == getattr(rm, v)
        assert re.search(r"\bAG_INTAKE_%s = %d\b" % (v, i), text)
    assert [rs.INTAKE_REQUEST_MISMATCH, rs.INTAKE_NO_ROOT, rs.INTAKE_WRONG_ROOT] == [9, 10, 11]
    assert rs.REPAIR_VERDICTS[9:] == ("request_mismatch", "no_root", "wrong_root")


@pytest.fixture(scope="module")
def hand():
    """Two blocks of slot 5 (leader A) and one of slot 9 (leader B), three slices of shred size 2
    each; of slices 1 and 2 of the slot-5 blocks the is_last version as well.  Datagrams 0..3."""
    rng = random.Random(0x4E9A)
    v = {}
    for b, (slot, seed) in enumerate([(5, SEED_A), (5, SEED_A), (9, SEED_B)]):
        for si in range(3):
            s_ = make_slice(rng, 2, slot, si, False)
            v[b, si] = so.shred(*s_, seed)[0][:4]
            if b < 2 and si:
                v[b, si, "last"] = so.shred(*(s_[:4] + (True,)), seed)[0][:4]
    return v


def hand_store(v, proved=True):
    st = rm.Store([5, 5, 9], [PKS[0], PKS[0], PKS[2]], 3)
    if proved:
        st.roots = [root_of(v[r // 3, r % 3][0]) for r in range(9)]
    return st


def test_model_request_mismatch_by_hand(hand):
    v, st = hand, hand_store(hand)
    M, S = rm.REQUEST_MISMATCH, rm.STORED
    p = v[0, 1][3]   # slot 5, slice 1, shred 3
    got = rm.intake(st, [(p, 2, 1, 3),     # asked of the slot-9 block: the slot
                         (p, 0, 2, 3),     # the slice index
                         (p, 0, 1, 2),     # the shred index
                         (p, 0, 1, 3)])
    assert got == [M, M, M, S]
    # the request names no row at all: before the header is looked at
    assert rm.intake(st, [(p, 3, 1, 3), (p, 0, 3, 3), (p, 0, 1, 64)]) == [rm.OUT_OF_WINDOW] * 3
    assert st.counts() == [0, 1, 0, 0, 0, 0, 0, 0, 0]


def test_model_roots_by_hand(hand):
    v = hand
    st = hand_store(v, proved=False)
    known = len(im._verified)
    assert rm.intake(st, [(v[0, 0][1], 0, 0, 1)]) == [rm.NO_ROOT]
    st = hand_store(v)
    # a payload byte altered: another root, and no signature is consulted (repair.rs:428-432)
    assert rm.intake(st, [(tamper(v[0, 0][1], 37), 0, 0, 1)]) == [rm.WRONG_ROOT]
    # the right coordinates, the other block of the slot
    assert rm.intake(st, [(v[1, 0][1], 0, 0, 1)]) == [rm.WRONG_ROOT]
    assert len(im._verified) == known and st.commitment == [None] * 9
    assert rm.intake(st, [(v[0, 0][1], 0, 0, 1), (v[1, 0][1], 1, 0, 1)]) == [rm.STORED] * 2


def test_model_signature_always_checked_by_hand(hand):
    v = hand
    stream = [v[0, 0][1], resign(v[0, 0][2], OTHER_SEED), resign(v[0, 0][1], OTHER_SEED), v[0, 0][2]]
    # dissemination: the row's commitment is accepted unverified (validated_shred.rs:62-64)
    d = im.Store([5], 3)
    assert im.intake(d, stream, PKS[0]) == [im.STORED, im.STORED, im.DUPLICATE, im.DUPLICATE]
    # repair: try_new(shred, None, pk) checks it every time (repair.rs:433-437)
    st = hand_store(v)
    got = rm.intake(st, [(p, 0, 0, j) for p, j in zip(stream, (1, 2, 1, 2))])
    assert got == [rm.STORED, rm.INVALID_SIGNATURE, rm.INVALID_SIGNATURE, rm.STORED]
    assert st.slots[0][2] == v[0, 0][2] and st.signature[0] == wire.deserialize(v[0, 0][1])[6]
    # the wrong block's leader: block 2's shred re-signed by leader A
    assert rm.intake(st, [(resign(v[2, 0][0], SEED_A), 2, 0, 0), (v[2, 0][0], 2, 0, 0)]) == \
        [rm.INVALID_SIGNATURE, rm.STORED]


def test_model_equivocation_and_size_by_hand(hand):
    v, st = hand, hand_store(hand)
    # the same proved root, is_last flipped, signed by the leader: another commitment
    flipped = relast(v[0, 0][2], SEED_A)
    assert root_of(flipped) == st.roots[0]
    assert rm.intake(st, [(v[0, 0][1], 0, 0, 1), (flipped, 0, 0, 2), (v[0, 0][2], 0, 0, 2)]) == \
        [rm.STORED, rm.EQUIVOCATION, rm.STORED]
    # a tree over leaves of sizes 24 and 26, signed by the leader
    m = mixed_slice(random.Random(0x517E), 5, 1, SEED_A)
    st.roots[1] = root_of(m[0])
    assert root_of(m[3]) == st.roots[1]
    assert rm.intake(st, [(m[0], 0, 1, 0), (m[3], 0, 1, 3), (m[33], 0, 1, 33)]) == \
        [rm.STORED, rm.SIZE_MISMATCH, rm.STORED]
    assert st.shred_bytes[:2] == [2, 24]
    # ... whose first arrival is the odd leaf: its size becomes the row's
    st = hand_store(v)
    st.roots[1] = root_of(m[0])
    assert rm.intake(st, [(m[3], 0, 1, 3), (m[0], 0, 1, 0)]) == [rm.STORED, rm.SIZE_MISMATCH]
    assert st.shred_bytes[1] == 26


def test_model_last_slice_per_block_by_hand(hand):
    v, st = hand, hand_store(hand)
    S, E, P, D = rm.STORED, rm.EQUIVOCATION, rm.PRUNED, rm.DUPLICATE
    got = rm.intake(st, [(v[0, 2][0], 0, 2, 0),            # block 0 slice 2 stored ...
                         (v[1, 2][0], 1, 2, 0),            # ... and block 1's, the same slot
                         (v[0, 1, "last"][0], 0, 1, 0),    # block 0 marks slice 1 last: its slice 2 is pruned
                         (v[0, 2][1], 0, 2, 1),            # beyond block 0's last slice
                         (v[1, 2][1], 1, 2, 1),            # block 1 has no last slice
                         (v[1, 2, "last"][2], 1, 2, 2),    # (its cache is the plain version)
                         (v[1, 2][0], 1, 2, 0)])
    assert got == [P, S, S, E, S, E, D]
    assert st.last_slice == [1, None, None]
    assert st.counts() == [0, 1, 0, 0, 0, 2, 0, 0, 0] and st.commitment[2] is not None
    # across calls: block 1 marks its slice 1; the stored slice 2 goes, the verdicts given stay
    assert rm.intake(st, [(v[1, 1, "last"][3], 1, 1, 3)]) == [S]
    assert st.last_slice == [1, 1, None] and st.counts() == [0, 1, 0, 0, 1, 0, 0, 0, 0]


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


def filled(shape, dev):
    return torch.full(shape if isinstance(shape, tuple) else (shape,), FILL, dtype=torch.uint8, device=dev)


class DevStore:
    """The caller-owned store on the device, 0xA5 where the call must not write, with the proved
    roots (None = not proved) and the blocks' keys."""

    def __init__(self, dev, roots):
        self.dev, self.nrows = dev, len(BLOCK_SLOTS) * SPB
        self.packets = filled((64 * self.nrows, PKT), dev)
        self.lens = torch.zeros(64 * self.nrows, dtype=torch.int32, device=dev)
        self.commitments = filled(49 * self.nrows, dev)
        self.signatures = filled(64 * self.nrows, dev)
        self.shred_bytes = torch.zeros(self.nrows, dtype=torch.int32, device=dev)
        self.last_slice = torch.full((len(BLOCK_SLOTS),), -1, dtype=torch.int32, device=dev)
        self.pks = to_dev(np.frombuffer(b"".join(PKS), np.uint8), dev)
        rows = np.full((self.nrows, 32), FILL, np.uint8)
        for r, x in enumerate(roots):
            if x is not None:
                rows[r] = np.frombuffer(x, np.uint8)
        self.roots = to_dev(rows, dev)
        self.have_root = to_dev(np.array([x is not None for x in roots], np.uint8), dev)

    def feed(self, ctx, replies):
        """One call: (verdicts, shred_bytes_out, counts_out); rx must come back unchanged."""
        n = len(replies)
        rx = np.full((max(n, 1), PKT), FILL, np.uint8)
        ln = np.zeros(max(n, 1), np.int32)
        req = np.zeros((3, max(n, 1)), np.uint32)
        for t, (p, b, s, i) in enumerate(replies):
            rx[t, :len(p)] = np.frombuffer(p, np.uint8)
            ln[t] = len(p)
            req[:, t] = (b, s, i)
        d_rx, d_ln, verdict = to_dev(rx, self.dev), to_dev(ln, self.dev), filled(max(n, 1), self.dev)
        d_req = [to_dev(req[k], self.dev) for k in range(3)]
        sizes, counts = rs.repair_intake_batch(ctx, BLOCK_SLOTS, self.pks, SPB, n, d_rx, PKT, d_ln, *d_req, self.roots,
                                               self.have_root, self.packets, PKT, self.lens, self.commitments,
                                               self.signatures, self.shred_bytes, self.last_slice, verdict)
        torch.cuda.synchronize()
        assert np.array_equal(d_rx.cpu().numpy(), rx), "rx was written"
        return verdict.cpu().numpy()[:n].tolist(), sizes.tolist(), counts.tolist()

    def host(self):
        return (self.packets.cpu().numpy(), self.lens.cpu().numpy(), self.commitments.cpu().numpy().reshape(-1, 49),
                self.signatures.cpu().numpy().reshape(-1, 64), self.shred_bytes.cpu().numpy(),
                self.last_slice.cpu().numpy())


def names(verdicts):
    return [rs.REPAIR_VERDICTS[v] if v < len(rs.REPAIR_VERDICTS) else v for v in verdicts]


def new_model(roots):
    model = rm.Store(BLOCK_SLOTS, PKS, SPB)
    model.roots = list(roots)
    return model


def check_store(store: DevStore, model: rm.Store, sizes=None, counts=None):
    """Every byte of the device store against the model's."""
    buf, ln, com, sig, sb, last = store.host()
    assert last.tolist() == [-1 if x is None else x for x in model.last_slice]
    assert sb.tolist() == model.shred_bytes
    if sizes is not None:
        assert sizes == model.shred_bytes and counts == model.counts()
    for r in range(model.nrows):
        if model.commitment[r] is None:
            assert (com[r] == FILL).all() and (sig[r] == FILL).all(), r
        else:
            assert com[r].tobytes() == model.commitment[r] and sig[r].tobytes() == model.signature[r], r
        l = model.last_slice[r // model.spb]
        pruned = l is not None and r % model.spb > l   # (bytes of pruned rows are unspecified)
        for j in range(64):
            t, want = 64 * r + j, model.slots[r][j]
            assert ln[t] == (len(want) if want is not None else 0), (r, j)
            if want is not None:
                assert buf[t, :ln[t]].tobytes() == want, (r, j)
            if not pruned:
                assert (buf[t, ln[t]:] == FILL).all(), (r, j)


class Blocks:
    """Three blocks of three slices (sizes SIZES, the third of each block is_last): blocks 0 and 1
    share a slot and differ in content, block 2 has another slot and another leader.  Of every
    slice a random 40 of its 64 datagrams, the replies shuffled across blocks.  Read-only."""

    def __init__(self):
        rng = random.Random(0x4E9A14)
        self.slices, self.full, self.roots, self.stream = [], [], [], []
        for r, S in enumerate(SIZES):
            b, si = divmod(r, SPB)
            s_ = make_slice(rng, S, BLOCK_SLOTS[b], si, si == SPB - 1)
            pkts, _, root, _ = so.shred(*s_, SEEDS[b])
            self.slices.append(s_)
            self.full.append(pkts)
            self.roots.append(root)
            self.stream += [(pkts[j], b, si, j) for j in sorted(rng.sample(range(64), 40))]
        rng.shuffle(self.stream)
        self.model = new_model(self.roots)
        self.verdicts = rm.intake(self.model, self.stream)


@pytest.fixture(scope="module")
def blocks():
    return Blocks()


@pytest.fixture(scope="module")
def honest(ctx, dev, blocks):
    """The honest stream in one call: (store, verdicts, shred_bytes_out, counts_out)."""
    store = DevStore(dev, blocks.roots)
    return (store,) + store.feed(ctx, blocks.stream)


@pytest.mark.gpu
def test_repair_honest_catch_up(ctx, dev, blocks, honest):
    store, verdicts, sizes, counts = honest
    assert blocks.verdicts == [rm.STORED] * len(blocks.stream) and len(blocks.stream) == 360
    assert names(verdicts) == names(blocks.verdicts)
    assert sizes == SIZES and counts == [40] * 9
    check_store(store, blocks.model, sizes, counts)
    # the deshred behind it, one call per leader key (on copies: it fills the absent slots)
    for first, nrows, b in ((0, 6, 0), (6, 3, 2)):
        cw = filled(nrows * STRIDE, dev)
        pk = to_dev(np.frombuffer(PKS[b], np.uint8), dev)
        res = rs.shredder_deshred_batch_var(ctx, nrows, sizes[first:first + nrows],
                                            store.packets[64 * first:64 * (first + nrows)].clone(), PKT,
                                            store.lens[64 * first:64 * (first + nrows)].clone(), pk, cw, STRIDE)
        torch.cuda.synchronize()
        assert res.status.tolist() == [0] * nrows
        cw = cw.cpu().numpy()
        for k in range(nrows):
            parent, data, slot, si, last = blocks.slices[first + k]
            at = k * STRIDE + int(res.data_offsets[k])
            assert cw[at:at + int(res.data_lens[k])].tobytes() == data, first + k
            assert (res.parents[k], int(res.slots[k]), int(res.slice_indices[k]), bool(res.is_last[k])) == \
                (parent, slot, si, last)
    # the block hashes over the proved roots: what repair.rs:447 asserts against the request
    hashes = filled(3 * 32, dev)
    rs.block_tree_batch(ctx, 3, [SPB] * 3, store.roots, hashes)
    torch.cuda.synchronize()
    hashes = hashes.cpu().numpy().reshape(3, 32)
    for b in range(3):
        assert hashes[b].tobytes() == mk.MerkleTree(blocks.roots[SPB * b:SPB * (b + 1)]).root(), b


@pytest.mark.gpu
@pytest.mark.parametrize("chunk", [1, 7, 64])
def test_repair_chunked_calls(ctx, dev, blocks, honest, chunk):
    """The stream in calls of `chunk` replies: the same store and verdicts as one call (the later
    calls inherit from the store's (commitment, signature) pairs)."""
    store, verdicts = DevStore(dev, blocks.roots), []
    for at in range(0, len(blocks.stream), chunk):
        v, sizes, counts = store.feed(ctx, blocks.stream[at:at + chunk])
        verdicts += v
    assert verdicts == honest[1]
    assert sizes == honest[2] and counts == honest[3]
    for x, y in zip(store.host(), honest[0].host()):
        assert np.array_equal(x, y)


def adversarial_stream(blocks):
    """What repair peers can answer, case by case (the model gives the verdicts; the ones a case
    is about are asserted by the test as well): (replies, {label: index}, proved roots).
    Rows: block 0 from `blocks`; row (1, 0) a slice of two leaf sizes, (1, 1) not proved; block 2
    in versions with and without is_last."""
    rng = random.Random(0xBAD4E9)
    out, at = [], {}

    def put(p, b, s, i, label=None):
        if label:
            at[label] = len(out)
        out.append((p, b, s, i))

    f = blocks.full
    roots = list(blocks.roots)
    mixed = mixed_slice(rng, SLOT_X, 0, SEED_A)
    roots[3], roots[4] = root_of(mixed[0]), None
    c = {}
    for si in range(3):
        s_ = make_slice(rng, [24, 1010, 2][si], SLOT_Y, si, False)
        c[si, False], c[si, True] = so.shred(*s_, SEED_B)[0], so.shred(*(s_[:4] + (True,)), SEED_B)[0]
        roots[6 + si] = root_of(c[si, False][0])
    # row (0, 0): its first root-matching reply has an invalid signature, so the pick fails and
    # the cache comes from the second verify launch; a payload altered after signing is no
    # signature matter at all
    put(tamper(f[0][4], 37), 0, 0, 4, "tampered")
    put(resign(f[0][5], OTHER_SEED), 0, 0, 5, "forged_first")
    put(f[0][5], 0, 0, 5, "genuine_after_forged")
    for j in (0, 40, 63):
        put(f[0][j], 0, 0, j)
    put(f[0][9], 1, 0, 9, "other_block_of_slot")      # block 0's shred for block 1's request
    # malformed
    put(f[1][2][:-1], 0, 1, 2, "truncated")
    put(f[1][2] + b"\x00", 0, 1, 2, "trailing")
    put(b"", 0, 1, 2, "empty")
    # the request names no row; the header answers another request
    put(f[1][3], 3, 1, 3, "req_block")
    put(f[1][3], 0, SPB, 3, "req_slice")
    put(f[1][3], 0, 1, 64, "req_index")
    put(f[1][3], 2, 1, 3, "mismatch_slot")
    put(f[1][3], 0, 2, 3, "mismatch_slice")
    put(f[1][3], 0, 1, 4, "mismatch_index")
    # implausible (and: the request is compared first)
    k, slot, si, last, j, data, sig, proof = wire.deserialize(f[1][4])
    put(wire.serialize(wire.CODING, slot, si, last, j, data, sig, proof), 0, 1, 4, "kind")
    put(wire.serialize(k, slot, si, last, j, data[:-1], sig, proof), 0, 1, 4, "odd")
    put(wire.serialize(k, slot, si, last, j, data, sig, proof[:5]), 0, 1, 4, "proof5")
    put(wire.serialize(k, slot, si, last, j, data + bytes(1100), sig, proof), 0, 1, 4, "wide")
    put(wire.serialize(k, slot, si, last, j, data + bytes(1100), sig, proof), 0, 1, 5, "wide_mismatch")
    # row (0, 1): the cache is set; its commitment under another signature is not accepted,
    # whether the slot is free or taken; is_last flipped and signed by the leader equivocates
    put(f[1][1], 0, 1, 1, "sets_cache")
    put(resign(f[1][2], OTHER_SEED), 0, 1, 2, "other_sig")
    put(f[1][2], 0, 1, 2, "genuine_after_other_sig")
    put(resign(f[1][1], OTHER_SEED), 0, 1, 1, "dup_other_sig")
    put(f[1][1], 0, 1, 1, "dup")
    put(relast(f[1][7], SEED_A), 0, 1, 7, "is_last_flipped")
    # row (1, 0): leaves of two sizes
    put(mixed[0], 1, 0, 0)
    put(mixed[3], 1, 0, 3, "two_sizes")
    put(mixed[33], 1, 0, 33)
    put(f[4][8], 1, 1, 8, "not_proved")
    # block 0's last slice, honestly; a late duplicate of the first row
    for j in (1, 2, 35):
        put(f[2][j], 0, 2, j)
    put(f[0][5], 0, 0, 5, "late_duplicate")
    # block 2: signed by the other block's leader; slice 2 stored, slice 1 marks itself last,
    # slice 2 again, is_last on another slice, slice 1 in a version that is not last
    put(resign(c[2, False][0], SEED_A), 2, 2, 0, "wrong_leader")
    put(c[2, False][0], 2, 2, 0, "pruned_0")
    put(c[0, False][0], 2, 0, 0)
    put(c[2, False][50], 2, 2, 50, "pruned_50")
    put(c[1, True][0], 2, 1, 0, "marks_last")
    put(c[2, False][1], 2, 2, 1, "after_last")
    put(c[0, True][1], 2, 0, 1, "second_last")
    put(c[1, False][1], 2, 1, 1, "last_not_last")
    put(c[1, True][1], 2, 1, 1)
    put(c[0, False][1], 2, 0, 1)
    return out, at, roots


@pytest.fixture(scope="module")
def adversarial(blocks):
    stream, at, roots = adversarial_stream(blocks)
    model = new_model(roots)
    return stream, at, roots, model, rm.intake(model, stream)


def check_adversarial_by_hand(at, want):
    """What the cases are about, from the model alone."""
    assert sorted(set(want)) == list(range(12))   # every verdict code occurs
    v = dict((k, rs.REPAIR_VERDICTS[want[i]]) for k, i in at.items())
    assert [v[k] for k in ("truncated", "trailing", "empty")] == ["malformed"] * 3
    assert [v[k] for k in ("req_block", "req_slice", "req_index")] == ["out_of_window"] * 3
    assert [v[k] for k in ("mismatch_slot", "mismatch_slice", "mismatch_index", "wide_mismatch")] == \
        ["request_mismatch"] * 4
    assert [v[k] for k in ("kind", "odd", "proof5", "wide")] == ["implausible"] * 4
    assert v["not_proved"] == "no_root"
    assert [v[k] for k in ("tampered", "other_block_of_slot")] == ["wrong_root"] * 2
    assert [v[k] for k in ("forged_first", "other_sig", "dup_other_sig", "wrong_leader")] == ["invalid_signature"] * 4
    assert [v[k] for k in ("genuine_after_forged", "sets_cache", "genuine_after_other_sig", "marks_last")] == \
        ["stored"] * 4
    assert [v[k] for k in ("dup", "late_duplicate")] == ["duplicate"] * 2
    assert [v[k] for k in ("is_last_flipped", "after_last", "second_last", "last_not_last")] == ["equivocation"] * 4
    assert v["two_sizes"] == "size_mismatch" and [v["pruned_0"], v["pruned_50"]] == ["pruned"] * 2


@pytest.mark.gpu
def test_repair_adversarial_stream(ctx, dev, adversarial):
    stream, at, roots, model, want = adversarial
    check_adversarial_by_hand(at, want)
    store = DevStore(dev, roots)
    got, sizes, counts = store.feed(ctx, stream)
    assert names(got) == names(want)
    check_store(store, model, sizes, counts)


@pytest.mark.gpu
@pytest.mark.parametrize("cut", ["genuine_after_forged", "other_sig", "late_duplicate", "marks_last", "after_last"])
def test_repair_adversarial_stream_in_two_calls(ctx, dev, adversarial, cut):
    """Cut before a row's setter (the first call leaves no cache), behind one (the cache, its
    signature and the occupancy then come from the store), between block 2's stored slice 2 and
    the reply that prunes it, and behind that one."""
    stream, at, roots = adversarial[:3]
    check_adversarial_by_hand(at, adversarial[4])
    model, store = new_model(roots), DevStore(dev, roots)
    for part in (stream[:at[cut]], stream[at[cut]:]):
        want = rm.intake(model, part)
        got, sizes, counts = store.feed(ctx, part)
        assert names(got) == names(want)
        check_store(store, model, sizes, counts)


@pytest.mark.gpu
def test_repair_argument_errors(ctx, dev, blocks):
    stream = blocks.stream[:5]
    nrows = len(BLOCK_SLOTS) * SPB

    def call(n=5, block_slots=BLOCK_SLOTS, spb=SPB, rx_stride=PKT, packet_stride=PKT, rx_off=0, packets_off=0,
             null=None):
        """One call on fresh 0xA5 buffers (the lengths too); every buffer must come back 0xA5."""
        b = dict(pks=filled(32 * len(block_slots), dev), rx=filled(8 * PKT + 64, dev), rx_lens=filled(4 * 8, dev),
                 req_block=filled(4 * 8, dev), req_slice=filled(4 * 8, dev), req_index=filled(4 * 8, dev),
                 slice_roots=filled(32 * nrows, dev), have_root=filled(nrows, dev),
                 packets=filled(64 * nrows * PKT + 64, dev), packet_lens=filled(4 * 64 * nrows, dev),
                 commitments=filled(49 * nrows, dev), signatures=filled(64 * nrows, dev),
                 shred_bytes=filled(4 * nrows, dev), last_slice=filled(4 * len(block_slots), dev),
                 verdict=filled(8, dev))
        a = {k: (None if k == null else x.data_ptr()) for k, x in b.items()}
        if a["rx"] is not None:
            a["rx"] += rx_off
        if a["packets"] is not None:
            a["packets"] += packets_off
        with pytest.raises(rs.RSError) as e:
            rs.repair_intake_batch(ctx, block_slots, a["pks"], spb, n, a["rx"], rx_stride, a["rx_lens"],
                                   a["req_block"], a["req_slice"], a["req_index"], a["slice_roots"], a["have_root"],
                                   a["packets"], packet_stride, a["packet_lens"], a["commitments"], a["signatures"],
                                   a["shred_bytes"], a["last_slice"], a["verdict"])
        torch.cuda.synchronize()
        assert e.value.kind == "InvalidArgument"
        for k, x in b.items():
            assert bool((x == FILL).all()), k

    for k in ("pks", "rx", "rx_lens", "req_block", "req_slice", "req_index", "slice_roots", "have_root", "packets",
              "packet_lens", "commitments", "signatures", "shred_bytes", "last_slice", "verdict"):
        call(null=k)
    call(block_slots=[])
    call(spb=0)
    call(spb=1025)
    call(block_slots=[5] * (1 << 14), spb=1024)   # nrows = 2^24
    call(n=1 << 24)
    need = rs.shred_datagram_bytes(1024, 6)
    assert need == 1325
    call(rx_stride=1312)          # a multiple of 16 below the largest datagram
    call(packet_stride=1312)
    call(rx_stride=1336)          # large enough, no multiple of 16
    call(packet_stride=1336)
    call(rx_off=8)
    call(packets_off=8)
    # n == 0 is a call like any other: OK, the host outputs filled from the store
    store = DevStore(dev, blocks.roots)
    assert store.feed(ctx, []) == ([], [0] * nrows, [0] * nrows)
    store.feed(ctx, stream)
    model = new_model(blocks.roots)
    rm.intake(model, stream)
    assert store.feed(ctx, []) == ([], model.shred_bytes, model.counts())
    check_store(store, model)
