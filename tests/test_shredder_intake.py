"""Shred intake on the device: ag_shredder_intake_batch (include/alpenglow_rs.h section 10)
against its sequential definition, tests/intake_model.py, which restates the reference's receive
path (validated_shred.rs:52-79, slot_block_data.rs:202-274) over the existing oracles.

CPU: the symbol, the model tied to shredder_oracle.receive, hand-checked last-slice cases.
GPU: an honest block (the store must equal the hand placement that
test_shredder_deshred_var.pack_rows makes, and deshred the same), the same stream in split calls,
an adversarial stream, the argument errors.  Buffers start at 0xA5 so stray writes show.
"""

import os
import random
import re

import numpy as np
import pytest

import ed25519_oracle as ed
import intake_model as im
import merkle_oracle as mk
import rs_oracle as o
import shred_wire_oracle as wire
import shredder_oracle as so
import slice_oracle as sl
from alpenglow_amd import build, rs
from test_shredder_deshred_var import pack_rows

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "alpenglow_rs.h")

FILL = 0xA5
PKT = 1536            # stride of the store's slots and of the receive rows
STRIDE = 64 * 1024    # one slice's codeword region (the deshred behind the intake)
SEED = bytes(range(7, 39))
PK = ed.secret_to_public(SEED)
OTHER_SEED = bytes(range(100, 132))

SLOT_IDS = [7_000_001, 12]   # the window: not ascending, so the caller's order matters
SPP = 4
SIZES = [2, 24, 1000, 1010, 1024, 1000, 2, 1024]   # row r's shred size


def make_slice(rng, S, slot, si, last):
    """A slice whose framed payload pads to shred size S; odd slice index: a parent."""
    parent = (rng.randrange(1 << 40), rng.randbytes(32)) if si % 2 else None
    lo, hi = max(32 * S - 64, sl.header_len(parent)), min(32 * S - 1, sl.MAX_DATA_PER_SLICE)
    return parent, rng.randbytes(rng.randrange(lo, hi + 1) - sl.header_len(parent)), slot, si, last


def shred(slice_, seed=SEED):
    return so.shred(*slice_, seed)[0]


def resign(pkt, seed):
    """The datagram with its signature replaced by `seed`'s over the same commitment."""
    kind, slot, si, last, j, data, _, proof = wire.deserialize(pkt)
    sig = ed.sign(seed, ed.slice_commitment(slot, si, last, mk.derive_root(data, j, proof)))
    return wire.serialize(kind, slot, si, last, j, data, sig, proof)


def tamper(pkt, at=40):
    b = bytearray(pkt)
    b[at] ^= 1
    return bytes(b)


# ------------------------------------------------------------------------------ CPU

def test_symbol_declared_exported_and_callable():
    build.build()
    lib = rs.load()
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = set(re.findall(r"\b(ag_\w+)\s*\(", text))
    name = "ag_shredder_intake_batch"
    assert name in declared and name in rs.EXPORTS and hasattr(lib, name)
    assert callable(rs.shredder_intake_batch)
    for i, v in enumerate(("STORED", "MALFORMED", "OUT_OF_WINDOW", "IMPLAUSIBLE", "INVALID_SIGNATURE", "EQUIVOCATION",
                           "SIZE_MISMATCH", "DUPLICATE", "PRUNED")):
        assert getattr(rs, "INTAKE_" + v) == i == getattr(im, v)
        assert re.search(r"\bAG_INTAKE_%s = %d\b" % (v, i), text)


@pytest.mark.parametrize("case", ["clean", "forged_first", "tampered", "foreign_size"])
def test_model_agrees_with_receive_oracle(case):
    """One slice fed in shred-index order: what the model stores is what
    shredder_oracle.receive keeps (the receive model of the deshreds)."""
    rng = random.Random(0x1A7)
    S, slot, si = 24, 99, 2
    rows = list(shred(make_slice(rng, S, slot, si, False)))
    keep = set(rng.sample(range(64), 40))
    first = min(keep)
    if case == "forged_first":
        rows[first] = resign(rows[first], OTHER_SEED)   # the first shred checked fails its signature
    elif case == "tampered":
        rows[sorted(keep)[5]] = tamper(rows[sorted(keep)[5]])
    elif case == "foreign_size":
        j = sorted(keep)[7]
        rows[j] = shred(make_slice(rng, 26, slot, si, False))[j]
    rows = [rows[j] if j in keep else None for j in range(64)]
    store = im.Store([slot], 4)
    verdicts = im.intake(store, [p for p in rows if p is not None], PK)
    kept = so.receive(rows, PK, S)
    assert [x is not None for x in store.slots[si]] == [x is not None for x in kept]
    assert verdicts.count(im.STORED) == sum(x is not None for x in kept) == (40 if case == "clean" else 39)
    assert store.shred_bytes[si] == S and store.counts()[si] == verdicts.count(im.STORED)
    for j, x in enumerate(kept):
        if x is not None:
            assert store.slots[si][j] == rows[j]
    want = {"forged_first": im.INVALID_SIGNATURE, "tampered": im.INVALID_SIGNATURE, "foreign_size": im.EQUIVOCATION}
    assert sorted(set(verdicts)) == sorted({im.STORED, want[case]} if case != "clean" else {im.STORED})


def _last_slice_block():
    """Slices 0..3 of one slot, each in a plain and an is_last version (two datagrams each)."""
    rng = random.Random(0x1A57)
    v = {}
    for si in range(4):
        s_ = make_slice(rng, 2, 5, si, False)
        for last in (False, True):
            v[si, last] = shred(s_[:4] + (last,))[:2]
    return v


def test_model_last_slice_cases_by_hand():
    v = _last_slice_block()
    S, E, P, D = im.STORED, im.EQUIVOCATION, im.PRUNED, im.DUPLICATE
    # is_last on slice 2, then slice 3 (slot_block_data.rs:228: 3 > l)
    st = im.Store([5], 4)
    assert im.intake(st, [v[2, True][0], v[3, False][0], v[1, False][0], v[2, True][1]], PK) == [S, E, S, S]
    assert st.last_slice == [2] and st.counts() == [0, 1, 2, 0] and st.shred_bytes == [0, 2, 2, 2]
    # slice 3 stored earlier: pruned when slice 2 marks itself last; the cache of slice 3 is kept
    # (its later datagrams pass try_new unverified) and the last-slice rule rejects them
    st = im.Store([5], 4)
    got = im.intake(st, [v[3, False][0], v[0, False][0], v[2, True][0], v[3, False][1], v[3, False][0]], PK)
    assert got == [P, S, S, E, E]
    assert st.last_slice == [2] and st.counts() == [1, 0, 1, 0] and st.commitment[3] is not None
    # ... and across calls the earlier datagram's verdict stays STORED, its slot is emptied
    st = im.Store([5], 4)
    assert im.intake(st, [v[3, False][0]], PK) == [S] and st.counts() == [0, 0, 0, 1]
    assert im.intake(st, [v[2, True][0]], PK) == [S] and st.counts() == [0, 0, 1, 0]
    # is_last on two different slices: the second is inconsistent, whichever side it is on
    st = im.Store([5], 4)
    got = im.intake(st, [v[1, True][0], v[2, True][0], v[0, True][0], v[1, True][1], v[1, True][0], v[0, False][0]],
                    PK)
    assert got == [S, E, E, S, D, E]   # (slice 0's cache was set by its is_last version: :219-221)
    assert st.last_slice == [1] and st.counts() == [0, 2, 0, 0]


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
    """The caller-owned store on the device, 0xA5 where the call must not write."""

    def __init__(self, dev, nslots=len(SLOT_IDS), spp=SPP):
        self.dev, self.nslots, self.spp, self.nrows = dev, nslots, spp, nslots * spp
        self.packets = filled((64 * self.nrows, PKT), dev)
        self.lens = torch.zeros(64 * self.nrows, dtype=torch.int32, device=dev)
        self.commitments = filled(49 * self.nrows, dev)
        self.shred_bytes = torch.zeros(self.nrows, dtype=torch.int32, device=dev)
        self.last_slice = torch.full((nslots,), -1, dtype=torch.int32, device=dev)
        self.pk = to_dev(np.frombuffer(PK, np.uint8), dev)

    def feed(self, ctx, datagrams, slot_ids=SLOT_IDS):
        """One intake call: (verdicts, shred_bytes_out, counts_out); rx must come back unchanged."""
        n = len(datagrams)
        rx = np.full((max(n, 1), PKT), FILL, np.uint8)
        ln = np.zeros(max(n, 1), np.int32)
        for t, p in enumerate(datagrams):
            rx[t, :len(p)] = np.frombuffer(p, np.uint8)
            ln[t] = len(p)
        d_rx, d_ln, verdict = to_dev(rx, self.dev), to_dev(ln, self.dev), filled(max(n, 1), self.dev)
        sizes, counts = rs.shredder_intake_batch(ctx, slot_ids, self.spp, n, d_rx, PKT, d_ln, self.pk, self.packets,
                                                 PKT, self.lens, self.commitments, self.shred_bytes,
                                                 self.last_slice, verdict)
        torch.cuda.synchronize()
        assert np.array_equal(d_rx.cpu().numpy(), rx), "rx was written"
        return verdict.cpu().numpy()[:n].tolist(), sizes.tolist(), counts.tolist()

    def host(self):
        return (self.packets.cpu().numpy(), self.lens.cpu().numpy(), self.commitments.cpu().numpy().reshape(-1, 49),
                self.shred_bytes.cpu().numpy(), self.last_slice.cpu().numpy())


def names(verdicts):
    return [rs.INTAKE_VERDICTS[v] if v < len(rs.INTAKE_VERDICTS) else v for v in verdicts]


def check_store(store: DevStore, model: im.Store, sizes=None, counts=None):
    """Every byte of the device store against the model's."""
    buf, ln, com, sb, last = store.host()
    assert last.tolist() == [-1 if x is None else x for x in model.last_slice]
    assert sb.tolist() == model.shred_bytes
    if sizes is not None:
        assert sizes == model.shred_bytes and counts == model.counts()
    for r in range(model.nrows):
        if model.commitment[r] is None:
            assert (com[r] == FILL).all(), r
        else:
            assert com[r].tobytes() == model.commitment[r], r
        l = model.last_slice[r // model.spp]
        pruned = l is not None and r % model.spp > l   # (bytes of pruned rows are unspecified)
        for j in range(64):
            t, want = 64 * r + j, model.slots[r][j]
            assert ln[t] == (len(want) if want is not None else 0), (r, j)
            if want is not None:
                assert buf[t, :ln[t]].tobytes() == want, (r, j)
            if not pruned:
                assert (buf[t, ln[t]:] == FILL).all(), (r, j)


class Block:
    """Two slots of four slices (sizes SIZES, the fourth of each slot is_last); of every slice a
    random 40 of its 64 datagrams, the stream shuffled across slices and slots.  Read-only."""

    def __init__(self):
        rng = random.Random(0x1A7A)
        self.rows = []
        for r, S in enumerate(SIZES):
            full = shred(make_slice(rng, S, SLOT_IDS[r // SPP], r % SPP, r % SPP == SPP - 1))
            keep = set(rng.sample(range(64), 40))
            self.rows.append([full[j] if j in keep else None for j in range(64)])
        self.stream = [p for row in self.rows for p in row if p is not None]
        rng.shuffle(self.stream)
        self.model = im.Store(SLOT_IDS, SPP)
        self.verdicts = im.intake(self.model, self.stream, PK)


@pytest.fixture(scope="module")
def block():
    return Block()


@pytest.fixture(scope="module")
def honest(ctx, dev, block):
    """The honest stream in one call: (store, verdicts, shred_bytes_out, counts_out)."""
    store = DevStore(dev)
    return (store,) + store.feed(ctx, block.stream)


def deshred_on(ctx, dev, sizes, d_buf, d_ln, pk):
    cw = filled(len(sizes) * STRIDE, dev)
    res = rs.shredder_deshred_batch_var(ctx, len(sizes), sizes, d_buf, PKT, d_ln, pk, cw, STRIDE)
    torch.cuda.synchronize()
    return res, d_buf.cpu().numpy(), d_ln.cpu().numpy(), cw.cpu().numpy()


@pytest.mark.gpu
def test_intake_honest_block(ctx, dev, block, honest):
    store, verdicts, sizes, counts = honest
    assert block.verdicts == [im.STORED] * len(block.stream) and len(block.stream) == 320
    assert names(verdicts) == names(block.verdicts)
    assert sizes == SIZES and counts == [40] * 8
    check_store(store, block.model, sizes, counts)
    # the store is the hand placement, byte for byte
    buf, ln = pack_rows(block.rows, PKT)
    got_buf, got_ln = store.host()[:2]
    assert np.array_equal(got_ln, ln) and np.array_equal(got_buf, buf)
    # ... and deshreds like it (on copies: the deshred fills the absent slots)
    a = deshred_on(ctx, dev, sizes, store.packets.clone(), store.lens.clone(), store.pk)
    b = deshred_on(ctx, dev, sizes, to_dev(buf, dev), to_dev(ln, dev), store.pk)
    assert a[0].status.tolist() == [0] * 8
    for f in ("status", "slots", "slice_indices", "is_last", "data_offsets", "data_lens"):
        assert np.array_equal(getattr(a[0], f), getattr(b[0], f)), f
    assert a[0].parents == b[0].parents and all(np.array_equal(x, y) for x, y in zip(a[1:], b[1:]))


@pytest.mark.gpu
@pytest.mark.parametrize("chunk", [1, 7, 64])
def test_intake_split_calls(ctx, dev, block, honest, chunk):
    """The stream in calls of `chunk` datagrams: the same store and verdicts as one call."""
    store, verdicts = DevStore(dev), []
    for at in range(0, len(block.stream), chunk):
        v, sizes, counts = store.feed(ctx, block.stream[at:at + chunk])
        verdicts += v
    assert verdicts == honest[1]
    assert sizes == honest[2] and counts == honest[3]
    for x, y in zip(store.host(), honest[0].host()):
        assert np.array_equal(x, y)


def adversarial_stream():
    """What a receive queue can hold, case by case (the model gives the verdicts; the ones a
    case is about are asserted by the test as well): (datagrams, {label: index})."""
    rng = random.Random(0xBAD)
    A, B = SLOT_IDS
    out, at = [], {}

    def put(p, label=None):
        if label:
            at[label] = len(out)
        out.append(p)

    a0 = shred(make_slice(rng, 2, A, 0, False))
    a1s = make_slice(rng, 1000, A, 1, False)
    a1, a1_other = shred(a1s), shred(make_slice(rng, 1000, A, 1, False))
    a3 = shred(make_slice(rng, 1024, A, 3, True))
    # row A0: its first datagram has an invalid signature (payload altered after signing), so the
    # cache comes from a later one; the genuine datagram of that slot arrives afterwards
    put(tamper(a0[5], 37), "forged_first")
    put(resign(a0[6], OTHER_SEED), "foreign_key")
    put(a0[5], "genuine_after_forged")
    for j in (0, 40, 63):
        put(a0[j])
    # malformed: truncated, trailing byte, empty
    put(a1[2][:-1], "truncated")
    put(a1[2][:30], "truncated_header")
    put(a1[2] + b"\x00", "trailing")
    put(b"", "empty")
    # out of the window: another slot, a slice index past slices_per_slot (one of them too wide as well)
    put(shred(make_slice(rng, 24, 999, 1, False))[3], "other_slot")
    put(shred(make_slice(rng, 24, A, SPP, False))[3], "slice_index")
    k, slot, si, last, j, data, sig, proof = wire.deserialize(a1[4])
    put(wire.serialize(k, 999, si, last, j, data + bytes(100), sig, proof), "other_slot_wide")
    # implausible: kind against the index, odd data length, five digests, too wide, empty payload
    put(wire.serialize(wire.CODING, slot, si, last, j, data, sig, proof), "kind")
    put(wire.serialize(k, slot, si, last, j, data[:-1], sig, proof), "odd")
    put(wire.serialize(k, slot, si, last, j, data, sig, proof[:5]), "proof5")
    put(wire.serialize(k, slot, si, last, j, data, sig, proof + proof[:1]), "proof7")
    put(wire.serialize(k, slot, si, last, j, data + bytes(100), sig, proof), "wide")
    put(wire.serialize(k, slot, si, last, j, b"", sig, proof), "no_data")
    # row A1: the cache is set, then a forged copy claims slot 7 before the genuine datagram
    put(a1[1])
    put(tamper(a1[7], 500), "forged_copy")
    put(a1[7], "genuine_after_copy")
    # the same commitment under other signature bytes: a duplicate keeps the first arrival, and
    # arriving first it is stored unverified (validated_shred.rs:62-64)
    put(a1[9], "first_9")
    put(resign(a1[9], OTHER_SEED), "dup_other_sig")
    put(resign(a1[10], OTHER_SEED), "first_10_other_sig")
    put(a1[10], "dup_genuine")
    # a second, validly signed slice for the occupied (slot, slice index)
    put(a1_other[20], "second_slice")
    put(tamper(a1_other[21], 600), "second_slice_forged")
    # row A2: a tree whose leaves have two sizes; the cache is set at 24
    raw = o.coder_shred(sl.payload_bytes(None, rng.randbytes(700)), 32)
    shards = list(raw.data) + list(raw.coding)
    assert len(shards[0]) == 24
    shards[3] += b"\x11\x22"
    a2 = so.datagrams(shards[:32], shards[32:], A, 2, False, SEED)[0]
    put(a2[0])
    put(a2[3], "two_sizes")
    put(a2[33])
    # slot A's last slice, honestly
    for j in (1, 2, 35):
        put(a3[j])
    put(a0[5], "late_duplicate")
    # slot B: slice 3 stored, slice 2 marks itself last, slice 3 again, is_last on another slice,
    # slice 2 in a version that is not last
    b = {}
    for si in range(4):
        s_ = make_slice(rng, [24, 1010, 2, 1024][si], B, si, False)
        b[si, False], b[si, True] = shred(s_), shred(s_[:4] + (True,))
    put(b[3, False][0], "pruned_0")
    put(b[0, False][0])
    put(b[3, False][50], "pruned_50")
    put(b[2, True][0], "marks_last")
    put(b[3, False][1], "after_last")
    put(b[1, True][0], "second_last")
    put(b[2, False][1], "last_not_last")
    put(b[2, True][1])
    put(b[1, False][1], "cached_as_last")   # slice 1's cache came from its is_last version
    put(b[0, False][1])
    return out, at


@pytest.fixture(scope="module")
def adversarial():
    stream, at = adversarial_stream()
    model = im.Store(SLOT_IDS, SPP)
    return stream, at, model, im.intake(model, stream, PK)


@pytest.mark.gpu
def test_intake_adversarial_stream(ctx, dev, adversarial):
    stream, at, model, want = adversarial
    v = dict((k, rs.INTAKE_VERDICTS[want[i]]) for k, i in at.items())
    # what the cases are about, by hand
    assert [v[k] for k in ("truncated", "truncated_header", "trailing", "empty")] == ["malformed"] * 4
    assert [v[k] for k in ("other_slot", "slice_index", "other_slot_wide")] == ["out_of_window"] * 3
    assert [v[k] for k in ("kind", "odd", "proof5", "proof7", "wide", "no_data")] == ["implausible"] * 6
    assert [v[k] for k in ("forged_first", "foreign_key", "forged_copy", "second_slice_forged")] == \
        ["invalid_signature"] * 4
    assert [v[k] for k in ("genuine_after_forged", "genuine_after_copy", "first_9", "first_10_other_sig",
                           "marks_last")] == ["stored"] * 5
    assert [v[k] for k in ("dup_other_sig", "dup_genuine", "late_duplicate")] == ["duplicate"] * 3
    assert [v[k] for k in ("second_slice", "after_last", "second_last", "last_not_last", "cached_as_last")] == \
        ["equivocation"] * 5
    assert v["two_sizes"] == "size_mismatch" and [v["pruned_0"], v["pruned_50"]] == ["pruned"] * 2
    assert model.slots[1][9] == stream[at["first_9"]] and model.slots[1][10] == stream[at["first_10_other_sig"]]
    store = DevStore(dev)
    got, sizes, counts = store.feed(ctx, stream)
    assert names(got) == names(want)
    check_store(store, model, sizes, counts)


@pytest.mark.gpu
@pytest.mark.parametrize("cut", ["genuine_after_forged", "dup_other_sig", "marks_last", "after_last"])
def test_intake_adversarial_stream_in_two_calls(ctx, dev, adversarial, cut):
    """Cut inside the fall-back row, between the two arrivals of a slot, between slot B's stored
    slice 3 and the datagram that prunes it, and behind that one: cache, occupancy and last slice
    then come from the store."""
    stream, cut = adversarial[0], adversarial[1][cut]
    model, store = im.Store(SLOT_IDS, SPP), DevStore(dev)
    for part in (stream[:cut], stream[cut:]):
        want = im.intake(model, part, PK)
        got, sizes, counts = store.feed(ctx, part)
        assert names(got) == names(want)
        check_store(store, model, sizes, counts)


@pytest.mark.gpu
def test_intake_argument_errors(ctx, dev, block):
    stream = block.stream[:5]

    def call(n=5, slot_ids=SLOT_IDS, spp=SPP, rx_stride=PKT, packet_stride=PKT, rx_off=0, packets_off=0, null=None):
        """One call on fresh 0xA5 buffers (the lengths too); every buffer must come back 0xA5."""
        nrows = 8   # (nothing is launched: the buffers need not match the arguments)
        b = dict(rx=filled(8 * PKT + 64, dev), rx_lens=filled(4 * 8, dev), pk=to_dev(np.frombuffer(PK, np.uint8), dev),
                 packets=filled(64 * nrows * PKT + 64, dev), packet_lens=filled(4 * 64 * nrows, dev),
                 commitments=filled(49 * nrows, dev), shred_bytes=filled(4 * nrows, dev),
                 last_slice=filled(4 * len(slot_ids), dev), verdict=filled(8, dev))
        a = {k: (None if k == null else x.data_ptr()) for k, x in b.items()}
        if a["rx"] is not None:
            a["rx"] += rx_off
        if a["packets"] is not None:
            a["packets"] += packets_off
        with pytest.raises(rs.RSError) as e:
            rs.shredder_intake_batch(ctx, slot_ids, spp, n, a["rx"], rx_stride, a["rx_lens"], a["pk"], a["packets"],
                                     packet_stride, a["packet_lens"], a["commitments"], a["shred_bytes"],
                                     a["last_slice"], a["verdict"])
        torch.cuda.synchronize()
        assert e.value.kind == "InvalidArgument"
        for k, x in b.items():
            if k != "pk":
                assert bool((x == FILL).all()), k

    for k in ("rx", "rx_lens", "pk", "verdict", "packets", "packet_lens", "commitments", "shred_bytes", "last_slice"):
        call(null=k)
    call(slot_ids=[5, 9, 5])
    call(spp=0)
    call(spp=1025)
    call(slot_ids=list(range(1 << 14)), spp=1024)   # nrows = 2^24
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
    store = DevStore(dev)
    assert store.feed(ctx, []) == ([], [0] * 8, [0] * 8)
    store.feed(ctx, stream)
    model = im.Store(SLOT_IDS, SPP)
    im.intake(model, stream, PK)
    assert store.feed(ctx, []) == ([], model.shred_bytes, model.counts())
