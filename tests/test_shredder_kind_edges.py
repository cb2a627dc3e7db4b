"""CodingOnly, PETS and AONT composed (ag_shredder_shred_batch_kind / ag_shredder_deshred_batch_kind)
at the edges their host code branches on, against oracle/shredder_oracle.py (shred_kind, datagrams,
receive, deshred_kind; the reference: shredder.rs:282-311, :361-528, validated_shred.rs:52-81).

A  shred side at the tail sizes S = 2 / 66 / 78 / 80 (S mod 64 = 2, 2, 14, 16), the shortest and
   longest framed lengths of each size, n = 5 and n = 1, and MAX_DATA_SIZE;
B  deshred side at the same sizes: honest and Byzantine slices, 0 / 31 / 32 / surplus / 64
   datagrams, n = 12 and n = 1, both routes of AONT below a 16-byte tail;
C  structured arrivals at S = 64: the present-word remap of PETS (output shred 63 alone in word
   1) and CodingOnly's two words;
D  decrypt_payload before check_merkle_tree: a decoded buffer shorter than the key is BadEncoding
   whatever the tree says (shredder.rs:293 against :303);
E  the receiver front (pipe_pick / pipe_cache / pipe_check) through every layout: two commitments
   in one slice's slots, cached commitments, the Data / Coding type of a slot.

Every buffer the calls write starts at 0xA5, the codeword stride is (32 + m) S + 12, rounded up
to the multiple of 4 the calls require (rows at 2-byte alignment inside 4-byte-aligned slices),
and every check looks for stray writes
(shredder_cases.check_shred / check_deshred).  Expected values are the oracle's.  One exception,
as in test_shredder_exact_rerun.py: where a PETS / AONT batch needs an honest leader only as the
source of datagrams, they come from the device's own shred call, at an S where part A (or
test_shredder_pipeline.py, S = 64) pins that call to so.shred_kind -- the oracle's AES is Python.
"""

import functools
import random

import pytest

import rs_oracle as o
import shred_wire_oracle as wire
import shredder_cases as sc
import shredder_oracle as so
import slice_oracle as sl

pytestmark = pytest.mark.gpu

KINDS = sc.KINDS
ALL_KINDS = [so.REGULAR] + KINDS
TAIL_SIZES = [2, 66, 78, 80]
FAILED = (so.BAD_ENCODING, so.INVALID_MERKLE_TREE)
ids = sc.NAMES.get


@pytest.fixture(scope="module")
def dev(ctx):
    import torch

    d = torch.device("cuda:0")
    s = torch.cuda.Stream(d)
    torch.cuda.set_stream(s)
    ctx.set_stream(s.cuda_stream)
    return d


def _leader(ctx, dev, kind, S):
    """slices -> [(datagrams, output RawShreds)]: the oracle, or for PETS / AONT the device's shred call."""
    if kind in (so.PETS, so.AONT):
        return lambda slices: sc.gpu_leader(ctx, dev, kind, slices, S)
    return lambda slices: sc.oracle_leader(kind, slices)


# ---- A: shred side ---------------------------------------------------------------------------------

def edge_slices(kind, S):
    """Five slices that pad to S: the shortest framed length without a parent (S = 2: no parent and
    no data, 9 bytes) and with one, the longest with each, one in between.  PETS / AONT stay 16
    bytes short for the key tail; at S = 2 that leaves a parent's 49-byte header no room, so their
    slices there have none."""
    rng = random.Random(1000 * kind + S)
    lo, hi = sc.framed_range(kind, S)
    par = sl.header_len((0, b"")) <= hi
    plan = [(max(lo, 9), False), (max(lo, 49) if par else lo + 1, par), (hi, False), (hi if par else hi - 1, par),
            (rng.randrange(max(lo, 9), hi + 1), False)]
    return [sc.make_slice(rng, kind, S, framed, parent, i) for i, (framed, parent) in enumerate(plan)]


SHRED_CASES = [(k, S) for k in KINDS for S in TAIL_SIZES] + [(so.CODING_ONLY, 1000)]


@pytest.mark.parametrize("kind,S", SHRED_CASES, ids=[f"{sc.NAMES[k]}-{S}" for k, S in SHRED_CASES])
def test_shred_tail_sizes(ctx, dev, kind, S):
    """Shredder::shred of the three shredders at S mod 64 != 0 (CodingOnly also at S = 1000): five
    slices at the length edges of the size, then the first of them alone."""
    slices = edge_slices(kind, S)
    if S == 2:
        assert slices[0][0] is None and slices[0][1] == b""
    want = [so.shred_kind(kind, *s_[:5], sc.SEED, s_[5]) for s_ in slices]
    sc.check_shred(sc.gpu_shred(ctx, dev, kind, slices, S), kind, slices, S, want)
    sc.check_shred(sc.gpu_shred(ctx, dev, kind, slices[:1], S), kind, slices[:1], S, want[:1])


@pytest.mark.parametrize("kind", KINDS, ids=ids)
def test_shred_max_data_size(ctx, dev, kind):
    """MAX_DATA_SIZE (shredder.rs:409, :457): the largest framed slice, 32767 bytes less the key
    tail of PETS / AONT, is shredded byte-exact; one byte more is TooMuchData for the call, and
    no output buffer is touched."""
    rng = random.Random(31 + kind)
    S, framed = 1024, sl.MAX_DATA_PER_SLICE - sc.extra_of(kind)
    s_ = (None, rng.randbytes(framed - sl.header_len(None)), rng.randrange(1 << 32), rng.randrange(1024), True,
          rng.randbytes(16))
    sc.check_shred(sc.gpu_shred(ctx, dev, kind, [s_], S), kind, [s_], S,
                   [so.shred_kind(kind, *s_[:5], sc.SEED, s_[5])])
    over = (s_[0], s_[1] + b"\x00") + s_[2:]
    with pytest.raises(o.RSError) as e:
        so.shred_kind(kind, *over[:5], sc.SEED, over[5])
    assert e.value.kind == "TooMuchData"
    got = sc.gpu_shred(ctx, dev, kind, [over], S)
    assert got.error is not None and got.error.kind == "TooMuchData"
    for a in (got.cw, got.pkts, got.roots, got.sigs):
        assert (a == sc.FILL).all()
    assert (got.lens == 0).all()


# ---- B: deshred side ---------------------------------------------------------------------------------

# (leader, datagrams received, the altered shred held or lacking): every third slice Byzantine
MIXED = [("H", 32), ("B", 32, "held"), ("H", "some"), ("H", 64), ("B", "some", "held"), ("H", 31), ("H", 0),
         ("B", 32, "lack"), ("H", 32), ("H", "some"), ("B", "some", "lack"), ("H", 64)]
# no slice with surplus shreds, none with all 32 data shreds: AONT's device-pattern pass below T = 16
NO_SURPLUS = [("H", 32), ("B", 32, "held"), ("H", 32), ("H", 32), ("B", 32, "lack"), ("H", 31), ("H", 0),
              ("B", 32, "held"), ("H", 32), ("H", 32), ("B", 32, "lack"), ("H", 32)]


def deshred_batch(kind, S, plan, leader):
    """rows received for `plan`; `some` is a random 33..63."""
    rng = random.Random(77 * S + 5 * kind + (1000 if plan is NO_SURPLUS else 0))
    slices = sc.random_slices(rng, kind, S, len(plan))
    rows = []
    for s_, (full, raw), (who, cnt, *how) in zip(slices, leader(slices), plan):
        cnt = rng.randrange(33, 64) if cnt == "some" else cnt
        while True:
            if who == "B":
                t = rng.randrange(64)
                rest = [j for j in range(64) if j != t]
                keep = ({t} | set(rng.sample(rest, cnt - 1))) if how[0] == "held" else set(rng.sample(rest, cnt))
            else:
                keep = set(rng.sample(range(64), cnt))
            if plan is not NO_SURPLUS or not set(range(32)) <= keep:
                break
        got = sc.altered(kind, s_, raw, t) if who == "B" else full
        rows.append([got[j] if j in keep else None for j in range(64)])
    return rows


def _deshred_case(ctx, dev, kind, S, plan):
    rows = deshred_batch(kind, S, plan, _leader(ctx, dev, kind, S))
    want = [sc.expect(r, S, kind) for r in rows]
    st = [w[0] for w in want]
    # the case mix, on the oracle's own verdicts
    assert st.count(so.OK) >= 4 and so.NOT_ENOUGH_SHARDS in st and set(st) & set(FAILED), st
    g = sc.gpu_deshred(ctx, dev, kind, rows, S)
    print(sc.NAMES[kind], S, "n = 12", "no surplus" if plan is NO_SURPLUS else "mixed", "window", sorted(g.window),
          "encode", sorted(g.encode), "rerun", g.rerun)
    sc.check_deshred(g, kind, rows, S, want)
    byz_surplus = sum(p[0] == "B" and p[1] == "some" for p in plan)
    route = sc.check_route(g, kind, S, rows, want, byz_surplus)
    # one failing and one succeeding slice alone: n = 1 never takes the device-pattern pass
    for b in (next(b for b, x in enumerate(st) if x in FAILED), st.index(so.OK)):
        g1 = sc.gpu_deshred(ctx, dev, kind, [rows[b]], S)
        sc.check_deshred(g1, kind, [rows[b]], S, [want[b]])
        assert g1.rerun == (0, 0), (sc.NAMES[kind], S, b, g1.rerun)
    return route


@pytest.mark.parametrize("S", TAIL_SIZES)
@pytest.mark.parametrize("kind", KINDS, ids=ids)
def test_deshred_tail_sizes(ctx, dev, kind, S):
    """Shredder::deshred at S mod 64 != 0: 12 slices -- honest ones received as exactly 32, as
    33..63 and as all 64 datagrams, one with 31 and one with none, and every third from a leader
    that altered one shred after encoding, received with exactly 32 and with surplus, the altered
    shred held and withheld.  CodingOnly and PETS leave the device-pattern pass at every tail, AONT
    below T = 16 when a slice has surplus shreds (here it has): the whole batch goes through EXACT.
    AONT at S = 80 stays on the device and re-runs the failed surplus slices."""
    route = _deshred_case(ctx, dev, kind, S, MIXED)
    assert route == ("device" if kind == so.AONT and S == 80 else "exact")


@pytest.mark.parametrize("S", [2, 66, 78])
def test_deshred_aont_short_tail_device_pass(ctx, dev, S):
    """AONT below a 16-byte tail with no surplus shreds and no slice holding all 32 data shreds:
    the device-pattern pass with the fused coding restore, nothing re-encoded, nothing re-run."""
    route = _deshred_case(ctx, dev, so.AONT, S, NO_SURPLUS)
    assert route == "device"


# ---- C: structured arrivals --------------------------------------------------------------------------

R = lambda a, b: set(range(a, b))  # noqa: E731
SHAPES = {
    so.PETS: [R(0, 31) | {63}, R(0, 32), R(31, 63), R(32, 64), R(31, 64), R(0, 9) | R(31, 64), R(0, 64), "31+9"],
    so.CODING_ONLY: [R(0, 32), R(32, 64), set(range(0, 64, 2)), R(16, 48), R(0, 31) | {63}, R(0, 64)],
    so.AONT: [R(0, 32), R(0, 33), R(32, 64), R(0, 31) | {63}, R(0, 64)],
}


@pytest.mark.parametrize("kind", KINDS, ids=ids)
def test_structured_arrivals(ctx, dev, kind):
    """An honest leader at S = 64, the kept output shreds chosen to hinge on the layout: PETS's
    present-word remap (data 0..30 in the low bits, coding 0..31 above them, output shred 63 =
    coding 32 alone in word 1), CodingOnly's two words of a W = 128 window, AONT's all-data and
    all-coding sets.  Every slice ends OK with all 64 slots the leader's datagrams and the payload
    restored; every exactly-32 shape cut by one shred ends NotEnoughShards, its slots untouched."""
    S = 64
    rng = random.Random(640 + kind)
    shapes = [s if s != "31+9" else R(0, 31) | set(rng.sample(range(31, 64), 9)) for s in SHAPES[kind]]
    shapes += [s - {max(s)} for s in shapes if len(s) == 32]
    assert sum(len(s) == 31 for s in shapes) == {so.PETS: 4, so.CODING_ONLY: 5, so.AONT: 3}[kind]
    slices = sc.random_slices(rng, kind, S, len(shapes))
    rows, want = [], []
    for s_, (full, _), keep in zip(slices, sc.oracle_leader(kind, slices), shapes):
        rows.append([full[j] if j in keep else None for j in range(64)])
        flags = [j in keep for j in range(64)]
        if len(keep) >= 32:
            want.append((so.OK, dict(parent=s_[0], data=s_[1], header=s_[2:5]), full, flags))
        else:
            want.append((so.NOT_ENOUGH_SHARDS, None, [x if x is not None else b"" for x in rows[-1]], flags))
    g = sc.gpu_deshred(ctx, dev, kind, rows, S)
    sc.check_deshred(g, kind, rows, S, want)
    assert sc.check_route(g, kind, S, rows, want) == "device" and g.rerun == (0, 0)


# ---- D: decrypt_payload before check_merkle_tree ---------------------------------------------------

SHORT = [0, 1, 15, 16, 17]
# (kept output shreds, the altered output shred or None)
ARRIVALS = [(R(0, 64), None), (R(20, 52), None), (R(0, 63), 63), (R(31, 63), 63), (R(8, 40), 40), (R(0, 64), 40)]


@functools.lru_cache(maxsize=None)
def short_buffers(kind):
    """Per (L, arrival): the rows received of a slice whose coder buffer is L random bytes -- below
    the 16-byte key no PETS / AONT payload, so only a Byzantine leader sends it -- shredded straight
    through the oracle's coder at S = 2, output shred t XORed with 0x5A where the arrival says so."""
    rng = random.Random(1600 + kind)
    nd = so.DATA_OUT[kind]
    cases, rows = [], []
    for L in SHORT:
        for keep, t in ARRIVALS:
            raw = so.output_raw(kind, o.coder_shred(rng.randbytes(L), so.CODING[kind]))
            assert len(raw.coding[0]) == 2
            shards = list(raw.data) + list(raw.coding)
            if t is not None:
                shards[t] = bytes(x ^ 0x5A for x in shards[t])
            full = so.datagrams(shards[:nd], shards[nd:], rng.randrange(1 << 32), rng.randrange(1024), bool(L % 2),
                                sc.SEED)[0]
            cases.append((L, keep, t))
            rows.append([full[j] if j in keep else None for j in range(64)])
    return cases, rows, [sc.expect(r, 2, kind) for r in rows]


@pytest.mark.parametrize("kind", KINDS, ids=ids)
def test_short_buffer_is_bad_encoding_before_the_tree(ctx, dev, kind):
    """decrypt_payload runs inside deshred_validated_shreds, before check_merkle_tree: for PETS /
    AONT a decoded buffer of L < 16 bytes is BadEncoding (23) whether or not the rebuilt tree has
    the signed root; from L = 16 on a withheld altered shred is InvalidMerkleTree (24).  CodingOnly,
    which has no key, is the control.  30 slices in one batch (S = 2: whole-batch EXACT), a failing
    slice alone, and for AONT the exactly-32 arrivals alone, which take the device-pattern pass.

    With the root comparison deciding first (the library before this rule was put into
    pipe_statuses) the L < 16 slices whose altered shred is withheld returned 24."""
    cases, rows, want = short_buffers(kind)
    st = {c[0:1] + (i % len(ARRIVALS),): w[0] for i, (c, w) in enumerate(zip(cases, want))}
    if kind != so.CODING_ONLY:
        assert all(v == so.BAD_ENCODING for (L, _), v in st.items() if L < 16), st
        assert any(v == so.INVALID_MERKLE_TREE for (L, _), v in st.items() if L >= 16), st
    g = sc.gpu_deshred(ctx, dev, kind, rows, 2)
    print(sc.NAMES[kind], "short buffers: library", g.res.status.tolist(), "oracle", [w[0] for w in want])
    sc.check_deshred(g, kind, rows, 2, want)
    assert sc.check_route(g, kind, 2, rows, want) == "exact"
    alone = cases.index((1, ARRIVALS[2][0], 63))  # L = 1, slots 0..62 of a slice whose shred 63 is altered
    sc.check_deshred(sc.gpu_deshred(ctx, dev, kind, [rows[alone]], 2), kind, [rows[alone]], 2, [want[alone]])
    if kind == so.AONT:
        sub = [i for i, c in enumerate(cases) if len(c[1]) == 32]
        assert len(sub) == 3 * len(SHORT)
        g = sc.gpu_deshred(ctx, dev, kind, [rows[i] for i in sub], 2)
        sc.check_deshred(g, kind, [rows[i] for i in sub], 2, [want[i] for i in sub])
        assert sc.check_route(g, kind, 2, [rows[i] for i in sub], [want[i] for i in sub]) == "device"


# ---- E: the receiver front ---------------------------------------------------------------------------

def _zero_sig(p, S):
    off = len(p) - 64 - 8 - 32 * so.HEIGHT
    assert off == 37 + S
    return p[:off] + bytes(64) + p[off + 64:]


def _other_type(p):
    kind, *rest = wire.deserialize(p)
    return wire.serialize(wire.CODING if kind == wire.DATA else wire.DATA, *rest)


def front_rows(kind, S):
    """The ten slot fillings of part E.  A and B: two honest slices with one slot, slice index,
    is_last and key; X: A signed by another key; four variants that carry A's raw shreds in slots
    40..63 and differ from A in exactly one field of the commitment (for the root: shred 5, outside
    those slots, altered before the tree is built)."""
    rng = random.Random(6400 + kind)
    a, b = sc.random_slices(rng, kind, S, 2)
    b = b[:2] + a[2:]
    (A, raw), (B, _) = sc.oracle_leader(kind, [a, b])
    nd = so.DATA_OUT[kind]
    slot, si, last = a[2:5]

    def dgrams(raw_, slot=slot, si=si, last=last, seed=sc.SEED):
        return so.datagrams(raw_.data, raw_.coding, slot, si, last, seed)[0]

    X = dgrams(raw, seed=sc.OTHER_SEED)
    shards = list(raw.data) + list(raw.coding)
    shards[5] = bytes(x ^ 0x5A for x in shards[5])
    variants = [dgrams(raw, slot=slot ^ 1), dgrams(raw, si=si ^ 1), dgrams(raw, last=not last),
                dgrams(o.RawShreds(data=shards[:nd], coding=shards[nd:]))]
    none = [None] * 64
    rows = [A[:40] + B[40:],
            A[:20] + B[20:],
            X[:1] + B[1:41] + A[41:],
            A[:1] + [_zero_sig(p, S) for p in A[1:40]] + none[40:],
            [_zero_sig(A[0], S)] + A[1:40] + none[40:],
            A[:31] + [_other_type(A[31])] + A[32:40] + none[40:]]
    for V in variants:
        assert all(wire.deserialize(V[j])[5] == wire.deserialize(A[j])[5] for j in range(40, 64))
        rows.append(A[:40] + V[40:])
    return rows, A, B


@pytest.mark.parametrize("kind", ALL_KINDS, ids=ids)
def test_receiver_front(ctx, dev, kind):
    """ValidatedShred::try_new's slot and commitment logic through a composed call of every layout
    (S = 64): leader equivocation (the first valid commitment of the slice wins, the other's
    datagrams are dropped and, where the slice still decodes, overwritten), a first datagram under
    another key (no cached commitment: every shred by its own signature), datagrams that ride the
    cached commitment with a zeroed signature (kept, and left as received), a zeroed signature on
    the first datagram (dropped), the wrong Data / Coding type for slot 31 (dropped in every
    layout), and a second commitment that differs in exactly one of slot, slice index, is_last
    and root."""
    S = 64
    rows, A, B = front_rows(kind, S)
    want = [sc.expect(r, S, kind) for r in rows]
    # the oracle's own verdicts: what is kept, who wins
    assert [(w[0], sum(w[3])) for w in want] == [(0, 40), (so.NOT_ENOUGH_SHARDS, 20), (0, 40), (0, 40), (0, 39),
                                                 (0, 39)] + [(0, 40)] * 4
    assert want[0][2] == A and want[2][2] == B and want[5][2] == A and not want[5][3][31]
    assert want[3][2][1:40] == rows[3][1:40] and want[3][2][40:] == A[40:] and want[4][2] == A
    assert all(w[2] == A for w in want[6:])
    g = sc.gpu_deshred(ctx, dev, kind, rows, S)
    sc.check_deshred(g, kind, rows, S, want)
