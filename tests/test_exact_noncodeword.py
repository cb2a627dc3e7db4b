"""AG_RS_DECODE_EXACT on non-codewords, across every decoder path that serves it.

EXACT is "the crate's decoder on every present shard, bit-identical for any input".  It can be
told from ANY_K (any k survivors) only when more than k shards are present AND the bytes are
inconsistent: the code is MDS, so on a codeword, or with exactly k shards, both give the same
originals.  The reference needs the property when a leader signs a non-codeword and a follower
holds more than k shreds: every node must derive the same bytes.

Here every original and every recovery shard is independent random bytes (nothing is encoded),
every pattern of a geometry keeps surplus recovery shards, and the expectation is the C oracle's
every-shard decode.  The same case list serves the CPU tests (the three restatements of the
oracle agree on this input class; absent shards' bytes are never read; the "teeth" condition: on
every case the every-shard result differs from the first-k-survivors result in every 64-byte
chunk of every restored shard, so a decoder that drops surplus shards fails everywhere, not in
one symbol) and the GPU tests (``ag_rs_decode_batch`` per decoder class and kernel variant, the
batched coder's deshred on crafted non-codeword slices, the per-call decoder, the fixture).
Integer / byte work: every comparison is bit-exact.
"""

import functools
import hashlib
import json
import os
import random
from collections import namedtuple

import numpy as np
import pytest

import ro_c
import rs_oracle as o
from alpenglow_amd import rs

GAP, ABSENT_O, ABSENT_R = 0xEE, 0x5A, 0xA5
GUARD = 64  # bytes of GAP before the first and after the last block of each buffer

# layout = (shift of both base pointers in bytes, pad after a block's originals, pad after its recovery)
PLAIN = (0, 0, 0)
PADS = (2, 6, 10)

Case = namedtuple("Case", "row k m S n patterns layout")


def _c(row, k, m, S, n, patterns="one", layout=PLAIN):
    return Case(row, k, m, S, n, patterns, layout)


CASES = [
    # 1: decode_x (W = 32), one pattern
    _c(1, 16, 4, 192, 7), _c(1, 16, 16, 64, 70, layout=PADS), _c(1, 24, 8, 4096, 3),
    # 2: decode_x, per block (S / 64 % 64 == 0; block_ids: some blocks restore nothing)
    _c(2, 16, 4, 4096, 6, "per_block"), _c(2, 24, 8, 4096, 5, "per_block", PADS),
    # 3: decode_x<4, per lane>
    _c(3, 16, 4, 192, 23, "per_block"), _c(3, 24, 8, 64, 70, "per_block", PADS), _c(3, 13, 4, 128, 9, "per_block"),
    # 4: decode_x16 (W = 64), one pattern
    _c(4, 32, 32, 256, 5), _c(4, 20, 30, 192, 7, layout=PADS), _c(4, 17, 17, 64, 70), _c(4, 48, 16, 2048, 3),
    _c(4, 32, 16, 4096, 2, layout=PADS), _c(4, 17, 15, 64, 9),
    # 5: decode_x16, per block
    _c(5, 32, 32, 4096, 6, "per_block"), _c(5, 48, 16, 4096, 4, "per_block", PADS), _c(5, 20, 30, 4096, 4, "per_block"),
    # 6: decode_h8<1>: per lane, chunk 32
    _c(6, 32, 32, 1024, 24, "per_block"), _c(6, 32, 32, 64, 70, "per_block", PADS), _c(6, 20, 30, 192, 23, "per_block"),
    _c(6, 25, 32, 128, 33, "per_block"),
    # 7: decode_h8<-1>: per lane, chunk != 32
    _c(7, 48, 16, 192, 23, "per_block"), _c(7, 40, 16, 64, 70, "per_block", PADS), _c(7, 60, 4, 128, 9, "per_block"),
    # 8: the generic kernel: LowRate; W = 128 HighRate; k > 64; window narrower than 32; per block
    _c(8, 32, 64, 128, 5), _c(8, 32, 33, 1024, 3, layout=PADS), _c(8, 20, 100, 64, 6),
    _c(8, 64, 64, 192, 4), _c(8, 40, 50, 64, 5, layout=PADS),
    _c(8, 65, 3, 64, 4), _c(8, 100, 28, 128, 3),
    _c(8, 5, 2, 64, 9),
    _c(8, 64, 64, 4096, 5, "per_block"),
    # 9: S % 64 != 0: the whole chunks in place, the tails restrided
    _c(9, 32, 32, 1000, 9, "per_block"), _c(9, 32, 32, 62, 9, "per_block", PADS), _c(9, 32, 32, 66, 9, "per_block"),
    _c(9, 32, 32, 1022, 5), _c(9, 16, 4, 1000, 5, "per_block", PADS), _c(9, 20, 30, 130, 9, "per_block"),
    _c(9, 32, 64, 1000, 3, "per_block"),
    # 10: byte-odd layouts: the whole shards restrided
    _c(10, 32, 32, 1024, 5, "per_block", (1, 4, 6)), _c(10, 16, 4, 192, 7, "per_block", (0, 1, 2)),
    _c(10, 32, 32, 1000, 5, "per_block", (3, 2, 4)),
]


def case_id(c):
    return f"r{c.row}-{c.k}:{c.m}-S{c.S}-n{c.n}-{c.patterns}" + ("" if c.layout == PLAIN else "-L%d.%d.%d" % c.layout)


def case_seed(c):
    return ((c.k * 131 + c.m) * 8191 + c.S) * 257 + c.n * 16 + c.row


# --------------------------------------------------------------------- patterns and data

def _pattern(rng, k, m, e, x, erase=(), keep=()):
    """(op, rp) flags: e originals erased (those of `erase` among them), e + x recovery shards
    kept (those of `keep` among them)."""
    assert 0 <= e <= k and x >= 0 and e + x <= m and len(erase) <= e and len(keep) <= e + x
    lost = set(erase)
    lost |= set(rng.sample([i for i in range(k) if i not in lost], e - len(lost)))
    kept = set(keep)
    kept |= set(rng.sample([j for j in range(m) if j not in kept], e + x - len(kept)))
    return (np.array([0 if i in lost else 1 for i in range(k)], np.uint8),
            np.array([1 if j in kept else 0 for j in range(m)], np.uint8))


def surplus_patterns(rng, k, m):
    """The surplus patterns of a geometry (x >= 1 recovery shards more than needed, 1 <= e <=
    min(k, m - x) originals erased), each kind where the geometry admits it: x = 1 (original 0
    erased, recovery 0 kept); x >= 2 (original k - 1 erased, recovery m - 1 kept); lost recovery
    shards and surplus together; the full recovery set with some originals present; every
    original erased; one random pattern."""
    pats = []
    e = rng.randint(1, min(k, m - 1))
    pats.append(_pattern(rng, k, m, e, 1, erase=[0], keep=[0]))
    if m >= 3:
        x = rng.randint(2, min(5, m - 1))
        e = rng.randint(1, min(k, m - x))
        pats.append(_pattern(rng, k, m, e, x, erase=[k - 1], keep=[m - 1]))
        x = rng.randint(1, min(3, m - 2))           # e + x < m
        e = rng.randint(1, min(k, m - 1 - x))
        pats.append(_pattern(rng, k, m, e, x))
    if k >= 2:                                      # every recovery shard present, some originals too
        e = rng.randint(1, min(k - 1, m - 1))
        pats.append(_pattern(rng, k, m, e, m - e, erase=[0, k - 1][:min(e, 2)]))
    if m - 1 >= k:                                  # e = k
        pats.append(_pattern(rng, k, m, k, rng.randint(1, min(3, m - k))))
    x = rng.randint(1, min(4, m - 1))
    pats.append(_pattern(rng, k, m, rng.randint(1, min(k, m - x)), x))
    for op, rp in pats:
        e, kept = k - int(op.sum()), int(rp.sum())
        assert 1 <= e <= k and kept > e
    return pats


Call = namedtuple("Call", "op rp")  # (npat, k) and (npat, m) uint8 flags, npat == 1 or n


@functools.lru_cache(maxsize=None)
def case_calls(c):
    """The decode calls of a case.  "one": one call per surplus pattern of the geometry, the
    same pattern for every block.  "per_block": calls of n blocks, each with one block that
    lost nothing, one with exactly k shards present (no surplus) and n - 2 surplus patterns,
    in shuffled block order, until every surplus pattern of the geometry has been used."""
    rng = random.Random(case_seed(c))
    pats = surplus_patterns(rng, c.k, c.m)
    if c.patterns == "one":
        return tuple(Call(op[None], rp[None]) for op, rp in pats)
    per_call = c.n - 2
    assert per_call >= 1
    calls = []
    for i in range(0, len(pats), per_call):
        blk = [pats[(i + j) % len(pats)] for j in range(per_call)]
        none_rp = np.array([rng.randint(0, 1) for _ in range(c.m)], np.uint8)
        blk.append((np.ones(c.k, np.uint8), none_rp))
        blk.append(_pattern(rng, c.k, c.m, rng.randint(1, min(c.k, c.m)), 0))
        rng.shuffle(blk)
        calls.append(Call(np.stack([b[0] for b in blk]), np.stack([b[1] for b in blk])))
    return tuple(calls)


def case_data(c):
    """(orig (n, k, S), rec (n, m, S)): independent random bytes, nothing encoded."""
    rng = np.random.default_rng(case_seed(c))
    return (rng.integers(0, 256, (c.n, c.k, c.S), dtype=np.uint8),
            rng.integers(0, 256, (c.n, c.m, c.S), dtype=np.uint8))


def block_flags(call, b):
    i = b if call.op.shape[0] > 1 else 0
    return call.op[i], call.rp[i]


def drop_surplus(op, rp):
    """The ANY_K rule of the window decoders: the present originals, then the present recovery
    shards in index order until k survivors are reached."""
    budget = len(op) - int(op.sum())
    out = np.zeros_like(rp)
    for j in np.flatnonzero(rp):
        if budget == 0:
            break
        out[j] = 1
        budget -= 1
    return out


def damage(orig, rec, op, rp):
    d_o, d_r = orig.copy(), rec.copy()
    d_o[op == 0] = ABSENT_O
    d_r[rp == 0] = ABSENT_R
    return d_o, d_r


def chunks_differ(a, b):
    """Whether shards a and b differ in every 64-byte chunk and in the tail."""
    S = len(a)
    return all(not np.array_equal(a[p:p + 64], b[p:p + 64]) for p in range(0, S, 64))


@functools.lru_cache(maxsize=4)
def reference(c):
    """Per call the (n, k, S) originals the C oracle's every-shard decode leaves.  Asserts the
    teeth condition on the way: in every block with surplus, dropping the surplus recovery
    shards changes every 64-byte chunk (and the tail) of every restored shard."""
    orig, rec = case_data(c)
    wants = []
    for ci, call in enumerate(case_calls(c)):
        want = np.empty_like(orig)
        surplus_blocks = 0
        for b in range(c.n):
            op, rp = block_flags(call, b)
            d_o, d_r = damage(orig[b], rec[b], op, rp)
            want[b] = ro_c.decode(d_o, op, d_r, rp)
            assert np.array_equal(want[b][op == 1], orig[b][op == 1])
            if int(op.sum()) + int(rp.sum()) > c.k and int(op.sum()) < c.k:
                surplus_blocks += 1
                alt = ro_c.decode(d_o, op, d_r, drop_surplus(op, rp))
                for i in np.flatnonzero(op == 0):
                    assert chunks_differ(want[b, i], alt[i]), ("no teeth", case_id(c), ci, b, int(i))
        assert surplus_blocks >= (c.n if call.op.shape[0] == 1 else 1), (case_id(c), ci)
        want.setflags(write=False)
        wants.append(want)
    return tuple(wants)


# ----------------------------------------------------------------------------- fixture

GOLDEN_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "rs_exact_noncodeword.json")


@functools.lru_cache(maxsize=None)
def exact_golden():
    with open(GOLDEN_PATH) as f:
        return json.load(f)["decode_exact"]


def golden_block(g):
    """(orig (k, S), rec (m, S), op, rp) of a fixture entry: shard i of splitmix64(seed)."""
    k, m, S = g["k"], g["m"], g["S"]
    raw = np.frombuffer(o.splitmix64_bytes(g["seed"], (k + m) * S), np.uint8).reshape(k + m, S)
    op = np.ones(k, np.uint8)
    op[g["erased_original"]] = 0
    rp = np.zeros(m, np.uint8)
    rp[g["present_recovery"]] = 1
    return raw[:k].copy(), raw[k:].copy(), op, rp


def restored_sha(restored, op):
    return hashlib.sha256(b"".join(restored[i].tobytes() for i in np.flatnonzero(op == 0))).hexdigest()


# --------------------------------------------------------------------------- CPU tests

def test_case_list_covers_the_pattern_kinds():
    """Every geometry's patterns hold what the window-offset mistakes need: surplus 1 and >= 2,
    lost recovery with surplus, the full recovery set with originals present, e = k, and the
    edge shards (original 0 / k - 1 erased, recovery 0 / m - 1 kept) -- each where m admits it;
    per-block calls also a block that lost nothing and one with exactly k present."""
    assert len({case_id(c) for c in CASES}) == len(CASES)
    for c in CASES:
        k, m = c.k, c.m
        calls = case_calls(c)
        flags = [(call.op[p], call.rp[p]) for call in calls for p in range(call.op.shape[0])]
        ex = [(k - int(op.sum()), int(rp.sum()) - (k - int(op.sum())), op, rp) for op, rp in flags]
        sur = [t for t in ex if t[0] >= 1 and t[1] >= 1]
        assert any(x == 1 for e, x, _, _ in sur), case_id(c)
        assert any(op[0] == 0 for _, _, op, _ in sur) and any(rp[0] == 1 for _, _, _, rp in sur)
        if m >= 3:
            assert any(x >= 2 for e, x, _, _ in sur), case_id(c)
            assert any(e + x < m for e, x, _, _ in sur), case_id(c)
            assert any(op[k - 1] == 0 for _, _, op, _ in sur) and any(rp[m - 1] == 1 for _, _, _, rp in sur)
        if k >= 2:
            assert any(e + x == m and e < k for e, x, _, _ in sur), case_id(c)
        if m - 1 >= k:
            assert any(e == k for e, x, _, _ in sur), case_id(c)
        for call in calls:
            assert call.op.shape[0] == (1 if c.patterns == "one" else c.n)
            if c.patterns == "per_block":
                per = [(k - int(call.op[b].sum()), int(call.rp[b].sum())) for b in range(c.n)]
                assert any(e == 0 for e, _ in per) and any(e >= 1 and kept == e for e, kept in per), case_id(c)
                assert any(kept > e >= 1 for e, kept in per), case_id(c)


def test_oracles_agree_on_noncodewords():
    """Python, C scalar and (whole chunks, AVX2 hosts) the restated Avx2 engine restore the same
    bytes from random shards with surplus: every case geometry at S <= 192, up to four blocks
    per call."""
    checked = avx = 0
    for c in CASES:
        if c.S > 192:
            continue
        orig, rec = case_data(c)
        for call in case_calls(c):
            for b in range(min(c.n, 4)):
                op, rp = block_flags(call, b)
                if int(op.sum()) == c.k:
                    continue
                d_o, d_r = damage(orig[b], rec[b], op, rp)
                want = ro_c.decode(d_o, op, d_r, rp)
                res = o.decode(c.k, c.m, {int(i): d_o[i].tobytes() for i in np.flatnonzero(op)},
                               {int(j): d_r[j].tobytes() for j in np.flatnonzero(rp)})
                assert sorted(res) == [int(i) for i in np.flatnonzero(op == 0)]
                for i, v in res.items():
                    assert v == want[i].tobytes(), (case_id(c), b, i)
                checked += 1
                if c.S % 64 == 0 and ro_c.avx2_available():
                    got = ro_c.decode_blocks(np.concatenate([d_o, d_r])[None], c.k, op, rp, engine="avx2")[0]
                    assert np.array_equal(got, want), (case_id(c), b)
                    avx += 1
    assert checked > 100 and (avx > 50 or not ro_c.avx2_available())


def test_absent_shards_are_never_read():
    """Two different garbage fills of the absent shards give the same oracle output (else the
    GPU expectations would depend on the filler)."""
    for c in CASES:
        if c.S > 256:
            continue
        orig, rec = case_data(c)
        call = case_calls(c)[0]
        op, rp = block_flags(call, min(1, c.n - 1))
        d_o, d_r = damage(orig[0], rec[0], op, rp)
        g_o, g_r = d_o.copy(), d_r.copy()
        rng = np.random.default_rng(5)
        g_o[op == 0] = rng.integers(0, 256, g_o[op == 0].shape, dtype=np.uint8)
        g_r[rp == 0] = rng.integers(0, 256, g_r[rp == 0].shape, dtype=np.uint8)
        a, b = ro_c.decode(d_o, op, d_r, rp), ro_c.decode(g_o, op, g_r, rp)
        assert np.array_equal(a[op == 0], b[op == 0]), case_id(c)


@pytest.mark.parametrize("row", sorted({c.row for c in CASES}))
def test_teeth_every_case_discriminates(row):
    """Oracle alone: on every block with surplus the every-shard result differs from the
    first-k-survivors result in every 64-byte chunk of every restored shard -- a decoder that
    drops surplus shards fails every case of the list, in every chunk."""
    for c in CASES:
        if c.row == row:
            reference(c)


def test_exact_fixture_matches_c_oracle():
    """tests/golden/rs_exact_noncodeword.json (written from the Python oracle by
    make_exact_golden.py) against the C oracle, and its entries are surplus non-codewords."""
    gold = exact_golden()
    assert 8 <= len(gold) <= 16
    for g in gold:
        orig, rec, op, rp = golden_block(g)
        assert int(rp.sum()) > g["k"] - int(op.sum()) >= 1
        d_o, d_r = damage(orig, rec, op, rp)
        want = ro_c.decode(d_o, op, d_r, rp)
        assert restored_sha(want, op) == g["restored_sha256"], g
        alt = ro_c.decode(d_o, op, d_r, drop_surplus(op, rp))
        assert all(chunks_differ(want[i], alt[i]) for i in np.flatnonzero(op == 0)), g


# --------------------------------------------------- coder slices (CPU-built, GPU-checked)

CODER_M = (32, 33, 64)
CODER_S = (1024, 96, 1000, 64, 2)
ABSENT_C = 0xAB

# verdict: the oracle's (payload, data shreds, coding shreds) or its error kind
Slice = namedtuple("Slice", "kind damaged keep honest_payload honest_data verdict")


def _payload_len(rng, S):
    """A payload length whose shred size is S, its padding inside the last min(64, S) bytes."""
    return 32 * S - rng.randint(1, min(64, S))


def _oracle_verdict(cw, keep, m, S):
    orig = {i: cw[i * S:(i + 1) * S].tobytes() for i in range(32) if i in keep}
    rec = {j: cw[(32 + j) * S:(33 + j) * S].tobytes() for j in range(m) if 32 + j in keep}
    try:
        payload, raw = o.coder_deshred_indexed(orig, rec, m)
    except o.RSError as err:  # the wrapper's NotEnoughShreds maps to the crate status code
        return {"NotEnoughShreds": "NotEnoughShards"}.get(err.kind, err.kind)
    return payload, b"".join(raw.data), b"".join(raw.coding)


def make_slice(kind, m, S, seed, surplus=1):
    """One coder slice of shred size S with num_coding m.
    a: honest, 32 + surplus shreds kept.
    b: crafted non-codeword with valid padding: the data shreds holding the padding kept, about
       20 other data shreds erased, enough coding shreds for `surplus`, one kept coding shred
       replaced by random bytes.
    c: like b with the padding's data shreds erased too.
    d: exactly 32 kept, one kept coding shred random (the codeword through them is unique).
    e: 31 kept."""
    rng = random.Random(seed)
    plen = _payload_len(rng, S)
    payload = o.splitmix64_bytes(seed, plen)
    raw = o.coder_shred(payload, m)
    assert len(raw.data[0]) == S
    cw = np.frombuffer(b"".join(raw.data) + b"".join(raw.coding), np.uint8).copy()
    pad_shreds = [i for i in range(32) if (i + 1) * S > plen]
    others = [i for i in range(32) if i not in pad_shreds]
    if kind == "a":
        keep = set(rng.sample(range(32 + m), 32 + surplus))
    elif kind == "e":
        keep = set(rng.sample(range(32 + m), 31))
    else:
        erased = set(rng.sample(others, min(20, len(others))))
        if kind == "c":
            erased |= set(pad_shreds)
        ncoding = len(erased) + (0 if kind == "d" else surplus)
        coding = rng.sample(range(m), ncoding)
        keep = {i for i in range(32) if i not in erased} | {32 + j for j in coding}
        t = 32 + rng.choice(coding)
        cw[t * S:(t + 1) * S] = np.frombuffer(o.splitmix64_bytes(seed ^ 0x7A3, S), np.uint8)
    damaged = cw.copy()
    for i in range(32 + m):
        if i not in keep:
            damaged[i * S:(i + 1) * S] = ABSENT_C
    return Slice(kind, damaged, frozenset(keep), payload, b"".join(raw.data), _oracle_verdict(cw, keep, m, S))


CODER_KINDS = (("a", 3), ("b", 1), ("b", 2), ("c", 2), ("d", 0), ("e", 0), ("b", 4), ("a", 1))


@functools.lru_cache(maxsize=None)
def coder_slices(m, S):
    return tuple(make_slice(kind, m, S, 7000 + 97 * m + 13 * S + b, x) for b, (kind, x) in enumerate(CODER_KINDS))


def check_slice_proves_something(s, S):
    """Oracle alone: a crafted slice with valid padding restores the honest length and a
    different payload (every restored data shred differs from the honest one); an honest one
    its own payload."""
    if s.kind == "a":
        assert s.verdict[0] == s.honest_payload
    if s.kind == "b":
        assert not isinstance(s.verdict, str), "the kept padding strips"
        assert len(s.verdict[0]) == len(s.honest_payload) and s.verdict[0] != s.honest_payload
        changed = [i for i in range(32) if s.verdict[1][i * S:(i + 1) * S] != s.honest_data[i * S:(i + 1) * S]]
        assert changed == [i for i in range(32) if i not in s.keep]  # every restored data shred, no kept one
    if s.kind == "e":
        assert s.verdict == "NotEnoughShards"


@pytest.mark.parametrize("m", CODER_M)
def test_crafted_slices_strip_to_a_changed_payload(m):
    """Oracle alone, every size of the GPU test."""
    for S in CODER_S:
        for s in coder_slices(m, S):
            check_slice_proves_something(s, S)


# --------------------------------------------------------------------------- GPU tests

def _torch():
    return pytest.importorskip("torch")


@pytest.fixture(scope="module")
def dev(ctx):
    """All torch work and every library launch go to one explicit (non-null) stream."""
    torch = _torch()
    d = torch.device("cuda:0")
    s = torch.cuda.Stream(d)
    torch.cuda.set_stream(s)
    ctx.set_stream(s.cuda_stream)
    return d


def to_dev(a, dev):
    return _torch().from_numpy(np.array(a, copy=True)).to(dev)


class Image:
    """Originals and recovery of n blocks in two buffers: GUARD + shift bytes of GAP, then block
    b at b * stride (stride = count * S + pad), GAP in the pads and GUARD bytes after."""

    def __init__(self, count, S, n, shift, pad):
        self.count, self.S, self.n, self.stride = count, S, n, count * S + pad
        self.base = GUARD + shift
        self.size = self.base + n * self.stride + GUARD

    def fill(self, shards):  # (n, count, S)
        img = np.full(self.size, GAP, np.uint8)
        for b in range(self.n):
            p = self.base + b * self.stride
            img[p:p + self.count * self.S] = shards[b].reshape(-1)
        return img

    def where(self, pos):
        """Names byte `pos` of the image for an assertion message."""
        q = pos - self.base
        if q < 0 or q >= self.n * self.stride:
            return f"byte {pos}: guard"
        b, r = divmod(q, self.stride)
        return f"block {b} gap byte {r}" if r >= self.count * self.S else f"block {b} shard {r // self.S} byte {r % self.S}"


def assert_image(got, want, image, what):
    if not np.array_equal(got, want):
        bad = np.flatnonzero(got != want)
        raise AssertionError(f"{what}: {bad.size} bytes differ, first at {image.where(int(bad[0]))}, "
                             f"last at {image.where(int(bad[-1]))}")


def run_exact_call(ctx, dev, c, call, want, orig, rec, mode=None):
    """One decode_batch of case c's data under `call`'s flags.  Checks the whole originals image
    (erased originals = `want`, present ones and every gap / guard byte unchanged) and that the
    recovery image is unchanged.  Returns the decode classes."""
    shift, pad_o, pad_r = c.layout
    io, ir = Image(c.k, c.S, c.n, shift, pad_o), Image(c.m, c.S, c.n, shift, pad_r)
    d_o, d_r = np.empty_like(orig), np.empty_like(rec)
    for b in range(c.n):
        d_o[b], d_r[b] = damage(orig[b], rec[b], *block_flags(call, b))
    img_o, img_r = io.fill(d_o), ir.fill(d_r)
    t_o, t_r = to_dev(img_o, dev), to_dev(img_r, dev)
    rs.decode_batch(ctx, c.k, c.m, c.S, c.n, t_o.data_ptr() + io.base, io.stride, t_r.data_ptr() + ir.base, ir.stride,
                    np.ascontiguousarray(call.op), np.ascontiguousarray(call.rp),
                    mode=rs.DECODE_EXACT if mode is None else mode)
    classes = rs.last_decode_classes(ctx)
    assert_image(t_r.cpu().numpy(), img_r, ir, "recovery buffer changed")
    assert_image(t_o.cpu().numpy(), io.fill(want), io, "originals")
    return classes


def expected_classes(c, call):
    """The decoder classes of a call, from classify_patterns' rules for EXACT: a pattern that
    lost no original is "none"; HighRate geometries with a window of 32 or 64 positions
    (next_pow2(next_pow2(m) + k)) take window64 whatever the surplus; every other geometry takes
    the generic kernel when surplus shards are present, and with exactly k present the W = 128
    window where the geometry has one (64:64, 32:64), else the generic kernel too.  A shard size
    with whole chunks and a tail counts every pattern twice (the whole-chunk pass and the
    restrided tail pass add up); a byte-odd layout restrides the whole shards: one pass."""
    passes = 1 if c.row != 9 else (c.S // 64 > 0) + (c.S % 64 > 0)
    windowed = c.row != 8 and (c.k, c.m) != (32, 64)
    want = {}
    for p in range(call.op.shape[0]):
        e, kept = c.k - int(call.op[p].sum()), int(call.rp[p].sum())
        if e == 0:
            name = "none"
        elif windowed:
            name = "window64"
        else:
            name = "window128" if kept == e and (c.k, c.m) in ((64, 64), (32, 64)) else "generic"
        want[name] = want.get(name, 0) + passes
    return want


def check_classes(c, call, classes):
    names = set(classes)
    if c.row <= 7:
        assert names <= {"window64", "none"} and classes.get("window64", 0) > 0, classes
    elif c.row == 8 and c.patterns == "per_block":
        # exactly k present: the W = 128 window (EXACT takes it only then); surplus: generic
        assert names == {"window128", "generic", "none"}, classes
    elif c.row == 8:
        assert classes.get("generic", 0) > 0 and "window64" not in names, classes
    else:
        # (32:64 per block: its exactly-k block has the W = 128 window, like row 8's per-block case)
        assert names <= {"window64", "generic", "none"} | ({"window128"} if (c.k, c.m) == (32, 64) else set()), classes
        assert classes.get("window64", 0) + classes.get("generic", 0) > 0, classes
    assert classes == expected_classes(c, call), (classes, expected_classes(c, call))


@pytest.mark.gpu
@pytest.mark.parametrize("c", CASES, ids=case_id)
def test_exact_decode_batch_on_noncodewords(ctx, dev, c):
    """ag_rs_decode_batch, EXACT, random bytes with surplus shards, against the C oracle: the
    erased originals are the every-shard result, everything else (present originals, the
    recovery buffer with its absent shards' filler, pads and guards) is untouched, and the call
    took the decoder class its row names."""
    wants = reference(c)  # asserts the teeth condition before anything runs on the GPU
    orig, rec = case_data(c)
    for ci, (call, want) in enumerate(zip(case_calls(c), wants)):
        classes = run_exact_call(ctx, dev, c, call, want, orig, rec)
        print(f"classes {case_id(c)} call {ci}: {classes}")
        check_classes(c, call, classes)


@pytest.mark.gpu
def test_exact_masks_not_stale_after_any_k(ctx, dev):
    """The window-mask cache across modes: EXACT and ANY_K masks of one pattern set differ only
    through the surplus shards.  EXACT A, ANY_K A (honest codewords), EXACT B, ANY_K B, EXACT A,
    EXACT A again (the cached masks) on one context."""
    c = next(x for x in CASES if (x.row, x.k, x.m, x.S, x.n) == (5, 32, 32, 4096, 6))
    calls, wants = case_calls(c), reference(c)
    assert len(calls) >= 2 and not np.array_equal(calls[0].rp, calls[1].rp)
    orig, rec = case_data(c)
    honest_rec = ro_c.encode_blocks(orig, c.m, threads=4)

    def exact(i):
        classes = run_exact_call(ctx, dev, c, calls[i], wants[i], orig, rec)
        assert classes.get("window64", 0) > 0 and set(classes) <= {"window64", "none"}, classes

    def any_k(i):
        run_exact_call(ctx, dev, c, calls[i], orig, orig, honest_rec, mode=rs.DECODE_ANY_K)

    for step, i in ((exact, 0), (any_k, 0), (exact, 1), (any_k, 1), (exact, 0), (exact, 0)):
        step(i)


@pytest.mark.gpu
@pytest.mark.parametrize("S", CODER_S)
@pytest.mark.parametrize("m", CODER_M)
def test_coder_deshred_batch_exact_on_crafted_slices(ctx, dev, m, S):
    """ag_rs_coder_deshred_batch, EXACT, against the oracle's ReedSolomonCoder::deshred on
    honest slices with surplus, crafted non-codewords whose padding still strips (the restored
    payload differs from the honest one; the tampered kept coding shred comes back as the
    re-encode of the restored data), crafted ones with the padding erased, exactly 32 kept with
    one random, and 31 kept."""
    slices = coder_slices(m, S)
    for s in slices:
        check_slice_proves_something(s, S)
    n, stride = len(slices), (32 + m) * S
    damaged = np.stack([s.damaged for s in slices])
    dp = [1 if i in s.keep else 0 for s in slices for i in range(32)]
    cp = [1 if 32 + j in s.keep else 0 for s in slices for j in range(m)]
    d_cw = to_dev(damaged, dev)
    res = rs.coder_deshred_batch(ctx, m, n, S, d_cw, stride, dp, cp, rs.DECODE_EXACT)
    host = d_cw.cpu().numpy()
    check_coder_results(slices, res, host, [S] * n, m)


def check_coder_results(slices, res, host, sizes, m):
    for b, (s, S) in enumerate(zip(slices, sizes)):
        if isinstance(s.verdict, str):
            assert res[b] == s.verdict, (b, s.kind, res[b])
            for i in s.keep:  # the kept shreds untouched (absent ones unspecified)
                assert host[b, i * S:(i + 1) * S].tobytes() == s.damaged[i * S:(i + 1) * S].tobytes(), (b, s.kind, i)
            continue
        payload, data, coding = s.verdict
        assert res[b] == len(payload), (b, s.kind, res[b])
        assert host[b, :len(payload)].tobytes() == payload, (b, s.kind)
        assert host[b, :32 * S].tobytes() == data, (b, s.kind)
        assert host[b, 32 * S:(32 + m) * S].tobytes() == coding, (b, s.kind)


@pytest.mark.gpu
def test_coder_deshred_batch_var_exact_on_crafted_slices(ctx, dev):
    """ag_rs_coder_deshred_batch_var with mixed shred sizes in one call, EXACT with surplus on
    crafted non-codewords: the documented fallback (no var_decode kernel), compared with the
    oracle directly."""
    m, sizes = 32, [2, 64, 96, 1000, 1010, 1024] * 2
    kinds = [("a", 2), ("b", 1), ("d", 0), ("b", 3), ("a", 1), ("b", 2), ("b", 4), ("d", 0), ("a", 3), ("d", 0),
             ("b", 1), ("b", 2)]
    slices = [make_slice(kind, m, S, 9100 + 31 * b + S, x) for b, (S, (kind, x)) in enumerate(zip(sizes, kinds))]
    for s, S in zip(slices, sizes):
        check_slice_proves_something(s, S)
    n, stride, fill = len(slices), 64 * 1024 + 32, 0x77
    damaged = np.full((n, stride), fill, np.uint8)
    for b, s in enumerate(slices):
        damaged[b, :64 * sizes[b]] = s.damaged
    dp = [1 if i in s.keep else 0 for s in slices for i in range(32)]
    cp = [1 if 32 + j in s.keep else 0 for s in slices for j in range(m)]
    d_cw = to_dev(damaged, dev)
    res = rs.coder_deshred_batch_var(ctx, m, n, sizes, d_cw, stride, dp, cp, rs.DECODE_EXACT)
    assert "var_decode" not in rs.last_window_kernels(ctx)
    host = d_cw.cpu().numpy()
    check_coder_results(slices, res, host, sizes, m)
    for b, S in enumerate(sizes):
        assert (host[b, 64 * S:] == fill).all(), (b, S)


@pytest.mark.gpu
@pytest.mark.parametrize("k,m,S", [(16, 4, 192), (20, 30, 64), (32, 64, 128), (32, 32, 1000)])
def test_decoder_crate_api_exact_on_noncodewords(ctx, k, m, S):
    """The per-call ReedSolomonDecoder on random bytes with surplus 2, against the C oracle."""
    rng = np.random.default_rng(k * 1000 + m * 10 + S)
    orig = rng.integers(0, 256, (k, S), dtype=np.uint8)
    rec = rng.integers(0, 256, (m, S), dtype=np.uint8)
    prng = random.Random(k + m + S)
    op, rp = _pattern(prng, k, m, prng.randint(1, min(k, m - 2)), 2, erase=[0], keep=[m - 1])
    d_o, d_r = damage(orig, rec, op, rp)
    want = ro_c.decode(d_o, op, d_r, rp)
    alt = ro_c.decode(d_o, op, d_r, drop_surplus(op, rp))
    assert all(chunks_differ(want[i], alt[i]) for i in np.flatnonzero(op == 0))
    dec = rs.ReedSolomonDecoder(ctx, k, m, S)
    for i in np.flatnonzero(op):
        dec.add_original_shard(int(i), orig[i].tobytes())
    for j in np.flatnonzero(rp):
        dec.add_recovery_shard(int(j), rec[j].tobytes())
    res = dec.decode()
    assert sorted(res) == [int(i) for i in np.flatnonzero(op == 0)]
    for i, v in res.items():
        assert v == want[i].tobytes(), i


@pytest.mark.gpu
def test_exact_fixture_through_decode_batch(ctx, dev):
    """The fixture entries through ag_rs_decode_batch, one block each: the SHA-256 of the
    restored originals."""
    for g in exact_golden():
        orig, rec, op, rp = golden_block(g)
        k, m, S = g["k"], g["m"], g["S"]
        io, ir = Image(k, S, 1, 0, 0), Image(m, S, 1, 0, 0)
        d_o, d_r = damage(orig, rec, op, rp)
        t_o, t_r = to_dev(io.fill(d_o[None]), dev), to_dev(ir.fill(d_r[None]), dev)
        rs.decode_batch(ctx, k, m, S, 1, t_o.data_ptr() + io.base, io.stride, t_r.data_ptr() + ir.base, ir.stride,
                        op, rp, mode=rs.DECODE_EXACT)
        out = t_o.cpu().numpy()
        got = out[io.base:io.base + k * S].reshape(k, S)
        assert restored_sha(got, op) == g["restored_sha256"], g
        assert np.array_equal(got[op == 1], orig[op == 1]), g
        assert (out[:io.base] == GAP).all() and (out[io.base + k * S:] == GAP).all(), g
