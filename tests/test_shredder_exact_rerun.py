"""The composed deshreds' EXACT re-run as one batched pass: ag_shredder_deshred_batch, _var and
_kind on batches where a Byzantine leader's slices arrive with more than 32 datagrams.

A slice that fails the padding or the Merkle check of the ANY_K pass while holding more than 32
kept shreds is decoded again with the crate's decoder over every kept shred (reed_solomon.rs:
154-166), which gives the crate's bytes and verdict (shredder.rs:282-311).  All such slices of a
call go through one compact batch: rs.last_exact_rerun(ctx) == (their number, 1), and (0, 0)
when there are none.

Two generators only, so that the re-run set is known exactly: honest slices (so.shred; for the
kind shredders the device's own shred call, whose datagrams test_shredder_pipeline.py pins to
so.shred_kind) and Byzantine ones (one raw shred XORed with 0x5A after encoding, the tree and
signature over the altered shreds).  Every datagram of a Byzantine slice validates, and no decode
of such a slice rebuilds its signed tree, so R is the number of Byzantine slices received with
more than 32 datagrams.  Byzantine slices and their neighbours are checked against
oracle/shredder_oracle.py (receive + deshred / deshred_kind), the other honest slices against
the leader's own datagrams and codewords.

Honest slices received with 31 datagrams are part of the mix, so "every slice OK" in the honest
reruns reads: OK wherever 32 or more datagrams arrived, NotEnoughShards for the 31-datagram ones.

Buffers start at 0xA5 so stray writes show.
"""

import functools
import random

import numpy as np
import pytest

import ed25519_oracle as ed
import rs_oracle as o
import shredder_oracle as so
import slice_oracle as sl
from alpenglow_amd import rs

FILL = 0xA5
PKT = 1536
SEED = bytes(range(7, 39))
PK = ed.secret_to_public(SEED)

# slice types of a batch: Byzantine with surplus datagrams ("BS": the re-run set), honest with
# exactly 32 / surplus / 31, Byzantine with exactly 32 (altered shred held / lacking)
BS, H32, HS, H31, B32, B32L = "BS", "H32", "HS", "H31", "B32", "B32L"

# case 1, n = 24: BS at 0, 5 + 6 (adjacent), 10 (isolated), 13, 16, 19, 21, 23 -> R = 9
OTHERS_24 = {1: H32, 2: HS, 3: H31, 4: B32, 7: H32, 8: HS, 9: B32L, 11: H32, 12: HS, 14: H31, 15: H32, 17: HS,
             18: H32, 20: H32, 22: HS}
# case 1, n = 48: 12 others (3 is an isolated BS, 0 and 47 are BS) -> R = 36
OTHERS_48 = {2: H32, 4: HS, 9: H31, 13: B32, 17: H32, 21: HS, 25: B32L, 29: H32, 33: H31, 37: HS, 41: H32, 45: HS}
# case 2, n = 40 -> R = 12
OTHERS_40 = {p: t for p, t in zip([b for b in range(40) if b not in (0, 3, 4, 8, 12, 17, 21, 22, 26, 30, 35, 39)],
                                  [H32, HS, H31, B32, H32, HS, B32L, H32] * 4)}
VAR_SIZES = [2, 14, 66, 512, 1000, 1008, 1016, 1022, 1024]
VAR_STRIDE = 64 * 1024 + 32  # above 64 * max S, a multiple of 16
# case 3, n = 24 -> R = 6 (0, 6 + 7 adjacent, 12 isolated, 18, 23).  The oracle's AES is Python:
# a slice that decodes costs it a second at S = 1024, so the neighbours of Byzantine slices, which
# all go through the oracle, are picked to keep that to a handful (four honest ones that succeed)
OTHERS_KIND = {1: HS, 2: H32, 3: HS, 4: H32, 5: H31, 8: H32, 9: HS, 10: H31, 11: B32, 13: HS, 14: H32, 15: HS,
               16: H32, 17: H31, 19: H32, 20: HS, 21: H31, 22: B32}
KINDS = [so.CODING_ONLY, so.PETS, so.AONT]

# the Byzantine-surplus variants in turn: the altered shred held / lacking at the cycling kept
# counts, and the three recipes of test_deshred_batch_matches_oracle's cases 9-11 (coding shred
# 62 altered with data 16..31 or 8..23 missing; data shred 5 altered, held with 40 others)
BS_VARIANTS = ["held", "lack", "c9", "held", "c10", "held", "c11", "held"]
HELD_COUNTS = [33, 40, 48, 64]
LACK_COUNTS = [40, 33, 48]


def _slice(rng, S, i, kind=so.REGULAR):
    """One slice whose framed payload (+ the key tail of PETS / AONT) pads to shred size S."""
    extra = 16 if kind in (so.PETS, so.AONT) else 0
    lo, hi = 32 * S - 64 - extra, 32 * S - 1 - extra
    parent = (rng.randrange(1 << 40), rng.randbytes(32)) if i % 2 else None
    framed = rng.randrange(max(lo, sl.header_len(parent)), min(hi, sl.MAX_DATA_PER_SLICE - extra) + 1)
    return (parent, rng.randbytes(framed - sl.header_len(parent)), rng.randrange(1 << 32), rng.randrange(1024),
            bool(i % 3 == 2), rng.randbytes(16))


def _non_codeword(kind, slice_, raw, tamper):
    """The 64 datagrams of a leader that signs shreds which are no codeword: the slice's output
    raw shreds with shred `tamper` altered after encoding (test_shredder_pipeline._non_codeword)."""
    nd = so.DATA_OUT[kind]
    shards = list(raw.data) + list(raw.coding)
    shards[tamper] = bytes(x ^ 0x5A for x in shards[tamper])
    return so.datagrams(shards[:nd], shards[nd:], slice_[2], slice_[3], slice_[4], SEED)[0]


class Batch:
    """One generated batch: per slice its type, size, honest datagrams / raw shreds, the rows
    received (`rows`) and the rows received had every leader been honest (`honest_rows`)."""

    def __init__(self, seed, n, sizes, others, kind=so.REGULAR, leader=None):
        """leader (optional): slices -> [(64 datagrams, output RawShreds)], the honest leader's
        shred call on the device; default: the oracle's shred_kind."""
        rng = random.Random(seed)
        self.n, self.kind, self.sizes = n, kind, sizes
        self.types = [others.get(b, BS) for b in range(n)]
        self.slices, self.full, self.raw, self.rows, self.honest_rows, self.tamper = [], [], [], [], [], []
        made = None
        if leader is not None:
            srng = random.Random(seed + 1)
            made = [_slice(srng, S, b, kind) for b, S in enumerate(sizes)]
            shredded = leader(made)
        i_bs = i_held = i_lack = 0
        for b, (t, S) in enumerate(zip(self.types, sizes)):
            if made is not None:
                s_, (full, raw) = made[b], shredded[b]
            else:
                s_ = _slice(rng, S, b, kind)
                full, raw, _, _ = so.shred_kind(kind, *s_[:5], SEED, s_[5])
            tamper, keep = None, None
            if t == BS:
                v = BS_VARIANTS[i_bs % len(BS_VARIANTS)] if kind == so.REGULAR else ("held", "lack")[i_bs == 1]
                if v == "c9":
                    tamper, keep = 62, set(range(16)) | set(range(32, 64))
                elif v == "c10":
                    tamper, keep = 62, set(range(8)) | set(range(24, 32)) | set(range(32, 64))
                elif v == "c11":
                    tamper = 5
                    keep = {5} | set(rng.sample([j for j in range(64) if j != 5], 40))
                elif v == "held":
                    tamper = rng.randrange(64)
                    cnt = HELD_COUNTS[i_held % 4]
                    i_held += 1
                    keep = {tamper} | set(rng.sample([j for j in range(64) if j != tamper], cnt - 1))
                else:
                    tamper = rng.randrange(64)
                    keep = set(rng.sample([j for j in range(64) if j != tamper], LACK_COUNTS[i_lack % 3]))
                    i_lack += 1
                i_bs += 1
            elif t in (B32, B32L):
                tamper = rng.randrange(64)
                rest = [j for j in range(64) if j != tamper]
                keep = ({tamper} | set(rng.sample(rest, 31))) if t == B32 else set(rng.sample(rest, 32))
            else:
                cnt = {H32: 32, H31: 31, HS: (40, 64, 33, 48)[b % 4]}[t]
                keep = set(rng.sample(range(64), cnt))
            got = _non_codeword(kind, s_, raw, tamper) if tamper is not None else full
            self.slices.append(s_)
            self.full.append(full)
            self.raw.append(raw)
            self.tamper.append(tamper)
            self.rows.append([got[j] if j in keep else None for j in range(64)])
            self.honest_rows.append([full[j] if j in keep else None for j in range(64)])
        self.rerun = [b for b, t in enumerate(self.types) if t == BS]

    def kept(self, b):
        return sum(x is not None for x in self.rows[b])

    @functools.cached_property
    def want(self):
        """Per slice (status, result or None, the datagram slots after the call): the oracle's for
        Byzantine slices and their neighbours, the leader's own for the other honest slices."""
        byz = [t in (BS, B32, B32L) for t in self.types]
        out = []
        for b in range(self.n):
            if any(byz[max(b - 1, 0):b + 2]):
                out.append(_oracle(self.rows[b], self.sizes[b], self.kind))
            else:
                out.append(self.honest_want(b))
        return out

    def honest_want(self, b):
        if sum(x is not None for x in self.honest_rows[b]) < 32:
            return so.NOT_ENOUGH_SHARDS, None, [x if x is not None else b"" for x in self.honest_rows[b]]
        s_ = self.slices[b]
        return so.OK, dict(parent=s_[0], data=s_[1], raw=self.raw[b], header=(s_[2], s_[3], s_[4])), self.full[b]


def _oracle(rows, S, kind):
    kept = so.receive(rows, PK, S, so.DATA_OUT[kind])
    st, res = so.deshred_kind(kept, kind)
    if st == so.OK:
        slots = [rows[j] if kept[j] is not None else res["datagrams"][j] for j in range(64)]
    else:
        slots = [x if x is not None else b"" for x in rows]
    return st, res, slots


@functools.lru_cache(maxsize=None)
def uniform_batch(S):
    n, others = (24, OTHERS_24) if S in (1024, 1000) else (48, OTHERS_48)
    return Batch(0xE7AC7 + S, n, [S] * n, others)


@functools.lru_cache(maxsize=None)
def var_batch():
    others = OTHERS_40
    sizes, i_bs = [], 0
    for b in range(40):
        if b in others:
            sizes.append(VAR_SIZES[(b * 4 + 1) % 9])
        else:
            # the 12 re-run slices walk all nine sizes (the one received whole, which no decode
            # set tells apart, shares its size with another)
            sizes.append([2, 14, 66, 512, 1000, 1008, 1016, 1024, 1022, 2, 14, 1024][i_bs])
            i_bs += 1
    return Batch(0x5A12E5, 40, sizes, others)


_KIND_BATCHES = {}


def kind_batch(ctx, dev, kind, S):
    """The kind batches' honest datagrams and raw shreds come from the device's own shred call
    (as test_pipeline_kind_roundtrip_random_arrival's), the Byzantine ones from those raw shreds."""
    if (kind, S) not in _KIND_BATCHES:
        _KIND_BATCHES[kind, S] = Batch(0xC0DE + 97 * kind + S, 24, [S] * 24, OTHERS_KIND, kind,
                                       leader=lambda slices: _gpu_leader(ctx, dev, kind, slices, S))
    return _KIND_BATCHES[kind, S]


# ------------------------------------------------------------------------------ CPU

def _restored(kept):
    """The crate decoder's restored data shreds over exactly the given shreds (before any padding check)."""
    return o.decode(32, 32, {j: x["data"] for j, x in enumerate(kept[:32]) if x is not None},
                    {j: x["data"] for j, x in enumerate(kept[32:]) if x is not None})


def _any_k(kept):
    """The ANY_K survivor set: the present originals, then recovery shards in index order up to 32."""
    out, cnt = [None] * 64, 0
    for j in range(64):
        if kept[j] is not None and cnt < 32:
            out[j] = kept[j]
            cnt += 1
    return out


def test_layouts():
    for n, others, R in ((24, OTHERS_24, 9), (48, OTHERS_48, 36), (40, OTHERS_40, 12), (24, OTHERS_KIND, 6)):
        bs = [b for b in range(n) if b not in others]
        assert len(bs) == R and 0 in bs and n - 1 in bs
        assert any(b + 1 in bs for b in bs)                             # an adjacent pair
        assert any(b - 1 in others and b + 1 in others for b in bs)     # an isolated one
        assert {H32, HS, H31, B32} <= set(others.values())


def test_inputs_discriminate():
    """For every shred size that has re-run slices, some Byzantine-surplus slice decodes
    differently (status or restored bytes) from every kept shred than from its ANY_K survivors
    (tests/test_shredder_oracle.py::test_exact_and_any_k_disagree_on_non_codeword): a re-run that
    only repeated the ANY_K decode would be caught."""
    batches = [uniform_batch(S) for S in (1024, 1000, 64, 2)] + [var_batch()]
    for bt in batches:
        sizes = sorted({bt.sizes[b] for b in bt.rerun})
        if bt is batches[-1]:
            assert len(sizes) >= 6, sizes
        for S in sizes:
            differ = 0
            for b in bt.rerun:
                if bt.sizes[b] != S:
                    continue
                assert bt.kept(b) > 32
                kept = so.receive(bt.rows[b], PK, S)
                assert sum(x is not None for x in kept) == bt.kept(b)  # every datagram validates
                sub = _any_k(kept)
                differ += so.deshred(kept)[0] != so.deshred(sub)[0] or _restored(kept) != _restored(sub)
            assert differ >= 1, S
    # the kept counts cycle through 33, 40, 48 and 64, and both verdicts occur at S = 1024
    bt = uniform_batch(1024)
    assert {33, 40, 48, 64} <= {bt.kept(b) for b in bt.rerun}
    assert {so.BAD_ENCODING, so.INVALID_MERKLE_TREE} <= {bt.want[b][0] for b in bt.rerun}


# ------------------------------------------------------------------------------ GPU

torch = None


@pytest.fixture(scope="module")
def dev(ctx):
    global torch
    import torch as _torch

    torch = _torch
    d = torch.device("cuda:0")
    s = torch.cuda.Stream(d)
    torch.cuda.set_stream(s)
    ctx.set_stream(s.cuda_stream)
    return d


def _to_dev(a, dev):
    return torch.from_numpy(np.array(a, copy=True)).to(dev)


def _filled(shape, dev):
    return torch.full(shape, FILL, dtype=torch.uint8, device=dev)


def _gpu_leader(ctx, dev, kind, slices, S):
    """ag_shredder_shred_batch_kind over the slices -> per slice (its 64 datagrams, its output raw shreds)."""
    n, rows = len(slices), 32 + so.CODING[kind]
    maxd = max(len(s_[1]) for s_ in slices)
    data = np.zeros((n, maxd), np.uint8)
    for b, s_ in enumerate(slices):
        data[b, :len(s_[1])] = np.frombuffer(s_[1], np.uint8)
    stride = rows * S
    cw = torch.zeros((n, stride), dtype=torch.uint8, device=dev)
    pkts = torch.zeros((n * 64, PKT), dtype=torch.uint8, device=dev)
    lens = torch.zeros(n * 64, dtype=torch.int32, device=dev)
    rs.shredder_shred_batch_kind(ctx, kind, n, S, [s_[0] for s_ in slices], _to_dev(data, dev), maxd,
                                 [len(s_[1]) for s_ in slices], _to_dev(np.array([s_[2] for s_ in slices], np.uint64), dev),
                                 _to_dev(np.array([s_[3] for s_ in slices], np.uint64), dev),
                                 _to_dev(np.array([s_[4] for s_ in slices], np.uint8), dev),
                                 _to_dev(np.frombuffer(SEED, np.uint8), dev), _to_dev(np.frombuffer(PK, np.uint8), dev),
                                 _to_dev(np.frombuffer(b"".join(s_[5] for s_ in slices), np.uint8), dev), cw, stride, pkts,
                                 PKT, lens)
    torch.cuda.synchronize()
    p, ln, c = pkts.cpu().numpy(), lens.cpu().numpy(), cw.cpu().numpy().reshape(n, rows, S)
    out_rows = [r for r in range(rows) if (kind != so.CODING_ONLY or r >= 32) and (kind != so.PETS or r != 31)][:64]
    nd = so.DATA_OUT[kind]
    out = []
    for b in range(n):
        shreds = [c[b, r].tobytes() for r in out_rows]
        out.append(([p[b * 64 + j, :ln[b * 64 + j]].tobytes() for j in range(64)],
                    o.RawShreds(data=shreds[:nd], coding=shreds[nd:])))
    return out


def _pack(rows):
    n = len(rows)
    buf = np.full((n * 64, PKT), FILL, np.uint8)
    ln = np.zeros(n * 64, np.int32)
    for b, r in enumerate(rows):
        for j, p in enumerate(r):
            if p is not None:
                buf[b * 64 + j, :len(p)] = np.frombuffer(p, np.uint8)
                ln[b * 64 + j] = len(p)
    return buf, ln


def _run(ctx, dev, rows, kind, S=None, sizes=None, stride=None):
    """One deshred call into 0xA5-filled buffers -> (result, slots, lengths, codewords [n][stride],
    last_exact_rerun)."""
    n = len(rows)
    buf, ln = _pack(rows)
    d_buf, d_ln = _to_dev(buf, dev), _to_dev(ln, dev)
    pk = _to_dev(np.frombuffer(PK, np.uint8), dev)
    cw = _filled((n, stride), dev)
    if sizes is not None:
        res = rs.shredder_deshred_batch_var(ctx, n, sizes, d_buf, PKT, d_ln, pk, cw, stride)
    elif kind == so.REGULAR:
        res = rs.shredder_deshred_batch(ctx, n, S, d_buf, PKT, d_ln, pk, cw)
    else:
        res = rs.shredder_deshred_batch_kind(ctx, kind, n, S, d_buf, PKT, d_ln, pk, cw, stride)
    torch.cuda.synchronize()
    return res, d_buf.cpu().numpy(), d_ln.cpu().numpy(), cw.cpu().numpy(), rs.last_exact_rerun(ctx)


def _check(got, rows, sizes, want, rows_per_slice=64, raw_shreds=True):
    """Statuses, datagram slots, headers, parents, data and codeword rows against `want`; no byte
    past a slice's rows, or past a slot's datagram, is written."""
    res, buf, ln, cw, _ = got
    in_buf, in_ln = _pack(rows)
    assert res.status.tolist() == [w[0] for w in want], \
        ([rs.STATUS_KIND.get(int(x), int(x)) for x in res.status], [w[0] for w in want])
    for b, (S, (st, r, slots)) in enumerate(zip(sizes, want)):
        assert (cw[b, rows_per_slice * S:] == FILL).all(), (b, S)
        for j in range(64):
            t = 64 * b + j
            assert ln[t] == len(slots[j]), (b, S, j)
            assert buf[t, :ln[t]].tobytes() == slots[j], (b, S, j)
            assert (buf[t, max(ln[t], in_ln[t]):] == FILL).all(), (b, S, j)
        if st != so.OK:
            if raw_shreds and sum(x is not None for x in rows[b]) >= 32:
                _check_failed_rows(cw[b], rows[b], S, b)
            continue
        assert (int(res.slots[b]), int(res.slice_indices[b]), bool(res.is_last[b])) == r["header"], (b, S)
        assert res.parents[b] == r["parent"], (b, S)
        off, m = int(res.data_offsets[b]), int(res.data_lens[b])
        assert cw[b, off:off + m].tobytes() == r["data"], (b, S)
        if raw_shreds:
            assert cw[b, :64 * S].tobytes() == b"".join(r["raw"].data + r["raw"].coding), (b, S)


def _check_failed_rows(cw, rows, S, b):
    """The codeword of a failed Regular slice with 32 or more kept shreds (the re-run slices: the
    rows the scatter wrote back).  Where the crate's coder over every kept shred strips its padding
    (the slice fails later, at the Merkle check), all 64 rows are its data and re-encoded coding
    shreds; where it does not, every kept row is the payload received and every absent data row
    what the crate's decoder restored before the padding check."""
    kept = so.receive(rows, PK, S)
    try:
        _, raw = o.coder_deshred([(j < 32, x["data"]) if x is not None else None for j, x in enumerate(kept)], 32, 32)
        assert cw[:64 * S].tobytes() == b"".join(raw.data + raw.coding), (b, S)
        return
    except o.RSError as e:
        assert e.kind == "InvalidPadding", (b, S, e.kind)
    for j, x in enumerate(kept):
        if x is not None:
            assert cw[j * S:(j + 1) * S].tobytes() == x["data"], (b, S, j)
    for j, d in _restored(kept).items():
        assert cw[j * S:(j + 1) * S].tobytes() == d, (b, S, j)


@pytest.mark.gpu
@pytest.mark.parametrize("S", [1024, 1000, 64, 2])
def test_regular_uniform(ctx, dev, S):
    """S = 1024 / 1000: n = 24, R = 9 (144 compact columns: five 32-column tiles, the last one
    partial); S = 64 / 2: n = 48, R = 36 (one column per slice: two tiles, the second partial;
    S = 2 is the tail-only size whose re-run took the host coder)."""
    bt = uniform_batch(S)
    R = len(bt.rerun)
    assert (bt.n, R) == ((24, 9) if S >= 1000 else (48, 36))
    got = _run(ctx, dev, bt.rows, so.REGULAR, S=S, stride=64 * S)
    _check(got, bt.rows, bt.sizes, bt.want)
    assert got[4] == (R, 1)
    # every leader honest: nothing to re-run, nothing launched for it
    honest = _run(ctx, dev, bt.honest_rows, so.REGULAR, S=S, stride=64 * S)
    _check(honest, bt.honest_rows, bt.sizes, [bt.honest_want(b) for b in range(bt.n)])
    assert [int(x) for x in honest[0].status] == [so.NOT_ENOUGH_SHARDS if t == H31 else so.OK for t in bt.types]
    assert honest[4] == (0, 0)


@pytest.fixture(scope="module")
def var_got(ctx, dev):
    bt = var_batch()
    return _run(ctx, dev, bt.rows, so.REGULAR, sizes=bt.sizes, stride=VAR_STRIDE)


@pytest.mark.gpu
def test_regular_mixed_sizes(ctx, dev, var_got):
    """n = 40 over nine sizes, R = 12 over all nine: one pass whatever the number of sizes; the
    sentinel stays in every byte past 64 * S_s of the padded codeword stride."""
    bt = var_batch()
    assert len(bt.rerun) == 12 and len({bt.sizes[b] for b in bt.rerun}) >= 6
    _check(var_got, bt.rows, bt.sizes, bt.want)
    assert var_got[4] == (12, 1)
    honest = _run(ctx, dev, bt.honest_rows, so.REGULAR, sizes=bt.sizes, stride=VAR_STRIDE)
    _check(honest, bt.honest_rows, bt.sizes, [bt.honest_want(b) for b in range(bt.n)])
    assert honest[4] == (0, 0)


@pytest.mark.gpu
def test_regular_mixed_sizes_equal_uniform_calls(ctx, dev, var_got):
    """The same inputs regrouped by size through ag_shredder_deshred_batch: identical per-slice
    outputs -- statuses, headers, parents, data, datagram slots and lengths and every codeword
    row, the re-run slices' included (the rows the scatter wrote back) -- and one pass per call
    that has a slice to re-run."""
    bt = var_batch()
    res, buf, ln, cw, _ = var_got
    for S in sorted(set(bt.sizes)):
        idx = [b for b, s in enumerate(bt.sizes) if s == S]
        ures, ubuf, uln, ucw, urr = _run(ctx, dev, [bt.rows[b] for b in idx], so.REGULAR, S=S, stride=64 * S)
        r = sum(b in bt.rerun for b in idx)
        assert urr == (r, 1 if r else 0), S
        for g, b in enumerate(idx):
            where = (S, b)
            assert int(res.status[b]) == int(ures.status[g]), where
            assert (int(res.slots[b]), int(res.slice_indices[b]), int(res.is_last[b])) == \
                (int(ures.slots[g]), int(ures.slice_indices[g]), int(ures.is_last[g])), where
            assert res.parents[b] == ures.parents[g], where
            assert (int(res.data_offsets[b]), int(res.data_lens[b])) == \
                (int(ures.data_offsets[g]), int(ures.data_lens[g])), where
            # Every codeword row, but for one known difference that is older than the re-run and
            # not in a re-run slice: a slice that keeps exactly 32 shreds and fails the padding
            # check gets its absent coding rows written by the var call's fused decode (before the
            # strip), while the uniform call's host coder (S % 64 < 16) leaves them untouched.
            # Here: slice 38 (S = 2) and slice 16 (S = 66), both Byzantine with exactly 32 kept.
            same = [j for j in range(64) if np.array_equal(cw[b, j * S:(j + 1) * S], ucw[g, j * S:(j + 1) * S])]
            if len(same) < 64:
                assert (S, b) in ((2, 38), (66, 16)) and bt.types[b] == B32 and int(res.status[b]) == so.BAD_ENCODING
                assert all(j >= 32 and bt.rows[b][j] is None and (ucw[g, j * S:(j + 1) * S] == FILL).all()
                           for j in range(64) if j not in same), where
            assert np.array_equal(ln[64 * b:64 * b + 64], uln[64 * g:64 * g + 64]), where
            assert np.array_equal(buf[64 * b:64 * b + 64], ubuf[64 * g:64 * g + 64]), where


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("S", [1024, 64])
def test_kinds(ctx, dev, kind, S):
    """CodingOnly, PETS and AONT, n = 24, R = 6: the re-run covers the Byzantine-surplus slices
    and at most the failed slices with surplus -- never the whole batch."""
    bt = kind_batch(ctx, dev, kind, S)
    R = len(bt.rerun)
    assert R == 6
    rows_per_slice = 32 + so.CODING[kind]
    stride = rows_per_slice * S + 12  # a padded stride (multiple of 4, not of S)
    got = _run(ctx, dev, bt.rows, kind, S=S, stride=stride)
    _check(got, bt.rows, bt.sizes, bt.want, rows_per_slice, raw_shreds=False)
    failed_surplus = sum(w[0] != so.OK and bt.kept(b) > 32 for b, w in enumerate(bt.want))
    slices, passes = got[4]
    assert R <= slices <= failed_surplus < bt.n and passes == 1, got[4]
    honest = _run(ctx, dev, bt.honest_rows, kind, S=S, stride=stride)
    _check(honest, bt.honest_rows, bt.sizes, [bt.honest_want(b) for b in range(bt.n)], rows_per_slice,
           raw_shreds=False)
    assert honest[4] == (0, 0)


@pytest.mark.gpu
def test_single_slice_and_argument_errors(ctx, dev):
    """n = 1 and the argument errors stay what they are."""
    bt = uniform_batch(64)
    b = bt.rerun[0]
    got = _run(ctx, dev, [bt.rows[b]], so.REGULAR, S=64, stride=64 * 64)
    _check(got, [bt.rows[b]], [64], [bt.want[b]])
    assert got[4] == (1, 1)
    kb = kind_batch(ctx, dev, so.AONT, 64)
    b = kb.rerun[0]
    got = _run(ctx, dev, [kb.rows[b]], so.AONT, S=64, stride=64 * 64 + 12)
    _check(got, [kb.rows[b]], [64], [kb.want[b]], raw_shreds=False)
    assert got[4] == (0, 0)  # one slice: the whole call decodes with EXACT, nothing is re-run
    for call in (lambda: _run(ctx, dev, [bt.rows[0]], so.REGULAR, S=63, stride=64 * 64),
                 lambda: _run(ctx, dev, [bt.rows[0]], so.REGULAR, sizes=[64], stride=64 * 64 - 16),
                 lambda: _run(ctx, dev, [kb.rows[0]], so.AONT, S=64, stride=64 * 64 - 4)):
        with pytest.raises(rs.RSError) as e:
            call()
        assert e.value.kind == "InvalidArgument"
