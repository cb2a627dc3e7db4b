"""Batched ReedSolomonCoder over slices of mixed shred sizes: ag_rs_coder_shred_bytes,
ag_rs_coder_shred_batch_var and ag_rs_coder_deshred_batch_var against the oracle's
ReedSolomonCoder (rs_oracle.coder_shred / coder_deshred_indexed) and against the uniform calls
run slice by slice."""

import os
import random
import re

import numpy as np
import pytest

import rs_oracle as o
from alpenglow_amd import build, rs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "alpenglow_rs.h")
NEW = ("ag_rs_coder_shred_bytes", "ag_rs_coder_shred_batch_var", "ag_rs_coder_deshred_batch_var")

# T = S % 64 in {0, 2, 14, 16, 30, 32, 34, 62}, one-column and 16- / 17-column slices; the mix
# makes slices straddle 32- and 64-column tile edges
SIZES = [2, 4, 14, 16, 18, 30, 32, 34, 62, 64, 66, 78, 126, 128, 130, 190, 960, 962, 974, 976, 990, 1006, 1008, 1010,
         1022, 1024]
STRIDE = 64 * 1024 + 64
FILL = 0xA5    # bytes the calls must not write
ABSENT = 0x5A  # shreds that did not arrive


# ------------------------------------------------------------------------------ CPU

@pytest.fixture(scope="module")
def lib():
    build.build()
    return rs.load()


def test_symbols_declared_exported_and_callable(lib):
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = set(re.findall(r"\b(ag_\w+)\s*\(", text))
    for s in NEW:
        assert s in declared and s in rs.EXPORTS and hasattr(lib, s)
    for f in ("coder_shred_bytes", "coder_shred_batch_var", "coder_deshred_batch_var"):
        assert callable(getattr(rs, f))
    assert "var_encode" in rs.ENCODE_KERNELS and "var_decode" in rs.WINDOW_KERNELS


def test_shred_bytes_closed_form(lib):
    got = [rs.coder_shred_bytes(L) for L in range(32768)]
    assert got == [(L + 64 - L % 64) // 32 for L in range(32768)]


@pytest.mark.parametrize("L", [0, 63, 64, 65, 2047, 32247, 32703, 32704, 32767])
def test_shred_bytes_matches_oracle(lib, L):
    assert rs.coder_shred_bytes(L) == len(o.coder_shred(bytes(L), 32).data[0])


def test_shred_bytes_too_much_data(lib):
    with pytest.raises(rs.RSError) as e:
        rs.coder_shred_bytes(32768)
    assert e.value.kind == "TooMuchData"


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


def lens_for(rng, sizes):
    """A payload length inside each size's 64-byte window (reed_solomon.rs:94-95)."""
    return [rng.randrange(32 * S - 64, 32 * S) for S in sizes]


class Batch:
    """Seeded payloads for the given sizes and the oracle's codewords (computed once)."""

    def __init__(self, sizes, seed, m=32):
        rng = random.Random(seed)
        self.sizes = list(sizes)
        self.n = len(self.sizes)
        self.m = m
        self.lens = lens_for(rng, self.sizes)
        self.payloads = [o.splitmix64_bytes(seed * 1000 + b, L) for b, L in enumerate(self.lens)]
        self.codewords = []
        for p in self.payloads:
            raw = o.coder_shred(p, m)
            self.codewords.append(np.frombuffer(b"".join(raw.data) + b"".join(raw.coding), np.uint8))

    def pick(self, idx):
        """The same slices in another order (the oracle's codewords are shared, not recomputed)."""
        import copy

        other = copy.copy(self)
        for name in ("sizes", "lens", "payloads", "codewords"):
            setattr(other, name, [getattr(self, name)[i] for i in idx])
        return other

    def filled(self, stride=STRIDE, fill=FILL):
        """Host buffer holding every codeword, `fill` elsewhere."""
        cw = np.full((self.n, stride), fill, np.uint8)
        for b, c in enumerate(self.codewords):
            cw[b, :c.size] = c
        return cw


def shred_var(ctx, dev, lens, payloads, m=32, stride=STRIDE, inplace=False):
    n = len(lens)
    cw = np.full((n, stride), FILL, np.uint8)
    if inplace:
        for b, p in enumerate(payloads):
            cw[b, :len(p)] = np.frombuffer(p, np.uint8)
        d_cw = to_dev(cw, dev)
        sizes = rs.coder_shred_batch_var(ctx, m, n, None, 0, lens, d_cw, stride)
    else:
        P = 32768
        pay = np.zeros((n, P), np.uint8)
        for b, p in enumerate(payloads):
            pay[b, :len(p)] = np.frombuffer(p, np.uint8)
        d_pay, d_cw = to_dev(pay, dev), to_dev(cw, dev)
        sizes = rs.coder_shred_batch_var(ctx, m, n, d_pay, P, lens, d_cw, stride)
    ctx.synchronize()
    return sizes, d_cw.cpu().numpy()


def check_shred(batch, sizes, host, stride=STRIDE):
    assert list(sizes) == batch.sizes
    for b, S in enumerate(batch.sizes):
        used = (32 + batch.m) * S
        assert host[b, :used].tobytes() == batch.codewords[b].tobytes(), (b, S)
        assert (host[b, used:] == FILL).all(), (b, S)


def uniform_shred(ctx, dev, S, lens, payloads, m=32):
    """The uniform call on its own packed buffer: (n, (32 + m) * S)."""
    n = len(lens)
    P = 32768
    pay = np.zeros((n, P), np.uint8)
    for b, p in enumerate(payloads):
        pay[b, :len(p)] = np.frombuffer(p, np.uint8)
    d_pay = to_dev(pay, dev)
    d_cw = torch.zeros((n, (32 + m) * S), dtype=torch.uint8, device=dev)
    rs.coder_shred_batch(ctx, m, n, S, d_pay, P, lens, d_cw, (32 + m) * S)
    ctx.synchronize()
    return d_cw.cpu().numpy()


def uniform_deshred_one(ctx, dev, S, m, codeword, dp, cp, mode):
    """The uniform call on one slice: (result, bytes)."""
    d_cw = to_dev(codeword[:(32 + m) * S].reshape(1, -1), dev)
    res = rs.coder_deshred_batch(ctx, m, 1, S, d_cw, (32 + m) * S, dp, cp, mode, as_array=True)
    return int(res[0]), d_cw.cpu().numpy()[0]


def flags(keep, m=32):
    dp = np.array([[1 if i in k else 0 for i in range(32)] for k in keep], np.uint8)
    cp = np.array([[1 if 32 + j in k else 0 for j in range(m)] for k in keep], np.uint8)
    return dp, cp


def damage(cw, sizes, keep, m=32):
    out = cw.copy()
    for b, S in enumerate(sizes):
        for i in range(32 + m):
            if i not in keep[b]:
                out[b, i * S:(i + 1) * S] = ABSENT
    return out


@pytest.fixture(scope="module")
def once():
    return Batch(SIZES, 11)


@pytest.fixture(scope="module")
def big():
    rng = random.Random(2024)
    sizes = [rng.choice(SIZES) if b % 2 == 0 else 2 * rng.randrange(1, 513) for b in range(300)]
    rng.shuffle(sizes)
    return Batch(sizes, 12)


@pytest.mark.gpu
@pytest.mark.parametrize("order", ["ascending", "descending", "shuffled"])
def test_shred_every_size_once(ctx, dev, once, order):
    idx = list(range(once.n))
    if order == "descending":
        idx.reverse()
    elif order == "shuffled":
        random.Random(5).shuffle(idx)
    batch = once.pick(idx)
    sizes, host = shred_var(ctx, dev, batch.lens, batch.payloads)
    kernels = rs.last_encode_kernels(ctx)
    assert "var_encode" in kernels and "restride" not in kernels, kernels
    check_shred(batch, sizes, host)


@pytest.mark.gpu
@pytest.mark.parametrize("inplace", [False, True])
def test_shred_300_slices(ctx, dev, big, inplace):
    sizes, host = shred_var(ctx, dev, big.lens, big.payloads, inplace=inplace)
    assert rs.last_encode_kernels(ctx) == {"var_encode"}
    check_shred(big, sizes, host)


@pytest.mark.gpu
@pytest.mark.parametrize("sizes", [[1010], [2] * 64, [2, 1024] * 32, [1024] * 64],
                         ids=["one", "all2", "alternating", "all1024"])
def test_shred_degenerate_shapes(ctx, dev, sizes):
    rng = random.Random(len(sizes) + sizes[0])
    lens = lens_for(rng, sizes)
    payloads = [o.splitmix64_bytes(7000 + b, L) for b, L in enumerate(lens)]
    got_sizes, host = shred_var(ctx, dev, lens, payloads)
    assert list(got_sizes) == sizes
    for S in sorted(set(sizes)):
        sel = [b for b, x in enumerate(sizes) if x == S]
        want = uniform_shred(ctx, dev, S, [lens[b] for b in sel], [payloads[b] for b in sel])
        for i, b in enumerate(sel):
            assert host[b, :64 * S].tobytes() == want[i].tobytes(), (b, S)
            assert (host[b, 64 * S:] == FILL).all()


@pytest.fixture(scope="module")
def arrival(big):
    """Exactly 32 of 64 shreds kept per slice, and the oracle's deshred of them."""
    rng = random.Random(77)
    keep = [set(rng.sample(range(64), 32)) for _ in range(big.n)]
    want = []
    for b, S in enumerate(big.sizes):
        c = big.codewords[b]
        orig = {i: c[i * S:(i + 1) * S].tobytes() for i in range(32) if i in keep[b]}
        rec = {j: c[(32 + j) * S:(33 + j) * S].tobytes() for j in range(32) if 32 + j in keep[b]}
        payload, raw = o.coder_deshred_indexed(orig, rec, 32)
        want.append((len(payload), b"".join(raw.data) + b"".join(raw.coding)))
    return keep, want


@pytest.mark.gpu
@pytest.mark.parametrize("mode", [rs.DECODE_ANY_K, rs.DECODE_EXACT], ids=["any_k", "exact"])
def test_deshred_random_arrival(ctx, dev, big, arrival, mode):
    keep, want = arrival
    dp, cp = flags(keep)
    d_cw = to_dev(damage(big.filled(), big.sizes, keep), dev)
    res = rs.coder_deshred_batch_var(ctx, 32, big.n, big.sizes, d_cw, STRIDE, dp, cp, mode, as_array=True)
    assert "var_decode" in rs.last_window_kernels(ctx)
    assert "restride" not in rs.last_encode_kernels(ctx)
    host = d_cw.cpu().numpy()
    for b, S in enumerate(big.sizes):
        assert res[b] == want[b][0] == big.lens[b], (b, S)
        assert host[b, :64 * S].tobytes() == want[b][1], (b, S)
        assert (host[b, 64 * S:] == FILL).all(), (b, S)


@pytest.mark.gpu
def test_deshred_per_slice_outcomes(ctx, dev, once):
    """Coding shreds only, every data shred (re-encode only), 31 kept, 40 kept, and a payload
    without its 0x80 marker, over every size: status and bytes are the uniform call's for that
    slice alone.  The absent shred slots of a failed slice hold unspecified bytes (header,
    section 2b), so there the received shreds are compared, and that they did not change."""
    rng = random.Random(31)
    cw = once.filled()
    keep = []
    for b, S in enumerate(SIZES):
        case = b % 5
        if case == 0:
            keep.append(set(range(32, 64)))
        elif case == 1:
            keep.append(set(range(32)))
        elif case == 2:
            keep.append(set(rng.sample(range(64), 31)))
        elif case == 3:
            keep.append(set(rng.sample(range(64), 40)))
        else:  # a consistent codeword whose last data shard is all zero and whose data ends in 0x55
            data = bytearray(o.splitmix64_bytes(900 + b, 32 * S))
            data[31 * S:] = bytes(S)
            data[31 * S - 1] = 0x55
            shards = [bytes(data[i * S:(i + 1) * S]) for i in range(32)]
            cw[b, :64 * S] = np.frombuffer(b"".join(shards) + b"".join(o.encode(shards, 32)), np.uint8)
            keep.append(set(rng.sample(range(64), 32)))
    dp, cp = flags(keep)
    damaged = damage(cw, SIZES, keep)
    d_cw = to_dev(damaged, dev)
    res = rs.coder_deshred_batch_var(ctx, 32, len(SIZES), SIZES, d_cw, STRIDE, dp, cp, rs.DECODE_ANY_K, as_array=True)
    assert "var_decode" in rs.last_window_kernels(ctx) and "var_encode" in rs.last_encode_kernels(ctx)
    assert "restride" not in rs.last_encode_kernels(ctx)
    host = d_cw.cpu().numpy()
    for b, S in enumerate(SIZES):
        want_res, want = uniform_deshred_one(ctx, dev, S, 32, damaged[b], dp[b], cp[b], rs.DECODE_ANY_K)
        assert res[b] == want_res, (b, S, res[b], want_res)
        assert res[b] == {2: -9, 4: -21}.get(b % 5, once.lens[b]), (b, S)  # -NOT_ENOUGH_SHARDS, -INVALID_PADDING
        assert (host[b, 64 * S:] == FILL).all(), (b, S)
        if res[b] >= 0:
            assert host[b, :64 * S].tobytes() == want.tobytes(), (b, S)
            continue
        for i in keep[b]:
            assert host[b, i * S:(i + 1) * S].tobytes() == damaged[b, i * S:(i + 1) * S].tobytes(), (b, S, i)
            assert want[i * S:(i + 1) * S].tobytes() == damaged[b, i * S:(i + 1) * S].tobytes(), (b, S, i)


@pytest.mark.gpu
@pytest.mark.parametrize("m", [64, 33])
def test_fallback_other_coding_counts(ctx, dev, m):
    rng = random.Random(m)
    sizes = [rng.choice(SIZES) for _ in range(40)]
    lens = lens_for(rng, sizes)
    payloads = [o.splitmix64_bytes(5000 + b, L) for b, L in enumerate(lens)]
    got_sizes, host = shred_var(ctx, dev, lens, payloads, m=m, stride=96 * 1024 + 64)
    assert list(got_sizes) == sizes
    assert "var_encode" not in rs.last_encode_kernels(ctx)
    keep = [set(rng.sample(range(32 + m), rng.randrange(32, 40))) for _ in sizes]
    dp, cp = flags(keep, m)
    for b, S in enumerate(sizes):
        want = uniform_shred(ctx, dev, S, [lens[b]], [payloads[b]], m=m)[0]
        assert host[b, :(32 + m) * S].tobytes() == want.tobytes(), (b, S)
        assert (host[b, (32 + m) * S:] == FILL).all(), (b, S)
    damaged = damage(host, sizes, keep, m)
    d_cw = to_dev(damaged, dev)
    res = rs.coder_deshred_batch_var(ctx, m, 40, sizes, d_cw, 96 * 1024 + 64, dp, cp, rs.DECODE_ANY_K, as_array=True)
    assert "var_decode" not in rs.last_window_kernels(ctx)
    after = d_cw.cpu().numpy()
    for b, S in enumerate(sizes):
        want_res, want = uniform_deshred_one(ctx, dev, S, m, damaged[b], dp[b], cp[b], rs.DECODE_ANY_K)
        assert res[b] == want_res == lens[b], (b, S)
        assert after[b, :(32 + m) * S].tobytes() == want.tobytes(), (b, S)
        assert (after[b, (32 + m) * S:] == FILL).all(), (b, S)


@pytest.mark.gpu
def test_fallback_exact_with_surplus(ctx, dev):
    """EXACT reads every kept shred: with surplus shreds and one of them tampered the result is
    whatever the uniform call gives for that slice."""
    rng = random.Random(99)
    batch = Batch([rng.choice(SIZES) for _ in range(40)], 13)
    keep = [set(rng.sample(range(64), 40 if b % 2 else 32)) for b in range(batch.n)]
    dp, cp = flags(keep)
    damaged = damage(batch.filled(), batch.sizes, keep)
    S7 = batch.sizes[7]
    i7 = sorted(keep[7])[3]
    damaged[7, i7 * S7] ^= 0x01  # one tampered kept shred of a surplus slice
    d_cw = to_dev(damaged, dev)
    res = rs.coder_deshred_batch_var(ctx, 32, batch.n, batch.sizes, d_cw, STRIDE, dp, cp, rs.DECODE_EXACT,
                                     as_array=True)
    assert "var_decode" not in rs.last_window_kernels(ctx)
    assert "var_encode" not in rs.last_encode_kernels(ctx)
    host = d_cw.cpu().numpy()
    for b, S in enumerate(batch.sizes):
        want_res, want = uniform_deshred_one(ctx, dev, S, 32, damaged[b], dp[b], cp[b], rs.DECODE_EXACT)
        assert res[b] == want_res, (b, S)
        if b != 7:
            assert res[b] == batch.lens[b]
        assert host[b, :64 * S].tobytes() == want.tobytes(), (b, S)
        assert (host[b, 64 * S:] == FILL).all(), (b, S)


@pytest.mark.gpu
def test_argument_errors(ctx, dev):
    n, stride = 3, 64 * 1024
    d_cw = torch.full((n, stride), 0x77, dtype=torch.uint8, device=dev)
    L = rs.load()
    INVALID_SHARD_SIZE, UNSUPPORTED_SHARD_COUNT, TOO_MUCH_DATA, INVALID_ARGUMENT = 1, 10, 20, 100  # header, section 0

    def shred(m, count, lens, cw, st, out):
        a = np.asarray(lens if lens is not None else [], np.uint32)
        return L.ag_rs_coder_shred_batch_var(ctx.handle, m, count, None, 0, a.ctypes.data if lens is not None else None,
                                             cw, st, out.ctypes.data)

    def deshred(m, count, sizes, cw, st, mode, out, dp=True):
        a = np.asarray(sizes if sizes is not None else [], np.uint32)
        f = np.ones(count * 64 + 64, np.uint8)
        return L.ag_rs_coder_deshred_batch_var(ctx.handle, m, count, a.ctypes.data if sizes is not None else None, cw,
                                               st, f.ctypes.data if dp else None, f.ctypes.data, mode, out.ctypes.data)

    p = d_cw.data_ptr()
    sent32 = np.full(n, 0xDEAD, np.uint32)
    sent64 = np.full(n, -777, np.int64)
    cases = [
        (shred(32, n, [10, 32768, 10], p, stride, sent32), TOO_MUCH_DATA),
        (shred(32, n, [10, 32767, 10], p, 64 * 1024 - 2, sent32), INVALID_ARGUMENT),     # stride below 64 * max S
        (shred(32, n, None, p, stride, sent32), INVALID_ARGUMENT),                       # null lens
        (shred(32, n, [10, 10, 10], None, stride, sent32), INVALID_ARGUMENT),            # null codewords
        (shred(0, n, [10, 10, 10], p, stride, sent32), UNSUPPORTED_SHARD_COUNT),
        (shred(65, n, [10, 10, 10], p, 97 * 1024, sent32), UNSUPPORTED_SHARD_COUNT),
        (deshred(32, n, [2, 0, 2], p, stride, rs.DECODE_ANY_K, sent64), INVALID_SHARD_SIZE),
        (deshred(32, n, [2, 7, 2], p, stride, rs.DECODE_ANY_K, sent64), INVALID_SHARD_SIZE),
        (deshred(32, n, [2, 1026, 2], p, 2 * stride, rs.DECODE_ANY_K, sent64), TOO_MUCH_DATA),
        (deshred(32, n, [2, 1024, 2], p, stride - 2, rs.DECODE_ANY_K, sent64), INVALID_ARGUMENT),
        (deshred(32, n, None, p, stride, rs.DECODE_ANY_K, sent64), INVALID_ARGUMENT),
        (deshred(32, n, [2, 2, 2], None, stride, rs.DECODE_ANY_K, sent64), INVALID_ARGUMENT),
        (deshred(32, n, [2, 2, 2], p, stride, rs.DECODE_ANY_K, sent64, dp=False), INVALID_ARGUMENT),
        (deshred(32, n, [2, 2, 2], p, stride, 7, sent64), INVALID_ARGUMENT),                   # bad mode
        (deshred(0, n, [2, 2, 2], p, stride, rs.DECODE_ANY_K, sent64), UNSUPPORTED_SHARD_COUNT),
        (deshred(65, n, [2, 2, 2], p, stride, rs.DECODE_ANY_K, sent64), UNSUPPORTED_SHARD_COUNT),
    ]
    for i, (got, want) in enumerate(cases):
        assert got == want, (i, got, want)
    ctx.synchronize()
    assert (d_cw.cpu().numpy() == 0x77).all()
    assert (sent32 == 0xDEAD).all() and (sent64 == -777).all()
    assert shred(32, 0, None, None, 0, sent32) == 0
    assert deshred(32, 0, None, None, 0, rs.DECODE_EXACT, sent64) == 0


@pytest.mark.gpu
def test_chain_frame_shred_deshred_parse(ctx, dev):
    """ag_slice_frame_batch (shred_bytes = 1024) -> shred_batch_var in place -> 32 shreds of
    every slice lost -> deshred_batch_var -> ag_slice_parse_batch: the original data, the
    codewords never leaving the device in between."""
    import slice_oracle as so

    rng = random.Random(8)
    n, stride = 48, 64 * 1024
    dlens = [rng.choice([0, 1, 55, 56, 900, 2000, 31000, 32200, 32700]) + rng.randrange(0, 8) for _ in range(n)]
    parents = [None if rng.random() < 0.5 else (rng.getrandbits(64), rng.randbytes(32)) for _ in range(n)]
    datas = [o.splitmix64_bytes(600 + b, L) for b, L in enumerate(dlens)]
    dbuf = np.zeros((n, 32768), np.uint8)
    for b, d in enumerate(datas):
        dbuf[b, :len(d)] = np.frombuffer(d, np.uint8)
    d_data = to_dev(dbuf, dev)
    d_cw = torch.full((n, stride), FILL, dtype=torch.uint8, device=dev)
    plens = rs.slice_frame_batch(ctx, n, 1024, parents, d_data, 32768, dlens, d_cw, stride)
    sizes = rs.coder_shred_batch_var(ctx, 32, n, None, 0, plens, d_cw, stride)
    assert list(sizes) == [rs.coder_shred_bytes(int(L)) for L in plens]
    assert len(set(sizes)) > 4
    keep = [set(rng.sample(range(64), 32)) for _ in range(n)]
    dp, cp = flags(keep)
    lost = np.zeros((n, stride), bool)
    for b, S in enumerate(sizes):
        for i in set(range(64)) - keep[b]:
            lost[b, i * S:(i + 1) * S] = True
    ctx.synchronize()
    d_cw[to_dev(lost, dev)] = ABSENT
    torch.cuda.current_stream().synchronize()
    res = rs.coder_deshred_batch_var(ctx, 32, n, sizes, d_cw, stride, dp, cp, rs.DECODE_ANY_K, as_array=True)
    assert list(res) == list(plens)
    st, got_parents, offs, dls = rs.slice_parse_batch(ctx, n, d_cw, stride, res)
    host = d_cw.cpu().numpy()
    for b in range(n):
        assert st[b] == 0 and got_parents[b] == parents[b] and dls[b] == dlens[b], b
        assert host[b, offs[b]:offs[b] + dls[b]].tobytes() == datas[b], b
        assert host[b, :int(plens[b])].tobytes() == so.payload_bytes(parents[b], datas[b]), b
