"""The streamed intake of the 32:32 full-recovery reconstruct (xform8_stream_kernel,
rs_tile64.hip): a tile's loads are issued with no control flow between them, each slot is
converted as its own pieces land, and the store predicates come from mask words loaded ahead of
the pieces.  Byte-exact against the C oracle, asserting the route through the launch records.
The encodes ran the same intake on xform_kernel while it was measured (neutral, not kept); their
cases stay: whole tiles, tiles that straddle blocks with a partial last one, and k < 32.

Run on an MI355X with ``python -m pytest tests -m gpu``.
"""

import random

import numpy as np
import pytest

import ro_c
from alpenglow_amd import rs

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def dev(ctx):
    d = torch.device("cuda:0")
    s = torch.cuda.Stream(d)
    torch.cuda.set_stream(s)
    ctx.set_stream(s.cuda_stream)
    return d


_CODED = {}


def coded(k, m, S, n):
    """(originals (n, k, S), recovery (n, m, S)) of a seeded batch, encoded once by the oracle
    and shared read-only by the tests."""
    key = (k, m, S, n)
    if key not in _CODED:
        blocks = np.random.default_rng(9100 + 131 * k + 7 * m + S + n).integers(0, 256, (n, k, S), dtype=np.uint8)
        rec = ro_c.encode_blocks(blocks, m, threads=8)
        blocks.setflags(write=False)
        rec.setflags(write=False)
        _CODED[key] = (blocks, rec)
    return _CODED[key]


def gpu_encode(ctx, dev, blocks, m):
    n, k, S = blocks.shape
    d_in = torch.from_numpy(blocks.reshape(n, k * S).copy()).to(dev)
    d_out = torch.zeros((n, m * S), dtype=torch.uint8, device=dev)
    rs.encode_batch(ctx, k, m, S, n, d_in, k * S, d_out, m * S)
    return d_out.cpu().numpy().reshape(n, m, S)


@pytest.mark.parametrize("S,n", [
    (4096, 256),  # 256 whole tiles: the smallest batch that takes xform_kernel
    (2112, 500),  # 33 chunks per shard: tiles straddle blocks, the last tile is partial
])
def test_encode_32_32_headline_kernel(ctx, dev, S, n):
    blocks, want = coded(32, 32, S, n)
    got = gpu_encode(ctx, dev, blocks, 32)
    assert rs.last_encode_kernels(ctx) == {"xform4"}
    assert np.array_equal(got, want)


@pytest.mark.parametrize("k,m", [(20, 30), (25, 32)])
def test_encode_partial_geometry(ctx, dev, k, m):
    """n_in < 32: shards k..31 are not loaded and read as zero."""
    blocks, want = coded(k, m, 4096, 256)
    got = gpu_encode(ctx, dev, blocks, m)
    assert rs.last_encode_kernels(ctx) == {"xform4"}
    assert np.array_equal(got, want)


def reconstruct(ctx, dev, blocks, d_rec, present):
    """Decode with the absent originals zeroed (a kernel that read them would restore wrong
    bytes); present: (npat, k) flags, one row for the batch or one per block."""
    n, k, S = blocks.shape
    m = k
    damaged = blocks.copy()
    damaged[np.broadcast_to(present, (n, k)) == 0] = 0
    d_o = torch.from_numpy(damaged.reshape(n, k * S)).to(dev)
    npat = present.shape[0]
    rs.decode_batch(ctx, k, m, S, n, d_o, k * S, d_rec, m * S, present.reshape(-1), np.ones(npat * m, np.uint8),
                    mode=rs.DECODE_ANY_K)
    return d_o.cpu().numpy().reshape(n, k, S)


@pytest.mark.parametrize("erased", [tuple(range(16)), (3, 17, 30)], ids=["low16_half", "3_17_30_full_fft"])
def test_reconstruct_single_pattern(ctx, dev, erased):
    """One pattern for the batch: every piece's predicate comes from mask word 0.
    Erasures 0..15 take the half-pruned FFT, {3, 17, 30} the full one."""
    S, n = 4096, 64
    blocks, rec = coded(32, 32, S, n)
    d_rec = torch.from_numpy(rec.reshape(n, 32 * S).copy()).to(dev)
    present = np.ones((1, 32), np.uint8)
    present[0, list(erased)] = 0
    got = reconstruct(ctx, dev, blocks, d_rec, present)
    assert set(rs.last_decode_classes(ctx)) == {"transform"}
    assert np.array_equal(got, blocks)


def _random16(rng, n):
    present = np.ones((n, 32), np.uint8)
    for b in range(n):
        present[b, rng.sample(range(32), 16)] = 0
    return present


def test_reconstruct_per_block_masks(ctx, dev):
    """A random 16 erased per block; 33 chunks per shard: tiles straddle blocks, last tile partial."""
    S, n = 2112, 130
    blocks, rec = coded(32, 32, S, n)
    d_rec = torch.from_numpy(rec.reshape(n, 32 * S).copy()).to(dev)
    got = reconstruct(ctx, dev, blocks, d_rec, _random16(random.Random(2112), n))
    assert rs.last_decode_classes(ctx) == {"transform": n}
    assert np.array_equal(got, blocks)


def test_reconstruct_per_block_masks_repeated(ctx, dev):
    """The per-block case 20 times over (fresh patterns each time): the store predicates are now
    packed while the tile's loads are in flight, so a correct result has to be a repeatable one."""
    S, n = 2048, 40
    blocks, rec = coded(32, 32, S, n)
    d_rec = torch.from_numpy(rec.reshape(n, 32 * S).copy()).to(dev)
    rng = random.Random(2048)
    for it in range(20):
        got = reconstruct(ctx, dev, blocks, d_rec, _random16(rng, n))
        assert rs.last_decode_classes(ctx) == {"transform": n}, it
        assert np.array_equal(got, blocks), it
