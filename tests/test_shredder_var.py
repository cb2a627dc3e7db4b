"""RegularShredder::shred over slices of mixed shred sizes: ag_merkle_build_batch_var,
ag_shredder_shred_batch_var and ag_shred_datagram_bytes against oracle/merkle_oracle.py and
oracle/shredder_oracle.py as they stand, and against the uniform calls run per size.

Reference: shredder.rs:337-345 (shred), :533-560 (output shreds), :628-632 (the slice tree);
block_producer.rs:453-474 and reed_solomon.rs:94-95 (where the sizes come from).
"""

import os
import random
import re

import numpy as np
import pytest

import ed25519_oracle as ed
import merkle_oracle as mk
import rs_oracle as o
import shred_wire_oracle as wire
import shredder_oracle as so
import slice_oracle as sl
from alpenglow_amd import build, rs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "alpenglow_rs.h")
NEW = ("ag_merkle_build_batch_var", "ag_shredder_shred_batch_var", "ag_shred_datagram_bytes")

FILL = 0xA5           # bytes the calls must not write
STRIDE = 64 * 1024    # one slice's codeword region
PKT = 1536            # datagram slot stride
SEED = bytes(range(7, 39))
NODES = 32 * 127      # a 64-leaf tree's nodes
PROOFS = 64 * 6 * 32  # and its 64 proofs

# SHA-256 padding edges (32 + S = 55 / 56 mod 64: S = 22 / 24, 86 / 88; 0 mod 64: S = 32, 96), zero
# (S < 32), one (S = 96) and many data-only blocks, and every even row alignment mod 16 (S = 2 and
# S = 1010 walk all eight)
MK_SIZES = [2, 22, 24, 30, 32, 34, 86, 88, 94, 96, 98, 512, 1000, 1008, 1010, 1022, 1024]
SH_SIZES = [2, 24, 66, 512, 1000, 1008, 1010, 1012, 1016, 1022, 1024, 1024, 2, 1010]


# ------------------------------------------------------------------------------ CPU

@pytest.fixture(scope="module")
def lib():
    build.build()
    return rs.load()


def test_symbols_declared_exported_and_callable(lib):
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = set(re.findall(r"\b(ag_\w+)\s*\(", text))
    for s in NEW:
        assert s in declared and s in rs.EXPORTS and hasattr(lib, s), s
    for f in ("merkle_build_batch_var", "shredder_shred_batch_var", "shred_datagram_bytes", "last_merkle_kernels"):
        assert callable(getattr(rs, f))
    assert "leaf_var" in rs.MERKLE_KERNELS


@pytest.mark.parametrize("S", [2, 64, 1010, 1024])
def test_datagram_bytes_matches_wire_oracle_and_closed_form(lib, S):
    pkt = wire.serialize(wire.CODING, 7, 3, True, 40, bytes(S), bytes(64), [bytes(32)] * 6)
    assert rs.shred_datagram_bytes(S, 6) == len(pkt) == 37 + S + 64 + 8 + 32 * 6
    if S == 1024:
        assert rs.shred_datagram_bytes(S, 6) == 1325


def test_datagram_bytes_over_the_mtu(lib):
    assert rs.shred_datagram_bytes(1024, 11) == 1485
    for S, h in ((1024, 12), (1392, 0), (1 << 40, 0), (2, 1 << 60)):
        with pytest.raises(rs.RSError) as e:
            rs.shred_datagram_bytes(S, h)
        assert e.value.kind == "InvalidArgument"


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


def tree_bytes(rows):
    """(root, nodes, proofs) of the slice tree over 64 rows, as the library lays them out."""
    t = mk.slice_tree(rows[:32], rows[32:])
    return t.root(), b"".join(t.nodes), b"".join(b"".join(t.create_proof(j)) for j in range(64))


@pytest.fixture(scope="module")
def mk_ref():
    """Per size of MK_SIZES: the slice's 64 * S bytes and its oracle tree (shared, read-only)."""
    ref = {}
    for S in MK_SIZES:
        blob = o.splitmix64_bytes(0x3E4C1E + S, 64 * S)
        ref[S] = (blob, tree_bytes([blob[j * S:(j + 1) * S] for j in range(64)]))
    return ref


def run_merkle_var(ctx, dev, sizes, blobs, stride=STRIDE, offset=0, want_nodes=True):
    """The var build over slices whose bytes are given; (roots, nodes, proofs) as numpy arrays."""
    n = len(sizes)
    buf = np.full(n * stride + 16, FILL, np.uint8)
    for s, b in enumerate(blobs):
        buf[offset + s * stride: offset + s * stride + len(b)] = np.frombuffer(b, np.uint8)
    d_buf = to_dev(buf, dev)
    roots, nodes, proofs = filled((n, 32), dev), filled((n, NODES), dev), filled((n, PROOFS), dev)
    rs.merkle_build_batch_var(ctx, n, sizes, d_buf.data_ptr() + offset, stride, roots,
                              nodes if want_nodes else None, NODES if want_nodes else 0, proofs, PROOFS)
    torch.cuda.synchronize()
    assert rs.last_merkle_kernels(ctx) == {"leaf_var"}
    return roots.cpu().numpy(), nodes.cpu().numpy(), proofs.cpu().numpy()


def check_trees(got, sizes, want):
    roots, nodes, proofs = got
    for s, (S, (root, nd, pr)) in enumerate(zip(sizes, want)):
        assert roots[s].tobytes() == root, (s, S)
        if nodes is not None:
            assert nodes[s].tobytes() == nd, (s, S)
        if proofs[s].tobytes() != pr:  # name the first leaf that differs
            j = next(j for j in range(64) if proofs[s, 192 * j:192 * (j + 1)].tobytes() != pr[192 * j:192 * (j + 1)])
            raise AssertionError((s, S, j))


@pytest.mark.gpu
@pytest.mark.parametrize("order", ["ascending", "descending", "shuffled"])
def test_merkle_var_matches_oracle(ctx, dev, mk_ref, order):
    sizes = sorted(MK_SIZES, reverse=order == "descending")
    if order == "shuffled":
        random.Random(5).shuffle(sizes)
    got = run_merkle_var(ctx, dev, sizes, [mk_ref[S][0] for S in sizes])
    check_trees(got, sizes, [mk_ref[S][1] for S in sizes])


@pytest.mark.gpu
def test_merkle_var_equals_uniform_calls(ctx, dev):
    """300 slices of a block's mix: roots and proofs of the one var call and of the uniform call
    per group of equal size, on the same bytes."""
    import bench_coder

    n = 300
    sizes = bench_coder.mixed_sizes(n)
    g = torch.Generator(device="cpu").manual_seed(0x51CE)
    buf = torch.randint(0, 256, (n, STRIDE), dtype=torch.uint8, generator=g).to(dev)
    roots, proofs = filled((n, 32), dev), filled((n, PROOFS), dev)
    rs.merkle_build_batch_var(ctx, n, sizes, buf, STRIDE, roots, None, 0, proofs, PROOFS)
    assert rs.last_merkle_kernels(ctx) == {"leaf_var"}
    roots_u, proofs_u = torch.zeros_like(roots), torch.zeros_like(proofs)
    for S in sorted(set(sizes.tolist())):
        idx = torch.from_numpy(np.flatnonzero(sizes == S)).to(dev)
        grp = buf[idx].contiguous()
        r, p = filled((len(idx), 32), dev), filled((len(idx), PROOFS), dev)
        rs.merkle_build_batch(ctx, 64, S, len(idx), grp, S, STRIDE, r, None, 0, p, PROOFS)
        assert rs.last_merkle_kernels(ctx) == ({"leaf_aligned"} if S % 16 == 0 else {"leaf_byte"})
        roots_u[idx], proofs_u[idx] = r, p
    torch.cuda.synchronize()
    assert torch.equal(roots, roots_u)
    assert torch.equal(proofs, proofs_u)


@pytest.mark.gpu
@pytest.mark.parametrize("sizes", [[1010], [2] * 64, [2, 1024] * 32], ids=["one", "64x2", "2-1024"])
def test_merkle_var_degenerate_shapes(ctx, dev, sizes):
    blobs = [o.splitmix64_bytes(0xDE6 + 7 * s, 64 * S) for s, S in enumerate(sizes)]
    want = [tree_bytes([b[j * S:(j + 1) * S] for j in range(64)]) for S, b in zip(sizes, blobs)]
    check_trees(run_merkle_var(ctx, dev, sizes, blobs), sizes, want)


@pytest.mark.gpu
def test_merkle_var_rows_two_bytes_off_a_16_byte_boundary(ctx, dev, mk_ref):
    """Base 2 bytes past a 16-byte boundary, slice stride an odd multiple of 2."""
    sizes = [1024, 1010, 96, 32, 2, 1008, 34]
    got = run_merkle_var(ctx, dev, sizes, [mk_ref[S][0] for S in sizes], stride=STRIDE + 2, offset=2)
    check_trees(got, sizes, [mk_ref[S][1] for S in sizes])


@pytest.mark.gpu
def test_merkle_var_argument_errors(ctx, dev):
    n = 3
    buf = filled((n, STRIDE), dev)
    roots, nodes, proofs = filled((n, 32), dev), filled((n, NODES + 16), dev), filled((n, PROOFS), dev)

    def call(sizes, stride=STRIDE, nodes_stride=NODES):
        rs.merkle_build_batch_var(ctx, n, sizes, buf, stride, roots, nodes, nodes_stride, proofs, PROOFS)

    cases = [("InvalidShardSize", dict(sizes=[64, 63, 64])),
             ("InvalidShardSize", dict(sizes=[64, 0, 64])),
             ("TooMuchData", dict(sizes=[64, 1026, 64])),
             ("InvalidArgument", dict(sizes=[64, 1024, 64], stride=64 * 1024 - 16)),
             ("InvalidArgument", dict(sizes=[64, 64, 64], nodes_stride=NODES + 8)),
             ("InvalidArgument", dict(sizes=[64, 64, 64], nodes_stride=NODES - 16))]
    for kind, kw in cases:
        with pytest.raises(rs.RSError) as e:
            call(**kw)
        assert e.value.kind == kind, (kind, kw)
    torch.cuda.synchronize()
    for t in (roots, nodes, proofs):
        assert bool((t == FILL).all())


# ---- the composed call ---------------------------------------------------------------------

def slices_for(rng, S, i):
    """One slice whose framed payload pads to shred size S (test_shredder_pipeline._slices); odd i: a parent."""
    lo, hi = 32 * S - 64, 32 * S - 1
    parent = (rng.randrange(1 << 40), bytes(rng.randrange(256) for _ in range(32))) if i % 2 else None
    framed = rng.randrange(max(lo, sl.header_len(parent)), min(hi, sl.MAX_DATA_PER_SLICE) + 1)
    data = bytes(rng.randrange(256) for _ in range(framed - sl.header_len(parent)))
    return (parent, data, rng.randrange(1 << 32), rng.randrange(1024), bool(i % 3 == 2))


class Shredded:
    """SH_SIZES slices through ag_shredder_shred_batch_var once (block counts 5, 1, 8), and the
    oracle's shred of each; shared by the tests below, read-only."""

    COUNTS = [5, 1, 8]

    def __init__(self, ctx, dev):
        rng = random.Random(0x5A7)
        self.slices = [slices_for(rng, S, i) for i, S in enumerate(SH_SIZES)]
        self.want = [so.shred(p, d, slot, si, last, SEED) for p, d, slot, si, last in self.slices]
        self.inputs = device_inputs(self.slices, dev)
        n = len(self.slices)
        self.out = run_shred_var(ctx, dev, self.slices, self.inputs, block_counts=self.COUNTS)
        self.encode_kernels = rs.last_encode_kernels(ctx)
        self.merkle_kernels = rs.last_merkle_kernels(ctx)
        assert n == sum(self.COUNTS)


def device_inputs(slices, dev):
    n = len(slices)
    maxd = max(len(s[1]) for s in slices)
    data = np.zeros((n, maxd), np.uint8)
    for b, s in enumerate(slices):
        data[b, :len(s[1])] = np.frombuffer(s[1], np.uint8)
    return dict(data=to_dev(data, dev), data_stride=maxd,
                slots=to_dev(np.array([s[2] for s in slices], np.uint64), dev),
                sidx=to_dev(np.array([s[3] for s in slices], np.uint64), dev),
                last=to_dev(np.array([s[4] for s in slices], np.uint8), dev),
                seed=to_dev(np.frombuffer(SEED, np.uint8), dev),
                pk=to_dev(np.frombuffer(ed.secret_to_public(SEED), np.uint8), dev))


def run_shred_var(ctx, dev, slices, inp, block_counts=None, cw_stride=STRIDE, pkt=PKT, cw_offset=0, hashes=None,
                  bufs=None):
    """One composed call into 0xA5-filled buffers; everything it can write, as numpy arrays."""
    n = len(slices)
    if bufs is None:
        bufs = dict(cw=filled(n * cw_stride + 16, dev), pk=filled((n * 64, pkt), dev),
                    lens=torch.full((n * 64,), -1, dtype=torch.int32, device=dev), roots=filled((n, 32), dev),
                    sigs=filled((n, 64), dev),
                    hashes=hashes if hashes is not None else filled((max(len(block_counts or []), 1), 32), dev))
    try:
        S = rs.shredder_shred_batch_var(ctx, n, [s[0] for s in slices], inp["data"], inp["data_stride"],
                                        [len(s[1]) for s in slices], inp["slots"], inp["sidx"], inp["last"],
                                        inp["seed"], inp["pk"], bufs["cw"].data_ptr() + cw_offset, cw_stride,
                                        bufs["pk"], pkt, bufs["lens"], roots_out=bufs["roots"], sigs_out=bufs["sigs"],
                                        block_counts=block_counts, block_hashes_out=bufs["hashes"])
    finally:
        torch.cuda.synchronize()
    out = {k: v.cpu().numpy() for k, v in bufs.items()}
    out["S"] = S
    return out


@pytest.fixture(scope="module")
def shredded(ctx, dev):
    return Shredded(ctx, dev)


@pytest.mark.gpu
def test_shred_var_matches_oracle(shredded):
    """Root, signature, packed raw shreds and all 64 datagrams per slice; nothing written past a
    slice's 64 * S_s codeword bytes or past a datagram's length."""
    out = shredded.out
    assert out["S"].tolist() == SH_SIZES
    assert "var_encode" in shredded.encode_kernels
    assert shredded.merkle_kernels == {"leaf_var"}
    cw = out["cw"][:len(SH_SIZES) * STRIDE].reshape(len(SH_SIZES), STRIDE)
    assert (out["cw"][len(SH_SIZES) * STRIDE:] == FILL).all()
    for b, (S, (pkts, raw, root, sig)) in enumerate(zip(SH_SIZES, shredded.want)):
        assert out["roots"][b].tobytes() == root, b
        assert out["sigs"][b].tobytes() == sig, b
        assert cw[b, :64 * S].tobytes() == b"".join(raw.data + raw.coding), b
        assert (cw[b, 64 * S:] == FILL).all(), b
        for j in range(64):
            t = 64 * b + j
            assert out["lens"][t] == len(pkts[j]) == rs.shred_datagram_bytes(S, 6), (b, j)
            assert out["pk"][t, :len(pkts[j])].tobytes() == pkts[j], (b, j)
            assert (out["pk"][t, len(pkts[j]):] == FILL).all(), (b, j)


@pytest.mark.gpu
def test_shred_var_block_hashes(ctx, dev, shredded):
    """Each group's double-Merkle root over its slice roots; nblocks = 0 writes none; counts that
    do not sum to nslices are refused."""
    roots = [w[2] for w in shredded.want]
    at = 0
    for b, cnt in enumerate(Shredded.COUNTS):
        assert shredded.out["hashes"][b].tobytes() == mk.MerkleTree(roots[at:at + cnt]).root(), b
        at += cnt
    hashes = filled((3, 32), dev)
    out = run_shred_var(ctx, dev, shredded.slices, shredded.inputs, block_counts=None, hashes=hashes)
    assert (out["hashes"] == FILL).all()
    assert [out["roots"][b].tobytes() for b in range(len(roots))] == roots
    for counts in ([5, 1, 7], [5, 1, 9], [14, 0], [6, 8, 0]):
        assert_refused(ctx, dev, shredded, "InvalidArgument", block_counts=counts)


@pytest.mark.gpu
def test_existing_follower_accepts_the_datagrams(ctx, dev, shredded):
    """The datagrams, regrouped by size into the uniform layout with a random 32 of 64 dropped,
    through ag_shredder_deshred_batch at that size: every slice decodes to its input."""
    rng = random.Random(0xF011)
    out = shredded.out
    for S in sorted(set(SH_SIZES)):
        idx = [b for b, s in enumerate(SH_SIZES) if s == S]
        buf = np.zeros((len(idx) * 64, PKT), np.uint8)
        ln = np.zeros(len(idx) * 64, np.int32)
        for g, b in enumerate(idx):
            for j in rng.sample(range(64), 32):
                buf[g * 64 + j] = out["pk"][b * 64 + j]
                ln[g * 64 + j] = out["lens"][b * 64 + j]
        cw = torch.zeros((len(idx), 64 * S), dtype=torch.uint8, device=dev)
        res = rs.shredder_deshred_batch(ctx, len(idx), S, to_dev(buf, dev), PKT, to_dev(ln, dev), shredded.inputs["pk"],
                                        cw)
        cwh = cw.cpu().numpy()
        assert res.status.tolist() == [0] * len(idx), (S, res.status.tolist())
        for g, b in enumerate(idx):
            parent, data, slot, si, last = shredded.slices[b]
            assert res.parents[g] == parent, (S, b)
            off, n = int(res.data_offsets[g]), int(res.data_lens[g])
            assert cwh[g, off:off + n].tobytes() == data, (S, b)
            assert (int(res.slots[g]), int(res.slice_indices[g]), bool(res.is_last[g])) == (slot, si, last)


def assert_refused(ctx, dev, shredded, kind, slices=None, **kw):
    """The call raises `kind` and leaves every output byte as it was."""
    slices = slices or shredded.slices
    inp = shredded.inputs if slices is shredded.slices else device_inputs(slices, dev)
    n, cw_stride, pkt = len(slices), kw.get("cw_stride", STRIDE), kw.get("pkt", PKT)
    bufs = dict(cw=filled(n * max(cw_stride, 64) + 16, dev), pk=filled((n * 64, pkt), dev),
                lens=torch.full((n * 64,), -1, dtype=torch.int32, device=dev), roots=filled((n, 32), dev),
                sigs=filled((n, 64), dev), hashes=filled((4, 32), dev))
    with pytest.raises(rs.RSError) as e:
        run_shred_var(ctx, dev, slices, inp, bufs=bufs, **kw)
    assert e.value.kind == kind, (kind, kw)
    for k, v in bufs.items():
        assert bool((v == (-1 if k == "lens" else FILL)).all()), (kind, kw, k)


@pytest.mark.gpu
def test_shred_var_argument_errors(ctx, dev, shredded):
    assert_refused(ctx, dev, shredded, "InvalidArgument", cw_stride=64 * 1024 - 16)  # the 1024-byte slices
    assert_refused(ctx, dev, shredded, "InvalidArgument", cw_stride=STRIDE + 8)
    assert_refused(ctx, dev, shredded, "InvalidArgument", cw_offset=8)
    assert_refused(ctx, dev, shredded, "InvalidArgument", pkt=rs.shred_datagram_bytes(1024, 6) - 1)
    big = list(shredded.slices[:3])
    big[1] = (None, bytes(sl.MAX_DATA_PER_SLICE - sl.header_len(None) + 1), 1, 2, False)
    assert_refused(ctx, dev, shredded, "TooMuchData", slices=big)
