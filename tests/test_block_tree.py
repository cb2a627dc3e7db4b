"""Block trees: the double-Merkle tree over a block's slice roots (DoubleMerkleTree,
crypto/merkle.rs:263; the BlockHash of slot_block_data.rs:390-394) and the repair responses'
proof checks (check_proof / check_proof_last, repair.rs:362-393), against
oracle/merkle_oracle.py as it stands.  Inputs: rs_oracle.splitmix64_bytes.
"""

import os
import random
import re

import numpy as np
import pytest
import torch  # before the library: torch's HIP runtime must be the process's first

import merkle_oracle as mo
import rs_oracle as o
from alpenglow_amd import rs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# 1: height 0.  5, 65, 129, 257, 513: odd at several levels (513 at every level: EMPTY_ROOTS[0..9]).
# 1023, 1024: capacity.  64, 65, 256, 257: wave and workgroup boundaries.
COUNTS = [1, 2, 3, 4, 5, 63, 64, 65, 127, 129, 255, 256, 257, 511, 513, 1000, 1023, 1024]


def _roots(seed, n):
    """n slice roots (32 B each) as an (n, 32) uint8 array."""
    return np.frombuffer(o.splitmix64_bytes(seed, 32 * n), np.uint8).reshape(n, 32).copy()


def _trees(roots, counts):
    out, at = [], 0
    for n in counts:
        out.append(mo.MerkleTree([roots[at + j].tobytes() for j in range(n)]))
        at += n
    return out


@pytest.fixture(scope="module")
def reference():
    """The COUNTS blocks' slice roots and their oracle trees (shared, read-only)."""
    roots = _roots(0xB10C, sum(COUNTS))
    roots.setflags(write=False)
    return roots, _trees(roots, COUNTS)


# ------------------------------------------------------------------------------------ CPU

def test_python_mirror_has_the_entry_points():
    assert callable(rs.block_tree_batch) and callable(rs.block_proof_check_batch)
    assert rs.BLOCK_MAX_SLICES == 1024


def test_symbols_in_header_and_exports():
    text = open(os.path.join(ROOT, "include", "alpenglow_rs.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for sym in ("ag_block_tree_batch", "ag_block_proof_check_batch"):
        assert re.search(r"\b%s\s*\(" % sym, text), sym
        assert sym in rs.EXPORTS
    assert re.search(r"#define\s+AG_BLOCK_MAX_SLICES\s+1024\b", text)


@pytest.mark.parametrize("n", [65, 513, 1000, 1023, 1024])
def test_height_and_node_count_of_block_sized_trees(n):
    t = mo.MerkleTree([b"x"] * n)
    assert rs.merkle_height(n) == t.height()
    assert rs.merkle_node_count(n) == len(t.nodes)


# --------------------------------------------------------------------------------- device

def _dev(a):
    return torch.from_numpy(np.array(a)).to("cuda:0")  # a copy: the shared reference is read-only


def _hashes_only(ctx, roots, counts):
    d_roots = _dev(roots.reshape(-1))
    hashes = torch.zeros(32 * len(counts), dtype=torch.uint8, device="cuda:0")
    rs.block_tree_batch(ctx, len(counts), counts, d_roots, hashes)
    return hashes.cpu().numpy().reshape(len(counts), 32)


@pytest.mark.gpu
def test_trees_match_oracle(ctx, reference):
    """Block hash, every node and every slice's proof, byte for byte; nothing past a block's own."""
    roots, trees = reference
    nb = len(COUNTS)
    nstride = 32 * rs.merkle_node_count(1024)
    pstride = 32 * rs.merkle_height(1024) * 1024
    hashes = torch.zeros(32 * nb, dtype=torch.uint8, device="cuda:0")
    nodes = torch.zeros(nb * nstride, dtype=torch.uint8, device="cuda:0")
    proofs = torch.zeros(nb * pstride, dtype=torch.uint8, device="cuda:0")
    rs.block_tree_batch(ctx, nb, COUNTS, _dev(roots.reshape(-1)), hashes, nodes, nstride, proofs, pstride)
    hashes = hashes.cpu().numpy().reshape(nb, 32)
    nodes = nodes.cpu().numpy().reshape(nb, nstride)
    proofs = proofs.cpu().numpy().reshape(nb, pstride)
    for b, (n, t) in enumerate(zip(COUNTS, trees)):
        h = t.height()
        assert rs.merkle_height(n) == h
        assert hashes[b].tobytes() == t.root(), n
        want_nodes = b"".join(t.nodes)
        assert nodes[b, : len(want_nodes)].tobytes() == want_nodes, n
        assert not nodes[b, len(want_nodes):].any(), n
        want_proofs = b"".join(b"".join(t.create_proof(j)) for j in range(n))
        assert len(want_proofs) == 32 * h * n
        got = proofs[b, : len(want_proofs)].tobytes()
        if got != want_proofs:  # name the first slice that differs
            j = next(j for j in range(n) if got[32 * h * j: 32 * h * (j + 1)] != want_proofs[32 * h * j: 32 * h * (j + 1)])
            raise AssertionError((n, j))
        assert not proofs[b, len(want_proofs):].any(), n


@pytest.mark.gpu
def test_nullable_outputs(ctx, reference):
    """Hashes only (nodes and proofs null), and proofs without nodes (context scratch)."""
    roots, trees = reference
    got = _hashes_only(ctx, roots, COUNTS)
    assert [got[b].tobytes() for b in range(len(COUNTS))] == [t.root() for t in trees]
    nb = len(COUNTS)
    pstride = 32 * rs.merkle_height(1024) * 1024
    hashes = torch.zeros(32 * nb, dtype=torch.uint8, device="cuda:0")
    proofs = torch.zeros(nb * pstride, dtype=torch.uint8, device="cuda:0")
    rs.block_tree_batch(ctx, nb, COUNTS, _dev(roots.reshape(-1)), hashes, None, 0, proofs, pstride)
    assert np.array_equal(hashes.cpu().numpy().reshape(nb, 32), got)
    proofs = proofs.cpu().numpy().reshape(nb, pstride)
    for b in (0, 4, 14, 17):  # counts 1, 5, 513, 1024
        n, t = COUNTS[b], trees[b]
        want = b"".join(b"".join(t.create_proof(j)) for j in range(n))
        assert proofs[b, : len(want)].tobytes() == want, n


@pytest.mark.gpu
def test_grid_wider_than_the_chip(ctx):
    """300 workgroups on 256 CUs; a block alone hashes as it does inside the batch."""
    rng = random.Random(0x300)
    counts = [rng.randint(1, 48) for _ in range(300)]
    roots = _roots(0x300B, sum(counts))
    got = _hashes_only(ctx, roots, counts)
    want = [t.root() for t in _trees(roots, counts)]
    assert [got[b].tobytes() for b in range(300)] == want
    alone = _hashes_only(ctx, roots[: counts[0]], counts[:1])
    assert alone[0].tobytes() == want[0]


def _proof_items():
    """(slice root, index, block hash, proof digests, last, pinned expectation or None)."""
    blocks = {}
    for k, n in enumerate([1, 2, 33, 34, 1000, 1024]):
        r = _roots(0x9E0 + k, n)
        blocks[n] = (r, mo.MerkleTree([r[j].tobytes() for j in range(n)]))
    items = []

    def add(n, j, last, want=None, index=None, root=None, hash_=None, proof=None):
        r, t = blocks[n]
        items.append((r[j].tobytes() if root is None else root, j if index is None else index,
                      t.root() if hash_ is None else hash_, t.create_proof(j) if proof is None else proof,
                      last, want))

    def flip(b, i, bit=1):
        return b[:i] + bytes([b[i] ^ bit]) + b[i + 1:]

    rng = random.Random(41)
    for n, (r, t) in blocks.items():
        h = t.height()
        for j in sorted({0, n // 2, n - 1}):
            add(n, j, 0, want=1)                      # untampered
            add(n, j, 1)                              # check_proof_last: the oracle decides
            add(n, j, 0, want=1, index=j + (1 << h))  # index bits above proof_len are ignored
            add(n, j, 0, want=0, root=flip(r[j].tobytes(), rng.randrange(32)))
            add(n, j, 0, want=0, hash_=flip(t.root(), rng.randrange(32), 0x80))
            add(n, j, 1, want=0, hash_=flip(t.root(), rng.randrange(32), 0x10))
            if h:
                p = t.create_proof(j)
                q = rng.randrange(h)
                p[q] = flip(p[q], rng.randrange(32), 4)
                add(n, j, 0, want=0, proof=p)
                add(n, j, 0, want=0, index=j ^ (1 << rng.randrange(h)))
        add(n, n - 1, 1, want=1)                      # the last slice passes check_proof_last
    add(33, 31, 1, want=0)  # merkle.rs proof_last: not the last leaf
    add(33, 32, 1, want=1)
    add(34, 32, 0, want=1)  # the sibling is leaf 33, not EMPTY_ROOTS[0]: a valid proof,
    add(34, 32, 1, want=0)  # but no proof that 32 is the last slice
    for last in (0, 1):     # proofs longer than EMPTY_ROOTS
        add(1024, 5, last, want=0, proof=[bytes(32)] * 33)
        add(1, 0, last, want=0, proof=[bytes(32)] * 33)
    add(1, 0, 0, want=1)    # proof_len 0: the block hash is the leaf hash
    add(1, 0, 1, want=1)
    add(1, 0, 0, want=0, hash_=blocks[1][0][0].tobytes())  # the bare slice root is not it
    return items


@pytest.mark.gpu
def test_proof_checks(ctx):
    """Proof lengths 0..10 and 33, check_proof and check_proof_last in one call: ok equals the
    oracle item by item, and the cases the reference's own tests pin have the pinned result."""
    items = _proof_items()
    n, stride = len(items), 34 * 32
    assert {len(it[3]) for it in items} == {0, 1, 6, 10, 33}
    want = np.array([(mo.check_proof_last if it[4] else mo.check_proof)(it[0], it[1], it[2], it[3])
                     for it in items], np.uint8)
    for t, it in enumerate(items):
        if it[5] is not None:
            assert want[t] == it[5], t
    roots = np.frombuffer(b"".join(it[0] for it in items), np.uint8)
    index = np.array([it[1] for it in items], np.uint32)
    hashes = np.frombuffer(b"".join(it[2] for it in items), np.uint8)
    proofs = np.zeros((n, stride), np.uint8)
    for t, it in enumerate(items):
        raw = b"".join(it[3])
        proofs[t, : len(raw)] = np.frombuffer(raw, np.uint8)
    plen = np.array([len(it[3]) for it in items], np.uint32)
    last = np.array([it[4] for it in items], np.uint8)
    ok = torch.full((n,), 7, dtype=torch.uint8, device="cuda:0")
    rs.block_proof_check_batch(ctx, n, _dev(roots), 32, _dev(index), _dev(hashes), 32, _dev(proofs.reshape(-1)),
                               stride, _dev(plen), _dev(last), ok)
    got = ok.cpu().numpy()
    assert np.array_equal(got, want), np.nonzero(got != want)[0].tolist()
    # last = null is all check_proof
    sel = np.nonzero(last == 0)[0]
    ok0 = torch.full((n,), 7, dtype=torch.uint8, device="cuda:0")
    rs.block_proof_check_batch(ctx, n, _dev(roots), 32, _dev(index), _dev(hashes), 32, _dev(proofs.reshape(-1)),
                               stride, _dev(plen), None, ok0)
    assert np.array_equal(ok0.cpu().numpy()[sel], want[sel])
    # a proof the item's stride cannot hold is rejected, not read: 2 digests of stride, 3 claimed
    ok1 = torch.full((2,), 7, dtype=torch.uint8, device="cuda:0")
    rs.block_proof_check_batch(ctx, 2, _dev(roots), 32, _dev(index), _dev(hashes), 32,
                               torch.zeros(128, dtype=torch.uint8, device="cuda:0"), 64,
                               _dev(np.array([3, 3], np.uint32)), None, ok1)
    assert ok1.cpu().numpy().tolist() == [0, 0]


@pytest.mark.gpu
def test_block_hashes_over_device_shreds(ctx):
    """coder_shred_batch -> slice trees -> block trees with no host copy in between: 6 slices
    as blocks [3, 1, 2] == the oracle's tree over the oracle's slice roots."""
    dev = torch.device("cuda:0")
    S, nslices, counts = 64, 6, [3, 1, 2]
    rng = random.Random(19)
    # every payload pads to shred size S (reed_solomon.rs:94-95): 32*S - 64 <= len < 32*S
    lens = [rng.randint(32 * S - 64, 32 * S - 1) for _ in range(nslices)]
    raw = o.splitmix64_bytes(0x5EED5, nslices * 32 * S)
    payloads = [raw[i * 32 * S: i * 32 * S + lens[i]] for i in range(nslices)]
    pay = torch.zeros((nslices, 32 * S), dtype=torch.uint8, device=dev)
    for i, p in enumerate(payloads):
        pay[i, : len(p)] = torch.frombuffer(bytearray(p), dtype=torch.uint8).to(dev)
    cw = torch.zeros((nslices, 64 * S), dtype=torch.uint8, device=dev)
    rs.coder_shred_batch(ctx, 32, nslices, S, pay, 32 * S, lens, cw, 64 * S)
    roots = torch.zeros(nslices * 32, dtype=torch.uint8, device=dev)
    rs.merkle_build_batch(ctx, 64, S, nslices, cw, S, 64 * S, roots)
    hashes = torch.zeros(len(counts) * 32, dtype=torch.uint8, device=dev)
    rs.block_tree_batch(ctx, len(counts), counts, roots, hashes)
    got = hashes.cpu().numpy().reshape(len(counts), 32)
    want_roots = []
    for p in payloads:
        shreds = o.coder_shred(p, 32)
        want_roots.append(mo.slice_tree(shreds.data, shreds.coding).root())
    at = 0
    for b, n in enumerate(counts):
        assert got[b].tobytes() == mo.MerkleTree(want_roots[at: at + n]).root(), b
        at += n


@pytest.mark.gpu
def test_errors_leave_outputs_untouched(ctx):
    dev = torch.device("cuda:0")
    roots = _dev(_roots(0xE44, 2048).reshape(-1))
    hashes = torch.full((3 * 32 + 16,), 0xAA, dtype=torch.uint8, device=dev)
    nstride = 32 * rs.merkle_node_count(1024)
    nodes = torch.full((2 * nstride,), 0xAA, dtype=torch.uint8, device=dev)
    proofs = torch.full((2 * 32 * 10 * 1024,), 0xAA, dtype=torch.uint8, device=dev)

    def refused(*args):
        with pytest.raises(rs.RSError) as e:
            rs.block_tree_batch(ctx, *args)
        assert e.value.kind == "InvalidArgument"

    refused(2, [5, 0], roots, hashes, nodes, nstride)
    refused(2, [1025, 5], roots, hashes, nodes, nstride)
    refused(1, [5], roots, hashes.data_ptr() + 8)
    refused(1, [5], roots, None)
    # the second block's proofs need 32 * 10 * 1024 bytes
    refused(2, [4, 1024], roots, hashes, nodes, nstride, proofs, 32 * 10 * 1024 - 16)
    refused(2, [4, 1024], roots, hashes, nodes, nstride - 32)
    refused(2, [4, 4], roots, hashes, nodes, nstride + 8)
    rs.block_tree_batch(ctx, 0, [], roots, hashes, nodes, nstride, proofs, 32 * 10 * 1024)
    rs.block_tree_batch(ctx, 0, [], None, None)
    torch.cuda.synchronize()
    for out in (hashes, nodes, proofs):
        assert bool((out == 0xAA).all().item())
