"""Length and alignment edges of the hash and cipher kernels (GPU): the SHA-256 leaf loaders of
merkle.hip, sha256_bytes and aes_ctr_kernel of cipher.hip.

The code paths that differ from the straight-line case sit at lengths a random draw almost never
reaches: the SHA-256 padding rule changes at total % 64 in {55, 56, 63, 0} (a leaf hashes 32 label
bytes + S), the pipelined whole-block loop hands over to the padding path at every multiple of 64,
and the CTR counter's segment term only matters past 32 KiB.  Every expectation below comes from
hashlib, oracle/merkle_oracle.py or oracle/cipher_oracle.py; "the bytes past the length do not
matter" and the round trips are checked on top of those comparisons.
"""

import hashlib
import struct

import numpy as np
import pytest
import torch  # before the library: torch's HIP runtime must be the process's first

import cipher_oracle as co
import merkle_oracle as mo
from alpenglow_amd import rs

# ------------------------------------------------------------------ uniform Merkle leaf loaders

MK_SIZES = list(range(0, 201)) + [1000, 1016, 1023, 1024, 1025]
N_LEAVES, NSLICES = 5, 3                      # an odd level at heights 0 and 2: pairs with EMPTY_ROOTS
ITEMS = N_LEAVES * NSLICES
HEIGHT, NODE_COUNT = 3, 11
NODES_B, PROOFS_B = 32 * NODE_COUNT, 32 * HEIGHT * N_LEAVES   # per slice; both multiples of 16
FLIP_ITEM = 1 * N_LEAVES + 3                  # the leaf whose last data byte the build test flips
LAYOUTS = ("aligned", "byte")
LEAF_KERNEL = {"aligned": "leaf_aligned", "byte": "leaf_byte"}


def _leaf_stride(layout, S):
    return max(16, (S + 1 + 15) // 16 * 16) if layout == "aligned" else S + 1


@pytest.fixture(scope="module")
def mk_ref():
    """Per size: the 15 leaves' data and the oracle's answers (computed once, read-only)."""
    assert rs.merkle_height(N_LEAVES) == HEIGHT and rs.merkle_node_count(N_LEAVES) == NODE_COUNT
    rng = np.random.default_rng(0x1EAF)
    ref = {}
    for S in MK_SIZES:
        data = rng.integers(0, 256, (ITEMS, S), dtype=np.uint8)
        rows = [data[t].tobytes() for t in range(ITEMS)]
        trees = [mo.MerkleTree(rows[N_LEAVES * s: N_LEAVES * (s + 1)]) for s in range(NSLICES)]
        flipped = None
        if S:
            alt = list(rows[N_LEAVES * 1: N_LEAVES * 2])
            alt[3] = alt[3][:-1] + bytes([alt[3][-1] ^ 1])
            flipped = mo.MerkleTree(alt)
        ref[S] = dict(
            data=data, rows=rows, trees=trees, flipped=flipped,
            leaves=[hashlib.sha256(mo.LEAF_LABEL + r).digest() for r in rows],
            nodes=[b"".join(t.nodes) for t in trees],
            proofs=[b"".join(b"".join(t.create_proof(j)) for j in range(N_LEAVES)) for t in trees])
        assert all(t.height() == HEIGHT and len(t.nodes) == NODE_COUNT for t in trees)
    return ref


def _pack(mk_ref, layout):
    """All sizes' rows in one buffer: size S at a 16-byte aligned offset (plus one byte in the byte
    layout), 15 rows of leaf_stride bytes.  Returns {variant: host array}, offsets, strides.
    Variants: "base" (random row padding), "pad" (every byte outside the S data bytes of each row
    flipped), "last" (every row's last data byte flipped), "one" (only FLIP_ITEM's)."""
    rng = np.random.default_rng(0xA11 + len(layout))
    offs, strides, at = {}, {}, 0
    for S in MK_SIZES:
        strides[S] = _leaf_stride(layout, S)
        offs[S] = at + (layout == "byte")
        at = (offs[S] + ITEMS * strides[S] + 15) // 16 * 16
    base = rng.integers(0, 256, at + 16, dtype=np.uint8)
    is_data = np.zeros(base.size, bool)
    last, one = np.zeros(base.size, np.uint8), np.zeros(base.size, np.uint8)
    for S in MK_SIZES:
        rows = base[offs[S]: offs[S] + ITEMS * strides[S]].reshape(ITEMS, strides[S])
        rows[:, :S] = mk_ref[S]["data"]
        is_data[offs[S]: offs[S] + ITEMS * strides[S]].reshape(ITEMS, strides[S])[:, :S] = True
        if S:
            last[offs[S]: offs[S] + ITEMS * strides[S]].reshape(ITEMS, strides[S])[:, S - 1] = 1
            one[offs[S] + FLIP_ITEM * strides[S] + S - 1] = 1
    variants = {"base": base, "pad": base ^ np.where(is_data, 0, 0xFF).astype(np.uint8), "last": base ^ last,
                "one": base ^ one}
    return variants, offs, strides


def _check_layout(layout, d, off, stride):
    """The launchers pick the loader from the base pointer and the strides alone."""
    ptr = d.data_ptr() + off
    if layout == "aligned":
        assert ptr % 16 == 0 and stride % 16 == 0
    else:
        assert ptr % 16 == 1


@pytest.mark.gpu
@pytest.mark.parametrize("layout", LAYOUTS)
def test_merkle_build_every_leaf_size(ctx, mk_ref, layout):
    """merkle_build_batch for every leaf size 0..200 and around 1000 / 1024, through the aligned
    loader (16-byte aligned rows) and the byte loader (rows at an odd address, stride S + 1): the
    leaves equal hashlib's SHA-256(LEAF_LABEL || data), the upper nodes, roots and every proof the
    oracle's.  The build is bit-identical with every byte of row padding flipped (the hash stops at
    the leaf's length), and flipping one leaf's last data byte changes that leaf and the root to
    the oracle's values for the changed data.  Each call must report the loader under test."""
    dev = torch.device("cuda:0")
    variants, offs, strides = _pack(mk_ref, layout)
    names = ("base", "pad", "one")
    d = {v: torch.from_numpy(variants[v]).to(dev) for v in names}
    nz = len(MK_SIZES)
    roots = torch.zeros((3, nz, NSLICES * 32), dtype=torch.uint8, device=dev)
    nodes = torch.zeros((3, nz, NSLICES * NODES_B), dtype=torch.uint8, device=dev)
    proofs = torch.zeros((3, nz, NSLICES * PROOFS_B), dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    for v, name in enumerate(names):
        for i, S in enumerate(MK_SIZES):
            _check_layout(layout, d[name], offs[S], strides[S])
            rs.merkle_build_batch(ctx, N_LEAVES, S, NSLICES, d[name].data_ptr() + offs[S], strides[S],
                                  N_LEAVES * strides[S], roots[v, i], nodes[v, i], NODES_B, proofs[v, i], PROOFS_B)
            assert rs.last_merkle_kernels(ctx) == {LEAF_KERNEL[layout]}, (S, name)
    ctx.synchronize()
    torch.cuda.synchronize()
    roots, nodes, proofs = (x.cpu().numpy() for x in (roots, nodes, proofs))
    for i, S in enumerate(MK_SIZES):
        ref = mk_ref[S]
        for s in range(NSLICES):
            got_nodes = nodes[0, i, NODES_B * s: NODES_B * (s + 1)].tobytes()
            assert got_nodes[: 32 * N_LEAVES] == b"".join(ref["leaves"][N_LEAVES * s: N_LEAVES * (s + 1)]), (S, s)
            assert got_nodes == ref["nodes"][s], (S, s)
            assert roots[0, i, 32 * s: 32 * (s + 1)].tobytes() == ref["trees"][s].root(), (S, s)
            assert proofs[0, i, PROOFS_B * s: PROOFS_B * (s + 1)].tobytes() == ref["proofs"][s], (S, s)
        # row padding flipped: nothing moves
        assert np.array_equal(nodes[1, i], nodes[0, i]) and np.array_equal(roots[1, i], roots[0, i]), S
        assert np.array_equal(proofs[1, i], proofs[0, i]), S
        if S:  # one data byte flipped: that leaf's node and its slice's root move, to the oracle's values
            s, j = divmod(FLIP_ITEM, N_LEAVES)
            alt = ref["flipped"]
            assert nodes[2, i, NODES_B * s: NODES_B * (s + 1)].tobytes() == b"".join(alt.nodes), S
            assert roots[2, i, 32 * s: 32 * (s + 1)].tobytes() == alt.root() != ref["trees"][s].root(), S
            assert alt.nodes[j] != ref["trees"][s].nodes[j]
            for q in range(NSLICES):
                if q != s:
                    assert roots[2, i, 32 * q: 32 * (q + 1)].tobytes() == ref["trees"][q].root(), (S, q)


@pytest.mark.gpu
@pytest.mark.parametrize("layout", LAYOUTS)
def test_merkle_verify_every_leaf_size(ctx, mk_ref, layout):
    """merkle_verify_batch (its own instantiations of both uniform loaders) over the same sizes and
    layouts, on the oracle's roots and proofs: valid items pass, still pass with the row padding
    flipped (the byte at offset S included), and fail with data byte S - 1 or one proof byte
    flipped.  Every verdict equals mo.check_proof on the same bytes.  The library reports the
    leaf-kernel class of builds only; here the test asserts the launcher's whole criterion for
    the loader instead: the alignment of the row pointer and stride."""
    dev = torch.device("cuda:0")
    variants, offs, strides = _pack(mk_ref, layout)
    d = {v: torch.from_numpy(variants[v]).to(dev) for v in ("base", "pad", "last")}
    nz = len(MK_SIZES)
    index = np.tile(np.arange(N_LEAVES, dtype=np.uint32), NSLICES)
    root_rows = np.zeros((nz, ITEMS, 32), np.uint8)
    proof_rows = np.zeros((nz, ITEMS, 32 * HEIGHT), np.uint8)
    for i, S in enumerate(MK_SIZES):
        for t in range(ITEMS):
            tree = mk_ref[S]["trees"][t // N_LEAVES]
            root_rows[i, t] = np.frombuffer(tree.root(), np.uint8)
            proof_rows[i, t] = np.frombuffer(b"".join(tree.create_proof(t % N_LEAVES)), np.uint8)
    bad_rows = proof_rows.copy()
    for i, S in enumerate(MK_SIZES):
        for t in range(ITEMS):
            bad_rows[i, t, (7 * t + S) % (32 * HEIGHT)] ^= 0x80
    d_index, d_roots = torch.from_numpy(index).to(dev), torch.from_numpy(root_rows).to(dev)
    d_proofs, d_bad = torch.from_numpy(proof_rows).to(dev), torch.from_numpy(bad_rows).to(dev)
    ok = torch.full((nz, 4, ITEMS), 7, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    runs = (("base", d_proofs), ("pad", d_proofs), ("last", d_proofs), ("base", d_bad))
    for i, S in enumerate(MK_SIZES):
        for r, (name, prf) in enumerate(runs):
            if name == "last" and S == 0:
                continue  # no data byte to flip
            _check_layout(layout, d[name], offs[S], strides[S])
            rs.merkle_verify_batch(ctx, ITEMS, S, d[name].data_ptr() + offs[S], strides[S], d_index, d_roots[i], 32,
                                   prf[i], 32 * HEIGHT, HEIGHT, ok[i, r])
    ctx.synchronize()
    torch.cuda.synchronize()
    got = ok.cpu().numpy()
    for i, S in enumerate(MK_SIZES):
        for r, (name, prf) in enumerate(runs):
            if name == "last" and S == 0:
                continue
            host = variants[name][offs[S]: offs[S] + ITEMS * strides[S]].reshape(ITEMS, strides[S])
            prows = bad_rows if prf is d_bad else proof_rows
            want = [int(mo.check_proof(host[t, :S].tobytes(), int(index[t]), root_rows[i, t].tobytes(),
                                       [prows[i, t, 32 * h: 32 * h + 32].tobytes() for h in range(HEIGHT)]))
                    for t in range(ITEMS)]
            assert want == [1 if r < 2 else 0] * ITEMS
            assert got[i, r].tolist() == want, (S, name, r)


@pytest.mark.gpu
def test_merkle_build_var_every_even_size(ctx):
    """One merkle_build_batch_var call whose 100 slices take every even leaf size 2..200 (the
    per-slice-size loader, rows packed at j * size): leaves against hashlib, nodes and roots against
    the oracle, and bit-identical with the bytes after each slice's 64 rows flipped."""
    dev = torch.device("cuda:0")
    sizes = list(range(2, 201, 2))
    n, stride = len(sizes), 64 * 200
    rng = np.random.default_rng(0x7A4)
    base = rng.integers(0, 256, (n, stride), dtype=np.uint8)
    pad = base.copy()
    for s, S in enumerate(sizes):
        pad[s, 64 * S:] ^= 0xFF
    cnt = rs.merkle_node_count(64)
    out = []
    for host in (base, pad):
        d = torch.from_numpy(host).to(dev)
        roots = torch.zeros(n * 32, dtype=torch.uint8, device=dev)
        nodes = torch.zeros((n, 32 * cnt), dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        rs.merkle_build_batch_var(ctx, n, sizes, d, stride, roots, nodes, 32 * cnt)
        assert rs.last_merkle_kernels(ctx) == {"leaf_var"}
        ctx.synchronize()
        torch.cuda.synchronize()
        out.append((roots.cpu().numpy().reshape(n, 32), nodes.cpu().numpy()))
    for s, S in enumerate(sizes):
        rows = [base[s, j * S: (j + 1) * S].tobytes() for j in range(64)]
        tree = mo.MerkleTree(rows)
        for roots, nodes in out:
            assert nodes[s, : 32 * 64].tobytes() == b"".join(hashlib.sha256(mo.LEAF_LABEL + r).digest() for r in rows), S
            assert nodes[s].tobytes() == b"".join(tree.nodes), S
            assert roots[s].tobytes() == tree.root(), S


# ------------------------------------------------------------------ sha256_batch

@pytest.mark.gpu
def test_sha256_batch_every_length(ctx):
    """One sha256_batch call over every length 0..260 and the lengths around 4 KiB, 32 KiB and
    64 KiB, at an odd stride so the bases take every residue mod 16; digests equal hashlib's, and
    still do after the byte at offset len of every row is flipped."""
    dev = torch.device("cuda:0")
    lens = list(range(0, 261)) + [4095, 4096, 4097, 32767, 32768, 32769, 65599, 65600]
    n, stride = len(lens), 65601
    assert {(b * stride) % 16 for b in range(n)} == set(range(16)) and max(lens) < stride
    host = np.random.default_rng(0x5A2).integers(0, 256, (n, stride), dtype=np.uint8)
    past = host.copy()
    past[np.arange(n), lens] ^= 0xFF
    want = [hashlib.sha256(host[b, :L].tobytes()).digest() for b, L in enumerate(lens)]
    for rows in (host, past):
        d = torch.from_numpy(rows).to(dev)
        assert d.data_ptr() % 16 == 0
        dig = torch.zeros(32 * n, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        rs.sha256_batch(ctx, n, d, stride, lens, dig)
        ctx.synchronize()
        torch.cuda.synchronize()
        got = dig.cpu().numpy().reshape(n, 32)
        for b, L in enumerate(lens):
            assert got[b].tobytes() == want[b], L


# ------------------------------------------------------------------ AES-128-CTR keystream

SEG = 32768                                   # aes_ctr_kernel: one workgroup per 32 KiB segment
SEG_BLOCKS, STEP_BLOCKS = SEG // 16, 256      # 2048 counters per segment, 256 per thread-group step


def _sample_counters(length):
    """Counters whose keystream blocks a long buffer is checked at: the first and last block of
    every segment, the blocks either side of every 4 KiB thread-group step (ctr % 256 in {0, 255})
    in the first two segments, and the last (possibly partial) block."""
    nb = (length + 15) // 16
    picks = set()
    for seg in range((length + SEG - 1) // SEG):
        picks |= {seg * SEG_BLOCKS, seg * SEG_BLOCKS + SEG_BLOCKS - 1}
        if seg < 2:
            for k in range(1, SEG_BLOCKS // STEP_BLOCKS):
                picks |= {seg * SEG_BLOCKS + k * STEP_BLOCKS - 1, seg * SEG_BLOCKS + k * STEP_BLOCKS}
    picks.add(nb - 1)
    return sorted(c for c in picks if 0 <= c < nb)


def _check_sampled(got, plain, key, length, what):
    """got[0..length) == plain ^ keystream at the sampled blocks (plain None: zero plaintext)."""
    rks = co.expand_key(key)
    for ctr in _sample_counters(length):
        ks = co.aes128_encrypt_block(key, struct.pack("<QQ", ctr, 0), rks)
        m = min(16, length - 16 * ctr)
        want = np.frombuffer(ks, np.uint8)[:m]
        if plain is not None:
            want = want ^ plain[16 * ctr: 16 * ctr + m]
        assert got[16 * ctr: 16 * ctr + m].tobytes() == want.tobytes(), (what, length, ctr)


@pytest.mark.gpu
def test_keystream_every_short_length(ctx):
    """cipher_apply_keystream_batch at every length 0..130 (whole blocks, partial tails, the empty
    buffer) at an odd stride, compared in full with the oracle; nothing past the length is written
    and a second call returns the original."""
    dev = torch.device("cuda:0")
    lens = list(range(0, 131))
    n, stride = len(lens), 133
    rng = np.random.default_rng(0xC7)
    host = rng.integers(0, 256, (n, stride), dtype=np.uint8)
    keys = rng.integers(0, 256, (n, 16), dtype=np.uint8)
    d, dk = torch.from_numpy(host).to(dev), torch.from_numpy(keys).to(dev)
    torch.cuda.synchronize()
    rs.cipher_apply_keystream_batch(ctx, n, dk, d, stride, lens)
    ctx.synchronize()
    torch.cuda.synchronize()
    got = d.cpu().numpy().copy()
    for b, L in enumerate(lens):
        assert got[b, :L].tobytes() == co.apply_keystream(keys[b].tobytes(), host[b, :L].tobytes()), L
        assert got[b, L:].tobytes() == host[b, L:].tobytes(), L
    rs.cipher_apply_keystream_batch(ctx, n, dk, d, stride, lens)
    ctx.synchronize()
    torch.cuda.synchronize()
    assert np.array_equal(d.cpu().numpy(), host)


@pytest.mark.gpu
def test_keystream_across_segment_edges(ctx):
    """Buffers either side of one, two and three 32 KiB segments and one of 1 MiB + 1 in a single
    call, with a buffer shorter than a segment among them (its other workgroups exit early).  The
    pure-Python CTR oracle is too slow for these lengths: the long buffers start as zeros, so the
    result is the keystream itself, checked block by block against
    co.aes128_encrypt_block(key, LE64(ctr) || 0^8) at the sampled counters of _sample_counters;
    one long buffer holds random plaintext (checked as plaintext ^ keystream at the same blocks).
    Bytes from len to the end of each row are untouched, and a second call restores every row.
    The counter's high word (blk >> 32) needs a 64 GiB buffer and stays untested."""
    dev = torch.device("cuda:0")
    lens = [32752, 32767, 32768, 32769, 32783, 32784, 100, 65535, 65536, 65537, 98305, 1048577, 65537]
    short, random_plain = lens.index(100), len(lens) - 1
    n, stride = len(lens), 1048579
    assert stride % 2 == 1 and stride > max(lens)
    rng = np.random.default_rng(0xC8)
    host = rng.integers(1, 256, (n, stride), dtype=np.uint8)   # rows' tails: non-zero filler
    for b, L in enumerate(lens):
        if b not in (short, random_plain):
            host[b, :L] = 0
    keys = rng.integers(0, 256, (n, 16), dtype=np.uint8)
    d, dk = torch.from_numpy(host).to(dev), torch.from_numpy(keys).to(dev)
    torch.cuda.synchronize()
    rs.cipher_apply_keystream_batch(ctx, n, dk, d, stride, lens)
    ctx.synchronize()
    torch.cuda.synchronize()
    got = d.cpu().numpy().copy()
    for b, L in enumerate(lens):
        key = keys[b].tobytes()
        if b == short:
            assert got[b, :L].tobytes() == co.apply_keystream(key, host[b, :L].tobytes())
        else:
            _check_sampled(got[b], host[b] if b == random_plain else None, key, L, "keystream")
        assert np.array_equal(got[b, L:], host[b, L:]), L
    rs.cipher_apply_keystream_batch(ctx, n, dk, d, stride, lens)
    ctx.synchronize()
    torch.cuda.synchronize()
    assert np.array_equal(d.cpu().numpy(), host)


@pytest.mark.gpu
@pytest.mark.parametrize("scheme", [rs.AON_AONT, rs.AON_PETS])
def test_aon_across_segment_edges(ctx, scheme):
    """aon_encrypt_batch / aon_decrypt_batch with payloads either side of a segment edge, so that
    decrypt's len - 16 and encrypt's len fall on both sides of it: the ciphertext equals
    payload ^ keystream at the sampled blocks, the 16-byte tail equals key ^ SHA-256(ciphertext)[:16]
    (AONT) or the key (PETS) by hashlib, nothing past the tail is written, and decrypt returns the
    payload lengths and the payloads."""
    dev = torch.device("cuda:0")
    lens = [32751, 32752, 32753, 32768, 32769, 65536]
    n, stride = len(lens), 65553
    assert stride % 2 == 1 and stride >= max(lens) + 16
    rng = np.random.default_rng(0xA0 + scheme)
    host = rng.integers(0, 256, (n, stride), dtype=np.uint8)
    keys = rng.integers(0, 256, (n, 16), dtype=np.uint8)
    d, dk = torch.from_numpy(host).to(dev), torch.from_numpy(keys).to(dev)
    torch.cuda.synchronize()
    rs.aon_encrypt_batch(ctx, scheme, n, dk, d, stride, lens)
    ctx.synchronize()
    torch.cuda.synchronize()
    enc = d.cpu().numpy().copy()
    for b, L in enumerate(lens):
        key = keys[b].tobytes()
        _check_sampled(enc[b], host[b], key, L, "aon")
        tail = key
        if scheme == rs.AON_AONT:
            tail = bytes(k ^ h for k, h in zip(key, hashlib.sha256(enc[b, :L].tobytes()).digest()))
        assert enc[b, L: L + 16].tobytes() == tail, L
        assert np.array_equal(enc[b, L + 16:], host[b, L + 16:]), L
    out = rs.aon_decrypt_batch(ctx, scheme, n, d, stride, [L + 16 for L in lens])
    ctx.synchronize()
    torch.cuda.synchronize()
    dec = d.cpu().numpy()
    assert out.tolist() == lens
    for b, L in enumerate(lens):
        assert np.array_equal(dec[b, :L], host[b, :L]), L
        assert np.array_equal(dec[b, L + 16:], host[b, L + 16:]), L
