"""Shared cases and checkers of tests/test_shredder_kind_edges.py (import-only): slices at
chosen framed lengths, honest and Byzantine leaders, structured arrivals, one composed call into
0xA5-filled buffers, and the comparison with the oracle (oracle/shredder_oracle.py: shred_kind,
datagrams, receive, deshred_kind).  The generators follow tests/test_shredder_pipeline.py and
tests/test_shredder_exact_rerun.py."""

import numpy as np

import ed25519_oracle as ed
import rs_oracle as o
import shredder_oracle as so
import slice_oracle as sl
from alpenglow_amd import rs

FILL = 0xA5
PKT = 1536  # datagram slot stride (>= 1325 bytes for a 1 KiB shred)
SEED = bytes(range(7, 39))
PK = ed.secret_to_public(SEED)
OTHER_SEED = bytes(range(100, 132))
KEY_BYTES = 16
KINDS = [so.CODING_ONLY, so.PETS, so.AONT]
NAMES = {so.REGULAR: "regular", so.CODING_ONLY: "coding_only", so.PETS: "pets", so.AONT: "aont"}


def wire_len(S):
    """Bytes of a datagram that carries an S-byte shred and a six-hash Merkle path."""
    return rs.shred_datagram_bytes(S, so.HEIGHT)


def rows_of(kind):
    """Codeword rows of a slice: the coder's 32 data + m coding shards."""
    return 32 + so.CODING[kind]


def stride_of(kind, S):
    """A padded codeword stride, (32 + m) S + 12: not a multiple of S, and a multiple of 4 as the
    calls require -- PETS's 65 rows of S = 2 mod 4 bytes take two bytes more for that.  (Regular:
    64 S, the stride its calls are defined with.)"""
    return 64 * S if kind == so.REGULAR else (rows_of(kind) * S + 12 + 3) // 4 * 4


def extra_of(kind):
    return KEY_BYTES if kind in (so.PETS, so.AONT) else 0


def framed_range(kind, S):
    """The framed lengths (header + data) whose payload -- with the key tail of PETS / AONT -- pads
    to shred size S: the coder pads len to (len + 64 - len % 64) / 32, so 32 S - 64 <= len <= 32 S - 1."""
    ex = extra_of(kind)
    return max(32 * S - 64 - ex, sl.header_len(None)), min(32 * S - 1, sl.MAX_DATA_PER_SLICE) - ex


def make_slice(rng, kind, S, framed, parent, i=0):
    """(parent, data, slot, slice index, is_last, key) with header + data = framed bytes."""
    par = (rng.randrange(1 << 40), rng.randbytes(32)) if parent else None
    lo, hi = framed_range(kind, S)
    assert max(lo, sl.header_len(par)) <= framed <= hi, (kind, S, framed, parent)
    return (par, rng.randbytes(framed - sl.header_len(par)), rng.randrange(1 << 32), rng.randrange(1024),
            bool(i % 3 == 2), rng.randbytes(16))


def random_slices(rng, kind, S, n):
    """n slices of random framed lengths that pad to S, parents alternating where one fits (at
    S = 2 a parent's 49-byte header leaves PETS / AONT no room for the key tail)."""
    lo, hi = framed_range(kind, S)
    out = []
    for i in range(n):
        parent = bool(i % 2) and sl.header_len((0, b"")) <= hi
        out.append(make_slice(rng, kind, S, rng.randrange(max(lo, 49 if parent else 9), hi + 1), parent, i))
    return out


def altered(kind, slice_, raw, t):
    """The 64 datagrams of a leader that signs a non-codeword: output shred t XORed with 0x5A
    after encoding, the tree and the signature over the altered shreds."""
    nd = so.DATA_OUT[kind]
    shards = list(raw.data) + list(raw.coding)
    shards[t] = bytes(x ^ 0x5A for x in shards[t])
    return so.datagrams(shards[:nd], shards[nd:], slice_[2], slice_[3], slice_[4], SEED)[0]


def oracle_leader(kind, slices):
    """Per slice (its 64 datagrams, its output RawShreds) from so.shred_kind."""
    out = []
    for s_ in slices:
        pkts, raw, _, _ = so.shred_kind(kind, *s_[:5], SEED, s_[5])
        out.append((pkts, raw))
    return out


def expect(rows, S, kind):
    """The oracle's verdict on one slice's 64 slots (bytes or None): (status, result or None, the
    slots after the call, the kept flags).  Kept slots stay as received; a successful slice gets
    every other slot filled, a failed one keeps all of them."""
    kept = so.receive(rows, PK, S, so.DATA_OUT[kind])
    st, res = so.deshred_kind(kept, kind)
    if st == so.OK:
        slots = [rows[j] if kept[j] is not None else res["datagrams"][j] for j in range(64)]
    else:
        slots = [x if x is not None else b"" for x in rows]
    return st, res, slots, [x is not None for x in kept]


def pack(rows):
    """The datagram slots of a batch as the call takes them: 0xA5 behind every datagram, length 0
    for an absent slot."""
    n = len(rows)
    buf = np.full((n * 64, PKT), FILL, np.uint8)
    ln = np.zeros(n * 64, np.int32)
    for b, r in enumerate(rows):
        for j, p in enumerate(r):
            if p is not None:
                buf[b * 64 + j, :len(p)] = np.frombuffer(p, np.uint8)
                ln[b * 64 + j] = len(p)
    return buf, ln


# ---- the composed calls (torch is imported by the test module's fixture: GPU tests only) ---------

def _dev(a, dev):
    import torch

    return torch.from_numpy(np.array(a, copy=True)).to(dev)


def _filled(shape, dev):
    import torch

    return torch.full(shape, FILL, dtype=torch.uint8, device=dev)


class Shredded:
    """The outputs of one ag_shredder_shred_batch_kind call into 0xA5-filled buffers (host copies)."""

    def __init__(self, cw, pkts, lens, roots, sigs):
        self.cw, self.pkts, self.lens, self.roots, self.sigs = cw, pkts, lens, roots, sigs

    def datagrams(self, b):
        return [self.pkts[b * 64 + j, :self.lens[b * 64 + j]].tobytes() for j in range(64)]


def gpu_shred(ctx, dev, kind, slices, S):
    """One shred call; a refused call's error is kept in .error, beside the buffers it must leave alone."""
    import torch

    n = len(slices)
    maxd = max(len(s_[1]) for s_ in slices)
    data = np.zeros((n, max(maxd, 1)), np.uint8)
    for b, s_ in enumerate(slices):
        data[b, :len(s_[1])] = np.frombuffer(s_[1], np.uint8)
    stride = stride_of(kind, S)
    cw = _filled((n, stride), dev)
    pkts = _filled((n * 64, PKT), dev)
    lens = torch.zeros(n * 64, dtype=torch.int32, device=dev)
    roots, sigs = _filled((n, 32), dev), _filled((n, 64), dev)
    err = None
    try:
        rs.shredder_shred_batch_kind(ctx, kind, n, S, [s_[0] for s_ in slices], _dev(data, dev) if maxd else None,
                                     maxd, [len(s_[1]) for s_ in slices],
                                     _dev(np.array([s_[2] for s_ in slices], np.uint64), dev),
                                     _dev(np.array([s_[3] for s_ in slices], np.uint64), dev),
                                     _dev(np.array([s_[4] for s_ in slices], np.uint8), dev),
                                     _dev(np.frombuffer(SEED, np.uint8), dev), _dev(np.frombuffer(PK, np.uint8), dev),
                                     _dev(np.frombuffer(b"".join(s_[5] for s_ in slices), np.uint8), dev)
                                     if extra_of(kind) else None, cw, stride, pkts, PKT, lens, roots_out=roots,
                                     sigs_out=sigs)
    except rs.RSError as e:
        err = e
    torch.cuda.synchronize()
    out = Shredded(cw.cpu().numpy(), pkts.cpu().numpy(), lens.cpu().numpy(), roots.cpu().numpy(), sigs.cpu().numpy())
    out.error = err
    return out


def output_rows(kind):
    """The codeword row of each of the 64 output shreds (CodingOnly: the coding rows; PETS: row 31,
    the data shred with the key, is no output shred)."""
    return [r for r in range(rows_of(kind)) if (kind != so.CODING_ONLY or r >= 32) and (kind != so.PETS or r != 31)][:64]


def check_shred(got, kind, slices, S, want):
    """Datagrams, roots and signatures byte-exact against want = [so.shred_kind(...)]; the output
    rows of the codeword are the raw shreds; nothing is written past a slice's rows or past a
    datagram's length."""
    assert got.error is None, got.error
    rows = rows_of(kind)
    for b, (pkts, raw, root, sig) in enumerate(want):
        where = (NAMES[kind], S, b)
        assert got.roots[b].tobytes() == root, where
        assert got.sigs[b].tobytes() == sig, where
        assert got.datagrams(b) == pkts, where
        shreds = list(raw.data) + list(raw.coding)
        for j, r in enumerate(output_rows(kind)):
            assert got.cw[b, r * S:(r + 1) * S].tobytes() == shreds[j], where + (j,)
        assert (got.cw[b, rows * S:] == FILL).all(), where
        for j in range(64):
            t = b * 64 + j
            assert got.lens[t] == wire_len(S), where + (j,)
            assert (got.pkts[t, got.lens[t]:] == FILL).all(), where + (j,)


def gpu_leader(ctx, dev, kind, slices, S):
    """The honest leader's shred call on the device: per slice (its 64 datagrams, its output
    RawShreds).  Used only at an S where a test pins this call to so.shred_kind."""
    got = gpu_shred(ctx, dev, kind, slices, S)
    assert got.error is None, got.error
    nd = so.DATA_OUT[kind]
    out = []
    for b in range(len(slices)):
        shreds = [got.cw[b, r * S:(r + 1) * S].tobytes() for r in output_rows(kind)]
        out.append((got.datagrams(b), o.RawShreds(data=shreds[:nd], coding=shreds[nd:])))
    return out


class Deshredded:
    """One composed deshred call into 0xA5-filled codewords: the result, the slots and lengths
    after the call, the codewords, and the context's route records right after it."""


def gpu_deshred(ctx, dev, kind, rows, S):
    import torch

    n = len(rows)
    buf, ln = pack(rows)
    d_buf, d_ln = _dev(buf, dev), _dev(ln, dev)
    stride = stride_of(kind, S)
    cw = _filled((n, stride), dev)
    g = Deshredded()
    g.res = rs.shredder_deshred_batch_kind(ctx, kind, n, S, d_buf, PKT, d_ln, _dev(np.frombuffer(PK, np.uint8), dev),
                                           cw, stride)
    torch.cuda.synchronize()
    g.buf, g.ln, g.cw = d_buf.cpu().numpy(), d_ln.cpu().numpy(), cw.cpu().numpy()
    g.rerun = rs.last_exact_rerun(ctx)
    g.window = rs.last_window_kernels(ctx)
    g.encode = rs.last_encode_kernels(ctx)
    return g


def check_deshred(g, kind, rows, S, want):
    """Statuses, every datagram slot, header, parent and payload bytes against want = [expect(...)];
    nothing written past the slice's rows of a codeword stride, past a datagram's written length,
    or into a datagram that was present and kept; a failed slice's present datagrams and every
    length of it stay as they were.  The bytes of a failed slice's absent slots are checked from
    the datagram size on for PETS / AONT, which serialize the absent datagrams before they decrypt
    (include/alpenglow_rs.h), and everywhere for the others."""
    in_buf, in_ln = pack(rows)
    name = NAMES[kind]
    assert g.res.status.tolist() == [w[0] for w in want], \
        (name, S, [rs.STATUS_KIND.get(int(x), int(x)) for x in g.res.status], [w[0] for w in want])
    for b, (st, r, slots, kept) in enumerate(want):
        where = (name, S, b)
        assert (g.cw[b, rows_of(kind) * S:] == FILL).all(), where
        for j in range(64):
            t = 64 * b + j
            assert g.ln[t] == len(slots[j]), where + (j,)
            assert g.buf[t, :g.ln[t]].tobytes() == slots[j], where + (j,)
            if kept[j] or (st != so.OK and in_ln[t]):
                assert np.array_equal(g.buf[t], in_buf[t]), where + (j,)
            elif st != so.OK and kind in (so.PETS, so.AONT):
                assert (g.buf[t, wire_len(S):] == FILL).all(), where + (j,)
            else:
                assert (g.buf[t, max(g.ln[t], in_ln[t]):] == FILL).all(), where + (j,)
        if st != so.OK:
            continue
        assert (int(g.res.slots[b]), int(g.res.slice_indices[b]), bool(g.res.is_last[b])) == r["header"], where
        assert g.res.parents[b] == r["parent"], where
        off, m = int(g.res.data_offsets[b]), int(g.res.data_lens[b])
        assert g.cw[b, off:off + m].tobytes() == r["data"], where


def device_route(kind, S, n, rows):
    """Whether ag_shredder_deshred_batch_kind decodes this batch with the device-pattern ANY_K
    pass (and re-runs failed surplus slices with EXACT) rather than the whole batch with EXACT
    (shredder_api.cpp: fast_ok and pipe_tail_ok).  It depends on the datagrams kept, which for the
    leaders of these tests are the datagrams present."""
    T = S % 64
    if n < 2:
        return False
    if T == 0:
        return True
    if kind != so.AONT:
        return False
    held = [[x is not None for x in r] for r in rows]
    reencode = any(sum(h) > 32 or all(h[:32]) for h in held)
    return T >= 16 or not reencode


def check_route(g, kind, S, rows, want, byzantine_surplus=0):
    """The context's records against the route the batch must take.  Device-pattern pass: the
    re-run holds every failed surplus slice that decoded or failed its padding in the ANY_K pass,
    so at least the Byzantine ones, never the whole batch; where nothing is re-run (the re-run's
    coder call resets the kernel records) AONT's window kernel is on record, decode_h8 with the
    fused coding restore (its TAIL variant at a tail size).  Whole-batch EXACT: no window kernel
    of the device path and no re-run."""
    n = len(rows)
    surplus_failed = sum(w[0] in (so.BAD_ENCODING, so.INVALID_MERKLE_TREE) and sum(x is not None for x in r) > 32
                         for w, r in zip(want, rows))
    if device_route(kind, S, n, rows):
        slices, passes = g.rerun
        if kind == so.AONT and not slices:
            # (S = 960 + T would take the packed decoder; no size here does)
            assert g.window == {"decode_h8_fused"}, (NAMES[kind], S, g.window)
        assert byzantine_surplus <= slices <= surplus_failed < n, (NAMES[kind], S, g.rerun)
        assert passes == (1 if slices else 0), (NAMES[kind], S, g.rerun)
        return "device"
    assert g.window == set() and g.rerun == (0, 0), (NAMES[kind], S, g.window, g.rerun)
    return "exact"
