"""Shared Ed25519 test cases (seeded): valid signatures plus the malformed encodings the
ZIP-215 rules of ed25519-zebra 4.2.0 decide (crypto/signature.rs:100-103).  Expected
verdicts come from the oracle (oracle/ed25519_oracle.py)."""

import random

import ed25519_oracle as eo

P, L = eo.P, eo.L


def le(x: int) -> bytes:
    return int(x).to_bytes(32, "little")


def verify_cases(seed: int = 7, n_random: int = 24):
    """List of (pk, msg, sig) triples."""
    rng = random.Random(seed)
    cases = []
    keys = [bytes(rng.getrandbits(8) for _ in range(32)) for _ in range(4)]
    pks = [eo.secret_to_public(k) for k in keys]
    for i in range(n_random):
        k = i % len(keys)
        msg = bytes(rng.getrandbits(8) for _ in range(rng.choice([0, 1, 49, 49, 64, 111, 112, 200])))
        sig = eo.sign(keys[k], msg)
        cases.append((pks[k], msg, sig))
        # tampered message / signature / key
        if i % 4 == 0:
            cases.append((pks[k], msg + b"x", sig))
        if i % 4 == 1:
            bad = bytearray(sig)
            bad[rng.randrange(64)] ^= 1 << rng.randrange(8)
            cases.append((pks[k], msg, bytes(bad)))
        if i % 4 == 2:
            cases.append((pks[(k + 1) % len(keys)], msg, sig))
        if i % 4 == 3:  # s + l: same group element, non-canonical scalar -> rejected
            s = int.from_bytes(sig[32:], "little") + L
            if s < 2**256:
                cases.append((pks[k], msg, sig[:32] + le(s)))
    ident = le(1)
    small = eo.small_order_encodings()
    # cofactored equation: small-order A and R with s = 0 verify under ZIP-215
    for a in small:
        for r in small[:3]:
            cases.append((a, b"zip215", r + le(0)))
    # non-canonical y (y >= p) for A and R, "negative zero" x
    nc_one = le(P + 1)                       # y = p + 1 == 1 (the identity)
    neg_zero = le(1 | (1 << 255))            # identity with the sign bit set
    for a in (ident, nc_one, neg_zero):
        for r in (ident, nc_one, neg_zero):
            cases.append((a, b"noncanonical", r + le(0)))
    for y in range(19):                      # every non-canonical y in [p, 2^255)
        enc = le(P + y)
        if eo.decompress(enc) is not None:
            cases.append((enc, b"nc-y", ident + le(0)))
            cases.append((pks[0], b"nc-y", enc + le(0)))
    # random 32-byte strings as keys (about half do not decode)
    for _ in range(8):
        junk = bytes(rng.getrandbits(8) for _ in range(32))
        cases.append((junk, b"junk", eo.sign(keys[0], b"junk")))
    # s = l - 1 (largest canonical), s = l (smallest non-canonical)
    cases.append((pks[0], b"edge", ident + le(L - 1)))
    cases.append((pks[0], b"edge", ident + le(L)))
    return cases


# ---- SHA-512 padding boundaries ---------------------------------------------------------------
# SHA-512 pads into the same block up to total % 128 == 111 and opens another from 112.  The
# challenge hashes R || A || M (64 + len): lengths 47 / 48 and 175 / 176; the signing nonce hashes
# prefix || M (32 + len): 79 / 80 and 207 / 208.  The rest are whole blocks and their neighbours.
SHA512_EDGE_LENS = [0, 1, 47, 48, 49, 79, 80, 111, 112, 113, 175, 176, 207, 208, 239, 240, 255, 256, 257]


def edge_messages(seeds_per_len: int = 1, seed: int = 21):
    """[(secret seed, message)], seeds_per_len entries for each length of SHA512_EDGE_LENS."""
    rng = random.Random(seed)
    return [(rng.randbytes(32), rng.randbytes(n)) for n in SHA512_EDGE_LENS for _ in range(seeds_per_len)]


def flip_last(msg: bytes) -> bytes:
    return msg[:-1] + bytes([msg[-1] ^ 1])


def _hx(b: bytes) -> str:
    return b.hex() if b else "-"


def edge_lines():
    """(lines for the host check program, the oracle's answers): per boundary length a sign, a
    verify of that signature and, from one byte on, a verify of the message with its last byte
    flipped (rejected)."""
    lines, want = [], []
    for sk, msg in edge_messages():
        pk, sig = eo.secret_to_public(sk), eo.sign(sk, msg)
        lines += [f"sign {sk.hex()} {_hx(msg)}", f"verify {pk.hex()} {_hx(msg)} {sig.hex()}"]
        want += [sig.hex(), "1" if eo.verify(pk, msg, sig) else "0"]
        if msg:
            bad = flip_last(msg)
            lines.append(f"verify {pk.hex()} {_hx(bad)} {sig.hex()}")
            want.append("1" if eo.verify(pk, bad, sig) else "0")
    assert want.count("0") == len(SHA512_EDGE_LENS) - 1 and want.count("1") == len(SHA512_EDGE_LENS)
    return lines, want


# ---- field operations on explicit limb vectors -------------------------------------------------
# Ten signed limbs, limb i at bit FE_OFF[i] (radix 2^25.5, ed25519_core.hpp).  A reduced limb is
# |x| <= 2^25 (even i) / 2^24 (odd i); "k x" below means k times that.
FE_OFF = [0, 26, 51, 77, 102, 128, 153, 179, 204, 230]
FE_RED = [1 << 25, 1 << 24] * 5
# The header's bound rule: fe_mul(f, g) takes g at most 3x (19 * g fits int32) and f * g at most
# ~60x.  With g at 3x the largest f is 20x.  The largest column sum is h[0]: with every limb at
# its bound, f0 g0 + 19 (2 f1 g9 + f2 g8 + ... + 2 f9 g1) = 2^50 (1 + 19 * (5 / 2 + 4)) = 124.5 * 2^50,
# times 60 = 7470 * 2^50 < 2^63 = 8192 * 2^50: no int64 overflow, and 2 * f = 40 * 2^24 fits int32.
FE_G_MAX, FE_F_MAX = 3, 20
FE_SIGNS = [[1] * 10, [-1] * 10, [1, -1] * 5, [-1, 1] * 5]
# A carried result: limbs within the reduced bound, plus the last carry into limbs 1 and 5 of a
# column sum below 2^63 (< 2^13).
FE_OUT_SLACK = 1 << 13


def fe_limbs(x: int):
    """x in [0, 4 * 2^255) as non-negative limbs: 26 / 25 bits each, the top limb takes the rest."""
    out = []
    for i in range(10):
        nxt = FE_OFF[i + 1] if i < 9 else None
        out.append((x >> FE_OFF[i]) & ((1 << (nxt - FE_OFF[i])) - 1) if nxt else x >> FE_OFF[i])
    return out


def fe_value(limbs) -> int:
    return sum(int(v) << FE_OFF[i] for i, v in enumerate(limbs))


def _bound(k, signs):
    return [s * k * r for s, r in zip(signs, FE_RED)]


def fe_cases(seed: int = 5):
    """[(line, want)] for the host check program's field ops.  want: an int for the ops that
    print limbs (their value mod p must equal it, each limb carried), or the hex of the canonical
    32 bytes for fe_to_words.  Python integers mod p are the reference."""
    rng = random.Random(seed)
    vals = [0, 1, 2, 18, 19, P - 1, P, P + 1, 2**255 - 20, 2**255 - 1] + [rng.getrandbits(255) for _ in range(50)]
    cases = []

    def add(op, *operands):
        v = [fe_value(o) for o in operands]
        want = {"fe_mul": lambda: v[0] * v[1], "fe_sq": lambda: v[0] ** 2, "fe_sq2": lambda: 2 * v[0] ** 2,
                "fe_invert": lambda: pow(v[0], P - 2, P), "fe_to_words": lambda: v[0]}[op]() % P
        line = op + " " + " ".join(str(x) for o in operands for x in o)
        cases.append((line, le(want).hex() if op == "fe_to_words" else want))

    for i, a in enumerate(vals):
        la = fe_limbs(a)
        add("fe_mul", la, fe_limbs(vals[(i + 1) % len(vals)]))
        add("fe_mul", la, la)
        for op in ("fe_sq", "fe_sq2", "fe_invert", "fe_to_words"):
            add(op, la)
    for sg in FE_SIGNS:                      # at the bound rule: g at 3x, f at 20x, every sign pattern
        for sf in FE_SIGNS:
            add("fe_mul", _bound(FE_F_MAX, sf), _bound(FE_G_MAX, sg))
            add("fe_mul", _bound(FE_G_MAX, sf), _bound(FE_G_MAX, sg))
        for op in ("fe_sq", "fe_sq2"):
            add(op, _bound(FE_G_MAX, sg))
        for k in (1, 2, 3):                  # fe_to_words reads differences of carried elements
            add("fe_to_words", _bound(k, sg))
    for _ in range(12):                      # limbs of both signs, up to 3x
        add("fe_to_words", [rng.randint(-3 * r, 3 * r) for r in FE_RED])
    for k in range(3):                       # p - 1 + k p: the largest canonical value and its aliases
        add("fe_to_words", fe_limbs(P - 1 + k * P))
        add("fe_to_words", [-x for x in fe_limbs(1 + k * P)])   # -(1 + k p) == p - 1
    return cases


def check_fe_output(cases, out):
    """out: the program's tokens, one per case."""
    assert len(out) == len(cases)
    for (line, want), got in zip(cases, out):
        if isinstance(want, str):
            assert got == want, line
        else:
            limbs = [int(x) for x in got.split(",")]
            assert len(limbs) == 10 and fe_value(limbs) % P == want, line
            assert all(abs(x) <= r + FE_OUT_SLACK for x, r in zip(limbs, FE_RED)), (line, limbs)
