"""Generates tests/golden/rs_exact_noncodeword.json from the numpy oracle (oracle/rs_oracle.py).

EXACT-mode goldens on NON-CODEWORDS: every original and every recovery shard is independent
splitmix64 output (nothing is encoded), more than k shards are present, and the stored hash is
what the crate's decoder -- every present shard used -- restores, as the oracle restates it.
On such input the every-shard result and an any-k-survivors result differ in every 16-bit
symbol, so these entries pin the one property that separates AG_RS_DECODE_EXACT from
AG_RS_DECODE_ANY_K.  Like rs_golden.json they are restatement goldens (parity unpinned against
the crate's bytes); they are the entries to add to oracle/crate_check when someone can run the
crate.

Shard bytes: raw = splitmix64_bytes(seed, (k + m) * S); original i = raw[i*S:(i+1)*S],
recovery j = raw[(k+j)*S:(k+j+1)*S].

Usage: python tests/golden/make_exact_golden.py
"""

from __future__ import annotations

import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "..", "oracle"))
import rs_oracle as o  # noqa: E402

CASES = [
    # (k, m, S, erased original indices, present recovery indices): |present| > |erased|
    (32, 32, 256, list(range(8)), list(range(0, 20, 2))),                  # W = 64, surplus 2
    (32, 32, 1000, [0, 5, 17, 31], [0, 3, 9, 20, 31]),                     # whole chunks + 40-byte tail
    (32, 32, 62, list(range(16, 32)), list(range(32))),                    # tail only; full recovery set
    (16, 4, 192, [0, 15], [0, 1, 3]),                                      # W = 32
    (20, 30, 64, list(range(20)), list(range(3, 27))),                     # every original lost, surplus 4
    (48, 16, 128, [0, 7, 47], [1, 2, 8, 15]),                              # chunk 16
    (60, 4, 128, [59], [0, 3]),                                            # chunk 4
    (32, 64, 128, list(range(0, 32, 3)), [0, 5, 31, 32, 33, 40, 41, 50, 62, 63, 7, 9, 11]),  # LowRate
    (32, 33, 66, [31], [0, 32]),                                           # PETS geometry, 2-byte tail
    (64, 64, 64, list(range(1, 64, 2)), list(range(0, 40))),               # W = 128
    (100, 28, 64, [0, 50, 99], [0, 1, 13, 27]),                            # k > 64
    (5, 2, 64, [4], [0, 1]),                                               # window narrower than 32
]


def shards(seed: int, k: int, m: int, S: int):
    raw = o.splitmix64_bytes(seed, (k + m) * S)
    cut = [raw[i * S:(i + 1) * S] for i in range(k + m)]
    return cut[:k], cut[k:]


def main():
    doc = {"note": "EXACT decodes of non-codewords (independent random shards, surplus present) from "
                   "oracle/rs_oracle.py; restatement goldens, parity unpinned vs the crate",
           "decode_exact": []}
    seed = 0xE8AC7
    for k, m, S, eo, pr in CASES:
        seed += 1
        assert len(pr) > len(eo) and len(set(pr)) == len(pr)
        orig, rec = shards(seed, k, m, S)
        res = o.decode(k, m, {i: orig[i] for i in range(k) if i not in eo}, {j: rec[j] for j in pr})
        assert sorted(res) == sorted(eo)
        doc["decode_exact"].append({"k": k, "m": m, "S": S, "seed": seed, "erased_original": sorted(eo),
                                    "present_recovery": sorted(pr),
                                    "restored_sha256": hashlib.sha256(b"".join(res[i] for i in sorted(res))).hexdigest()})
    path = os.path.join(HERE, "rs_exact_noncodeword.json")
    with open(path, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(path)


if __name__ == "__main__":
    main()
