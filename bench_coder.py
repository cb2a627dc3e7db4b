#!/usr/bin/env python3
"""bench_coder.py -- the ReedSolomonCoder contract over batches of slices (SURVEY.md §8(f)
row 1), shaped like the reference's own benchmark (benches/shredder.rs:40-60): a maximum
slice (32 767-byte payload -> 32 data + 32 coding shreds of 1 KiB) is shredded, its 32
data shreds are dropped, and it is deshredded (restore, padding strip, re-encode of all
coding shreds; reed_solomon.rs:88-128, 140-208).

One step over n slices = ag_rs_coder_shred_batch (pad + encode, in place) then
ag_rs_coder_deshred_batch with every data shred absent (ANY_K by default; --exact for the
crate decoder).  Device-resident codewords (64 KiB per slice).  Prints one JSON line:
slices/s, payload GiB/s, per-call ms, and a CPU baseline (the C oracle: pad + encode,
decode + re-encode, 16 threads, bounded sample).

--mixed-sizes: a block's real mix of shred sizes (80 % full slices, S uniform over 1008, 1010,
.. 1024; 20 % timed-out slices, S uniform over the even sizes 2 .. 1006; seeded) through
ag_rs_coder_shred_batch_var / ag_rs_coder_deshred_batch_var, the deshred from a random 32 of
the 64 shreds per slice.  With --presorted-uniform the same population goes the old way: already
sorted and compacted by size, one uniform call per distinct size (the caller's gather and
scatter are not timed).  One JSON line: slices/s of the shred and of the deshred.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
GIB = float(1 << 30)


def mixed_sizes(n: int, seed: int = 0xB10C):
    """Seeded shred sizes of a block's slices: 80 % full (1008 .. 1024), 20 % timed out (2 .. 1006)."""
    import numpy as np

    rng = np.random.default_rng(seed)
    full = 1008 + 2 * rng.integers(0, 9, n)
    short = 2 + 2 * rng.integers(0, 503, n)
    return np.where(rng.random(n) < 0.8, full, short).astype(np.uint32)


def run_mixed(args):
    import numpy as np
    import torch

    from alpenglow_amd import rs

    dev = torch.device("cuda:0")
    ctx = rs.Context(0)
    stream = torch.cuda.Stream(dev)
    torch.cuda.set_stream(stream)
    ctx.set_stream(stream.cuda_stream)
    n, m = args.slices, 32
    sizes = mixed_sizes(n)
    lens = (32 * sizes - 1).astype(np.uint32)  # the longest payload of each size
    rng = np.random.default_rng(0xA221)
    arrived = np.argsort(rng.random((n, 64)), axis=1)[:, :32]  # first 32 arrivals per slice
    present = np.zeros((n, 64), np.uint8)
    np.put_along_axis(present, arrived, 1, axis=1)
    dpres, cpres = np.ascontiguousarray(present[:, :32]), np.ascontiguousarray(present[:, 32:])
    mode = rs.DECODE_EXACT if args.exact else rs.DECODE_ANY_K
    distinct = np.unique(sizes)
    groups = [np.flatnonzero(sizes == S) for S in distinct]
    if args.presorted_uniform:
        bufs = []
        for S, idx in zip(distinct, groups):
            S = int(S)
            b = torch.empty((len(idx), 64 * S), dtype=torch.uint8, device=dev)
            rs.fill_splitmix(ctx, b, len(idx), 32 * S, 64 * S, 0xC0DE0000 + S)
            bufs.append((S, len(idx), b, lens[idx], np.ascontiguousarray(dpres[idx]), np.ascontiguousarray(cpres[idx])))

        def shred():
            for S, cnt, b, ln, _, _ in bufs:
                rs.coder_shred_batch(ctx, m, cnt, S, None, 0, ln, b, 64 * S)

        def deshred():
            return np.concatenate([rs.coder_deshred_batch(ctx, m, cnt, S, b, 64 * S, dp, cp, mode=mode, as_array=True)
                                   for S, cnt, b, _, dp, cp in bufs])

        want_lens = np.concatenate([ln for _, _, _, ln, _, _ in bufs])
    else:
        stride = 64 * 1024
        cw = torch.empty((n, stride), dtype=torch.uint8, device=dev)
        rs.fill_splitmix(ctx, cw, n, 32 * 1024, stride, 0xC0DE0000)  # payload bytes in the data regions

        def shred():
            rs.coder_shred_batch_var(ctx, m, n, None, 0, lens, cw, stride)

        def deshred():
            return rs.coder_deshred_batch_var(ctx, m, n, sizes, cw, stride, dpres, cpres, mode=mode, as_array=True)

        want_lens = lens
    shred()
    for _ in range(args.warmup):
        shred()
        deshred()
    torch.cuda.synchronize()
    t_sh = t_de = 0.0
    for _ in range(args.steps):
        a = time.perf_counter()
        shred()
        torch.cuda.synchronize()
        b = time.perf_counter()
        res = deshred()  # synchronous
        c = time.perf_counter()
        t_sh += b - a
        t_de += c - b
    ok = bool((res == want_lens).all())
    verify = {"all_slices_restored": ok}
    if not args.presorted_uniform:
        # zero every absent shred, deshred once more, compare with the shredded codewords; spot
        # check the smallest, a middle and the largest slice against the oracle's coder
        want = cw.clone()
        pres = torch.from_numpy(present).to(dev)
        for S, idx in zip(distinct, groups):
            S = int(S)
            rows = torch.from_numpy(idx).to(dev)
            kept = cw[rows, :64 * S].view(-1, 64, S) * pres[rows].unsqueeze(-1)
            cw[rows, :64 * S] = kept.view(-1, 64 * S)
        res2 = deshred()
        verify["all_slices_restored"] = ok and bool((res2 == lens).all()) and bool(torch.equal(cw, want))
        sys.path.insert(0, os.path.join(ROOT, "oracle"))
        import rs_oracle as o
        spot = True
        for i in (int(np.argmin(sizes)), n // 2, int(np.argmax(sizes))):
            S, host = int(sizes[i]), cw[i].cpu().numpy()
            raw = o.coder_shred(host[:int(lens[i])].tobytes(), m)
            spot &= host[:64 * S].tobytes() == b"".join(raw.data) + b"".join(raw.coding)
        verify["shreds_match_oracle"] = bool(spot)
        verify["encode_kernels"] = sorted(rs.last_encode_kernels(ctx))
        verify["window_kernels"] = sorted(rs.last_window_kernels(ctx))
    how = "one uniform call per distinct size, presorted" if args.presorted_uniform else "one mixed-size call"
    line = {
        "metric": f"slices/s ReedSolomonCoder shred and deshred (random 32 of 64 shreds per slice), mixed shred sizes, {how}",
        "value": n * args.steps / (t_sh + t_de),
        "unit": "slices/s",
        "n_gpus": 1,
        "steps": args.steps,
        "warmup": args.warmup,
        "higher_is_better": True,
        "shred_slices_per_s": n * args.steps / t_sh,
        "deshred_slices_per_s": n * args.steps / t_de,
        "calls_ms": {"shred": t_sh * 1e3 / args.steps, "deshred": t_de * 1e3 / args.steps},
        "config": {"workload": f"{n} slices, 32:32, 80 % S in 1008..1024, 20 % even S in 2..1006 "
                               f"({len(distinct)} distinct sizes, {int(sizes.astype(np.int64).sum()) * 64} codeword bytes)",
                   "calls_per_step": 2 * len(distinct) if args.presorted_uniform else 2,
                   "mode": "EXACT" if args.exact else "ANY_K"},
        "verify": verify,
    }
    print(json.dumps(line), flush=True)
    ctx.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--slices", type=int, default=65536)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--exact", action="store_true", help="crate decoder (EXACT) instead of ANY_K")
    ap.add_argument("--coding-only", action="store_true",
                    help="CodingOnlyShredder shape: 32:64, deshred from coding shreds 32..63 (the "
                         "reference bench drops the first 32 output shreds)")
    ap.add_argument("--random-patterns", action="store_true",
                    help="the follower's real deshred: per slice, the first 32 of its 64 shreds to arrive "
                         "in a seeded random order (slot_block_data.rs:331-370 deshreds at the 32nd), so data "
                         "and coding shreds are lost in arbitrary per-slice patterns")
    ap.add_argument("--payload-len", type=int, default=32767,
                    help="payload bytes per slice (default MAX_DATA_PER_SLICE = 32767: 1 KiB shreds); the "
                         "shred size is the padded length / 32 (reed_solomon.rs:94-95), e.g. 16383 -> 512 B")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--mixed-sizes", action="store_true",
                    help="a block's mix of shred sizes through the _var calls (see the module text)")
    ap.add_argument("--presorted-uniform", action="store_true",
                    help="with --mixed-sizes: the same slices sorted and compacted by size, one uniform call per size")
    args = ap.parse_args()
    if args.mixed_sizes:
        return run_mixed(args)
    import numpy as np
    import torch

    from alpenglow_amd import rs

    dev = torch.device("cuda:0")
    ctx = rs.Context(0)
    stream = torch.cuda.Stream(dev)
    torch.cuda.set_stream(stream)
    ctx.set_stream(stream.cuda_stream)
    L = args.payload_len  # MAX_DATA_PER_SLICE by default: pads to S = 1024 (reed_solomon.rs:94-95)
    if not 0 <= L <= 32767:
        raise SystemExit("--payload-len must be in [0, 32767]")
    n, S, m = args.slices, (L + 64 - L % 64) // 32, (64 if args.coding_only else 32)
    stride = (32 + m) * S
    cw = torch.empty((n, stride), dtype=torch.uint8, device=dev)
    rs.fill_splitmix(ctx, cw, n, 32 * S, stride, 0xC0DE0000)  # payload bytes in the data regions
    lens = np.full(n, L, np.uint32)
    dpres, cpres = np.zeros(32 * n, np.uint8), np.ones(m * n, np.uint8)
    if args.coding_only:  # output shreds are the 64 coding shreds; the first 32 are dropped
        cpres = np.tile(np.array([0] * 32 + [1] * 32, np.uint8), n)
    if args.random_patterns:
        rng = np.random.default_rng(0xA221)
        arrived = np.argsort(rng.random((n, 64)), axis=1)[:, :32]  # first 32 arrivals per slice
        present = np.zeros((n, 64), np.uint8)
        np.put_along_axis(present, arrived, 1, axis=1)
        if args.coding_only:  # the 64 output shreds are the coding shreds (shredder.rs:362-395)
            dpres = np.zeros(32 * n, np.uint8)
            cpres = np.ascontiguousarray(present).reshape(-1)
        else:
            dpres = np.ascontiguousarray(present[:, :32]).reshape(-1)
            cpres = np.ascontiguousarray(present[:, 32:]).reshape(-1)
    mode = rs.DECODE_EXACT if args.exact else rs.DECODE_ANY_K

    def shred():
        rs.coder_shred_batch(ctx, m, n, S, None, 0, lens, cw, stride)

    def deshred():
        return rs.coder_deshred_batch(ctx, m, n, S, cw, stride, dpres, cpres, mode=mode, as_array=True)

    shred()
    for _ in range(args.warmup):
        shred()
        deshred()
    torch.cuda.synchronize()
    t_sh = t_de = 0.0
    t0 = time.perf_counter()
    for _ in range(args.steps):
        a = time.perf_counter()
        shred()
        torch.cuda.synchronize()
        b = time.perf_counter()
        res = deshred()  # synchronous (payload lengths come back to the host)
        c = time.perf_counter()
        t_sh += b - a
        t_de += c - b
    wall = time.perf_counter() - t0
    ok = bool((res == L).all())
    if args.random_patterns:
        # zero every absent shred, deshred once more, compare with the original codewords
        want = cw.clone()
        pres = torch.from_numpy(np.concatenate([dpres.reshape(n, 32), cpres.reshape(n, m)], axis=1)).to(dev)
        view = cw.view(n, 32 + m, S)
        view.mul_(pres.unsqueeze(-1))
        res2 = deshred()
        ok = ok and bool((res2 == L).all()) and bool(torch.equal(cw, want))
        del want
    # spot check vs the oracle's ReedSolomonCoder (checker only)
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import rs_oracle as o
    host = cw[:2].cpu().numpy()
    spot = True
    for i in range(2):
        raw = o.coder_shred(host[i, :L].tobytes(), m)
        spot &= host[i, :32 * S].tobytes() == b"".join(raw.data)
        spot &= host[i, 32 * S:].tobytes() == b"".join(raw.coding)
    size = "max slices" if L == 32767 else f"{L}-byte slices"
    line = {
        "metric": (f"slices/s ReedSolomonCoder shred + deshred (random 32 of 64 output shreds per slice), {size}"
                   if args.random_patterns else
                   f"slices/s ReedSolomonCoder shred + deshred (first 32 output shreds lost), {size}"),
        "value": n * args.steps / wall,
        "unit": "slices/s",
        "n_gpus": 1,
        "steps": args.steps,
        "warmup": args.warmup,
        "ms_per_step": wall * 1e3 / args.steps,
        "higher_is_better": True,
        "scaling": "weak",
        "vs_baseline": None,
        "dtype": "u8 (GF(2^16) symbols)",
        "data": "synthetic (splitmix64 payloads, device-generated)",
        "config": {"workload": f"{n} slices x {L} B payload, 32:{m} shreds of {S} B, deshred from "
                               + ("a random 32 of the 64 coding shreds per slice (CodingOnlyShredder)"
                      if args.coding_only and args.random_patterns else
                      "coding shreds 32..63 (CodingOnlyShredder)" if args.coding_only else
                                  "a random 32 of the 64 shreds per slice (RegularShredder)" if args.random_patterns
                                  else "the 32 coding shreds (RegularShredder)"),
                   "mode": "EXACT" if args.exact else "ANY_K"},
        "payload_GiBps": n * L * args.steps / wall / GIB,
        "calls_ms": {"shred_batch": t_sh * 1e3 / args.steps, "deshred_batch": t_de * 1e3 / args.steps},
        "verify": {"all_slices_restored": ok, "shreds_match_oracle": bool(spot)},
    }
    if not args.no_cpu_baseline and not args.coding_only and not args.random_patterns:
        import ro_c
        threads = max(1, min(16, len(os.sched_getaffinity(0))))
        ns = min(n, 2048)
        blocks = host_blocks = cw[:ns, :32 * S].cpu().numpy().reshape(ns, 32, S)
        t = time.perf_counter()
        par = ro_c.encode_blocks(host_blocks, m, threads=threads)  # shred: encode
        t1 = time.perf_counter()
        codewords = np.concatenate([np.zeros_like(blocks).reshape(ns, -1), par.reshape(ns, -1)], axis=1)
        restored = ro_c.decode_blocks(codewords.reshape(ns, 64, S), 32, [0] * 32, [1] * 32, threads=threads)
        ro_c.encode_blocks(np.ascontiguousarray(restored.reshape(ns, 32, S)), m, threads=threads)  # re-encode
        t2 = time.perf_counter()
        line["cpu_baseline"] = {"value": ns / (t2 - t), "unit": "slices/s (shred + deshred)", "cores": threads,
                                "kind": "port",
                                "sample": f"{ns} slices, C oracle encode / decode / re-encode, {threads} threads",
                                "shred_slices_per_s": ns / (t1 - t), "deshred_slices_per_s": ns / (t2 - t1)}
    print(json.dumps(line), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
