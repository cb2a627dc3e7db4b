#!/usr/bin/env python3
"""bench_merkle.py -- slice Merkle trees on the device.

Workload: S-byte shreds, 64 per slice (TOTAL_SHREDS, shredder.rs:47; Regular shredder:
32 data + 32 coding shreds of <= 1 KiB), laid out like the RS codeword buffer (slice s =
64 contiguous shreds).  One step =
  build:  MerkleTree::new + get_root + create_proof for every shred of every slice
          (crypto/merkle.rs:281-370; shredder.rs:538-606 on the producer side)
  verify: check_proof for every shred against its slice root (merkle.rs:374-387; the
          receiver's per-shred check, shredder.rs:130-140)
Inputs are device-resident random shreds (splitmix64).  Prints one JSON line: slices/s of
build+verify, per-kernel HIP-event times, the HBM-read roofline of each kernel (each kernel
reads the shreds once; the work is SHA-256 on the VALU), and a CPU baseline (the oracle:
Python hashlib / OpenSSL SHA-256, one thread, bounded sample).

--block-tree times the block trees instead (ag_block_tree_batch: the double-Merkle tree over a
block's slice roots), one JSON line per shape; see block_tree_leg.

--mixed-sizes times the slice trees of a block's mix of shred sizes (bench_coder.mixed_sizes)
through ag_merkle_build_batch_var against the uniform call; see mixed_leg.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
HBM_PEAK_GBPS = 8000.0


def block_tree_leg(args):
    """--block-tree: ag_block_tree_batch (the double-Merkle tree over a block's slice roots) at
    1 x 1024 and 64 x 1024 slices, hashes only and hashes + every slice's proof.  Per call, HIP
    events around it on the context stream (the upload of the counts, the tree kernel, the proof
    kernel) and the host's wall time from the call to the end of a synchronise; median and
    minimum over --steps calls.  One JSON line per shape; the same trees through
    oracle/merkle_oracle.py on one host thread ride along as context."""
    import statistics

    import torch

    from alpenglow_amd import rs

    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import merkle_oracle as mo

    dev = torch.device("cuda:0")
    ctx = rs.Context(0)
    stream = torch.cuda.Stream(dev)
    torch.cuda.set_stream(stream)
    ctx.set_stream(stream.cuda_stream)
    n, steps = 1024, max(args.steps, 20)
    h = rs.merkle_height(n)
    pstride = 32 * h * n
    for nblocks in (1, 64):
        counts = [n] * nblocks
        roots = torch.empty((nblocks * n, 32), dtype=torch.uint8, device=dev)
        rs.fill_splitmix(ctx, roots, nblocks * n, 32, 32, 0xB10C7EE0)
        hashes = torch.empty((nblocks, 32), dtype=torch.uint8, device=dev)
        proofs = torch.empty((nblocks, pstride), dtype=torch.uint8, device=dev)
        host = roots.cpu().numpy()
        t0 = time.perf_counter()
        tree = mo.MerkleTree([host[j].tobytes() for j in range(n)])
        cpu_tree_us = (time.perf_counter() - t0) * 1e6
        t0 = time.perf_counter()
        want_proofs = b"".join(b"".join(tree.create_proof(j)) for j in range(n))
        cpu_proofs_us = (time.perf_counter() - t0) * 1e6
        modes = {}
        for mode, pr in (("hashes", None), ("hashes_and_proofs", proofs)):
            def call():
                rs.block_tree_batch(ctx, nblocks, counts, roots, hashes, None, 0, pr, pstride if pr is not None else 0)
            for _ in range(max(args.warmup, 3)):
                call()
            torch.cuda.synchronize()
            dev_us, wall_us = [], []
            for _ in range(steps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0 = time.perf_counter()
                e0.record(stream)
                call()
                e1.record(stream)
                torch.cuda.synchronize()
                wall_us.append((time.perf_counter() - t0) * 1e6)
                dev_us.append(e0.elapsed_time(e1) * 1e3)
            modes[mode] = {"device_us_median": statistics.median(dev_us), "device_us_min": min(dev_us),
                           "wall_us_median": statistics.median(wall_us), "wall_us_min": min(wall_us)}
        ok = hashes[0].cpu().numpy().tobytes() == tree.root() and \
            proofs[0].cpu().numpy().tobytes() == want_proofs
        us = modes["hashes"]["device_us_median"]
        print(json.dumps({
            "metric": "us per ag_block_tree_batch call (double-Merkle tree over slice roots, SHA-256)",
            "value": us, "unit": "us", "higher_is_better": False, "n_gpus": 1, "steps": steps,
            "config": {"blocks": nblocks, "slices_per_block": n},
            "blocks_per_s": nblocks / (us * 1e-6),
            "sha256_blocks": nblocks * (2 * n + 3 * (rs.merkle_node_count(n) - n)),
            "modes": modes,
            "verify": {"block_0_hash_and_proofs_match_oracle": ok},
            "cpu_context": {"tree_us_per_block": cpu_tree_us, "proofs_us_per_block": cpu_proofs_us, "cores": 1,
                            "kind": "oracle/merkle_oracle.py (hashlib SHA-256), one block, one thread"},
        }), flush=True)
    ctx.close()


def mixed_leg(args):
    """--mixed-sizes: roots + proofs of --slices slice trees, one 64 KiB codeword region per slice
    (the var coder's packed layout), legs interleaved step by step:
      uniform_1024   ag_merkle_build_batch at S = 1024: every row 16-byte aligned, the ceiling
      uniform_1010   the same at S = 1010: rows 2-byte aligned, the per-byte loader
      var_1024       ag_merkle_build_batch_var, every slice 1024: the var loader on aligned rows
      var_1010       ag_merkle_build_batch_var, every slice 1010
      var_mix        ag_merkle_build_batch_var on bench_coder.mixed_sizes
      presorted_mix  the mix sorted by size, one uniform call per distinct size (the caller's
                     gather and scatter are not timed)
      runs_mix       the mix in block order, one uniform call per run of equal sizes -- what a
                     caller can do without the var call (host-bound: timed over 2 steps)
    Per leg the median over --steps of the host's wall time from the call to the end of a
    synchronise, and of the HIP events around it.  One JSON line."""
    import statistics

    import numpy as np
    import torch

    import bench_coder
    from alpenglow_amd import rs

    dev = torch.device("cuda:0")
    ctx = rs.Context(0)
    stream = torch.cuda.Stream(dev)
    torch.cuda.set_stream(stream)
    ctx.set_stream(stream.cuda_stream)
    n, L, stride = args.slices, 64, 64 * 1024
    pstride = 32 * rs.merkle_height(L) * L
    buf = torch.empty((n, stride), dtype=torch.uint8, device=dev)
    rs.fill_splitmix(ctx, buf, n, stride, stride, 0x3E2C1E00)
    roots = torch.empty((n, 32), dtype=torch.uint8, device=dev)
    proofs = torch.empty((n, pstride), dtype=torch.uint8, device=dev)
    mix = bench_coder.mixed_sizes(n)
    order = np.argsort(mix, kind="stable")
    srt = mix[order]
    starts = np.flatnonzero(np.r_[True, srt[1:] != srt[:-1]]).tolist() + [n]
    cuts = np.flatnonzero(np.r_[True, mix[1:] != mix[:-1]]).tolist() + [n]
    all1010, all1024 = np.full(n, 1010, np.uint32), np.full(n, 1024, np.uint32)

    def uniform(S, b=0, e=n):
        rs.merkle_build_batch(ctx, L, S, e - b, buf[b:e], S, stride, roots[b:e], None, 0, proofs[b:e], pstride)

    def var(sizes):
        rs.merkle_build_batch_var(ctx, n, sizes, buf, stride, roots, None, 0, proofs, pstride)

    def per_run(sizes, edges, limit=n):
        for b, e in zip(edges[:-1], edges[1:]):
            if b >= limit:
                break
            uniform(int(sizes[b]), b, e)

    legs = {"uniform_1024": lambda: uniform(1024), "uniform_1010": lambda: uniform(1010),
            "var_1024": lambda: var(all1024), "var_1010": lambda: var(all1010), "var_mix": lambda: var(mix),
            "presorted_mix": lambda: per_run(srt, starts)}

    def timed(f):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        e0.record(stream)
        f()
        e1.record(stream)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, e0.elapsed_time(e1)

    # the outputs agree where the legs hash the same leaves: var_mix against runs_mix (block order)
    var(mix)
    want = roots.clone(), proofs.clone()
    per_run(mix, cuts)
    torch.cuda.synchronize()
    same = torch.equal(roots, want[0]) and torch.equal(proofs, want[1])
    del want
    for _ in range(max(args.warmup, 2)):
        for f in legs.values():
            f()
    torch.cuda.synchronize()
    times = {k: [] for k in legs}
    for _ in range(args.steps):
        for k, f in legs.items():
            times[k].append(timed(f))
    times["runs_mix"] = [timed(lambda: per_run(mix, cuts)) for _ in range(2)]
    out = {}
    for k, v in times.items():
        wall, devms = statistics.median(t[0] for t in v), statistics.median(t[1] for t in v)
        out[k] = {"wall_ms": wall, "device_ms": devms, "slices_per_s": n / (wall * 1e-3), "steps": len(v)}
    print(json.dumps({
        "metric": "slices/s slice Merkle trees (roots + proofs) over a block's mix of shred sizes, one var call",
        "value": out["var_mix"]["slices_per_s"], "unit": "slices/s", "higher_is_better": True, "n_gpus": 1,
        "steps": args.steps, "warmup": max(args.warmup, 2),
        "config": {"slices": n, "slice_stride": stride, "distinct_sizes": len(starts) - 1, "runs": len(cuts) - 1,
                   "mean_shred_bytes": float(mix.mean())},
        "legs": out,
        "ratios": {"var_1010_over_uniform_1010": out["uniform_1010"]["wall_ms"] / out["var_1010"]["wall_ms"],
                   "var_1010_over_uniform_1024": out["uniform_1024"]["wall_ms"] / out["var_1010"]["wall_ms"],
                   "var_1024_over_uniform_1024": out["uniform_1024"]["wall_ms"] / out["var_1024"]["wall_ms"],
                   "var_mix_over_runs_mix": out["runs_mix"]["wall_ms"] / out["var_mix"]["wall_ms"],
                   "var_mix_over_presorted_mix": out["presorted_mix"]["wall_ms"] / out["var_mix"]["wall_ms"]},
        "verify": {"var_mix_equals_runs_mix": same},
    }), flush=True)
    ctx.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--slices", type=int, default=65536)
    ap.add_argument("--shred-bytes", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--cpu-seconds", type=float, default=10.0)
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--block-tree", action="store_true",
                    help="time ag_block_tree_batch (block hashes over slice roots) instead of the slice trees")
    ap.add_argument("--mixed-sizes", action="store_true",
                    help="time ag_merkle_build_batch_var on a block's mix of shred sizes against the uniform call")
    args = ap.parse_args()
    if args.block_tree:
        return block_tree_leg(args)
    if args.mixed_sizes:
        return mixed_leg(args)
    import torch

    from alpenglow_amd import rs

    dev = torch.device("cuda:0")
    ctx = rs.Context(0)
    stream = torch.cuda.Stream(dev)
    torch.cuda.set_stream(stream)
    ctx.set_stream(stream.cuda_stream)
    n, S, L = args.slices, args.shred_bytes, 64
    h = rs.merkle_height(L)
    shreds = torch.empty((n, L * S), dtype=torch.uint8, device=dev)
    rs.fill_splitmix(ctx, shreds, n, L * S, L * S, 0x3E2C1E00)
    roots = torch.empty((n, 32), dtype=torch.uint8, device=dev)
    pstride = 32 * h * L
    proofs = torch.empty((n, pstride), dtype=torch.uint8, device=dev)
    index = torch.arange(n * L, dtype=torch.int64, device=dev).remainder(L).to(torch.int32)
    slice_of = torch.arange(n * L, device=dev) // L
    root_rep = None
    ok = torch.empty(n * L, dtype=torch.uint8, device=dev)

    def build():
        rs.merkle_build_batch(ctx, L, S, n, shreds, S, L * S, roots, None, 0, proofs, pstride)

    def verify():
        rs.merkle_verify_batch(ctx, n * L, S, shreds, S, index, root_rep, 32, proofs, 32 * h, h, ok)

    build()
    root_rep = roots[slice_of].contiguous()  # per shred: its slice's root (as received)
    for _ in range(args.warmup):
        build()
        verify()
    ev = [[torch.cuda.Event(enable_timing=True) for _ in range(3)] for _ in range(args.steps)]
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for s in range(args.steps):
        ev[s][0].record(stream)
        build()
        ev[s][1].record(stream)
        verify()
        ev[s][2].record(stream)
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    b_ms = sum(e[0].elapsed_time(e[1]) for e in ev) / args.steps
    v_ms = sum(e[1].elapsed_time(e[2]) for e in ev) / args.steps
    all_ok = bool(ok.all().item())

    # spot check against the oracle (test infrastructure: the checker, not the product)
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import merkle_oracle as mo
    host = shreds[:2].cpu().numpy().reshape(2, L, S)
    spot = all(roots[i].cpu().numpy().tobytes() == mo.MerkleTree([host[i, j].tobytes() for j in range(L)]).root()
               for i in range(2))

    read = n * L * S
    kern = {"build": {"ms": b_ms, "bytes_read": read, "achieved_GBps": read / (b_ms * 1e-3) / 1e9,
                      "sha256_blocks": n * (L * ((32 + S + 9 + 63) // 64) + 3 * (L - 1))},
            "verify": {"ms": v_ms, "bytes_read": read + n * L * 32 * (h + 1),
                       "achieved_GBps": (read + n * L * 32 * (h + 1)) / (v_ms * 1e-3) / 1e9,
                       "sha256_blocks": n * L * (((32 + S + 9 + 63) // 64) + 3 * h)}}
    for k in kern.values():
        k["sha256_blocks_per_s"] = k["sha256_blocks"] / (k["ms"] * 1e-3)
    line = {
        "metric": "slices/s slice Merkle trees (SHA-256): build roots+proofs and verify every shred",
        "value": n * args.steps / wall,
        "unit": "slices/s",
        "n_gpus": 1,
        "steps": args.steps,
        "warmup": args.warmup,
        "ms_per_step": wall * 1e3 / args.steps,
        "higher_is_better": True,
        "scaling": "weak",
        "vs_baseline": None,
        "dtype": "u32 (SHA-256)",
        "data": "synthetic (splitmix64 shreds, device-generated)",
        "config": {"workload": f"{n} slices x {L} shreds x {S} B", "slices": n, "shreds_per_slice": L,
                   "shred_bytes": S},
        "roofline": {"bound": "hbm", "kernel": "build", "achieved": kern["build"]["achieved_GBps"],
                     "peak": HBM_PEAK_GBPS, "unit": "GB/s",
                     "frac": kern["build"]["achieved_GBps"] / HBM_PEAK_GBPS, "traffic": None,
                     "note": "SHA-256 is VALU-bound; the HBM fraction shows the headroom, not the limit"},
        "kernels": kern,
        "verify": {"all_proofs_accepted": all_ok, "roots_match_oracle": spot},
    }
    if not args.no_cpu_baseline:
        t0, done = time.perf_counter(), 0
        hostall = shreds[:4096].cpu().numpy().reshape(-1, L, S)
        while time.perf_counter() - t0 < args.cpu_seconds and done < len(hostall):
            t = mo.MerkleTree([hostall[done, j].tobytes() for j in range(L)])
            for j in range(L):
                t.create_proof(j)
            done += 1
        bt = time.perf_counter() - t0
        line["cpu_baseline"] = {"value": done / bt, "unit": "slices/s (build + proofs)", "cores": 1,
                                "kind": "port",
                                "sample": f"{done} slices, oracle/merkle_oracle.py (hashlib SHA-256), one thread"}
    print(json.dumps(line), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
