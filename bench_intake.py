#!/usr/bin/env python3
"""bench_intake.py -- shred intake on the device: ag_shredder_intake_batch (received datagrams in
arrival order -> the slice slots of ag_shredder_deshred_batch_var, with the reference's
per-datagram verdicts; validated_shred.rs:52-79, slot_block_data.rs:202-248).

Workload: one block of --slices slices (default 1024, one slot, the last slice is_last) at the
leader's size mix (bench_coder.mixed_sizes, the var case of bench_shredder.py), shredded on the
device.  The follower receives a random 40 of each slice's 64 datagrams plus 5 % duplicates, the
whole stream shuffled, in ONE intake call into an empty store; ag_shredder_deshred_batch_var
then runs on that store.  Wall clock around each (synchronous) call, the store reset between
steps (not timed); the median over --steps.  Prints one JSON line: datagrams/s and GB/s (datagram
bytes in) of the intake call and, for context, the time of the deshred behind it.  The verify block
counts the verdicts (40 per slice stored, every duplicate a duplicate) and the deshred's statuses.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
PKT = 1344  # datagram slot (1325 bytes for a 1 KiB shred, rounded to 64)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--slices", type=int, default=1024, help="slices of the block (<= 1024)")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--arrived", type=int, default=40, help="datagrams received per slice (32..64)")
    ap.add_argument("--dup-frac", type=float, default=0.05)
    args = ap.parse_args()

    import numpy as np
    import torch

    import bench_coder
    from alpenglow_amd import rs

    dev = torch.device("cuda:0")
    torch.zeros(1, device=dev)
    ctx = rs.Context(0)
    stream = torch.cuda.Stream(dev)
    torch.cuda.set_stream(stream)
    ctx.set_stream(stream.cuda_stream)
    n, stride = args.slices, 64 * 1024
    assert 1 <= n <= 1024 and 32 <= args.arrived <= 64
    mix = bench_coder.mixed_sizes(n)
    dmix = (32 * mix.astype(np.int64) - 1 - 9).astype(np.uint32)  # data bytes: framed payload 32 S - 1
    data = torch.empty((n, 32 * 1024), dtype=torch.uint8, device=dev)
    rs.fill_splitmix(ctx, data, n, 32 * 1024, 32 * 1024, 0x5EED0000)
    slot_id = 0x1A7A4E
    slots = torch.full((n,), slot_id, dtype=torch.int64, device=dev)
    sidx = torch.arange(n, dtype=torch.int64, device=dev)
    last = (torch.arange(n) == n - 1).to(torch.uint8).to(dev)
    seed = torch.arange(32, dtype=torch.uint8).to(dev)
    pk = torch.empty(32, dtype=torch.uint8, device=dev)
    rs.ed25519_public_key_batch(ctx, 1, seed, pk)
    cw = torch.zeros(n * stride, dtype=torch.uint8, device=dev)
    pkts = torch.zeros((n * 64, PKT), dtype=torch.uint8, device=dev)
    lens = torch.zeros(n * 64, dtype=torch.int32, device=dev)
    rs.shredder_shred_batch_var(ctx, n, [None] * n, data, 32 * 1024, dmix, slots, sidx, last, seed, pk, cw, stride, pkts,
                                PKT, lens)
    # the receive queue: per slice a random `arrived` of 64, 5 % of them twice, shuffled
    rng = np.random.default_rng(0x1A7A)
    got = np.concatenate([64 * s + rng.permutation(64)[:args.arrived] for s in range(n)])
    dups = rng.choice(got, int(round(args.dup_frac * got.size)), replace=False)
    order = rng.permutation(np.concatenate([got, dups]))
    N = order.size
    sel = torch.from_numpy(order).to(dev)
    rx, rx_lens = pkts[sel].contiguous(), lens[sel].contiguous()
    rx_bytes = int(rx_lens.sum().item())
    del pkts, data

    store = torch.zeros((n * 64, PKT), dtype=torch.uint8, device=dev)
    store_lens = torch.zeros(n * 64, dtype=torch.int32, device=dev)
    commitments = torch.zeros(49 * n, dtype=torch.uint8, device=dev)
    shred_bytes = torch.zeros(n, dtype=torch.int32, device=dev)
    last_slice = torch.full((1,), -1, dtype=torch.int32, device=dev)
    verdict = torch.zeros(N, dtype=torch.uint8, device=dev)

    def step():
        store_lens.zero_()
        shred_bytes.zero_()
        last_slice.fill_(-1)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        sizes, counts = rs.shredder_intake_batch(ctx, [slot_id], n, N, rx, PKT, rx_lens, pk, store, PKT, store_lens,
                                                 commitments, shred_bytes, last_slice, verdict)
        t1 = time.perf_counter()
        res = rs.shredder_deshred_batch_var(ctx, n, sizes, store, PKT, store_lens, pk, cw, stride)
        t2 = time.perf_counter()
        return (t1 - t0) * 1e3, (t2 - t1) * 1e3, sizes, counts, res

    for _ in range(max(args.warmup, 1)):
        step()
    runs = [step() for _ in range(args.steps)]
    t_in = statistics.median(r[0] for r in runs)
    t_de = statistics.median(r[1] for r in runs)
    _, _, sizes, counts, res = runs[-1]
    v = np.bincount(verdict.cpu().numpy(), minlength=9).tolist()
    print(json.dumps({
        "metric": "datagrams/s shred intake, one block of mixed shred sizes, one call",
        "value": N / (t_in * 1e-3), "unit": "datagrams/s", "higher_is_better": True, "n_gpus": 1,
        "steps": args.steps, "warmup": max(args.warmup, 1),
        "config": {"slices": n, "arrived": args.arrived, "dup_frac": args.dup_frac, "datagrams": int(N),
                   "datagram_bytes": rx_bytes, "packet_stride": PKT, "mean_shred_bytes": float(mix.mean())},
        "intake": {"wall_ms": t_in, "datagrams_per_s": N / (t_in * 1e-3), "gb_per_s": rx_bytes / (t_in * 1e-3) / 1e9},
        "deshred_var_after": {"wall_ms": t_de, "slices_per_s": n / (t_de * 1e-3)},
        "verify": {"stored": v[rs.INTAKE_STORED] == n * args.arrived, "duplicates": v[rs.INTAKE_DUPLICATE] == dups.size,
                   "sizes": bool(np.array_equal(sizes, mix)), "counts": bool((counts == args.arrived).all()),
                   "last_slice": int(last_slice.item()) == n - 1,
                   "deshred_ok": bool((res.status == 0).all()), "verdicts": dict(zip(rs.INTAKE_VERDICTS, v))},
    }), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
