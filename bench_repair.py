#!/usr/bin/env python3
"""bench_repair.py -- repair intake on the device: ag_repair_intake_batch (repair replies in
arrival order, each with its request's coordinates -> the block rows of
ag_shredder_deshred_batch_var, with the verdicts of repair.rs:410-445 and BlockData::add_shred).

Workload: one block of --slices slices (default 1024, the last slice is_last) at the leader's size
mix (bench_coder.mixed_sizes), shredded on the device.  The node receives a random 40 of each
slice's 64 shreds plus 5 % duplicates, the whole stream shuffled, in ONE repair intake call into
an empty store with every slice root proved.  In the same process, on the same datagrams,
ag_shredder_intake_batch (the dissemination intake: the existing path and the yardstick) is timed
the same way.  Wall clock around each (synchronous) call, the stores reset between steps (not
timed); the median over --steps.  Prints one JSON line: both times and their ratio, and a verify
block that counts the verdicts of both (40 per slice stored, every duplicate a duplicate).
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
    ap.add_argument("--arrived", type=int, default=40, help="shreds received per slice (32..64)")
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
    roots = torch.zeros(n * 32, dtype=torch.uint8, device=dev)   # the proved slice roots
    rs.shredder_shred_batch_var(ctx, n, [None] * n, data, 32 * 1024, dmix, slots, sidx, last, seed, pk, cw, stride, pkts,
                                PKT, lens, roots_out=roots)
    have_root = torch.ones(n, dtype=torch.uint8, device=dev)
    # the replies: per slice a random `arrived` of 64, 5 % of them twice, shuffled
    rng = np.random.default_rng(0x4E9A14)
    got = np.concatenate([64 * s + rng.permutation(64)[:args.arrived] for s in range(n)])
    dups = rng.choice(got, int(round(args.dup_frac * got.size)), replace=False)
    order = rng.permutation(np.concatenate([got, dups]))
    N = order.size
    sel = torch.from_numpy(order).to(dev)
    rx, rx_lens = pkts[sel].contiguous(), lens[sel].contiguous()
    rx_bytes = int(rx_lens.sum().item())
    req_block = torch.zeros(N, dtype=torch.int32, device=dev)
    req_slice = torch.from_numpy((order // 64).astype(np.int32)).to(dev)
    req_index = torch.from_numpy((order % 64).astype(np.int32)).to(dev)
    del pkts, data, cw

    store = torch.zeros((n * 64, PKT), dtype=torch.uint8, device=dev)
    store_lens = torch.zeros(n * 64, dtype=torch.int32, device=dev)
    commitments = torch.zeros(49 * n, dtype=torch.uint8, device=dev)
    signatures = torch.zeros(64 * n, dtype=torch.uint8, device=dev)
    shred_bytes = torch.zeros(n, dtype=torch.int32, device=dev)
    last_slice = torch.full((1,), -1, dtype=torch.int32, device=dev)
    verdict = torch.zeros(N, dtype=torch.uint8, device=dev)

    def reset():
        store_lens.zero_()
        shred_bytes.zero_()
        last_slice.fill_(-1)
        torch.cuda.synchronize()

    def step():
        reset()
        t0 = time.perf_counter()
        sizes, counts = rs.repair_intake_batch(ctx, [slot_id], pk, n, N, rx, PKT, rx_lens, req_block, req_slice,
                                               req_index, roots, have_root, store, PKT, store_lens, commitments,
                                               signatures, shred_bytes, last_slice, verdict)
        t1 = time.perf_counter()
        v_rep = np.bincount(verdict.cpu().numpy(), minlength=12).tolist()
        ok_rep = bool(np.array_equal(sizes, mix)) and bool((counts == args.arrived).all()) and \
            int(last_slice.item()) == n - 1
        reset()
        t2 = time.perf_counter()
        rs.shredder_intake_batch(ctx, [slot_id], n, N, rx, PKT, rx_lens, pk, store, PKT, store_lens, commitments,
                                 shred_bytes, last_slice, verdict)
        t3 = time.perf_counter()
        v_in = np.bincount(verdict.cpu().numpy(), minlength=12).tolist()
        return (t1 - t0) * 1e3, (t3 - t2) * 1e3, v_rep, v_in, ok_rep

    for _ in range(max(args.warmup, 1)):
        step()
    runs = [step() for _ in range(args.steps)]
    t_rep = statistics.median(r[0] for r in runs)
    t_in = statistics.median(r[1] for r in runs)
    _, _, v_rep, v_in, ok_rep = runs[-1]
    print(json.dumps({
        "metric": "replies/s repair intake, one block of mixed shred sizes, one call",
        "value": N / (t_rep * 1e-3), "unit": "replies/s", "higher_is_better": True, "n_gpus": 1,
        "steps": args.steps, "warmup": max(args.warmup, 1),
        "config": {"slices": n, "arrived": args.arrived, "dup_frac": args.dup_frac, "replies": int(N),
                   "reply_bytes": rx_bytes, "packet_stride": PKT, "mean_shred_bytes": float(mix.mean())},
        "repair_intake": {"wall_ms": t_rep, "replies_per_s": N / (t_rep * 1e-3),
                          "gb_per_s": rx_bytes / (t_rep * 1e-3) / 1e9},
        "shredder_intake_same_datagrams": {"wall_ms": t_in, "datagrams_per_s": N / (t_in * 1e-3)},
        "repair_over_intake": t_rep / t_in,
        "verify": {"repair_stored": v_rep[rs.INTAKE_STORED] == n * args.arrived,
                   "repair_duplicates": v_rep[rs.INTAKE_DUPLICATE] == dups.size, "repair_store": ok_rep,
                   "intake_stored": v_in[rs.INTAKE_STORED] == n * args.arrived,
                   "intake_duplicates": v_in[rs.INTAKE_DUPLICATE] == dups.size,
                   "repair_verdicts": dict(zip(rs.REPAIR_VERDICTS, v_rep))},
    }), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
