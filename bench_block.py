#!/usr/bin/env python3
"""bench_block.py -- block assembly on the device: ag_block_assemble_batch (reconstructed slices
-> BlockData::try_reconstruct_block's verdict, block hash, parent and transaction table;
slot_block_data.rs:376-454).

Workload: --nblocks blocks (default: 1 and 64) of 1024 slices at the leader's size mix
(bench_coder.mixed_sizes, bench_intake.py's).  Each slice's data is real transaction framing:
transactions of 1 .. 512 bytes until fewer than 520 bytes of the slice's budget (32 S - 1 bytes
framed) are left, written straight into a codeword buffer of stride 32 KiB with random slice roots
at stride 49 (no intake needed to time this call; the blocks are copies of one block, the roots
are not).  Every block is COMPLETE.  Wall clock around each (synchronous) call, table on (capacity =
the total, learned from a first call without a table) and off; the median over --steps.

Yardsticks, in the same process: ag_block_tree_batch alone on the same roots (the floor: the call
contains it) and, for one block, ag_shredder_deshred_batch_var on a store built as bench_intake.py
builds it (the stage in front, which this one must not dwarf).  Prints one JSON line per (nblocks,
table).
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
SLICES, STRIDE, PKT = 1024, 32 * 1024, 1344


def frame_block(np, mix, rng):
    """One block's rows on the host: (rows u8[1024][STRIDE], flags, ids, offsets, lens, txs, tx bytes)."""
    rows = np.zeros((SLICES, STRIDE), np.uint8)
    flags, ids = np.zeros(SLICES, np.uint8), np.zeros((SLICES, 40), np.uint8)
    offs, lens = np.zeros(SLICES, np.uint32), np.zeros(SLICES, np.uint32)
    flags[0] = 1
    ids[0] = rng.integers(0, 256, 40, dtype=np.uint8)
    ntx = nbytes = 0
    for i, S in enumerate(mix.tolist()):
        off = 49 if flags[i] else 9
        budget = max(32 * S - 1 - off, 8)   # (a 2-byte-shred slice with a parent has room for the count only)
        sizes, used = [], 8
        while budget - used >= 520:
            n = int(rng.integers(1, 513))
            sizes.append(n)
            used += 8 + n
        body = np.zeros(used, np.uint8)
        body[:8] = np.frombuffer(len(sizes).to_bytes(8, "little"), np.uint8)
        at = 8
        for n in sizes:
            body[at:at + 8] = np.frombuffer(n.to_bytes(8, "little"), np.uint8)
            body[at + 8:at + 8 + n] = (at * 31 + 7) & 0xFF
            at += 8 + n
        head = bytes([int(flags[i])]) + (ids[i].tobytes() if flags[i] else b"") + used.to_bytes(8, "little")
        rows[i, :off] = np.frombuffer(head, np.uint8)
        rows[i, off:off + used] = body
        offs[i], lens[i] = off, used
        ntx += len(sizes)
        nbytes += sum(sizes)
    return rows, flags, ids, offs, lens, ntx, nbytes


def deshred_yardstick(np, torch, rs, ctx, dev, mix, steps, warmup):
    """ag_shredder_deshred_batch_var on one block's store after an intake of 40 of 64 datagrams
    per slice (bench_intake.py's store): median wall ms."""
    n, stride = SLICES, 64 * 1024
    dmix = (32 * mix.astype(np.int64) - 1 - 9).astype(np.uint32)
    data = torch.empty((n, 32 * 1024), dtype=torch.uint8, device=dev)
    rs.fill_splitmix(ctx, data, n, 32 * 1024, 32 * 1024, 0x5EED0000)
    slots = torch.full((n,), 0x1A7A4E, dtype=torch.int64, device=dev)
    sidx = torch.arange(n, dtype=torch.int64, device=dev)
    last = (torch.arange(n) == n - 1).to(torch.uint8).to(dev)
    seed = torch.arange(32, dtype=torch.uint8).to(dev)
    pk = torch.empty(32, dtype=torch.uint8, device=dev)
    rs.ed25519_public_key_batch(ctx, 1, seed, pk)
    cw = torch.zeros(n * stride, dtype=torch.uint8, device=dev)
    pkts = torch.zeros((n * 64, PKT), dtype=torch.uint8, device=dev)
    lens = torch.zeros(n * 64, dtype=torch.int32, device=dev)
    rs.shredder_shred_batch_var(ctx, n, [None] * n, data, 32 * 1024, dmix, slots, sidx, last, seed, pk, cw, stride,
                                pkts, PKT, lens)
    rng = np.random.default_rng(0x1A7A)
    order = rng.permutation(np.concatenate([64 * s + rng.permutation(64)[:40] for s in range(n)]))
    sel = torch.from_numpy(order).to(dev)
    rx, rx_lens = pkts[sel].contiguous(), lens[sel].contiguous()
    del pkts, data
    store = torch.zeros((n * 64, PKT), dtype=torch.uint8, device=dev)
    store_lens = torch.zeros(n * 64, dtype=torch.int32, device=dev)
    commitments = torch.zeros(49 * n, dtype=torch.uint8, device=dev)
    shred_bytes = torch.zeros(n, dtype=torch.int32, device=dev)
    last_slice = torch.full((1,), -1, dtype=torch.int32, device=dev)
    verdict = torch.zeros(order.size, dtype=torch.uint8, device=dev)
    times, ok = [], True
    for k in range(warmup + steps):
        store_lens.zero_()
        shred_bytes.zero_()
        last_slice.fill_(-1)
        sizes, _ = rs.shredder_intake_batch(ctx, [0x1A7A4E], n, order.size, rx, PKT, rx_lens, pk, store, PKT,
                                            store_lens, commitments, shred_bytes, last_slice, verdict)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = rs.shredder_deshred_batch_var(ctx, n, sizes, store, PKT, store_lens, pk, cw, stride)
        t1 = time.perf_counter()
        ok = ok and bool((res.status == 0).all())
        if k >= warmup:
            times.append((t1 - t0) * 1e3)
    return statistics.median(times), ok


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--nblocks", type=int, nargs="+", default=[1, 64])
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--no-yardsticks", action="store_true", help="time the assembly call only (profiling runs)")
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
    warmup = max(args.warmup, 1)
    mix = bench_coder.mixed_sizes(SLICES)
    rng = np.random.default_rng(0xB10CA55E)
    rows, flags1, ids1, offs1, lens1, ntx, nbytes = frame_block(np, mix, rng)
    d_block = torch.from_numpy(rows.reshape(-1)).to(dev)
    t_de = None
    if not args.no_yardsticks and 1 in args.nblocks:
        t_de, de_ok = deshred_yardstick(np, torch, rs, ctx, dev, mix, args.steps, warmup)

    def median_ms(fn):
        for _ in range(warmup):
            fn()
        times = []
        for _ in range(args.steps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = fn()
            times.append((time.perf_counter() - t0) * 1e3)
        return statistics.median(times), out

    for nb in args.nblocks:
        nrows = nb * SLICES
        cw = d_block.repeat(nb)
        commitments = torch.from_numpy(rng.integers(0, 256, 49 * nrows, dtype=np.uint8)).to(dev)
        roots = commitments.view(nrows, 49)[:, 17:].contiguous().view(-1)
        last_slice = torch.full((nb,), SLICES - 1, dtype=torch.int32, device=dev)
        hashes = torch.zeros(32 * nb, dtype=torch.uint8, device=dev)
        tree_hashes = torch.zeros(32 * nb, dtype=torch.uint8, device=dev)
        ok = np.ones(nrows, np.uint8)
        parents = (np.tile(flags1, nb), np.tile(ids1, (nb, 1)))
        offs, lens = np.tile(offs1, nb), np.tile(lens1, nb)

        def assemble(table=None, cap=0):
            return rs.block_assemble_batch(ctx, nb, SLICES, ok, parents, offs, lens, cw, STRIDE, commitments[17:], 49,
                                           last_slice, hashes, tx_offsets=table and table[0],
                                           tx_lens=table and table[1], tx_capacity=cap)

        def tree():
            rs.block_tree_batch(ctx, nb, [SLICES] * nb, roots, tree_hashes)
            ctx.synchronize()

        total = assemble().tx_total
        table = (torch.zeros(max(total, 1), dtype=torch.int64, device=dev),
                 torch.zeros(max(total, 1), dtype=torch.int32, device=dev))
        t_tree = None if args.no_yardsticks else median_ms(tree)[0]
        for on in (True, False):
            t, got = median_ms((lambda: assemble(table, total)) if on else assemble)
            verify = {"complete": bool((got.verdict == rs.BLOCK_COMPLETE).all()),
                      "tx_total": got.tx_total == nb * ntx, "tx_bytes": int(got.tx_bytes.sum()) == nb * nbytes,
                      "parent": got.parents[0] is not None and got.parents[0][1] == ids1[0, 8:].tobytes()}
            if not args.no_yardsticks:
                verify["hash_is_the_trees"] = bool(torch.equal(hashes, tree_hashes))
            if on:
                o, l = table[0].cpu().numpy(), table[1].cpu().numpy()
                verify["table"] = bool(int(l.sum()) == nb * nbytes and (np.diff(o) > 0).all())
            print(json.dumps({
                "metric": "blocks/s block assembly, blocks of 1024 slices of mixed shred sizes, one call",
                "value": nb / (t * 1e-3), "unit": "blocks/s", "higher_is_better": True, "n_gpus": 1,
                "steps": args.steps, "warmup": warmup,
                "config": {"nblocks": nb, "slices_per_block": SLICES, "table": on, "codeword_stride": STRIDE,
                           "transactions": nb * ntx, "transaction_bytes": nb * nbytes,
                           "mean_shred_bytes": float(mix.mean())},
                "assemble": {"wall_ms": t, "ms_per_block": t / nb, "transactions_per_s": nb * ntx / (t * 1e-3)},
                "block_tree_alone": None if t_tree is None else {"wall_ms": t_tree},
                "deshred_var_before": None if (t_de is None or nb != 1) else {"wall_ms": t_de, "all_ok": de_ok},
                "verify": verify,
            }), flush=True)
        del cw, table
    ctx.close()


if __name__ == "__main__":
    main()
