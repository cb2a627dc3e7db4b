#!/usr/bin/env python3
"""bench_shredder.py -- the composed RegularShredder on the device (SURVEY.md §8 a10 end to
end; VERDICT r01 "composed Shredder pipeline"): ag_shredder_shred_batch (Slice framing ->
ReedSolomonCoder::shred -> slice Merkle tree -> slice signature -> 64 Shred datagrams per
slice; shredder.rs:337-345, :533-560) and ag_shredder_deshred_batch (datagrams -> parse ->
ValidatedShred::try_new with the cached commitment -> ReedSolomonCoder::deshred ->
check_merkle_tree -> SlicePayload::try_from -> fill_missing_shreds; shredder.rs:282-311,
validated_shred.rs:52-81).

Workload: n maximum slices (32 758 data bytes + 9-byte header = 32 767-byte payload, 1 KiB
shreds).  Shred builds all 64 datagrams per slice; deshred receives, per slice, the first
32..64 datagrams of a seeded random arrival order (the follower deshreds once 32 arrived,
slot_block_data.rs:331-370) and fills in the rest.  Device-resident buffers; wall clock
around each (synchronous) call.  Prints one JSON line; the verify block checks the round
trip (every payload and datagram restored) and a spot check against the CPU composition of
the reference (oracle/shredder_oracle.py, checker only).

--mixed-sizes times both sides over a block's mix of shred sizes (bench_coder.mixed_sizes):
ag_shredder_shred_batch_var and ag_shredder_deshred_batch_var against loops of the uniform
calls; see mixed_leg and mixed_deshred_leg.

--adversarial-frac F (with --arrived 40): a fraction F of the slices comes from a leader that
alters one shred after encoding and signs the tree over the altered shreds (byzantine_datagrams).
Every such datagram validates, the slice fails the follower's ANY_K pass and, arriving with more
than 32 datagrams, is decoded again with the crate's decoder over every kept shred: the line's
rerun_slices / rerun_passes say how many slices that was and in how many batched passes.
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
PKT = 1344  # datagram slot (1325 bytes for a 1 KiB shred, rounded to 64)
# name -> (AG_SHREDDER_*, coding shreds of its coder, key bytes appended to the payload)
NAMES = {"regular": "RegularShredder", "coding_only": "CodingOnlyShredder", "pets": "PetsShredder",
         "aont": "AontShredder"}
KINDS = {"regular": (0, 32, 0), "coding_only": (1, 64, 0), "pets": (2, 33, 16), "aont": (3, 32, 16)}


def adversarial_slices(n, frac):
    """The slices of a Byzantine leader: round(frac * n) of n, seeded, ascending (numpy)."""
    import numpy as np

    r = int(round(frac * n))
    return np.sort(np.random.default_rng(0xB12A).permutation(n)[:r])


def byzantine_datagrams(ctx, leaves, num_data, slots, sidx, last, seed, pk, pkt):
    """The 64 datagrams per slice of a leader that signs shreds which are no codeword, built on
    the device from the public calls.  leaves: [R][64][S], a copy of R slices' 64 output raw
    shreds as the shred call left them; one shred of each is XORed with 0x5A, then
    ag_merkle_build_batch, ag_slice_sign_batch and ag_shred_serialize_batch over the altered
    shreds -> (datagrams [R * 64][pkt], lengths [R * 64])."""
    import torch

    from alpenglow_amd import rs

    R, _, S = leaves.shape
    dev = leaves.device
    g = torch.Generator(device="cpu").manual_seed(0x7A3)
    tamper = torch.randint(0, 64, (R,), generator=g).to(dev)
    leaves[torch.arange(R, device=dev), tamper] ^= 0x5A
    roots = torch.empty((R, 32), dtype=torch.uint8, device=dev)
    proofs = torch.empty((R * 64, 192), dtype=torch.uint8, device=dev)
    rs.merkle_build_batch(ctx, 64, S, R, leaves, S, 64 * S, roots, proofs=proofs, proofs_stride=64 * 192)
    sigs = torch.empty((R, 64), dtype=torch.uint8, device=dev)
    rs.slice_sign_batch(ctx, R, seed, pk, slots, sidx, last, roots, sigs)
    j = torch.arange(64, device=dev).repeat(R)
    cols = dict(kind=(j >= num_data).to(torch.uint8), slot=slots.repeat_interleave(64).contiguous(),
                slice_index=sidx.repeat_interleave(64).contiguous(), is_last=last.repeat_interleave(64).contiguous(),
                shred_index=j.to(torch.int32), data_len=torch.full((R * 64,), S, dtype=torch.int32, device=dev),
                sig=sigs.repeat_interleave(64, dim=0).contiguous(),
                height=torch.full((R * 64,), 6, dtype=torch.int32, device=dev))
    c = rs.ShredColumns.of(cols["kind"], cols["slot"], cols["slice_index"], cols["is_last"], cols["shred_index"], leaves,
                           S, cols["data_len"], cols["sig"], proofs, 192, cols["height"])
    out = torch.zeros((R * 64, pkt), dtype=torch.uint8, device=dev)
    lens = torch.zeros(R * 64, dtype=torch.int32, device=dev)
    rs.shred_serialize_batch(ctx, R * 64, c, out, pkt, lens)
    torch.cuda.synchronize()
    return out, lens


def last_rerun(ctx):
    """(slices, passes) of the context's last composed deshred, or (None, None) on a library
    built before the counters (an A/B against an older build)."""
    from alpenglow_amd import rs

    if not hasattr(rs.load(), "ag_rs_internal_last_exact_rerun"):
        return None, None
    return rs.last_exact_rerun(ctx)


def mixed_leg(args):
    """--mixed-sizes: RegularShredder::shred of --slices slices whose shred sizes are a block's mix
    (the longest payload of each size, no parents), legs interleaved step by step:
      var_mix        ag_shredder_shred_batch_var, one call
      presorted_mix  the mix sorted by size, ag_shredder_shred_batch once per distinct size (the
                     caller's gather and scatter are not timed)
      uniform_1024   ag_shredder_shred_batch on maximum slices (the uniform rate, beside both)
      runs_mix       the mix in block order, ag_shredder_shred_batch once per run of equal sizes --
                     what a caller can do without the var call (host-bound: timed once)
    Per leg the median over --steps of the host's wall time from the call to the end of a
    synchronise.  One JSON line; the verify block compares var_mix's datagrams, lengths and roots
    with runs_mix's.  The deshred side of the same block follows (mixed_deshred_leg), under the
    line's "deshred" key."""
    import statistics

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
    mix = bench_coder.mixed_sizes(n)
    dmix = (32 * mix.astype(np.int64) - 1 - 9).astype(np.uint32)  # data bytes: framed payload 32 S - 1
    data = torch.empty((n, 32 * 1024), dtype=torch.uint8, device=dev)
    rs.fill_splitmix(ctx, data, n, 32 * 1024, 32 * 1024, 0x5EED0000)
    g = torch.Generator(device="cpu").manual_seed(0xA221)
    slots = torch.randint(0, 1 << 40, (n,), generator=g, dtype=torch.int64).to(dev)
    sidx = torch.randint(0, 1024, (n,), generator=g, dtype=torch.int64).to(dev)
    last = (torch.arange(n) % 1024 == 1023).to(torch.uint8).to(dev)
    seed = torch.arange(32, dtype=torch.uint8).to(dev)
    pk = torch.empty(32, dtype=torch.uint8, device=dev)
    rs.ed25519_public_key_batch(ctx, 1, seed, pk)
    cw = torch.zeros(n * stride, dtype=torch.uint8, device=dev)
    pkts = torch.zeros((n * 64, PKT), dtype=torch.uint8, device=dev)
    lens = torch.zeros(n * 64, dtype=torch.int32, device=dev)
    roots = torch.zeros((n, 32), dtype=torch.uint8, device=dev)
    parents = [None] * n
    order = np.argsort(mix, kind="stable")
    srt, dsrt = mix[order], dmix[order]
    starts = np.flatnonzero(np.r_[True, srt[1:] != srt[:-1]]).tolist() + [n]
    cuts = np.flatnonzero(np.r_[True, mix[1:] != mix[:-1]]).tolist() + [n]
    d1024 = np.full(n, 32 * 1024 - 1 - 9, np.uint32)

    def var():
        rs.shredder_shred_batch_var(ctx, n, parents, data, 32 * 1024, dmix, slots, sidx, last, seed, pk, cw, stride,
                                    pkts, PKT, lens, roots_out=roots)

    def uniform(S, dl, b=0, e=n):
        rs.shredder_shred_batch(ctx, e - b, S, parents[b:e], data[b:e], 32 * 1024, dl[b:e], slots[b:e], sidx[b:e],
                                last[b:e], seed, pk, cw.data_ptr() + b * stride, pkts[64 * b:64 * e], PKT,
                                lens[64 * b:64 * e], roots_out=roots[b:e])

    def per_run(sizes, dl, edges):
        for b, e in zip(edges[:-1], edges[1:]):
            uniform(int(sizes[b]), dl, b, e)

    def timed(f):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        f()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    var()
    torch.cuda.synchronize()
    want = pkts.clone(), lens.clone(), roots.clone()
    pkts.zero_()
    t_runs = timed(lambda: per_run(mix, dmix, cuts))
    same = torch.equal(pkts, want[0]) and torch.equal(lens, want[1]) and torch.equal(roots, want[2])
    del want
    legs = {"var_mix": var, "presorted_mix": lambda: per_run(srt, dsrt, starts),
            "uniform_1024": lambda: uniform(1024, d1024)}
    for _ in range(max(args.warmup, 2)):
        for f in legs.values():
            f()
    times = {k: [] for k in legs}
    for _ in range(args.steps):
        for k, f in legs.items():
            times[k].append(timed(f))
    times["runs_mix"] = [t_runs]
    out = {k: {"wall_ms": statistics.median(v), "slices_per_s": n / (statistics.median(v) * 1e-3), "steps": len(v)}
           for k, v in times.items()}
    var()  # the block's datagrams again (the uniform leg ran last)
    deshred = mixed_deshred_leg(args, ctx, dev, mix, dmix, order, starts, data, pk, cw, pkts, lens, timed,
                                lambda: uniform(1024, d1024), (slots.cpu().numpy(), sidx.cpu().numpy(), last.cpu().numpy()))
    print(json.dumps({
        "metric": "slices/s composed RegularShredder shred over a block's mix of shred sizes, one var call",
        "value": out["var_mix"]["slices_per_s"], "unit": "slices/s", "higher_is_better": True, "n_gpus": 1,
        "steps": args.steps, "warmup": max(args.warmup, 2),
        "config": {"slices": n, "codeword_stride": stride, "packet_stride": PKT, "distinct_sizes": len(starts) - 1,
                   "runs": len(cuts) - 1, "mean_shred_bytes": float(mix.mean())},
        "legs": out,
        "ratios": {"var_mix_over_runs_mix": out["runs_mix"]["wall_ms"] / out["var_mix"]["wall_ms"],
                   "var_mix_over_presorted_mix": out["presorted_mix"]["wall_ms"] / out["var_mix"]["wall_ms"],
                   "var_mix_over_uniform_1024": out["uniform_1024"]["wall_ms"] / out["var_mix"]["wall_ms"]},
        "verify": {"var_mix_equals_runs_mix": same},
        "deshred": deshred,
    }), flush=True)
    ctx.close()


def mixed_deshred_leg(args, ctx, dev, mix, dmix, order, starts, data, pk, cw, pkts, lens, timed, shred_1024, hdrs):
    """The follower's side of --mixed-sizes: the block mixed_leg shredded (pkts / lens hold
    ag_shredder_shred_batch_var's datagrams), a random --arrived (default 32) of 64 datagrams per slice received,
    legs interleaved step by step:
      var_mix        ag_shredder_deshred_batch_var, one call
      presorted_mix  the datagrams already regrouped by size, ag_shredder_deshred_batch once per
                     distinct size (the regrouping is not timed)
      runs_mix       the same with the regrouping copy timed: what a caller does without the var
                     call (the deshred fills datagram slots in place, so slices of one size have
                     to sit together)
      uniform_1024   ag_shredder_deshred_batch on maximum slices
    Before each timed call only the lengths are reset (absent slots: length 0).  verify: every
    slice of every leg has status OK, and var_mix's payloads equal the input."""
    import statistics

    import numpy as np
    import torch

    from alpenglow_amd import rs

    n, stride = args.slices, 64 * 1024
    g = torch.Generator(device="cpu").manual_seed(0xF011)
    pick = torch.argsort(torch.rand((n, 64), generator=g), dim=1)[:, :args.arrived]
    keep = torch.zeros((n, 64), dtype=torch.bool).scatter_(1, pick, True).reshape(-1).to(dev)
    # --adversarial-frac: the Byzantine leader's slices get their datagrams in place, size by size
    adv = adversarial_slices(n, args.adversarial_frac)
    bad = torch.zeros(n, dtype=torch.bool, device=dev)
    if len(adv):
        hdr = [torch.from_numpy(x).to(dev) for x in hdrs]
        seed = torch.arange(32, dtype=torch.uint8).to(dev)
        for S in np.unique(mix[adv]).tolist():
            idx = torch.from_numpy(adv[mix[adv] == S]).to(dev)
            leaves = cw.view(n, stride)[idx, :64 * S].reshape(len(idx), 64, S).contiguous()
            bp, bl = byzantine_datagrams(ctx, leaves, 32, hdr[0][idx], hdr[1][idx], hdr[2][idx], seed, pk, PKT)
            at = (idx[:, None] * 64 + torch.arange(64, device=dev)[None, :]).reshape(-1)
            assert torch.equal(lens[at], bl)
            pkts[at] = bp
        bad[torch.from_numpy(adv).to(dev)] = True
    got = lens * keep  # the received lengths, var layout
    ord_t = torch.from_numpy(order).to(dev)
    rows = (ord_t[:, None] * 64 + torch.arange(64, device=dev)[None, :]).reshape(-1)  # datagram rows, sorted by size
    spk = torch.empty_like(pkts)
    slens, sgot = torch.empty_like(lens), torch.empty_like(lens)
    srt = mix[order]
    offs = np.r_[0, np.cumsum(64 * srt.astype(np.int64))]  # codewords of the sorted slices, packed at 64 S
    cwu = torch.zeros(int(offs[-1]), dtype=torch.uint8, device=dev)

    def regroup():
        torch.index_select(pkts, 0, rows, out=spk)
        torch.index_select(got, 0, rows, out=sgot)

    def var():
        return [rs.shredder_deshred_batch_var(ctx, n, mix, pkts, PKT, lens, pk, cw, stride)]

    def per_size():
        return [rs.shredder_deshred_batch(ctx, e - b, int(srt[b]), spk[64 * b:64 * e], PKT, slens[64 * b:64 * e], pk,
                                          cwu.data_ptr() + int(offs[b])) for b, e in zip(starts[:-1], starts[1:])]

    def runs():
        regroup()
        slens.copy_(sgot)
        return per_size()

    pkts_u, lens_u, cw_u = torch.empty_like(pkts), torch.empty_like(lens), torch.empty_like(cw)
    held = pkts.clone(), lens.clone()
    shred_1024()  # maximum slices into pkts / lens, moved aside; then the block's datagrams back
    torch.cuda.synchronize()
    pkts_u.copy_(pkts)
    got_u = lens * keep
    pkts.copy_(held[0])
    lens.copy_(held[1])
    del held

    def uniform():
        return [rs.shredder_deshred_batch(ctx, n, 1024, pkts_u, PKT, lens_u, pk, cw_u)]

    regroup()
    legs = {"var_mix": (var, lambda: lens.copy_(got)), "presorted_mix": (per_size, lambda: slens.copy_(sgot)),
            "runs_mix": (runs, lambda: None), "uniform_1024": (uniform, lambda: lens_u.copy_(got_u))}
    res, times = {}, {k: [] for k in legs}
    rerun = (None, None)
    for step in range(max(args.warmup, 2) + args.steps):
        for k, (f, reset) in legs.items():
            reset()
            out = []
            t = timed(lambda: out.extend(f()))
            res[k] = out
            if k == "var_mix":
                rerun = last_rerun(ctx)
            if step >= max(args.warmup, 2):
                times[k].append(t)
    # every honest slice OK, every Byzantine one failed (var layout; the regrouped legs: sorted by size)
    bad_h = bad.cpu().numpy()
    fails = {"var_mix": bad_h, "presorted_mix": bad_h[order], "runs_mix": bad_h[order], "uniform_1024": np.zeros(n, bool)}
    ok = {k: bool(np.array_equal(np.concatenate([np.asarray(r.status) for r in v]) != 0, fails[k])) for k, v in res.items()}
    r = res["var_mix"][0]
    good = ~bad_h
    same = bool((np.asarray(r.data_offsets)[good] == 9).all()) and bool((np.asarray(r.data_lens)[good] == dmix[good]).all())
    dl = torch.from_numpy(np.where(good, dmix, 0).astype(np.int64)).to(dev)
    col = torch.arange(32 * 1024 - 10, device=dev)[None, :]
    cwv = cw.view(n, stride)
    for b in range(0, n, 4096):  # payload bytes against the input, a few thousand slices at a time
        e = min(n, b + 4096)
        same = same and bool(((cwv[b:e, 9:9 + col.shape[1]] == data[b:e, :col.shape[1]]) | (col >= dl[b:e, None])).all())
    out = {k: {"wall_ms": statistics.median(v), "slices_per_s": n / (statistics.median(v) * 1e-3), "steps": len(v)}
           for k, v in times.items()}
    return {"metric": "slices/s composed RegularShredder deshred over a block's mix of shred sizes from a random "
                      f"{args.arrived} "
                      "of 64 datagrams per slice, one var call",
            "value": out["var_mix"]["slices_per_s"], "unit": "slices/s", "legs": out,
            "arrived": args.arrived, "adversarial_frac": args.adversarial_frac, "adversarial_slices": int(len(adv)),
            "rerun_slices": rerun[0], "rerun_passes": rerun[1],
            "ratios": {"var_mix_over_runs_mix": out["runs_mix"]["wall_ms"] / out["var_mix"]["wall_ms"],
                       "var_mix_over_presorted_mix": out["presorted_mix"]["wall_ms"] / out["var_mix"]["wall_ms"],
                       "var_mix_over_uniform_1024": out["uniform_1024"]["wall_ms"] / out["var_mix"]["wall_ms"]},
            "verify": {"every_status_ok": ok, "var_mix_payloads_equal_input": same}}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--slices", type=int, default=65536)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--arrived", type=int, default=32, help="datagrams received per slice before deshred (32..64)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--shred-bytes", type=int, default=1024,
                    help="shred size S (even, <= 1024): payloads of 32 S - 1 bytes; 1024 = maximum slices")
    ap.add_argument("--kind", choices=list(KINDS), default="regular",
                    help="the shredder (shredder.rs:336-500); the CPU baseline is timed for regular only")
    ap.add_argument("--adversarial-frac", type=float, default=0.0,
                    help="fraction of the slices from a leader that signs altered shreds (use with --arrived 40)")
    ap.add_argument("--mixed-sizes", action="store_true",
                    help="time ag_shredder_shred_batch_var on a block's mix of shred sizes against the uniform call")
    args = ap.parse_args()
    if args.mixed_sizes:
        return mixed_leg(args)
    import numpy as np
    import torch

    from alpenglow_amd import rs

    dev = torch.device("cuda:0")
    torch.zeros(1, device=dev)
    ctx = rs.Context(0)
    stream = torch.cuda.Stream(dev)
    torch.cuda.set_stream(stream)
    ctx.set_stream(stream.cuda_stream)
    n, S = args.slices, args.shred_bytes
    assert S % 2 == 0 and 64 <= S <= 1024, "--shred-bytes: even, 64..1024"
    kind, m, extra = KINDS[args.kind]
    D = 32 * S - 1 - 9 - extra  # data bytes: framed payload (+ key) = MAX_DATA_PER_SLICE
    stride = (32 + m) * S
    data = torch.empty((n, 32 * S), dtype=torch.uint8, device=dev)
    rs.fill_splitmix(ctx, data, n, 32 * S, 32 * S, 0x5EED0000)
    g = torch.Generator(device="cpu").manual_seed(0xA221)
    slots = torch.randint(0, 1 << 40, (n,), generator=g, dtype=torch.int64).to(dev)
    sidx = torch.randint(0, 1024, (n,), generator=g, dtype=torch.int64).to(dev)
    last = (torch.arange(n) % 1024 == 1023).to(torch.uint8).to(dev)
    seed = torch.arange(32, dtype=torch.uint8).to(dev)
    pk = torch.empty(32, dtype=torch.uint8, device=dev)
    rs.ed25519_public_key_batch(ctx, 1, seed, pk)
    cw = torch.empty((n, stride), dtype=torch.uint8, device=dev)
    keys = torch.randint(0, 256, (n * 16,), generator=g, dtype=torch.uint8).to(dev)
    pkts = torch.zeros((n * 64, PKT), dtype=torch.uint8, device=dev)
    lens = torch.zeros(n * 64, dtype=torch.int32, device=dev)
    parents, dlens = [None] * n, np.full(n, D, np.uint32)
    # arrival: per slice the first `arrived` of a random order
    order = torch.argsort(torch.rand((n, 64), generator=g), dim=1)
    keep = torch.zeros((n, 64), dtype=torch.bool)
    keep.scatter_(1, order[:, :args.arrived], True)
    keep = keep.reshape(-1).to(dev)

    def shred():
        if kind == 0:
            rs.shredder_shred_batch(ctx, n, S, parents, data, 32 * S, dlens, slots, sidx, last, seed, pk, cw, pkts,
                                    PKT, lens)
        else:
            rs.shredder_shred_batch_kind(ctx, kind, n, S, parents, data, 32 * S, dlens, slots, sidx, last, seed, pk,
                                         keys, cw, stride, pkts, PKT, lens)

    def deshred():
        if kind == 0:
            return rs.shredder_deshred_batch(ctx, n, S, pkts, PKT, lens, pk, cw)
        return rs.shredder_deshred_batch_kind(ctx, kind, n, S, pkts, PKT, lens, pk, cw, stride)

    shred()
    torch.cuda.synchronize()
    full_lens = lens.clone()
    full_pkts = pkts[: 64 * 8].clone()
    # --adversarial-frac: the Byzantine leader's datagrams, built once from the shredded codewords
    # and put into their slots after every shred call
    adv = adversarial_slices(n, args.adversarial_frac)
    bad = torch.zeros(n, dtype=torch.bool, device=dev)
    if len(adv):
        idx = torch.from_numpy(adv).to(dev)
        out_rows = [r for r in range(32 + m) if (kind != 1 or r >= 32) and (kind != 2 or r != 31)][:64]
        leaves = cw.view(n, 32 + m, S)[idx][:, out_rows].contiguous()
        adv_pkts, adv_lens = byzantine_datagrams(ctx, leaves, {0: 32, 1: 0, 2: 31, 3: 32}[kind], slots[idx], sidx[idx],
                                                 last[idx], seed, pk, PKT)
        adv_at = (idx[:, None] * 64 + torch.arange(64, device=dev)[None, :]).reshape(-1)
        assert torch.equal(full_lens[adv_at], adv_lens)
        bad[idx] = True

    def arrive():
        """The datagrams that did not arrive dropped, the Byzantine leader's slices in place."""
        lens.mul_(keep)
        if len(adv):
            pkts[adv_at] = adv_pkts

    for _ in range(args.warmup):
        arrive()
        deshred()
        shred()
    torch.cuda.synchronize()
    t_sh = t_de = 0.0
    for _ in range(args.steps):
        a = time.perf_counter()
        shred()
        torch.cuda.synchronize()
        b = time.perf_counter()
        arrive()
        torch.cuda.synchronize()
        c = time.perf_counter()
        res = deshred()  # synchronous
        d = time.perf_counter()
        t_sh += b - a
        t_de += d - c
    rerun = last_rerun(ctx)
    # every honest slice restored, every Byzantine one failed with its datagram lengths as received
    bad_h = bad.cpu().numpy()
    good = torch.from_numpy(~bad_h).to(dev)
    ok = bool(np.array_equal(np.asarray(res.status) != 0, bad_h)) and \
        bool(torch.equal(lens.view(n, 64)[good], full_lens.view(n, 64)[good])) and \
        bool((np.asarray(res.data_lens)[~bad_h] == D).all())
    if len(adv):
        ok = ok and bool(torch.equal(lens.view(n, 64)[bad], (full_lens * keep).view(n, 64)[bad]))
    first = [b for b in range(n) if not bad_h[b]][:64]  # the spot checks' slices: honest ones
    head = [b for b in first if b < 8]
    ok = ok and bool(torch.equal(pkts.view(n, 64, PKT)[head], full_pkts.view(8, 64, PKT)[head]))
    off = res.data_offsets.tolist()
    ok = ok and all(torch.equal(cw[b, off[b]:off[b] + D], data[b, :D]) for b in first)
    # spot check: two slices against the CPU composition of the reference (checker only)
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import shredder_oracle as so
    spot = True
    for b in first[:2]:
        hp, hl = pkts[64 * b:64 * b + 64].cpu().numpy(), lens[64 * b:64 * b + 64].cpu().numpy()
        want, *_ = so.shred_kind(kind, None, data[b, :D].cpu().numpy().tobytes(), int(slots[b]), int(sidx[b]),
                                 bool(last[b]), bytes(range(32)), keys[16 * b:16 * b + 16].cpu().numpy().tobytes())
        spot &= all(hp[j, :hl[j]].tobytes() == want[j] for j in range(64))
    steps = args.steps
    line = {
        "metric": f"slices/s composed {NAMES[args.kind]} shred + deshred (datagrams in, datagrams out), "
                  + ("max slices" if S == 1024 else f"{S}-byte shreds"),
        "value": n * steps / (t_sh + t_de),
        "unit": "slices/s",
        "n_gpus": 1,
        "steps": steps,
        "warmup": args.warmup,
        "ms_per_step": (t_sh + t_de) * 1e3 / steps,
        "higher_is_better": True,
        "scaling": "weak",
        "vs_baseline": None,
        "dtype": "u8",
        "data": "synthetic (splitmix64 payloads, device-generated; one leader key)",
        "config": {"workload": f"{n} slices x {D + 9} B payload, 64 datagrams of {S + 301} B per slice; deshred from a "
                               f"random {args.arrived} of 64 datagrams per slice"},
        "arrived": args.arrived,
        "adversarial_frac": args.adversarial_frac,
        "adversarial_slices": int(len(adv)),
        "rerun_slices": rerun[0],
        "rerun_passes": rerun[1],
        "payload_GiBps": n * (D + 9) * steps / (t_sh + t_de) / GIB,
        "calls_ms": {"shred_batch": t_sh * 1e3 / steps, "deshred_batch": t_de * 1e3 / steps},
        "shred_slices_per_s": n * steps / t_sh,
        "deshred_slices_per_s": n * steps / t_de,
        "verify": {"roundtrip_restores_everything": ok, "datagrams_match_oracle": bool(spot)},
    }
    if not args.no_cpu_baseline and kind == 0:
        line["cpu_baseline"] = _cpu_baseline(args, data, slots, sidx, last, cw, pkts, D, S)
    print(json.dumps(line), flush=True)
    ctx.close()


def _host_cpus():
    n = len(os.sched_getaffinity(0))
    try:
        quota, period = open("/sys/fs/cgroup/cpu.max").read().split()[:2]
        if quota != "max":
            n = min(n, max(1, int(int(quota) // int(period))))
    except (OSError, ValueError):
        pass
    return n


def _cpu_baseline(args, data, slots, sidx, last, cw, pkts, D, S):
    """The composed RegularShredder on this host's CPU (oracle/shredder_cpu.c, a port: the
    crate's Avx2 RS engine restated, OpenSSL's SHA-256 and Ed25519), on a bounded sample of
    the same slices: shred (RS + Merkle tree + signature + proofs), the reference bench's
    deshred from the 32 coding shreds (RS decode + re-encode + Merkle check + parse + proofs;
    benches/shredder.rs:19-61) and the receive-side validation the device deshred also does
    (each shred's root from its path, one signature verified per slice).  1 thread and every
    host CPU; its coding shreds and signatures are compared with the device's."""
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import numpy as np

    import ed25519_oracle as ed
    import shredder_cpu as sc

    seed = bytes(range(32))
    pk = ed.secret_to_public(seed)
    nall = _host_cpus()
    n = min(data.shape[0], max(64, nall * 64))
    framed = np.zeros((n, 32 * S), np.uint8)
    framed[:, 1:9] = np.frombuffer(int(D).to_bytes(8, "little"), np.uint8)
    framed[:, 9:9 + D] = data[:n, :D].cpu().numpy()
    lens = np.full(n, D + 9, np.uint32)
    sl, si, ls = slots[:n].cpu().numpy(), sidx[:n].cpu().numpy(), last[:n].cpu().numpy()

    def rate(what, threads, cnt):
        t = time.perf_counter()
        st, *_ = sc.run(what, threads, framed[:cnt], lens[:cnt], sl[:cnt], si[:cnt], ls[:cnt], seed, pk)
        dt = time.perf_counter() - t
        if st:
            raise RuntimeError(f"shredder_cpu failed ({st})")
        return cnt / dt

    out = {"unit": "slices/s", "kind": "port", "cores": nall, "cpu": _cpu_model()}
    # device comparison: the first 8 slices' coding shreds and slice signatures
    st, coding, _, sigs = sc.run(sc.SHRED, 1, framed[:8], lens[:8], sl[:8], si[:8], ls[:8], seed, pk, outputs=True)
    gc = cw[:8, 32 * S:64 * S].cpu().numpy().reshape(8, 32, S)
    gsig = pkts.view(-1, 64, pkts.shape[1])[:8, 0, 37 + S:37 + S + 64].cpu().numpy()
    out["gpu_matches_cpu"] = bool(st == 0 and np.array_equal(coding, gc) and np.array_equal(sigs, gsig))
    for threads in (1, nall):
        cnt = min(n, 64 * threads)
        r_sh = rate(sc.SHRED, threads, cnt)
        r_bench = rate(sc.SHRED | sc.DESHRED, threads, cnt)
        r_all = rate(sc.SHRED | sc.DESHRED | sc.RECEIVE, threads, cnt)
        t_sh, t_de, t_rx = 1 / r_sh, 1 / r_bench - 1 / r_sh, 1 / r_all - 1 / r_bench
        out[f"threads_{threads}"] = {
            "slices": cnt, "threads": threads,
            "shred_slices_per_s": r_sh, "deshred_slices_per_s": 1 / t_de,
            "receive_slices_per_s": 1 / t_rx,
            "reference_bench_roundtrip_slices_per_s": r_bench,
            "device_shape_roundtrip_slices_per_s": r_all,
        }
    out["value"] = out[f"threads_{nall}"]["device_shape_roundtrip_slices_per_s"]
    out["sample"] = (f"{n} of the same maximum slices (framed 32 767-byte payloads), shred + receive validation + "
                     f"deshred from the 32 coding shreds, one slice per task; RS by oracle/rs_cpu_avx2.c, SHA-256 "
                     f"and Ed25519 by OpenSSL libcrypto")
    return out


def _cpu_model():
    try:
        for ln in open("/proc/cpuinfo"):
            if ln.startswith("model name"):
                return ln.split(":", 1)[1].strip()
    except OSError:
        pass
    return None


if __name__ == "__main__":
    main()
