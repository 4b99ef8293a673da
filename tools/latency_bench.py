#!/usr/bin/env python3
"""Small batches: a default context against a latency context (include/sayuri_hip.h, SAYURI_HIP_LATENCY), in one process.

For n in {1, 2, 4, 8, 16, 32, 64} boards of 19x19, and one board of 9x9 and of 13x13, on 20b x 256 and 40b x 384:
  device_ms  device time per forward, inputs resident (sayuri_hip_time_runs)
  rt_ms      wall time of one sayuri_hip_submit_packed / sayuri_hip_wait round trip (packed records in pinned memory)
each for both contexts, interleaved default / latency / default / latency; a point is --warmup forwards, then --rounds rounds
of --iters timed ones per context, and the MEDIAN of the rounds is reported.  Only the same-process ratios count (boxes differ
by a few percent).  At n = 1 of 19x19 the per-kernel-class device time of one forward (events around every launch) shows
where a latency context's time goes: heads and pack_input stay one workgroup per sample.

--mode default measures the default context alone: it uses nothing newer than the first ABI, so it runs on older trees.
--se-one measures two LATENCY contexts against each other instead: the SE unit as one launch (`latency`, se_unit_kernel, the
default) and as se_pool / se_fc / se_scale (`latency_se_three`, SAYURI_SE_ONE=0), interleaved in the same way, with
se_one_device_ratio / se_one_rt_ratio = one / three per point and the per-kernel-class rows of a lone board for both.
--ring measures the weight ring of the split convolutions in the same way: `latency` (the engine's rule, split_ring) against
`latency_ring3` (SAYURI_LATENCY_RING=3, the three-stage kernel everywhere) with ring_device_ratio / ring_rt_ratio = rule / three,
and a second =3 context, `latency_ring3_again`, whose ratio to the first (same_config_device_ratio) is the spread of the method:
a depth belongs in the rule only where its ratio is below 1 by more than that.  --ring-depths 8,5 adds a context per forced
depth, timed at the points whose strips have a variant of that depth (sayuri_hip_split_ring_plan says).  Every arm's point names the ring that ran (sayuri_hip_last_split_ring).
Prints ONE JSON object.

    python tools/latency_bench.py > profiles/r07_latency_small_batch.json
    python tools/latency_bench.py --se-one > profiles/r10_latency_se_one.json
    python tools/latency_bench.py --ring --ring-depths 8 > profiles/r11_latency_ring.json
"""
import argparse
import json
import os
import time

import numpy as np

import _ab
from _ab import B, W, _lib, device_ms
from sayuri_amd import hipraw
from sayuri_amd.engine import pack_planes

WORDS = 37 * 12 + 8
NETS = {"20b256": (W.spec_20b256, 22), "40b384": (W.spec_40b384, 23)}
POINTS = [(n, 19) for n in (1, 2, 4, 8, 16, 32, 64)] + [(1, 9), (1, 13)]
SMALL_POINTS = [(16, 9)]  # --se-one, --ring: also a batch of small boards


def round_trips(ctx, stage, n, iters):
    """-> wall ms per submit_packed / wait round trip of the set's first n records."""
    t0 = time.perf_counter()
    for _ in range(iters):
        hipraw.wait(ctx, hipraw.submit_packed(ctx, stage, n, 37))
    return (time.perf_counter() - t0) * 1e3 / iters


def kernel_classes(lib, ctx):
    rows = (_lib.KernelStat * 64)()
    k = lib.sayuri_hip_profile_run(ctx, rows, 64)
    if k < 0:
        raise RuntimeError(lib.sayuri_hip_last_error().decode())
    return {rows[i].name.decode(): {"launches": rows[i].launches, "ms": round(rows[i].total_ms, 5)} for i in range(k)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=["both", "default"], default="both")
    ap.add_argument("--nets", default="20b256,40b384")
    _ab.timing_args(ap)
    ap.add_argument("--split", default="", help="also time latency contexts with these forced strips per board at n = 1 (e.g. 4,7,10)")
    ap.add_argument("--se-one", action="store_true", help="two latency contexts: one launch per SE unit against SAYURI_SE_ONE=0")
    ap.add_argument("--ring", action="store_true", help="latency contexts: the ring rule against SAYURI_LATENCY_RING=3, and =3 against =3")
    ap.add_argument("--ring-depths", default="", help="--ring: also time latency contexts with these forced weight stages where the batch has such a variant (e.g. 8)")
    args = ap.parse_args()
    if args.ring and args.se_one:
        ap.error("--ring and --se-one are two measurements")
    lib = _lib.hip()
    out = _ab.header("tools/latency_bench.py", args, mode=args.mode)
    kinds = [] if args.se_one or args.ring else ["default"] + (["latency"] if args.mode == "both" else [])
    if args.ring:
        out["ring"] = True
        os.environ.pop("SAYURI_LATENCY_RING", None)  # the arms say which ring they run
    if args.se_one:
        out["se_one"] = True
        os.environ.pop("SAYURI_SE_ONE", None)  # the two arms say which form they run
    for net in args.nets.split(","):
        path = _ab.weights_path(NETS, net)
        channels = int(net.split("b")[1])
        make = lambda env=None, latency=True: _ab.pipe_under(tuple(env or ()), path, env or {}, latency, 64)  # noqa: E731
        pipes = {k: make(latency=k == "latency") for k in kinds}
        if args.se_one:
            pipes["latency"] = make()
            pipes["latency_se_three"] = make({"SAYURI_SE_ONE": "0"})
        if args.ring:
            pipes["latency"] = make()
            for k, depth in [("latency_ring3", 3), ("latency_ring3_again", 3)] + [(f"latency_forced_ring{d}", int(d)) for d in args.ring_depths.split(",") if d]:
                pipes[k] = make({"SAYURI_LATENCY_RING": str(depth)})
        for s in (int(x) for x in args.split.split(",") if x and args.mode == "both" and not args.se_one and not args.ring):
            pipes[f"latency_split{s}"] = make({"SAYURI_LATENCY_SPLIT": str(s)})
        stage = hipraw.PinnedSet(64, B, WORDS)
        res = {"points": [], "tower_state": {k: lib.sayuri_hip_tower_state(p.ctx(0)) for k, p in pipes.items()}}
        try:
            for n, bs in POINTS + (SMALL_POINTS if args.se_one or args.ring else []):
                planes, grid, bsz = _ab.boards(n, bs)
                stage.records[:n * WORDS] = np.stack([pack_planes(p, 37) for p in planes]).astype(np.uint32).ravel()
                stage.bsz[:n] = bsz
                use = {k: p for k, p in pipes.items() if n == 1 or "split" not in k}
                for k in [k for k in use if "forced_ring" in k]:  # a forced depth only where this batch's variant has it
                    depth = int(k.rsplit("ring", 1)[1])
                    if lib.sayuri_hip_split_ring_plan(n, _lib.ip(bsz), B, channels, 0, depth) != depth:
                        del use[k]
                dev = {k: [] for k in use}
                rt = {k: [] for k in use}
                for r in range(-1, args.rounds):  # round -1: the warm-up
                    for k, p in use.items():
                        ctx = p.ctx(0)
                        _ab.check(lib, lib.sayuri_hip_upload(ctx, n, _lib.fp(grid), _lib.ip(bsz)))
                        it = args.warmup if r < 0 else args.iters
                        d, w = device_ms(lib, ctx, it), round_trips(ctx, stage, n, it)
                        if r >= 0:
                            dev[k].append(d)
                            rt[k].append(w)
                pt = {"n": n, "board": bs}
                for k in use:
                    pt[k] = {"device_ms": round(float(np.median(dev[k])), 5), "rt_ms": round(float(np.median(rt[k])), 5)}
                if args.ring:
                    three = pt["latency_ring3"]
                    for k, p in use.items():
                        pt[k]["ring"] = int(lib.sayuri_hip_last_split_ring(p.ctx(0)))
                        if k != "latency_ring3":
                            tag = {"latency": "ring", "latency_ring3_again": "same_config"}.get(k, k[len("latency_"):])
                            pt[f"{tag}_device_ratio"] = round(pt[k]["device_ms"] / three["device_ms"], 4)
                            pt[f"{tag}_rt_ratio"] = round(pt[k]["rt_ms"] / three["rt_ms"], 4)
                elif args.se_one:
                    pt["se_one_device_ratio"] = round(pt["latency"]["device_ms"] / pt["latency_se_three"]["device_ms"], 4)
                    pt["se_one_rt_ratio"] = round(pt["latency"]["rt_ms"] / pt["latency_se_three"]["rt_ms"], 4)
                elif "latency" in use:
                    pt["device_ratio"] = round(pt["latency"]["device_ms"] / pt["default"]["device_ms"], 4)
                    pt["rt_ratio"] = round(pt["latency"]["rt_ms"] / pt["default"]["rt_ms"], 4)
                if n == 1 and bs == 19:
                    for k, p in use.items():
                        if "split" in k or "forced" in k or "again" in k:
                            continue
                        lib.sayuri_hip_upload(p.ctx(0), n, _lib.fp(grid), _lib.ip(bsz))
                        pt[k]["kernel_classes_one_forward"] = kernel_classes(lib, p.ctx(0))
                res["points"].append(pt)
        finally:
            stage.close()
            for p in pipes.values():
                p.Destroy()
        if args.mode == "both" and not args.se_one and not args.ring:
            # the batch size of 19x19 boards from which the default context's device time is the smaller one
            cross = [pt["n"] for pt in res["points"] if pt["board"] == 19 and pt["device_ratio"] > 1.0]
            res["default_wins_from_n"] = min(cross) if cross else None
        out["nets"][net] = res
    print(json.dumps(out))


if __name__ == "__main__":
    main()
