#!/usr/bin/env python3
"""The depthwise convolutions on conv_dw.h against depthwise_kernel (SAYURI_DW=0), in one process.

Synthetic networks written with weights.write_weights: 10 mixer blocks at 256 channels (feed-forward 384, 7x7 depthwise) and 10
residual blocks at 256 channels with a RepLK policy head (one 7x7 depthwise layer on the policy channels).  Per network and point --
default contexts at 1 to 256 boards of 19x19, latency contexts at 1, 8 and 32 boards of 19x19 and one board of 9x9 -- four
contexts, interleaved:
  dw0        SAYURI_DW=0: every depthwise layer on depthwise_kernel (the code before conv_dw.h)
  dw0_again  the same once more: its ratio to dw0 (`spread`) is what the method cannot tell apart
  dw         the default: conv_dw.h where the engine's speed rule routes it (engine_plan.h, dw_pays)
  dw_all     SAYURI_DW=1: conv_dw.h wherever it applies, the rule not asked -- the rows that show where the rule's boundary belongs
device_ms is the device time per forward, inputs resident (sayuri_hip_time_runs): --warmup forwards, then --rounds rounds of --iters
per context, the MEDIAN of the rounds.  ratio = dw / dw0 and all_ratio = dw_all / dw0; `wins` says whether 1 - ratio exceeds the
spread.  dw_launches / all_launches are sayuri_hip_last_dw_launches of the two arms: 0 where depthwise_kernel ran.  --strips a,b
adds an arm per forced SAYURI_DW_STRIPS, under SAYURI_DW=1.
At the --kernel-points (32 and 256 boards, default contexts) `depthwise_us` is the device time PER LAUNCH of the `depthwise` row of
sayuri_hip_profile_run (events around every launch of one forward), the median of --profile-runs forwards, for dw0 (depthwise_kernel)
and dw_all (conv_dw_kernel), with the row's algorithmic bytes per launch over that time.  Prints ONE JSON object.

    python tools/dw_bench.py > profiles/r13_dw_conv.json
"""
import argparse
import ctypes
import json
import os
import socket
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from sayuri_amd import _lib  # noqa: E402
from sayuri_amd import weights as W  # noqa: E402
from sayuri_amd.pipe import HipForwardPipe  # noqa: E402

B = 19
SWITCHES = ("SAYURI_DW", "SAYURI_DW_STRIPS")


def mixer(channels, ffn):
    return W.NetSpec(channels, [W.BlockSpec("MixerBlock", se=(i % 3 == 2), ffn_channels=ffn) for i in range(10)], 32, 32)


def replk(channels):
    return W.NetSpec(channels, [W.BlockSpec("ResidualBlock", se=(i % 3 == 2)) for i in range(10)], 32, 32, policy_head="RepLK")


NETS = {"mixer10_256": (lambda: mixer(256, 384), 43), "res10_256_replk": (lambda: replk(256), 44)}
POINTS = [("default", n, 19) for n in (1, 16, 32, 64, 128, 256)] + [("latency", n, 19) for n in (1, 8, 32)] + [("latency", 1, 9)]


def weights_path(net):
    spec, seed = NETS[net]
    path = f"/tmp/sayuri_bench_{net}_seed{seed}_{os.getuid()}.bin"
    if not os.path.exists(path):
        W.write_weights(path, spec(), seed=seed)
    return path


def pipe_under(path, env, latency, batch):
    keep = {k: os.environ.pop(k, None) for k in SWITCHES}
    os.environ.update(env)
    try:
        return HipForwardPipe(path, board_size=B, batch_size=batch, fp16=True, **({"latency": True} if latency else {}))
    finally:
        for k, v in keep.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


def device_ms(lib, ctx, iters):
    ms = ctypes.c_float(0)
    if lib.sayuri_hip_time_runs(ctx, iters, ctypes.byref(ms)):
        raise RuntimeError(lib.sayuri_hip_last_error().decode())
    return ms.value / iters


def depthwise_row(lib, ctx, runs):
    """-> {launches, us per launch (median of `runs` profiled forwards), GB/s of the row's algorithmic bytes} of the `depthwise` row"""
    rows = (_lib.KernelStat * 64)()
    per, launches, nbytes = [], 0, 0.0
    for _ in range(runs):
        k = lib.sayuri_hip_profile_run(ctx, rows, 64)
        if k < 0:
            raise RuntimeError(lib.sayuri_hip_last_error().decode())
        for i in range(k):
            if rows[i].name.decode() == "depthwise":
                launches, nbytes = rows[i].launches, rows[i].bytes
                per.append(rows[i].total_ms * 1e3 / rows[i].launches)
    us = float(np.median(per))
    return {"launches": int(launches), "us_per_launch": round(us, 2), "algorithmic_gb_per_s": round(nbytes / launches / us / 1e3, 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nets", default=",".join(NETS))
    ap.add_argument("--iters", type=int, default=200, help="timed forwards per round and context")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--strips", default="", help="also time contexts with these forced SAYURI_DW_STRIPS (e.g. 1,2,4)")
    ap.add_argument("--kernel-points", default="32,256", help="boards of the default contexts whose depthwise row is profiled")
    ap.add_argument("--profile-runs", type=int, default=9)
    args = ap.parse_args()
    lib = _lib.hip()
    try:
        commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip()
    except OSError:
        commit = ""
    out = {"tool": "tools/dw_bench.py", "box": socket.gethostname(), "commit": commit or "unknown", "iters": args.iters, "rounds": args.rounds,
           "warmup": args.warmup, "statistic": "median of rounds", "nets": {}}
    arms = [("dw0", {"SAYURI_DW": "0"}), ("dw0_again", {"SAYURI_DW": "0"}), ("dw", {}), ("dw_all", {"SAYURI_DW": "1"})]
    arms += [(f"dw_strips{s}", {"SAYURI_DW": "1", "SAYURI_DW_STRIPS": s}) for s in args.strips.split(",") if s]
    kernel_points = {int(n) for n in args.kernel_points.split(",") if n}
    for net in args.nets.split(","):
        path = weights_path(net)
        rows = []
        for kind, n, bs in POINTS:
            pipes = {k: pipe_under(path, env, kind == "latency", max(n, 16)) for k, env in arms}
            try:
                planes = W.synthetic_planes(n, [bs] * n, seed=100 + n)
                grid = np.zeros((n, 43, B * B), np.float32)
                for i, p in enumerate(planes):
                    grid[i].reshape(43, B, B)[:, :bs, :bs] = p.reshape(43, bs, bs)
                bsz = np.full(n, bs, np.int32)
                dev = {k: [] for k in pipes}
                for r in range(-1, args.rounds):  # round -1: the warm-up
                    for k, p in pipes.items():
                        if r < 0 and lib.sayuri_hip_upload(p.ctx(0), n, _lib.fp(grid), _lib.ip(bsz)):
                            raise RuntimeError(lib.sayuri_hip_last_error().decode())
                        d = device_ms(lib, p.ctx(0), args.warmup if r < 0 else args.iters)
                        if r >= 0:
                            dev[k].append(d)
                med = {k: float(np.median(v)) for k, v in dev.items()}
                row = {"context": kind, "n": n, "board": bs, "device_ms": {k: round(v, 5) for k, v in med.items()},
                       "dw_launches": int(lib.sayuri_hip_last_dw_launches(pipes["dw"].ctx(0))),
                       "all_launches": int(lib.sayuri_hip_last_dw_launches(pipes["dw_all"].ctx(0))),
                       "spread": round(abs(med["dw0_again"] / med["dw0"] - 1.0), 4), "ratio": round(med["dw"] / med["dw0"], 4),
                       "all_ratio": round(med["dw_all"] / med["dw0"], 4)}
                row["wins"] = bool(1.0 - row["ratio"] > row["spread"])
                for k in med:
                    if k.startswith("dw_strips"):
                        row[f"{k}_ratio"] = round(med[k] / med["dw0"], 4)
                if kind == "default" and n in kernel_points:
                    row["depthwise_us"] = {"depthwise_kernel": depthwise_row(lib, pipes["dw0"].ctx(0), args.profile_runs),
                                           "conv_dw_kernel": depthwise_row(lib, pipes["dw_all"].ctx(0), args.profile_runs)}
                rows.append(row)
            finally:
                for p in pipes.values():
                    p.Destroy()
        out["nets"][net] = rows
    print(json.dumps(out))


if __name__ == "__main__":
    main()
