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
import numpy as np

import _ab
from _ab import W, _lib

def mixer(channels, ffn):
    return W.NetSpec(channels, [W.BlockSpec("MixerBlock", se=(i % 3 == 2), ffn_channels=ffn) for i in range(10)], 32, 32)


def replk(channels):
    return W.NetSpec(channels, [W.BlockSpec("ResidualBlock", se=(i % 3 == 2)) for i in range(10)], 32, 32, policy_head="RepLK")


NETS = {"mixer10_256": (lambda: mixer(256, 384), 43), "res10_256_replk": (lambda: replk(256), 44)}
POINTS = [("default", n, 19) for n in (1, 16, 32, 64, 128, 256)] + [("latency", n, 19) for n in (1, 8, 32)] + [("latency", 1, 9)]


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


def more_args(ap):
    ap.add_argument("--kernel-points", default="32,256", help="boards of the default contexts whose depthwise row is profiled")
    ap.add_argument("--profile-runs", type=int, default=9)


def more_row(row, kind, n, pipes, args, lib):
    if kind == "default" and n in {int(k) for k in args.kernel_points.split(",") if k}:
        row["depthwise_us"] = {"depthwise_kernel": depthwise_row(lib, pipes["dw0"].ctx(0), args.profile_runs),
                               "conv_dw_kernel": depthwise_row(lib, pipes["dw_all"].ctx(0), args.profile_runs)}


if __name__ == "__main__":
    _ab.feature_ab("tools/dw_bench.py", NETS, POINTS, "dw", "strips", more_args, more_row)
