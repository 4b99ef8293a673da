#!/usr/bin/env python3
"""The tower's 1x1 convolutions on conv_pw.h against the generic kernel (SAYURI_PW=0), in one process.

Synthetic networks written with weights.write_weights: 10 nested-bottleneck blocks at 256 / 128 and at 384 / 192 channels (outer /
inner), and 10 mixer blocks at 256 channels (feed-forward 384).  Per network and point -- default contexts at 1 to 256 boards of
19x19, latency contexts at 1 to 32 boards of 19x19 and one board of 9x9 -- three contexts, interleaved:
  pw0        SAYURI_PW=0: every 1x1 layer on the generic kernel (the code before conv_pw.h)
  pw0_again  the same once more: its ratio to pw0 (`spread`) is what the method cannot tell apart
  pw         the default: conv_pw.h where the engine's speed rule routes it (engine_plan.h, pw_pays)
  pw_all     SAYURI_PW=1: conv_pw.h wherever it applies, the rule not asked -- the rows that show where the rule's boundary belongs
device_ms is the device time per forward, inputs resident (sayuri_hip_time_runs): --warmup forwards, then --rounds rounds of --iters
per context, the MEDIAN of the rounds.  ratio = pw / pw0 and all_ratio = pw_all / pw0; `wins` says whether 1 - ratio exceeds the
spread.  pw_launches / all_launches are sayuri_hip_last_pw_launches of the two arms: 0 where the generic kernel ran.  --pieces a,b
adds an arm per forced SAYURI_PW_PIECES, under SAYURI_PW=1.  Prints ONE JSON object.

    python tools/pw_bench.py > profiles/r12_pw_conv.json
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


def nested(channels, inner):
    return W.NetSpec(channels, [W.BlockSpec("NestedBottleneckBlock", se=(i % 3 == 2), bottleneck_channels=inner) for i in range(10)], 32, 32)


def mixer(channels, ffn):
    return W.NetSpec(channels, [W.BlockSpec("MixerBlock", se=(i % 3 == 2), ffn_channels=ffn) for i in range(10)], 32, 32)


NETS = {"nested10_256_128": (lambda: nested(256, 128), 41), "nested10_384_192": (lambda: nested(384, 192), 42), "mixer10_256": (lambda: mixer(256, 384), 43)}
POINTS = ([("default", n, 19) for n in (1, 16, 32, 64, 128, 256)] + [("latency", n, 19) for n in (1, 2, 4, 8, 16, 32)] +
          [("latency", 1, 9)])


def weights_path(net):
    spec, seed = NETS[net]
    path = f"/tmp/sayuri_bench_{net}_seed{seed}_{os.getuid()}.bin"
    if not os.path.exists(path):
        W.write_weights(path, spec(), seed=seed)
    return path


def pipe_under(path, env, latency, batch):
    keep = {k: os.environ.pop(k, None) for k in ("SAYURI_PW", "SAYURI_PW_PIECES")}
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nets", default=",".join(NETS))
    ap.add_argument("--iters", type=int, default=200, help="timed forwards per round and context")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--pieces", default="", help="also time contexts with these forced SAYURI_PW_PIECES (e.g. 1,2,4)")
    args = ap.parse_args()
    lib = _lib.hip()
    try:
        commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip()
    except OSError:
        commit = ""
    out = {"tool": "tools/pw_bench.py", "box": socket.gethostname(), "commit": commit or "unknown", "iters": args.iters, "rounds": args.rounds,
           "warmup": args.warmup, "statistic": "median of rounds", "nets": {}}
    arms = [("pw0", {"SAYURI_PW": "0"}), ("pw0_again", {"SAYURI_PW": "0"}), ("pw", {}), ("pw_all", {"SAYURI_PW": "1"})]
    arms += [(f"pw_pieces{p}", {"SAYURI_PW": "1", "SAYURI_PW_PIECES": p}) for p in args.pieces.split(",") if p]
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
                       "pw_launches": int(lib.sayuri_hip_last_pw_launches(pipes["pw"].ctx(0))),
                       "all_launches": int(lib.sayuri_hip_last_pw_launches(pipes["pw_all"].ctx(0))),
                       "spread": round(abs(med["pw0_again"] / med["pw0"] - 1.0), 4), "ratio": round(med["pw"] / med["pw0"], 4),
                       "all_ratio": round(med["pw_all"] / med["pw0"], 4)}
                row["wins"] = bool(1.0 - row["ratio"] > row["spread"])
                for k in med:
                    if k.startswith("pw_pieces"):
                        row[f"{k}_ratio"] = round(med[k] / med["pw0"], 4)
                rows.append(row)
            finally:
                for p in pipes.values():
                    p.Destroy()
        out["nets"][net] = rows
    print(json.dumps(out))


if __name__ == "__main__":
    main()
