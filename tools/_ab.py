"""What the same-process A/B tools share (pw_bench.py, dw_bench.py, latency_bench.py): synthetic weights written once, a context
created under exactly the switches of its arm, device time per forward with the inputs resident, the interleaved loop (a warm-up
round, then --rounds rounds of --iters per arm, the MEDIAN of the rounds) and -- feature_ab -- the whole program of a tool that
measures a kernel family against the kernel before it: a table of networks, points and arms goes in, ONE JSON object comes out."""
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


def weights_path(nets, net):
    """the weights of nets[net] = (spec, seed), written once per user"""
    spec, seed = nets[net]
    path = f"/tmp/sayuri_bench_{net}_seed{seed}_{os.getuid()}.bin"
    if not os.path.exists(path):
        W.write_weights(path, spec(), seed=seed)
    return path


def pipe_under(switches, path, env, latency, batch):
    """a context created with exactly these switches set as `env` says; they are put back afterwards"""
    keep = {k: os.environ.pop(k, None) for k in switches}
    os.environ.update(env)
    try:
        return HipForwardPipe(path, board_size=B, batch_size=batch, fp16=True, **({"latency": True} if latency else {}))
    finally:
        for k, v in keep.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


def check(lib, rc):
    if rc:
        raise RuntimeError(lib.sayuri_hip_last_error().decode())


def device_ms(lib, ctx, iters):
    ms = ctypes.c_float(0)
    check(lib, lib.sayuri_hip_time_runs(ctx, iters, ctypes.byref(ms)))
    return ms.value / iters


def timing_args(ap):
    ap.add_argument("--iters", type=int, default=200, help="timed forwards per round and context")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=30)


def header(tool, args, **more):
    try:
        commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip()
    except OSError:
        commit = ""
    return {"tool": tool, "box": socket.gethostname(), "commit": commit or "unknown", **more, "iters": args.iters, "rounds": args.rounds,
            "warmup": args.warmup, "statistic": "median of rounds", "nets": {}}


def boards(n, bs):
    """n synthetic positions on bs x bs boards -> (planes, planes on the NN grid, board sizes)"""
    planes = W.synthetic_planes(n, [bs] * n, seed=100 + n)
    grid = np.zeros((n, 43, B * B), np.float32)
    for i, p in enumerate(planes):
        grid[i].reshape(43, B, B)[:, :bs, :bs] = p.reshape(43, bs, bs)
    return planes, grid, np.full(n, bs, np.int32)


def interleaved(lib, pipes, n, grid, bsz, args):
    """-> {arm: median device ms per forward}; the inputs are uploaded once, in the warm-up round"""
    dev = {k: [] for k in pipes}
    for r in range(-1, args.rounds):  # round -1: the warm-up
        for k, p in pipes.items():
            if r < 0:
                check(lib, lib.sayuri_hip_upload(p.ctx(0), n, _lib.fp(grid), _lib.ip(bsz)))
            d = device_ms(lib, p.ctx(0), args.warmup if r < 0 else args.iters)
            if r >= 0:
                dev[k].append(d)
    return {k: float(np.median(v)) for k, v in dev.items()}


def feature_ab(tool, nets, points, name, cut, more_args=None, more_row=None):
    """The program of pw_bench.py / dw_bench.py.  name = "pw" | "dw": the switch SAYURI_<NAME> (0: the old kernel, 1: the new one
    wherever it applies), the arms <name>0, <name>0_again, <name>, <name>_all, the counter sayuri_hip_last_<name>_launches; cut =
    "pieces" | "strips": --<cut> a,b adds an arm per forced SAYURI_<NAME>_<CUT> under SAYURI_<NAME>=1.  points: (context kind, boards,
    board size).  more_args(ap) / more_row(row, kind, n, pipes, args, lib): a tool's own options and row fields."""
    switch, cut_switch = f"SAYURI_{name.upper()}", f"SAYURI_{name.upper()}_{cut.upper()}"
    ap = argparse.ArgumentParser()
    ap.add_argument("--nets", default=",".join(nets))
    timing_args(ap)
    ap.add_argument(f"--{cut}", default="", help=f"also time contexts with these forced {cut_switch} (e.g. 1,2,4)")
    if more_args:
        more_args(ap)
    args = ap.parse_args()
    lib = _lib.hip()
    launches = getattr(lib, f"sayuri_hip_last_{name}_launches")
    out = header(tool, args)
    arms = [(f"{name}0", {switch: "0"}), (f"{name}0_again", {switch: "0"}), (name, {}), (f"{name}_all", {switch: "1"})]
    arms += [(f"{name}_{cut}{c}", {switch: "1", cut_switch: c}) for c in getattr(args, cut).split(",") if c]
    for net in args.nets.split(","):
        path = weights_path(nets, net)
        rows = []
        for kind, n, bs in points:
            pipes = {k: pipe_under((switch, cut_switch), path, env, kind == "latency", max(n, 16)) for k, env in arms}
            try:
                _, grid, bsz = boards(n, bs)
                med = interleaved(lib, pipes, n, grid, bsz, args)
                base = med[f"{name}0"]
                row = {"context": kind, "n": n, "board": bs, "device_ms": {k: round(v, 5) for k, v in med.items()},
                       f"{name}_launches": int(launches(pipes[name].ctx(0))), "all_launches": int(launches(pipes[f"{name}_all"].ctx(0))),
                       "spread": round(abs(med[f"{name}0_again"] / base - 1.0), 4), "ratio": round(med[name] / base, 4),
                       "all_ratio": round(med[f"{name}_all"] / base, 4)}
                row["wins"] = bool(1.0 - row["ratio"] > row["spread"])
                for k in med:
                    if k.startswith(f"{name}_{cut}"):
                        row[f"{k}_ratio"] = round(med[k] / base, 4)
                if more_row:
                    more_row(row, kind, n, pipes, args, lib)
                rows.append(row)
            finally:
                for p in pipes.values():
                    p.Destroy()
        out["nets"][net] = rows
    print(json.dumps(out))
