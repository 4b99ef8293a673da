#!/usr/bin/env python3
"""kAverage (the evaluation averaged over the eight board symmetries) through the Network facade, one process:
NetworkOptions::device_ensemble off (eight evaluations in a row) against on (one ensemble request, the symmetries expanded on
the device; HipForwardPipe ensemble=2), on a latency pipe and on a default pipe.

net_20b256, one 19x19 position of tests/golden/go_games.npz, cache off; off / on interleaved, --warmup calls each, then
--rounds rounds of --iters calls per setting; the MEDIAN of the rounds' wall time per call is reported.  Only the same-process
ratios count (boxes differ by a few percent).  Prints ONE JSON object.

    python tools/ensemble_bench.py > profiles/r08_ensemble.json
"""
import argparse
import json
import os
import socket
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from go_replay import GAME_CONFIGS  # noqa: E402
from sayuri_amd import search as S  # noqa: E402
from sayuri_amd import weights as W  # noqa: E402
from sayuri_amd.engine import Game  # noqa: E402
from sayuri_amd.pipe import HipForwardPipe  # noqa: E402

K_AVERAGE = 2


def position(step):
    """Game 0 of the golden file (19x19) after `step` recorded operations."""
    cfg = GAME_CONFIGS[0]
    moves = np.load(os.path.join(ROOT, "tests", "golden", "go_games.npz"))["g0_moves"]
    g = Game(cfg["board"], cfg["komi"], cfg["scoring"])
    for op, move in moves[:step]:
        if int(op) == 0:
            g.play(int(move))
        elif int(op) == 1:
            g.undo()
        else:
            g.set_territory_helper_from_ownership()
    return g


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=100, help="timed calls per round and setting")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--step", type=int, default=120, help="operations of the golden game played before the position is taken")
    args = ap.parse_args()
    path = f"/tmp/sayuri_bench_20b256_seed22_{os.getuid()}.bin"
    if not os.path.exists(path):
        W.write_weights(path, W.spec_20b256(), seed=22)
    try:
        commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip()
    except OSError:
        commit = ""
    game = position(args.step)
    out = {"tool": "tools/ensemble_bench.py", "box": socket.gethostname(), "commit": commit or "unknown", "net": "20b256", "board": 19,
           "position": f"golden game 0 after {args.step} operations", "iters": args.iters, "rounds": args.rounds, "warmup": args.warmup,
           "statistic": "median of rounds, wall ms per kAverage call", "pipes": {}}
    for kind in ("latency", "default"):
        pipe = HipForwardPipe(path, board_size=19, batch_size=16, fp16=True, waittime_ms=0, latency=kind == "latency", ensemble=2)
        try:
            nets = {k: S.Network(pipe=pipe, options=dict(device_ensemble=(k == "on"), no_cache=True)) for k in ("off", "on")}
            ref = {k: n.output(game, ensemble=K_AVERAGE) for k, n in nets.items()}
            ms = {k: [] for k in nets}
            for r in range(-1, args.rounds):  # round -1: the warm-up
                for k, net in nets.items():
                    it = args.warmup if r < 0 else args.iters
                    t0 = time.perf_counter()
                    for _ in range(it):
                        net.output(game, ensemble=K_AVERAGE)
                    if r >= 0:
                        ms[k].append((time.perf_counter() - t0) * 1e3 / it)
            off, on = float(np.median(ms["off"])), float(np.median(ms["on"]))
            out["pipes"][kind] = {"off_ms": round(off, 4), "on_ms": round(on, 4), "ratio": round(on / off, 4),
                                  "same_bits": bool(np.array_equal(ref["on"].view(np.uint32), ref["off"].view(np.uint32))),
                                  "fallbacks": pipe.ensemble_fallbacks()}
            for n in nets.values():
                n.close()
        finally:
            pipe.Destroy()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
