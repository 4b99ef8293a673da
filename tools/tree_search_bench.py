#!/usr/bin/env python3
"""One tree searched with K playouts in flight (option playouts_in_flight; csrc/engine/search.h), one process: K = 1 (one
playout at a time, a device batch of one per leaf) against K = 2, 4, 8, 16 (rounds: the leaves of up to K descents as ONE
group request, one device batch).

net_20b256 on a latency pipe (batch 16), one mid-game 19x19 position of tests/golden/go_games.npz, cache off, --playouts
playouts per search from a fresh tree.  The settings are interleaved; the MEDIAN of --rounds searches is reported per K:
playouts per second, leaves per round, collisions, and where a round's wall time went (host collect: descents and encoding;
evaluate: the group's round trip and its post-processing; apply: children and back-up).  Only the same-process ratios count
(boxes differ by a few percent).  Prints ONE JSON object.

    python tools/tree_search_bench.py > profiles/r09_tree_batch.json
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
    ap.add_argument("--playouts", type=int, default=400)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--flights", type=int, nargs="+", default=[1, 2, 4, 8, 16])
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
    out = {"tool": "tools/tree_search_bench.py", "box": socket.gethostname(), "commit": commit or "unknown", "net": "20b256", "board": 19,
           "position": f"golden game 0 after {args.step} operations", "pipe": "latency, batch 16, waittime 0", "playouts": args.playouts,
           "rounds": args.rounds, "statistic": "median of rounds", "flights": {}}
    pipe = HipForwardPipe(path, board_size=19, batch_size=16, fp16=True, waittime_ms=0, latency=True)
    try:
        net = S.Network(pipe=pipe, options=dict(no_cache=True))
        rows = {k: [] for k in args.flights}
        for r in range(-1, args.rounds):  # round -1: the warm-up
            for k in args.flights:
                search = S.Search(game, net, dict(playouts=args.playouts, playouts_in_flight=k), seeds=(5, 6))
                before = pipe.pump_times()
                t0 = time.perf_counter()
                res = search.computation(args.playouts if r >= 0 else max(16, args.playouts // 4))
                took = time.perf_counter() - t0
                after = pipe.pump_times()
                st, sec = search.flight_stats(), search.round_seconds()
                search.close()
                if r < 0:
                    continue
                rounds = max(1, st["rounds"])
                rows[k].append({"playouts_per_s": res["playouts"] / took, "ms_per_playout": took * 1e3 / res["playouts"],
                                "leaves_per_round": st["leaves"] / rounds if k > 1 else 1.0, "collisions": st["collisions"],
                                "batches": after["batches"] - before["batches"], "evals": after["evals"] - before["evals"],
                                "round_ms_collect": sec["collect"] * 1e3 / rounds, "round_ms_evaluate": sec["evaluate"] * 1e3 / rounds,
                                "round_ms_apply": sec["apply"] * 1e3 / rounds})
        for k, rs in rows.items():
            out["flights"][str(k)] = {f: round(float(np.median([x[f] for x in rs])), 4) for f in rs[0]}
        base = out["flights"].get("1")
        if base:
            for k, row in out["flights"].items():
                row["speedup_vs_1"] = round(row["playouts_per_s"] / base["playouts_per_s"], 3)
        net.close()
    finally:
        pipe.Destroy()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
