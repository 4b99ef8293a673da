#!/usr/bin/env python3
"""What a weights roll-over costs a self-play rank, with and without live reload (option live_weights).

    python tools/rollover_bench.py [--arm a|b|both] [--appear 120] [--window 600] [--games 512] [--playouts 400] [--net 20b256]
                                   [--out profiles/r14_live_weights.json]

One GPU, the settings of tools/selfplay_bench.py (19x19, random-init weights).  Self-play starts on network A; `--appear` seconds
into the run a second file of the same architecture is renamed into the weights directory.  Two arms:
  a  live_weights=0: the rank winds down as the reference does (games in flight + 25, rounded up to 25), its process exits, and this
     tool starts the next one on the newest file, as bash/selfplay-worker.sh's loop does;
  b  live_weights=1: the file goes into the running pipe.
Every self-play process is a child of this tool (a restart is a fresh process, never a replaced one).  A child samples its own
counters: the stats hook every 0.25 s, and a thread every millisecond the pipe's finished-batch counter (for the longest gap
between two finished batches) and every 5 ms sayuri_hip_device_bytes.  Reported per arm, over the `--window` seconds after the file
appeared: NN evals/s (positions the device evaluated), finished games, whether arm a was still winding down at the end, the longest
batch gap within 5 s of the commit (arm b) and over the window, the peak of device_bytes.  `--reload-time` measures the host time of
one HipForwardPipe::Reload (parse; begin + tensors + prepare + commit) under netbench load on the same network.
"""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys
import tempfile
import threading
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def spec_of(net):
    from sayuri_amd import weights as W
    return {"20b256": W.spec_20b256, "6b96": W.spec_6b96, "40b384": W.spec_40b384}[net]()


def newest(wdir):
    files = [os.path.join(wdir, f) for f in os.listdir(wdir)]
    return max(files, key=lambda p: os.stat(p).st_mtime_ns)


def child(args):
    """one self-play process: plays until `--seconds` are over or its games are done (a wind-down); samples into --log"""
    from sayuri_amd import _lib
    from sayuri_amd import search as S
    from sayuri_amd.pipe import HipForwardPipe
    wfile = newest(args.wdir)
    t_start = time.time()
    pipe = HipForwardPipe(wfile, board_size=args.board, batch_size=args.batch)
    ctx, hip = pipe.ctx(0), _lib.hip()
    log = open(args.log, "a")
    emit = lambda **kw: (log.write(json.dumps(kw) + "\n"), log.flush())
    emit(kind="start", t=t_start, ready=time.time(), file=os.path.basename(wfile))
    stop = threading.Event()
    gaps = {"last_batches": 0, "last_t": time.time(), "peak_bytes": 0}

    def sampler():
        k = 0
        while not stop.is_set():
            now = time.time()
            b = pipe.pump_times()["batches"]
            if b != gaps["last_batches"]:
                if gaps["last_batches"] and now - gaps["last_t"] > 0.02:   # every gap above 20 ms is kept with its time
                    emit(kind="gap", t=gaps["last_t"], seconds=now - gaps["last_t"])
                gaps["last_batches"], gaps["last_t"] = b, now
            k += 1
            if k % 5 == 0:
                gaps["peak_bytes"] = max(gaps["peak_bytes"], int(hip.sayuri_hip_device_bytes(ctx)))
            time.sleep(0.001)

    th = threading.Thread(target=sampler, daemon=True)
    th.start()

    def on_stats(st, halt):
        emit(kind="stats", t=time.time(), games_done=st["games_done"], swaps=st["weight_swaps"], evals=pipe.pump_times()["evals"],
             halt=bool(halt), bytes=gaps["peak_bytes"])
        return halt

    out = tempfile.mkdtemp(prefix="sayuri_rollover_chunks_")
    st = S.selfplay(pipe, dict(playouts=args.playouts, parallel_games=args.games, num_games=1000000, seed=args.seed,
                               selfplay_query=[f"bkp:{args.board}:7:1"], live_weights=args.live, weights_dir=args.wdir, weights_file=wfile,
                               target_directory=out, stagger_moves=args.stagger),
                    seconds=args.seconds, on_stats=on_stats, stats_interval=0.25, move_cap=args.move_cap)
    stop.set()
    th.join()
    emit(kind="end", t=time.time(), games_done=st["games_done"], max_games=st["max_games"], swaps=st["weight_swaps"],
         evals=pipe.pump_times()["evals"], bytes=gaps["peak_bytes"], generation=pipe.weights_generation())
    pipe.Destroy()
    import shutil
    shutil.rmtree(out, ignore_errors=True)


def run_arm(args, arm):
    from sayuri_amd import weights as W
    work = tempfile.mkdtemp(prefix=f"sayuri_rollover_{arm}_")
    wdir = os.path.join(work, "weights")
    os.mkdir(wdir)
    spec = spec_of(args.net)
    W.write_weights(os.path.join(wdir, "net-0001.bin"), spec, seed=22)
    W.write_weights(os.path.join(work, "next.tmp"), spec, seed=23)   # written ahead: only the rename falls into the run
    t0 = time.time()
    t_end = t0 + args.appear + args.window
    t_appear = None
    segments = []
    while time.time() < t_end - 1.0:
        log = os.path.join(work, f"segment{len(segments)}.jsonl")
        segments.append(log)
        cmd = [sys.executable, os.path.abspath(__file__), "--child", "--wdir", wdir, "--log", log, "--live", "1" if arm == "b" else "0",
               "--seconds", str(t_end - time.time()), "--games", str(args.games), "--playouts", str(args.playouts), "--board", str(args.board),
               "--batch", str(args.batch), "--seed", str(args.seed + len(segments)), "--stagger", str(args.stagger),
               "--move-cap", str(args.move_cap)]
        p = subprocess.Popen(cmd)
        deadline = t_end + 180.0   # a child ends by itself at t_end and then flushes its writer; one that does not is killed
        while p.poll() is None:
            if time.time() > deadline:
                p.kill()
                p.wait()
                raise RuntimeError(f"arm {arm}: a self-play process was still running {deadline - t_end:.0f} s after the window's end")
            if t_appear is None and time.time() >= t0 + args.appear:
                os.rename(os.path.join(work, "next.tmp"), os.path.join(wdir, "net-0002.bin"))
                t_appear = time.time()
            time.sleep(0.05)
        if p.returncode != 0:
            raise RuntimeError(f"arm {arm}: a self-play process ended with status {p.returncode}")
    return summarise(arm, args, segments, t_appear, t_end)


def summarise(arm, args, segments, t_appear, t_end):
    evals = games = 0
    peak, swaps, gaps, seg_info, swap_seen = 0, 0, [], [], None
    for log in segments:
        rows = [json.loads(l) for l in open(log)]
        stats = [r for r in rows if r["kind"] in ("stats", "end")]
        start = next(r for r in rows if r["kind"] == "start")
        end = next((r for r in rows if r["kind"] == "end"), None)
        # seconds relative to the moment the file appeared; pipe_ready - started = process start-up until the pipe exists
        seg_info.append({"file": start["file"], "started": round(start["t"] - t_appear, 2), "pipe_ready": round(start["ready"] - t_appear, 2),
                         "ended": round(end["t"] - t_appear, 2) if end else None, "max_games": end["max_games"] if end else None})
        inside = [r for r in stats if t_appear <= r["t"] <= t_end]
        before = [r for r in stats if r["t"] < t_appear]
        if inside:
            base = before[-1] if before else {"evals": 0, "games_done": 0}
            evals += inside[-1]["evals"] - base["evals"]
            games += inside[-1]["games_done"] - base["games_done"]
        peak = max([peak] + [r.get("bytes", 0) for r in stats])
        for a, b in zip(stats, stats[1:]):
            if b["swaps"] > a["swaps"] and swap_seen is None:
                swap_seen = b["t"]
        swaps += stats[-1]["swaps"] if stats else 0
        gaps += [r for r in rows if r["kind"] == "gap" and t_appear <= r["t"] <= t_end]
    window = t_end - t_appear
    row = {"arm": arm, "live_weights": 1 if arm == "b" else 0, "window_seconds": round(window, 1), "file_appeared_at_seconds": args.appear,
           "nn_evals_per_second": round(evals / window, 1), "finished_games": games, "processes": seg_info, "weight_swaps": swaps,
           "longest_batch_gap_seconds_in_window": round(max([g["seconds"] for g in gaps] + [0.0]), 4),
           "peak_device_bytes": peak}
    if arm == "a":
        first = seg_info[0]
        row["winding_down_at_window_end"] = first["ended"] is None or first["ended"] >= window - 1.0
    if swap_seen is not None:
        near = [g["seconds"] for g in gaps if abs(g["t"] - swap_seen) <= 5.0]
        row["swap_seen_at_seconds"] = round(swap_seen - t_appear, 2)
        row["longest_batch_gap_seconds_within_5s_of_the_swap"] = round(max(near + [0.0]), 4)
    return row


def reload_time(args):
    """One Reload under netbench load (512 threads blocked in Forward: full batches, as 512 games give them): host seconds of the
    parse alone and of begin + tensors + prepare + commit; the longest gap between two finished batches (sampled every
    millisecond) before the reload, during it, and in the 3 s behind it in which the old set is freed; the peak of device_bytes."""
    from sayuri_amd import _lib
    from sayuri_amd import weights as W
    from sayuri_amd.pipe import HipForwardPipe, Weights
    work = tempfile.mkdtemp(prefix="sayuri_rollover_reload_")
    a, b = os.path.join(work, "a.bin"), os.path.join(work, "b.bin")
    W.write_weights(a, spec_of(args.net), seed=22)
    W.write_weights(b, spec_of(args.net), seed=23)
    pipe = HipForwardPipe(a, board_size=args.board, batch_size=args.batch)
    ctx, hip = pipe.ctx(0), _lib.hip()
    res, marks, stop = {}, [], threading.Event()
    phase = {"name": "before"}
    longest = {"before": 0.0, "reload": 0.0, "after": 0.0}
    peak = {"bytes": 0}

    def sampler():
        last_b, last_t, k = 0, time.perf_counter(), 0
        while not stop.is_set():
            now = time.perf_counter()
            n = pipe.pump_times()["batches"]
            if n != last_b:
                if last_b:
                    longest[phase["name"]] = max(longest[phase["name"]], now - last_t)
                last_b, last_t = n, now
            k += 1
            if k % 5 == 0:
                peak["bytes"] = max(peak["bytes"], int(hip.sayuri_hip_device_bytes(ctx)))
            time.sleep(0.001)

    th = threading.Thread(target=lambda: res.update(netbench=pipe.netbench(512, 12.0, args.board)))
    th.start()
    time.sleep(2.0)   # (the queue has filled)
    sm = threading.Thread(target=sampler, daemon=True)
    sm.start()
    time.sleep(3.0)
    before = int(hip.sayuri_hip_device_bytes(ctx))
    t = time.perf_counter()
    Weights(b).close()
    parse = time.perf_counter() - t
    phase["name"] = "reload"
    t = time.perf_counter()
    pipe.Reload(b)
    total = time.perf_counter() - t
    phase["name"] = "after"
    time.sleep(3.0)
    stop.set()
    sm.join()
    after = int(hip.sayuri_hip_device_bytes(ctx))
    th.join()
    pipe.Destroy()
    return {"net": args.net, "parse_seconds": round(parse, 3), "reload_seconds": round(total, 3),
            "stage_prepare_commit_seconds": round(max(total - parse, 0.0), 3), "netbench_evals_per_second_meanwhile": round(res["netbench"][0], 1),
            "longest_batch_gap_seconds": {k: round(v, 4) for k, v in longest.items()},
            "device_bytes": {"before": before, "peak": peak["bytes"], "after": after}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--arm", default="both", choices=["a", "b", "both", "none"])
    ap.add_argument("--appear", type=float, default=120.0, help="seconds into the run at which the second file appears")
    ap.add_argument("--window", type=float, default=600.0, help="seconds measured after the file appeared")
    ap.add_argument("--games", type=int, default=512)
    ap.add_argument("--playouts", type=int, default=400)
    ap.add_argument("--net", default="20b256")
    ap.add_argument("--board", type=int, default=19)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--stagger", type=int, default=0)
    ap.add_argument("--move-cap", type=int, default=0, help="both sides pass once a game has this many moves (0: none).  Worker 0 looks for "
                    "a newer file once per game: a cap makes its games, and with them a whole roll-over, fit a short window")
    ap.add_argument("--reload-time", action="store_true")
    ap.add_argument("--out", default="")
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--wdir", default="")
    ap.add_argument("--log", default="")
    ap.add_argument("--live", type=int, default=0)
    ap.add_argument("--seconds", type=float, default=0.0)
    args = ap.parse_args()
    if args.child:
        return child(args)
    rows = [run_arm(args, arm) for arm in (("a", "b") if args.arm == "both" else () if args.arm == "none" else (args.arm,))]
    result = {"tool": "tools/rollover_bench.py", "net": args.net, "games": args.games, "playouts": args.playouts, "board": args.board,
              "arms": rows}
    if args.reload_time:
        result["reload_host_time"] = reload_time(args)
    text = json.dumps(result, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
