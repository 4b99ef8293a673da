"""Live weight reload on a box without a GPU: the host side (HipForwardPipe::Reload, Network::SwapWeights, the self-play roll-over
of option live_weights) on tests/fake_hip/fake_hip_reload.c, the CPU stand-in whose replies carry a checksum of the tensors that
were live when their batch was enqueued -- so every reply says which network answered it.

Networks "A" and "B" are one spec under two seeds; "solo" results come from a fresh pipe (or facade) created on that file.
The parts that need the stand-in run in subprocesses: symbol interposition needs a process that has not loaded the real device
library."""
import os
import subprocess
import sys
import textwrap

import pytest

from sayuri_amd import search as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE_DIR = os.path.join(ROOT, "tests", "fake_hip")


def build_fake(tmp, name):
    out = str(tmp / f"lib{name}.so")
    subprocess.check_call(["gcc", "-O2", "-fPIC", "-shared", os.path.join(FAKE_DIR, name + ".c"), "-o", out, "-lpthread", "-lm"])
    return out


@pytest.fixture(scope="module")
def fake_reload(tmp_path_factory):
    return build_fake(tmp_path_factory.mktemp("fake_hip_reload"), "fake_hip_reload")


@pytest.fixture(scope="module")
def fake_plain(tmp_path_factory):
    return build_fake(tmp_path_factory.mktemp("fake_hip_plain"), "fake_hip")


def run_driver(code, fake, tmp, env=None, timeout=300):
    r = subprocess.run([sys.executable, "-c", code, fake, ROOT, str(tmp)], capture_output=True, text=True, timeout=timeout,
                       env=dict(os.environ, **(env or {})))
    assert r.returncode == 0, (r.returncode, r.stdout[-1500:], r.stderr[-3000:])
    return r


COMMON = textwrap.dedent(r"""
    import ctypes, os, sys, threading, time
    import numpy as np
    ctypes.CDLL(sys.argv[1], mode=ctypes.RTLD_GLOBAL)      # the fake device side wins symbol resolution
    sys.path[:0] = [sys.argv[2], os.path.join(sys.argv[2], "tests")]
    from sayuri_amd import search as S
    from sayuri_amd import weights as W
    from sayuri_amd.engine import Game
    from sayuri_amd.pipe import HipForwardPipe
    tmp = sys.argv[3]
    SPEC = W.NetSpec.residual(2, 16, 8)
    def write(name, seed, spec=SPEC, where=tmp):
        path = os.path.join(where, name)
        W.write_weights(path, spec, seed=seed)
        return path
    def same(a, b):
        return len(a) == len(b) and all(x.shape == y.shape and np.array_equal(x, y) for x, y in zip(a, b))
""")

# ---------------------------------------------------------------- the pipe under load (GPU test 3 on the stand-in)
PIPE_DRIVER = COMMON + textwrap.dedent(r"""
    A, B = write("a.bin", 1), write("b.bin", 2)
    threads, rounds = 4, 200
    bsz = [19, 9, 13, 19]
    planes = W.synthetic_planes(threads, bsz, seed=9)
    def solo(path):
        p = HipForwardPipe(path, board_size=19, batch_size=8)
        try:
            return p.Forward(planes, bsz)
        finally:
            p.Destroy()
    sa, sb = solo(A), solo(B)
    assert not any(same([x], [y]) for x, y in zip(sa, sb)), "the stand-in does not tell A from B"
    pipe = HipForwardPipe(A, board_size=19, batch_size=8)
    assert pipe.AcceptsReload() and pipe.weights_generation() == 0
    seen, errs, begun_after = [[] for _ in range(threads)], [], [None] * threads
    reloaded = threading.Event()
    def worker(k):
        try:
            for _ in range(rounds):
                after = reloaded.is_set()
                got = pipe.Forward([planes[k]], [bsz[k]])[0]
                kind = "A" if same([got], [sa[k]]) else "B" if same([got], [sb[k]]) else "?"
                seen[k].append(kind)
                if after and begun_after[k] is None:
                    begun_after[k] = kind
        except Exception as e:       # noqa: BLE001
            errs.append(repr(e))
    ths = [threading.Thread(target=worker, args=(k,)) for k in range(threads)]
    [t.start() for t in ths]
    while min(len(s) for s in seen) < rounds // 2 and not errs and any(t.is_alive() for t in ths):
        time.sleep(0.001)
    pipe.Reload(B)
    reloaded.set()
    [t.join() for t in ths]
    assert not errs, errs
    for k, s in enumerate(seen):
        text = "".join(s)
        assert len(s) == rounds and "?" not in s, (k, text)
        assert text == "A" * s.count("A") + "B" * s.count("B") and s[0] == "A" and s[-1] == "B", (k, text)
        assert begun_after[k] in (None, "B"), (k, begun_after[k])
    assert pipe.weights_generation() == 1 and same(pipe.Forward(planes, bsz), sb)
    # a refusal leaves the pipe on the network it had: another architecture, a file that does not parse
    other = write("other.bin", 3, W.NetSpec.residual(3, 16, 8))
    for bad, word in ((other, "residual_blocks"), (os.path.join(tmp, "missing.bin"), "")):
        try:
            pipe.Reload(bad)
            raise AssertionError("accepted " + bad)
        except RuntimeError as e:
            assert word in str(e), str(e)
        assert pipe.weights_generation() == 1 and same(pipe.Forward(planes, bsz), sb)
    pipe.Reload(A)
    assert pipe.weights_generation() == 2 and same(pipe.Forward(planes, bsz), sa)
    print("pipe reload ok", ["".join(s).index("B") for s in seen])
    pipe.Destroy()
""")


def test_pipe_reload_under_load_on_the_stand_in(fake_reload, tmp_path):
    r = run_driver(PIPE_DRIVER, fake_reload, tmp_path, env={"FAKE_HIP_DELAY_US": "2000"})
    assert "pipe reload ok" in r.stdout


# ---------------------------------------------------------------- a device library without the entry points
PLAIN_DRIVER = COMMON + textwrap.dedent(r"""
    wdir = os.path.join(tmp, "weights"); os.mkdir(wdir)
    out = os.path.join(tmp, "out"); os.mkdir(out)
    A = write("net-0001.bin", 1, where=wdir)
    pipe = HipForwardPipe(A, board_size=9, batch_size=8)
    assert not pipe.AcceptsReload() and pipe.weights_generation() == 0
    try:
        pipe.Reload(A)
        raise AssertionError("a library without sayuri_hip_reload_* reloaded")
    except RuntimeError as e:
        assert "reload" in str(e)
    net = S.Network(pipe=pipe)
    try:
        net.reload(A)
        raise AssertionError("the facade reloaded on a pipe that cannot")
    except RuntimeError as e:
        assert "does not take a weight reload" in str(e)
    net.close()
    # self-play with live_weights=1: the newer file cannot go in live, so the loop winds down as it always did
    dropped = []
    def on_stats(st, halt):
        if st["games_done"] >= 8 and not dropped:
            write("b.tmp", 2)
            os.rename(os.path.join(tmp, "b.tmp"), os.path.join(wdir, "net-0002.bin"))
            dropped.append(1)
        return halt
    st = S.selfplay(pipe, dict(playouts=4, parallel_games=8, num_games=100000, seed=5, selfplay_query=["bkp:9:7:1"], live_weights=1,
                               weights_dir=wdir, weights_file=A, target_directory=out), on_stats=on_stats, stats_interval=0.05, move_cap=60)
    assert st["games_done"] == st["max_games"] < 100000 and st["max_games"] % 25 == 0 and st["weight_swaps"] == 0, st
    print("plain ok", st["max_games"])
    pipe.Destroy()
""")


def test_library_without_reload_entry_points_winds_down_as_before(fake_plain, tmp_path):
    r = run_driver(PLAIN_DRIVER, fake_plain, tmp_path)
    assert "plain ok" in r.stdout
    assert r.stderr.count("[selfplay] live_weights:") == 1 and "does not take a weight reload" in r.stderr, r.stderr[-2000:]


# ---------------------------------------------------------------- the position cache across a swap, and the race
CACHE_DRIVER = COMMON + textwrap.dedent(r"""
    A, B = write("a.bin", 1), write("b.bin", 2)
    def position(moves):
        g = Game(9, 7.0)
        for m in moves:
            g.play(m)
        return g
    g1, g2 = position((40, 30, 50)), position((20, 21, 22, 60))
    def solo(path, game):
        p = HipForwardPipe(path, board_size=9, batch_size=8, waittime_ms=0)
        n = S.Network(pipe=p)
        try:
            return n.output(game, use_cache=True)
        finally:
            n.close(); p.Destroy()
    a1, b1, a2, b2 = solo(A, g1), solo(B, g1), solo(A, g2), solo(B, g2)
    assert not np.array_equal(a1, b1) and not np.array_equal(a2, b2)
    pipe = HipForwardPipe(A, board_size=9, batch_size=8, waittime_ms=0)
    net = S.Network(pipe=pipe)
    assert np.array_equal(net.output(g1, use_cache=True), a1)
    q = net.queries()
    assert np.array_equal(net.output(g1, use_cache=True), a1) and net.queries() == q, "the cache is off: the test checks nothing"
    net.reload(B)
    assert np.array_equal(net.output(g1, use_cache=True), b1), "after the swap the cache served network A"
    assert net.queries() == q + 1
    assert np.array_equal(net.output(g1, use_cache=True), b1) and net.queries() == q + 1   # ... and caches B's
    # the race: a request is on the device (50 ms) while the weights are swapped back to A; what it returns must not be cached
    late = []
    t = threading.Thread(target=lambda: late.append(net.output(g2, use_cache=True)))
    t.start()
    time.sleep(0.005)
    net.reload(A)
    t.join()
    assert np.array_equal(late[0], b2) or np.array_equal(late[0], a2)
    q = net.queries()
    again = net.output(g2, use_cache=True)
    assert np.array_equal(again, a2), "the result of a request that began before the swap was served from the cache"
    print("cache ok", "late request answered by", "B" if np.array_equal(late[0], b2) else "A", "queries", net.queries() - q)
    net.close(); pipe.Destroy()
""")


def test_cache_never_serves_the_old_network_after_a_swap(fake_reload, tmp_path):
    r = run_driver(CACHE_DRIVER, fake_reload, tmp_path, env={"FAKE_HIP_DELAY_US": "50000"})
    assert "cache ok" in r.stdout


# ---------------------------------------------------------------- self-play rolls over
ROLLOVER_DRIVER = COMMON + textwrap.dedent(r"""
    mode = sys.argv[4]
    wdir = os.path.join(tmp, "weights"); os.mkdir(wdir)
    out = os.path.join(tmp, "out"); os.mkdir(out)
    A = write("net-0001.bin", 1, where=wdir)
    pipe = HipForwardPipe(A, board_size=9, batch_size=8)
    step = []
    def drop(name, make):
        make(os.path.join(tmp, name + ".tmp"))
        os.rename(os.path.join(tmp, name + ".tmp"), os.path.join(wdir, name))
    def on_stats(st, halt):
        assert not halt or mode == "other_arch" or mode.startswith("off"), "a halt wish was raised"   # local_halt stays 0 on a swap
        if st["games_done"] >= 8 and not step:
            step.append(st["games_done"])
            if mode == "truncated":      # a file still being written: the first third of B
                drop("net-0002.bin", lambda p: open(p, "wb").write(open(write("b_full.bin", 2), "rb").read()[:4000]))
            elif mode == "other_arch":
                drop("net-0002.bin", lambda p: W.write_weights(p, W.NetSpec.residual(3, 16, 8), seed=2))
            else:
                drop("net-0002.bin", lambda p: W.write_weights(p, SPEC, seed=2))
        elif mode == "truncated" and len(step) == 1 and st["games_done"] >= step[0] + 8:
            step.append(st["games_done"])   # the complete file follows, under a newer name
            drop("net-0003.bin", lambda p: W.write_weights(p, SPEC, seed=2))
        return halt
    live = 0 if mode.startswith("off") else 1
    games = 100000 if mode in ("other_arch", "off_long") else 40
    st = S.selfplay(pipe, dict(playouts=4, parallel_games=8, num_games=games, seed=5, selfplay_query=["bkp:9:7:1"], live_weights=live,
                               weights_dir=wdir, weights_file=A, target_directory=out), on_stats=on_stats, stats_interval=0.05, move_cap=60)
    log_dir = os.path.join(out, "weights_log")
    logs = [open(os.path.join(log_dir, f)).read().splitlines() for f in os.listdir(log_dir)] if os.path.isdir(log_dir) else []
    print("STATS", mode, st["games_done"], st["max_games"], st["weight_swaps"], pipe.weights_generation(), logs)
    if mode in ("swap", "truncated"):
        assert st["games_done"] == 40 == st["max_games"], st            # no cap from WindDown
        assert st["weight_swaps"] == 1 and pipe.weights_generation() == 1, st
        assert len(logs) == 1 and len(logs[0]) == 2, logs
        first, second = (l.split() for l in logs[0])
        assert first[0] == "0" and first[2] == "net-0001.bin" and int(second[0]) >= 8 and int(second[1]) >= int(first[1])
        assert second[2] == ("net-0003.bin" if mode == "truncated" else "net-0002.bin"), logs
        # the pipe now IS network B
        planes = W.synthetic_planes(2, [9, 9], seed=4)
        solo = HipForwardPipe(os.path.join(wdir, second[2]), board_size=9, batch_size=8)
        assert same(pipe.Forward(planes, [9, 9]), solo.Forward(planes, [9, 9]))
        solo.Destroy()
    elif mode == "other_arch":
        assert st["games_done"] == st["max_games"] < 100000 and st["max_games"] % 25 == 0, st
        assert st["weight_swaps"] == 0 and pipe.weights_generation() == 0 and len(logs[0]) == 1, (st, logs)
    elif mode == "off_long":    # today's behaviour: the cap of WindDown, nothing swapped, no log
        assert st["games_done"] == st["max_games"] < 100000 and st["max_games"] % 25 == 0, st
        assert st["weight_swaps"] == 0 and pipe.weights_generation() == 0 and not logs, (st, logs)
    else:                       # "off": the same script as "swap" with live_weights=0
        assert st["weight_swaps"] == 0 and pipe.weights_generation() == 0 and not logs, (st, logs)
        assert st["games_done"] == st["max_games"] == 40, st
    pipe.Destroy()
    print("rollover ok")
""")


@pytest.mark.parametrize("mode", ["swap", "truncated", "other_arch", "off", "off_long"])
def test_selfplay_rolls_over(fake_reload, tmp_path, mode):
    """swap: GPU test 6 on the stand-in.  truncated: a file that does not parse is said once and skipped, the complete one that
    follows is swapped in.  other_arch: one stderr line, then the reference's wind-down.  off / off_long: live_weights=0 is today's
    behaviour -- WindDown caps max_games at (games begun + 25) rounded up to 25, which is at least 50 with 8 games in flight: it
    binds on a long run (off_long) and leaves a 40-game run at 40 (off)."""
    r = subprocess.run([sys.executable, "-c", ROLLOVER_DRIVER, fake_reload, ROOT, str(tmp_path), mode], capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0 and "rollover ok" in r.stdout, (r.returncode, r.stdout[-1500:], r.stderr[-3000:])
    said = [l for l in r.stderr.splitlines() if l.startswith("[selfplay] live_weights:")]
    if mode == "truncated":
        assert len(said) == 1 and "does not parse" in said[0] and "net-0002.bin" in said[0], said
    elif mode == "other_arch":
        assert len(said) == 1 and "is refused" in said[0] and "residual_blocks" in said[0], said
    else:
        assert not said, said


# ---------------------------------------------------------------- options
def test_live_weights_option_parses_and_refuses_other_values():
    st = S.selfplay(None, dict(playouts=2, parallel_games=2, num_games=2, seed=3, selfplay_query=["bkp:5:7:1"], live_weights=1), move_cap=12)
    assert st["games_done"] == 2 and st["weight_swaps"] == 0
    st = S.selfplay(None, dict(playouts=2, parallel_games=2, num_games=2, seed=3, selfplay_query=["bkp:5:7:1"], live_weights=0), move_cap=12)
    assert st["games_done"] == 2
    for bad in ("2", "-1", "yes", "true", ""):
        with pytest.raises(RuntimeError, match="live_weights must be 0 or 1"):
            S.selfplay(None, {"num_games": 1, "live_weights": bad})
