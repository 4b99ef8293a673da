"""Several playouts in flight inside one tree (option playouts_in_flight = K; csrc/engine/search.h) on a box without a GPU:

  * K = 1 is the search it was (a golden game with the option spelled out);
  * K > 1 on the dummy backend and on the CPU oracle's 6b96 network: reproducible, caps met exactly, nothing left in flight,
    virtual loss spreads a round's descents, the group route and the one-by-one route give the same search;
  * the collector's group request (HipForwardPipe::ForwardGroup) on tests/fake_hip/fake_hip.c, in subprocesses (symbol
    interposition needs a process that has not loaded the real device library)."""
import ctypes
import os
import subprocess
import sys
import textwrap
import zlib

import numpy as np
import pytest

from _golden import Golden
from sayuri_amd import search as S
from sayuri_amd import weights as W
from sayuri_amd.engine import Game
from search_replay import DUMMY_GAMES, options, records_close

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE_DIR = os.path.join(ROOT, "tests", "fake_hip")


@pytest.fixture(scope="module")
def port_net(tmp_weights_dir):
    from _oracle import PortNet
    path = os.path.join(tmp_weights_dir, "search_6b96.bin")
    if not os.path.exists(path):
        W.write_weights(path, W.spec_6b96(), seed=21)
    return PortNet(path, True)


def network(backend, port_net, **opts):
    if backend == "dummy":
        return S.Network(options=opts)
    fn = ctypes.cast(port_net.lib().so_forward, ctypes.c_void_p)
    return S.Network(callback=fn, callback_kind=1, callback_user=port_net._h, options=opts)


def run(backend, port_net, search_opts, playouts=200, tag=0, net_opts=None, board=9):
    """One Computation from the empty board with fixed seeds -> (result, flight statistics, facade queries)."""
    net = network(backend, port_net, **(net_opts or {}))
    game = Game(board, 7.0)
    search = S.Search(game, net, dict(playouts=playouts, **search_opts), seeds=(3, 4))
    res = search.computation(playouts, tag)
    stats = search.flight_stats()
    queries = net.queries()
    search.close()
    net.close()
    return res, stats, queries


_RUNS = {}


def run_once(backend, port_net, flight):
    """The default search at K = `flight` (200 playouts, cache on, group_forward at its default of 1), computed once per
    module run and shared; nobody changes what it returns."""
    if (backend, flight) not in _RUNS:
        _RUNS[backend, flight] = run(backend, port_net, dict(playouts_in_flight=flight))
    return _RUNS[backend, flight]


def same_result(a, b):
    return all(np.array_equal(a[k], b[k]) if isinstance(a[k], np.ndarray) else a[k] == b[k] for k in a) and a.keys() == b.keys()


def mean_group(stats):
    return stats["leaves"] / max(1, stats["rounds"])


# ------------------------------------------------------------------------------------------------- 1. K = 1 is today's search
def test_one_playout_in_flight_is_the_golden_game():
    golden = np.load(os.path.join(ROOT, "tests", "golden", "search_games.npz"))
    seed, board, komi, scoring, opts = DUMMY_GAMES[0]
    opts = dict(options(opts), playouts_in_flight=1)
    game = Game(board, komi, scoring)
    search = S.Search(game, S.Network(options=options(DUMMY_GAMES[0][4])), opts, seeds=(seed, seed + 77))
    moves = []
    while not game.info()[10]:
        moves.append(search.selfplay_move())
        assert game.play(moves[-1])
        assert search.flight_stats()["rounds"] == 0
    search.update_territory_helper()
    racy = search.single_candidate_records()
    text = search.gather_training_text()
    search.close()
    assert moves == golden["dummy0_moves"].tolist()
    assert records_close(zlib.decompress(golden["dummy0_records"].tobytes()), text, racy_records=racy) is None


# ------------------------------------------------------------------------------------------------- 2. determinism, invariants
@pytest.mark.parametrize("backend", ["dummy", "portnet"])
@pytest.mark.parametrize("flight", [4, 8])
def test_rounds_are_reproducible_and_leave_nothing_in_flight(port_net, backend, flight):
    """Two runs with the same seeds are the same search; the playout cap is met exactly; groups are no larger than K and do
    hold more than one leaf.  At K = 8 a mean of two leaves per round is a quarter of K: a floor that only broken grouping
    misses (measured: DESIGN.md section 12)."""
    a, st, _ = run_once(backend, port_net, flight)
    b, st_b, _ = run(backend, port_net, dict(playouts_in_flight=flight))
    assert same_result(a, b) and st == st_b
    assert a["playouts"] == 200
    assert st["in_flight"] == 0 and st["playouts_in_flight"] == flight
    assert 0 < st["largest_group"] <= flight
    assert st["rounds"] < st["leaves"]
    assert st["leaves"] + st["direct"] == 200
    print(f"[tree batch] {backend} K={flight}: {st['leaves']} leaves in {st['rounds']} rounds = {mean_group(st):.2f} per round, "
          f"{st['collisions']} collisions")
    if flight == 8:
        assert mean_group(st) >= 2.0, st


# ------------------------------------------------------------------------------------------------- 3. virtual loss is wired
@pytest.mark.parametrize("backend", ["dummy", "portnet"])
def test_virtual_loss_spreads_the_descents_of_a_round(port_net, backend):
    """Without virtual loss nothing in the tree tells a round's second descent from its first: it walks to the same, now
    pending, leaf.  With it the descents part."""
    _, off, _ = run(backend, port_net, dict(playouts_in_flight=8, virtual_loss_count=0), net_opts=dict(no_cache=1))
    _, on, _ = run(backend, port_net, dict(playouts_in_flight=8, virtual_loss_count=1), net_opts=dict(no_cache=1))
    assert mean_group(off) < 1.5 and off["collisions"] > 0, off
    assert mean_group(on) >= 2.0 and on["collisions"] < off["collisions"], (on, off)


# ------------------------------------------------------------------------------------------------- 4. caps and reuse
@pytest.mark.parametrize("cap", [203, 64, 7])
def test_caps_are_met_exactly(port_net, cap):
    res, st, _ = run("dummy", port_net, dict(playouts_in_flight=8), playouts=cap, tag=S.TAG_UNREUSED)
    assert res["visits"] - 1 == cap and st["in_flight"] == 0      # the visit cap (the root's own visit does not count)
    res, st, _ = run("portnet" if cap < 100 else "dummy", port_net, dict(playouts_in_flight=8), playouts=cap)
    assert res["playouts"] == cap and st["in_flight"] == 0         # the playout cap


@pytest.mark.parametrize("reuse", [0, 1])
def test_a_think_game_to_its_end(reuse):
    """7x7, territory scoring (the rule switch inside playouts and the ownership recovery stay single evaluations), K = 8:
    after every move nothing is in flight -- tree reuse sees a clean tree -- and the game ends by the rules."""
    game = Game(7, 9.0, 1)
    search = S.Search(game, S.Network(), dict(playouts=150, resign_threshold=0.0, playouts_in_flight=8, reuse_tree=reuse), seeds=(23, 100))
    moves = 0
    while not game.info()[10] and moves < 1000:
        mv = search.think()
        assert mv >= 0 and game.play(mv)
        assert search.flight_stats()["in_flight"] == 0
        moves += 1
    assert game.info()[10] and search.flight_stats()["rounds"] > 0
    search.close()


def test_a_selfplay_game_through_the_move_chooser():
    seed, board, komi, scoring, opts = DUMMY_GAMES[2]   # 7x7, Gumbel root
    game = Game(board, komi, scoring)
    search = S.Search(game, S.Network(options=options(opts)), dict(options(opts), playouts_in_flight=4), seeds=(seed, seed + 77))
    moves = []
    while not game.info()[10] and len(moves) < 1000:
        moves.append(search.selfplay_move())
        assert game.play(moves[-1])
        assert search.flight_stats()["in_flight"] == 0
    assert game.info()[10]
    search.update_territory_helper()
    text = search.gather_training_text()
    assert search.flight_stats()["rounds"] > 0
    search.close()
    assert text.count(b"\n") == 53 * len(moves)                  # one 53-line record per move played


# ------------------------------------------------------------------------------------------------- 5. group == one by one
def test_group_route_and_one_by_one_route_are_the_same_search(port_net):
    a, st_a, qa = run_once("portnet", port_net, 8)   # group_forward = 1 is the default
    b, st_b, qb = run("portnet", port_net, dict(playouts_in_flight=8), net_opts=dict(group_forward=0))
    assert same_result(a, b) and st_a == st_b and qa == qb > 0


# ------------------------------------------------------------------------------------------------- 6. refusals
def test_selfplay_refuses_several_playouts_in_flight():
    with pytest.raises(RuntimeError, match="playouts_in_flight"):
        S.selfplay(None, dict(playouts=10, num_games=1, parallel_games=1, playouts_in_flight=2, default_boardsize=7), move_cap=2)


@pytest.mark.parametrize("bad", [0, 65, -3])
def test_out_of_range_is_refused_with_a_message(bad):
    with pytest.raises(ValueError, match="playouts_in_flight must be in 1..64"):
        S.Search(Game(9, 7.0), S.Network(), dict(playouts_in_flight=bad))


# ------------------------------------------------------------------------------------------------- 7. the collector
@pytest.fixture(scope="module")
def fake_plain(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("fake_hip_group") / "libfake_hip.so")
    subprocess.check_call(["gcc", "-O2", "-fPIC", "-shared", "-Wall", os.path.join(FAKE_DIR, "fake_hip.c"), "-o", out, "-lpthread"])
    return out


COMMON = textwrap.dedent(r"""
    import ctypes, sys, threading, time
    import numpy as np
    ctypes.CDLL(sys.argv[1], mode=ctypes.RTLD_GLOBAL)      # the fake device side wins symbol resolution
    sys.path.insert(0, sys.argv[3])
    from sayuri_amd.pipe import HipForwardPipe

    B, C = 19, 43
    def expected(planes, bs, off):                         # fake_hip.c: fake_eval, in Forward()'s packing
        grid = np.zeros((C, B, B), np.float32)
        grid[:, :bs, :bs] = planes.reshape(C, bs, bs)
        x = grid.reshape(C, B * B).astype(np.float64)
        w = 1 + (np.arange(C * B * B) % 7)
        s = float((x.ravel() * w).sum())
        prob = (x[off] + 0.5 * x[5] + off).reshape(B, B)[:bs, :bs].ravel()
        own = (x[7] - x[8]).reshape(B, B)[:bs, :bs].ravel()
        misc = np.float32(s * 0.002) - np.arange(15, dtype=np.float32) + np.float32(bs)
        tail = [np.float32(s * 0.001) + off, misc[0], misc[1], misc[2], misc[3], misc[8], misc[13], misc[14], off]
        return np.concatenate([prob, own, np.asarray(tail, np.float64)])
    def close(got, exp):
        return got.shape == exp.shape and np.abs(got - exp).max() <= 1e-3 * max(1.0, np.abs(exp).max())
    def packable(rng, bs=None):
        bs = int(rng.choice([19, 13, 9, 7, 2])) if bs is None else bs
        p = np.zeros((C, bs * bs), np.float32)
        p[:C - 6] = rng.integers(0, 2, size=(C - 6, bs * bs))
        p[C - 6:] = rng.normal(size=(6, 1)).astype(np.float32)
        return p, bs, int(rng.integers(0, 5))
    def group(pipe, cases, label):
        outs = pipe.ForwardGroup([(p, bs, 7.5, off) for p, bs, off in cases])
        assert len(outs) == len(cases), label
        for c, got in zip(cases, outs):
            assert close(got, expected(*c)), label
""")

IDLE_DRIVER = COMMON + textwrap.dedent(r"""
    pipe = HipForwardPipe(sys.argv[2], board_size=19, batch_size=16, fp16=True, waittime_ms=2000)
    assert pipe.AcceptsGroup()
    rng = np.random.default_rng(11)
    t0 = time.perf_counter()
    for k, n in enumerate([1, 5, 16, 1, 5, 16, 5, 1, 16, 5]):
        before = pipe.pump_times()
        group(pipe, [packable(rng) for _ in range(n)], ("idle", k, n))
        after = pipe.pump_times()
        assert after["batches"] - before["batches"] == 1 and after["evals"] - before["evals"] == n, (k, n, before, after)
    took = time.perf_counter() - t0
    assert took < 2.0, f"ten groups from an idle caller took {took:.2f} s: one of them waited for the idle timer"
    before = pipe.pump_times()
    group(pipe, [packable(rng) for _ in range(40)], "forty")
    after = pipe.pump_times()
    assert after["batches"] - before["batches"] == 3 and after["evals"] - before["evals"] == 40, (before, after)
    print("group idle ok", round(took, 3))
    pipe.Destroy()
""")

MIXED_DRIVER = COMMON + textwrap.dedent(r"""
    pipe = HipForwardPipe(sys.argv[2], board_size=19, batch_size=16, fp16=True, waittime_ms=int(sys.argv[4]))
    errs = []
    def worker(seed, kind):
        try:
            r = np.random.default_rng(seed)
            for k in range(15):
                cs = [packable(r) for _ in range(int(r.integers(1, 12)))]
                if kind == "group":
                    group(pipe, cs, (kind, seed, k))
                    continue
                planes, bsz, offs = [c[0] for c in cs[:3]], [c[1] for c in cs[:3]], [c[2] for c in cs[:3]]
                outs = pipe.ForwardPacked(planes, bsz, offsets=offs) if kind == "packed" else pipe.Forward(planes, bsz, offsets=offs)
                for c, got in zip(cs, outs):
                    assert close(got, expected(*c)), (kind, seed, k)
        except Exception as e:       # noqa: BLE001
            errs.append(repr(e))
    ths = [threading.Thread(target=worker, args=(200 + i, kind)) for i, kind in enumerate(["group"] * 4 + ["packed"] * 2 + ["fp32"] * 2)]
    [t.start() for t in ths]; [t.join() for t in ths]
    assert not errs, errs
    print("group mixed ok", pipe.pump_times()["batches"], pipe.pump_times()["evals"])
    pipe.Destroy()
""")

FAIL_DRIVER = COMMON + textwrap.dedent(r"""
    pipe = HipForwardPipe(sys.argv[2], board_size=19, batch_size=16, fp16=True, waittime_ms=2000)
    rng = np.random.default_rng(5)
    try:
        group(pipe, [packable(rng) for _ in range(5)], "the failed one")
        raise SystemExit("the failed batch went unnoticed")
    except RuntimeError as e:
        assert "failed" in str(e), e
    group(pipe, [packable(rng) for _ in range(5)], "after the failure")
    group(pipe, [packable(rng)], "after the failure, one")
    print("group failure ok")
    pipe.Destroy()
""")

SEARCH_DRIVER = COMMON + textwrap.dedent(r"""
    from sayuri_amd import search as S
    from sayuri_amd.engine import Game
    pipe = HipForwardPipe(sys.argv[2], board_size=9, batch_size=16, fp16=True, waittime_ms=int(sys.argv[4]))
    results = []
    for grouped in (1, 0):
        net = S.Network(pipe=pipe, options=dict(group_forward=grouped))
        game = Game(9, 7.0)
        for mv in (40, 30, 50):
            game.play(mv)
        search = S.Search(game, net, dict(playouts=120, playouts_in_flight=8), seeds=(3, 4))
        before = pipe.pump_times()
        results.append(search.computation(120))
        after = pipe.pump_times()
        evals, batches = after["evals"] - before["evals"], after["batches"] - before["batches"]
        assert results[-1]["playouts"] == 120 and search.flight_stats()["in_flight"] == 0
        assert evals == net.queries() > 120, (evals, net.queries())
        if grouped:
            assert batches < evals / 2, (batches, evals)
            print("group search ok", batches, evals)
        else:
            assert batches == evals, (batches, evals)
        search.close(); net.close()
    a, b = results
    assert all(np.array_equal(a[k], b[k]) for k in a), "the group route and the one-by-one route searched differently"
    pipe.Destroy()
""")


def run_driver(driver, lib, weights, *args, env=None):
    e = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""), **(env or {}))
    r = subprocess.run([sys.executable, "-c", driver, lib, weights, os.path.join(ROOT, "tests")] + [str(a) for a in args], env=e, cwd=ROOT,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return r.stdout


def test_groups_from_an_idle_caller_do_not_wait_for_the_timer(fake_plain, tmp_weights_dir):
    """batch 16, gpu_waittime 2 s: ten groups of 1, 5 and 16 from one caller are one batch each, the replies are the
    stand-in's for exactly these requests, and all ten are back in under 2 s together; 40 requests are three batches."""
    assert "group idle ok" in run_driver(IDLE_DRIVER, fake_plain, Golden("tiny_res", tmp_weights_dir).weights_path)


@pytest.mark.parametrize("waittime_ms", [2, 0])
def test_groups_beside_single_requests(fake_plain, tmp_weights_dir, waittime_ms):
    """Four threads send groups while two send packed and two fp32 requests: every reply belongs to its request, whether a
    group shared its set with others or straddled two sets."""
    assert "group mixed ok" in run_driver(MIXED_DRIVER, fake_plain, Golden("tiny_res", tmp_weights_dir).weights_path, waittime_ms)


def test_a_failed_batch_fails_its_group_and_the_pipe_goes_on(fake_plain, tmp_weights_dir):
    out = run_driver(FAIL_DRIVER, fake_plain, Golden("tiny_res", tmp_weights_dir).weights_path, env=dict(FAKE_HIP_FAIL_SUBMIT="1"))
    assert "group failure ok" in out


@pytest.mark.parametrize("waittime_ms", [2, 0])
def test_a_search_sends_its_rounds_as_groups(fake_plain, tmp_weights_dir, waittime_ms):
    """K = 8 over the stand-in: every facade query is one evaluation of the pipe, in fewer than half as many batches -- also
    on a pipe that closes a set the moment it holds a request (waittime 0): a group is not cut up while it is being
    written.  The same search with group_forward = 0 sends one batch per evaluation and finds the same result."""
    assert "group search ok" in run_driver(SEARCH_DRIVER, fake_plain, Golden("tiny_res", tmp_weights_dir).weights_path, waittime_ms)
