"""Ensemble requests (the eight board symmetries of one position as ONE request of the pipe; reference Network::kAverage,
src/neural/network.cc:258) on a box without a GPU:

  * the index rule: the host helper PackedPlanes::Symmetry, and the tests' own numpy permutation, against the record the
    engine's encoder builds for each symmetry (Encoder::Packed(state, s)) over positions of the golden games;
  * the collector (csrc/host/hip_forward_pipe.cc) on tests/fake_hip/fake_hip_symm.c, the CPU stand-in with the two new
    entry points, whose replies are a function of (record, symmetry): ensembles mixed with packed and fp32 requests from
    many threads and from fibers, the capacity fallback, a failed batch;
  * the existing stand-in, which lacks the entry points: AcceptsEnsemble() is false and kAverage is what it was.

The collector parts run in subprocesses: symbol interposition needs a process that has not loaded the real device library."""
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest

from _ensemble import GAME_OF_SIZE, GOLDEN_GAMES, golden_game_at, permute_record
from _golden import Golden
from go_replay import GAME_CONFIGS
from sayuri_amd.pipe import packed_symmetry

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE_DIR = os.path.join(ROOT, "tests", "fake_hip")


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN_GAMES)


# games on 19 / 13 / 9 / 5 / 2 boards, both encoder versions (43 planes: 37 bit planes; 38 planes: 34)
@pytest.mark.parametrize("gi", [0, 3, 4, 5, 7, 8])
def test_symmetry_helpers_give_the_encoders_records(golden, gi):
    cfg = GAME_CONFIGS[gi]
    n_moves = len(golden[f"g{gi}_moves"])
    for step in sorted({0, min(7, n_moves), n_moves // 2, n_moves}):
        g = golden_game_at(golden, gi, step)
        ident, binary = g.planes_packed(0, cfg["version"])
        seen = set()
        for s in range(8):
            want, _ = g.planes_packed(s, cfg["version"])
            assert np.array_equal(packed_symmetry(ident, binary, cfg["board"], s), want), (gi, step, s, "PackedPlanes::Symmetry")
            assert np.array_equal(permute_record(ident, binary, cfg["board"], s), want), (gi, step, s, "numpy rule")
            seen.add(want.tobytes())
        if step == n_moves // 2 and cfg["board"] >= 9:
            assert len(seen) == 8, "a mid-game position whose symmetries coincide checks nothing"


def build_fake(tmp, name):
    out = str(tmp / f"lib{name}.so")
    subprocess.check_call(["gcc", "-O2", "-fPIC", "-shared", "-Wall", os.path.join(FAKE_DIR, name + ".c"), "-o", out, "-lpthread"])
    return out


@pytest.fixture(scope="module")
def fake_symm(tmp_path_factory):
    return build_fake(tmp_path_factory.mktemp("fake_hip_symm"), "fake_hip_symm")


@pytest.fixture(scope="module")
def fake_plain(tmp_path_factory):
    return build_fake(tmp_path_factory.mktemp("fake_hip_plain"), "fake_hip")


COMMON = textwrap.dedent(r"""
    import ctypes, sys, threading
    import numpy as np
    ctypes.CDLL(sys.argv[1], mode=ctypes.RTLD_GLOBAL)      # the fake device side wins symbol resolution
    sys.path.insert(0, sys.argv[3])
    from _ensemble import symm_index
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
    def check_ensemble(pipe, case, label):
        p, bs, off = case
        full, res = pipe.ForwardEnsemble(p, bs, offset=off)
        assert len(res) == (8 if full else 1), label
        for s, got in enumerate(res):                      # symmetry s: every plane taken through the index rule
            assert close(got, expected(p[:, symm_index(bs, s)], bs, off)), (label, bs, off, s)
        if bs > 2:                                         # (a reply of another symmetry would not have passed)
            assert not close(res[0], expected(p[:, symm_index(bs, 5)], bs, off)), label
        return full
""")

MIXED_DRIVER = COMMON + textwrap.dedent(r"""
    pipe = HipForwardPipe(sys.argv[2], board_size=19, batch_size=16, fp16=True, ensemble=int(sys.argv[4]))
    assert pipe.AcceptsEnsemble()
    errs, seen = [], []
    def worker(seed, kind):
        try:
            r = np.random.default_rng(seed)
            for k in range(12):
                if kind == "ensemble":
                    seen.append(check_ensemble(pipe, packable(r), f"ensemble thread {seed} round {k}"))
                    continue
                cs = [packable(r) for _ in range(int(r.integers(1, 9)))]
                planes, bsz, offs = [c[0] for c in cs], [c[1] for c in cs], [c[2] for c in cs]
                outs = pipe.ForwardPacked(planes, bsz, offsets=offs) if kind == "packed" else pipe.Forward(planes, bsz, offsets=offs)
                for c, got in zip(cs, outs):
                    assert close(got, expected(*c)), (kind, seed, k)
        except Exception as e:       # noqa: BLE001
            errs.append(repr(e))
    for kinds in (["ensemble"] * 6 + ["packed"] * 3, ["ensemble"] * 6 + ["packed"] * 2 + ["fp32"] * 2, ["ensemble"] * 12):
        ths = [threading.Thread(target=worker, args=(100 + i, kind)) for i, kind in enumerate(kinds)]
        [t.start() for t in ths]; [t.join() for t in ths]
        assert not errs, errs
    pt = pipe.pump_times()
    fulls = [seen.count(False), seen.count(True)]
    assert fulls[1] > 0, "no request was expanded"
    assert fulls[0] == pipe.ensemble_fallbacks()
    assert pt["evals"] >= 8 * fulls[1] + fulls[0]
    print("ensemble collector ok", fulls, pt["batches"], pt["evals"])
    pipe.Destroy()
""")

FIBER_DRIVER = COMMON + textwrap.dedent(r"""
    slots = int(sys.argv[4])
    pipe = HipForwardPipe(sys.argv[2], board_size=19, batch_size=16, fp16=True, ensemble=slots)
    assert pipe.AcceptsEnsemble()
    rng = np.random.default_rng(77)
    # kinds (sayuri_pipe_ensemble_mix): 0 / 1 ensemble from a fiber / a thread, 2 / 3 packed from a fiber / a thread, 4 fp32
    full = fell = 0
    for rnd, kinds in enumerate(([0] * 10, [0] * 6 + [1] * 4 + [2] * 4 + [3] * 3, [0] * 8 + [1] * 3 + [2] * 3 + [4] * 4,
                                 [0] * 24 + [2] * 12, [0] * 5 + [1] * 5 + [2] * 2 + [3] * 2 + [4] * 2) * 3):
        kinds = list(rng.permutation(kinds))
        cases = [packable(rng) for _ in kinds]
        before = pipe.ensemble_fallbacks()
        res = pipe.ensemble_mix([c[0] for c in cases], [c[1] for c in cases], kinds, offsets=[c[2] for c in cases],
                                fiber_threads=1 + rnd % 3)
        fell_now = 0
        for (p, bs, off), kind, got in zip(cases, kinds, res):
            assert len(got) in ((8, 1) if kind <= 1 else (1,)), (rnd, kind, len(got))
            for s, g in enumerate(got):                    # every reply: this request's record under symmetry s
                assert close(g, expected(p[:, symm_index(bs, s)], bs, off)), (rnd, kind, bs, off, s)
            if kind <= 1:
                full += len(got) == 8
                fell_now += len(got) == 1
        assert pipe.ensemble_fallbacks() - before == fell_now, (rnd, fell_now)
        fell += fell_now
    assert full > 0, "no request was expanded"
    print("ensemble fibers ok", full, fell)
    pipe.Destroy()
""")

FAIL_DRIVER = COMMON + textwrap.dedent(r"""
    pipe = HipForwardPipe(sys.argv[2], board_size=19, batch_size=16, fp16=True, ensemble=2)
    rng = np.random.default_rng(5)
    try:
        pipe.ForwardEnsemble(*packable(rng)[:2])
        raise SystemExit("the failed batch went unnoticed")
    except RuntimeError as e:
        assert "failed" in str(e), e
    assert check_ensemble(pipe, packable(rng), "after the failure")
    print("ensemble failure ok")
    pipe.Destroy()
""")

PLAIN_DRIVER = COMMON + textwrap.dedent(r"""
    from sayuri_amd import search as S
    from sayuri_amd.engine import Game
    pipe = HipForwardPipe(sys.argv[2], board_size=9, batch_size=16, fp16=True, ensemble=2)
    assert not pipe.AcceptsEnsemble()                      # this stand-in has no sayuri_hip_submit_packed_symm
    try:
        pipe.ForwardEnsemble(*packable(np.random.default_rng(1), 9)[:2])
        raise SystemExit("ForwardEnsemble on a device library without the entry point")
    except RuntimeError:
        pass
    game = Game(9, 7.0)
    for mv in (40, 30, 50, 31):
        game.play(mv)
    outs = []
    for on in (True, False):
        net = S.Network(pipe=pipe, options=dict(device_ensemble=on))
        before = pipe.pump_times()["evals"]
        outs.append(net.output(game, ensemble=2))
        assert net.queries() == 8 and pipe.pump_times()["evals"] - before == 8
        net.close()
    assert np.array_equal(outs[0].view(np.uint32), outs[1].view(np.uint32))
    # ... which is the mean of the eight single evaluations (kDirect under symmetry s), accumulated as the facade always
    # did: result += one / 8 in float32, s = 0..7 (a division by 8 is exact, so the sum has one rounding per step)
    net = S.Network(pipe=pipe, options=dict(no_cache=True))
    mean = np.zeros_like(outs[0])
    for s in range(8):
        mean += net.output(game, ensemble=0, symmetry=s) / np.float32(8)
    net.close()
    assert np.array_equal(outs[0].view(np.uint32), mean.view(np.uint32)), float(np.abs(outs[0] - mean).max())
    print("plain stand-in ok")
    pipe.Destroy()
""")


def run_driver(driver, lib, weights, *args, env=None):
    e = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""), **(env or {}))
    r = subprocess.run([sys.executable, "-c", driver, lib, weights, os.path.join(ROOT, "tests")] + [str(a) for a in args], env=e, cwd=ROOT,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return r.stdout


@pytest.mark.parametrize("delay_us,slots", [(0, 2), (300, 2), (300, 1), (3000, 1)])
def test_collector_routes_every_symmetry_to_its_request(fake_symm, tmp_weights_dir, delay_us, slots):
    """Twelve threads at a time: every ensemble request gets, for each symmetry, the reply of ITS record under THAT symmetry,
    whether its batch also holds packed requests (travels packed), fp32 requests (the pump expands all eight on the host) or
    only ensembles; a request past the batch's capacity gets the identity alone and is counted as a fallback."""
    out = run_driver(MIXED_DRIVER, fake_symm, Golden("tiny_res", tmp_weights_dir).weights_path, slots,
                     env=dict(FAKE_HIP_DELAY_US=str(delay_us)))
    assert "ensemble collector ok" in out
    if slots == 1 and delay_us >= 300:   # twelve callers at once and one expansion per batch: some must have fallen back
        assert int(out.split("[")[1].split(",")[0]) > 0, out


@pytest.mark.parametrize("delay_us,slots", [(0, 2), (300, 1), (3000, 2)])
def test_ensembles_from_fibers_and_threads_at_once(fake_symm, tmp_weights_dir, delay_us, slots):
    """ForwardEnsemble from inside fibers (one FiberPool over one to three threads: Reserve as a fiber, WaitWhileEqual, the
    result taken through the finished batch's snapshot) beside ensemble, packed and fp32 callers on OS threads: every reply
    of every request is its own (record, symmetry), and the pipe's fallback counter is the number of requests that got the
    identity alone.  Ten and more ensembles at once against one or two expansions per batch of 16: some fall back."""
    out = run_driver(FIBER_DRIVER, fake_symm, Golden("tiny_res", tmp_weights_dir).weights_path, slots,
                     env=dict(FAKE_HIP_DELAY_US=str(delay_us)))
    assert "ensemble fibers ok" in out
    assert int(out.split("ensemble fibers ok")[1].split()[1]) > 0, out


def test_a_failed_batch_fails_its_ensemble_caller(fake_symm, tmp_weights_dir):
    out = run_driver(FAIL_DRIVER, fake_symm, Golden("tiny_res", tmp_weights_dir).weights_path, env=dict(FAKE_HIP_FAIL_SUBMIT="1"))
    assert "ensemble failure ok" in out


def test_a_device_library_without_the_entry_point_changes_nothing(fake_plain, tmp_weights_dir):
    out = run_driver(PLAIN_DRIVER, fake_plain, Golden("tiny_res", tmp_weights_dir).weights_path)
    assert "plain stand-in ok" in out
