"""Context-level helpers that more than one GPU test module uses: a pipe created under exactly the engine switches a test asks
for, planes on the NN grid, a forward against the CPU oracle, interleaved device timing, the fuzz's pool of positions and its page-locked ticket buffers, and the whole-network parity check with its fp16 bound
(test_gpu_net.py's docstring accounts for the tolerances)."""
import ctypes
import os

import numpy as np

from _oracle import PortNet
from sayuri_amd import _lib, hipraw
from sayuri_amd import weights as W
from sayuri_amd.engine import pack_planes
from sayuri_amd.pipe import HipForwardPipe

B = 19
MAXB = 640
WORDS = 37 * 12 + 8
MAIN_SIZES, ODD_SIZES = (9, 13, 19), (2, 3, 5, 7, 11, 14, 16, 17)
# every switch the engine reads at creation that a test sets
SWITCHES = ("SAYURI_SE_FUSED", "SAYURI_SE_SPLIT", "SAYURI_TOWER", "SAYURI_LATENCY", "SAYURI_LATENCY_SPLIT", "SAYURI_CHAINS", "SAYURI_CONV",
            "SAYURI_DEBUG_RECYCLE_INPUT")


def make_pipe(path, env=None, latency=False, batch=MAXB, fp16=True, switches=()):
    """A pipe created under exactly `env` of the engine's switches (they are read once, at creation); `switches`: a feature's
    own, set as `env` says and put back afterwards like the rest."""
    keep = {k: os.environ.pop(k, None) for k in SWITCHES + tuple(switches)}
    os.environ.update(env or {})
    try:
        return HipForwardPipe(path, board_size=B, batch_size=batch, fp16=fp16, latency=latency)
    finally:
        for k, v in keep.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


def make_pipe_under(switches, path, env=None, **kw):
    """make_pipe with exactly these switches of a feature set as `env` says, and put back afterwards"""
    return make_pipe(path, env, switches=switches, **kw)


def grid_of(planes, bsz, board=B):
    """per-sample planes [43][bs*bs] on the NN grid of `board`: [n][43][board*board], zero outside a sample's board"""
    gr = np.zeros((len(bsz), 43, board * board), np.float32)
    for i, (p, bs) in enumerate(zip(planes, bsz)):
        gr[i].reshape(43, board, board)[:, :bs, :bs] = p.reshape(43, bs, bs)
    return gr


class Pool:
    """Positions of the fuzz: planes on the NN grid, packed records, board sizes -- 40 per main size, 6 per odd size."""

    def __init__(self, seed=606):
        sizes = [s for s in MAIN_SIZES for _ in range(40)] + [s for s in ODD_SIZES for _ in range(6)]
        planes = W.synthetic_planes(len(sizes), sizes, seed=seed)
        self.bsz = np.asarray(sizes, np.int32)
        self.grid = np.zeros((len(sizes), 43, B * B), np.float32)
        for i, (p, bs) in enumerate(zip(planes, sizes)):
            self.grid[i].reshape(43, B, B)[:, :bs, :bs] = p.reshape(43, bs, bs)
        self.rec = np.stack([pack_planes(p, 37) for p in planes]).astype(np.uint32)
        self.by_size = {s: np.flatnonzero(self.bsz == s) for s in set(sizes)}

    def draw(self, rng, n, mix):
        if mix == "uniform19":
            return rng.choice(self.by_size[19], size=n)
        if mix == "mixed":
            return np.asarray([rng.choice(self.by_size[int(s)]) for s in rng.choice(MAIN_SIZES, size=n)])
        return rng.integers(0, len(self.bsz), size=n)  # "wild": anything from 2x2 to 19x19


class Pinned:
    """Two sets of page-locked staging buffers for submit / wait (what the pump owns), filled from a Pool."""

    def __init__(self):
        self.sets = [hipraw.PinnedSet(MAXB, B, 43 * B * B) for _ in range(2)]

    def close(self):
        for s in self.sets:
            s.close()

    def submit(self, ctx, i, pool, idx, packed):
        s, n = self.sets[i], len(idx)
        s.bsz[:n] = pool.bsz[idx]
        if packed:
            s.records[:n * WORDS] = pool.rec[idx].ravel()
            return hipraw.submit_packed(ctx, s, n, 37)
        s.planes[:n * 43 * B * B] = pool.grid[idx].ravel()
        return hipraw.submit(ctx, s, n)

    def wait(self, ctx, i, tick, n):
        hipraw.wait(ctx, tick)
        return tuple(a.copy() for a in self.sets[i].outputs(n))


def wrong_samples(ref, got, idx):
    """Samples of a batch whose bits differ from their position's reference bits (any of the four outputs)."""
    bad = np.zeros(len(idx), bool)
    for a, b in zip(ref, got):
        a = a[idx]
        bad |= (a.reshape(len(idx), -1).view(np.uint32) != b.reshape(len(idx), -1).view(np.uint32)).any(axis=1)
    return np.flatnonzero(bad)


FP16_ATOL = 4e-3  # times max(1, output scale): fp16_tol()


def fp16_tol(exp):
    return FP16_ATOL * max(1.0, float(np.abs(exp).max()))


def within_oracle(exp, outs, i, bs, what):
    """sample i of a forward's raw outputs against the CPU oracle's (prob, pass, misc, own) of its position"""
    e_prob, e_pass, e_misc, e_own = exp
    tol = fp16_tol(np.concatenate([e_prob.ravel(), e_own.ravel(), e_misc.ravel()]))
    crop = lambda a: a.reshape(B, B)[:bs, :bs].ravel()
    for k in range(e_prob.shape[0]):
        assert np.abs(crop(outs[0][i, k]) - e_prob[k]).max() <= tol, (what, i, bs, "prob", k)
    assert np.abs(outs[1][i] - e_pass).max() <= tol and np.abs(outs[2][i] - e_misc).max() <= tol, (what, i, bs)
    assert np.abs(crop(outs[3][i]) - e_own).max() <= tol, (what, i, bs, "own")


def device_ms(pipes, gr, sizes, rounds=3, iters=100):
    """device ms per forward (sayuri_hip_time_runs), inputs resident, the contexts interleaved: medians of `rounds` x `iters`"""
    lib = _lib.hip()
    bs = np.asarray(sizes, np.int32)
    times = {k: [] for k in pipes}
    for p in pipes.values():
        assert lib.sayuri_hip_upload(p.ctx(0), len(sizes), _lib.fp(gr), bs.ctypes.data_as(_lib.c_int_p)) == 0
        ms = ctypes.c_float(0)
        assert lib.sayuri_hip_time_runs(p.ctx(0), 30, ctypes.byref(ms)) == 0   # warm-up
    for _ in range(rounds):
        for k, p in pipes.items():
            ms = ctypes.c_float(0)
            assert lib.sayuri_hip_time_runs(p.ctx(0), iters, ctypes.byref(ms)) == 0, lib.sayuri_hip_last_error()
            times[k].append(ms.value / iters)
    return {k: float(np.median(v)) for k, v in times.items()}


def self_check_l2(got, exp, bs):
    """reference Network::SelfCheck (network.cc:333-359) on post-processed outputs."""
    a, b = PortNet.postprocess(got, bs), PortNet.postprocess(exp, bs)
    s = bs * bs
    va = np.concatenate([a[:s + 1], [a[2 * s + 1 + 3]]])
    vb = np.concatenate([b[:s + 1], [b[2 * s + 1 + 3]]])
    return float(np.sqrt(((va - vb) ** 2).sum()))


def check(pipe, cases, atol, label):
    planes = [c[0] for c in cases]
    bsz = [c[1] for c in cases]
    offs = [c[2] for c in cases]
    for mode, outs in (("batch", pipe.BatchForward(planes, bsz, offsets=offs)),
                       ("queue", pipe.Forward(planes, bsz, offsets=offs))):
        for (p, bs, off, exp), got in zip(cases, outs):
            assert got.shape == exp.shape
            assert np.isfinite(got).all(), (label, mode)
            err = float(np.abs(got - exp).max())
            assert err <= (atol(exp) if callable(atol) else atol), (label, mode, bs, off, err)
            assert self_check_l2(got, exp, bs) <= 0.2
