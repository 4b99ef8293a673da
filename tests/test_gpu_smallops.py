"""Kernel-level parity of the non-GEMM kernels -- se_pool / se_fc / se_scale and head_tail (csrc/hip/small_ops.h) --
against the CPU oracle's restatements of the reference layers they replace:
GlobalPooling<false/true> (src/neural/blas/se_unit.cc:9-68), FullyConnect (fullyconnect.cc:7-19), SEUnit::Forward
(se_unit.cc:70-128) and the head tail of BlasForwardPipe::Forward (blas_forward_pipe.cc:496-580), through the oracle's
layer taps (oracle/sayuri_oracle.c so_tap_*).  Board sizes 2..19, mixed batches, all eight activations.

fp32 engine: abs <= 2e-5 * scale.  fp16 engine: the kernels see fp16-rounded activations (the oracle is given the same
rounded values) and store fp16 -> 2e-3 * scale on activations, 1e-4 on the fp32 outputs of the heads / gates.

The convolutions with the SE unit inside: conv_board_se_kernel / the tower's SE stage against a float64 convolution + the
oracle's unit (test_conv_with_se_unit_inside), and the split-channel form conv_board_sx_kernel (conv_board_sx.h, test_sx_*)
against a float64 convolution + se_unit_f64 -- a float64 restatement of the unit that tests/test_sx_reference_cpu.py pins to
the oracle's -- on inputs drawn so that the unit matters (sx_trunk / sx_fc: the same CPU module proves that a wrong mean
term, a wrong pixel count, a neighbour's maximum or gate, a missing eighth of the pool and a missing sibling partial each
move the result by >= 4x the tolerance).  3e-3 * max(1, |ref|max), as for the one-workgroup form: fp32 accumulators gated
in registers, fp16 FC images, fp16 store."""
import ctypes
import functools

import numpy as np
import pytest

from _oracle import PortNet
from sayuri_amd import _lib
from test_gpu_layers import act_np

pytestmark = pytest.mark.gpu

FP = ctypes.POINTER(ctypes.c_float)


def _fp(a):
    return a.ctypes.data_as(FP)


def oracle():
    lib = PortNet.lib()
    lib.so_tap_se_unit.argtypes = [ctypes.c_int] * 3 + [FP] * 6 + [ctypes.c_int]
    lib.so_tap_global_pool.argtypes = [ctypes.c_int, ctypes.c_int, FP, FP, ctypes.c_int]
    lib.so_tap_fully_connect.argtypes = [ctypes.c_int, ctypes.c_int, FP, FP, FP, FP, ctypes.c_int]
    lib.so_tap_head_tail.argtypes = [ctypes.c_int] * 7 + [FP] * 18
    return lib


def r16(a, fp16):
    return a.astype(np.float16).astype(np.float32) if fp16 else a


BOARDS = [[19], [9, 13, 19], [2, 3, 5, 7, 19, 4], [19] * 5, [13, 13, 9, 9, 9, 19, 6]]


@pytest.mark.parametrize("fp16", [False, True], ids=["fp32", "fp16"])
@pytest.mark.parametrize("act", range(8))
def test_se_unit_kernels(act, fp16):
    lib, o = _lib.hip(), oracle()
    rng = np.random.default_rng(100 + act)
    for bsz, C, se, with_res in ((BOARDS[act % len(BOARDS)], 64, 16, True), (BOARDS[(act + 1) % len(BOARDS)], 96, 24, False),
                                 ([19, 9], 256, 64, True)):
        n = len(bsz)
        xs = [r16(rng.standard_normal((C, b * b)).astype(np.float32), fp16) for b in bsz]
        rs = [r16(rng.standard_normal((C, b * b)).astype(np.float32), fp16) for b in bsz] if with_res else None
        w1 = (rng.standard_normal((se, 3 * C)) / np.sqrt(3 * C)).astype(np.float32)
        b1 = (rng.standard_normal(se) * 0.1).astype(np.float32)
        w2 = (rng.standard_normal((2 * C, se)) / np.sqrt(se)).astype(np.float32)
        b2 = (rng.standard_normal(2 * C) * 0.1).astype(np.float32)
        xcat = np.concatenate([x.ravel() for x in xs])
        rcat = np.concatenate([r.ravel() for r in rs]) if rs else None
        y = np.zeros_like(xcat)
        gate = np.zeros((n, 2 * C), np.float32)
        bs_arr = np.asarray(bsz, np.int32)
        lib.sayuri_hip_test_se_unit.argtypes = [ctypes.c_int] * 3 + [_lib.c_int_p] + [ctypes.c_int] * 4 + [FP] * 8
        rc = lib.sayuri_hip_test_se_unit(0, int(fp16), n, bs_arr.ctypes.data_as(_lib.c_int_p), 19, C, se, act, _fp(xcat),
                                         _fp(rcat) if rs else None, _fp(w1), _fp(b1), _fp(w2), _fp(b2), _fp(y), _fp(gate))
        assert rc == 0, lib.sayuri_hip_last_error().decode()
        off = 0
        for i, b in enumerate(bsz):
            S = b * b
            # GlobalPooling<false> + both FullyConnects -> the gate
            pool = np.zeros(3 * C, np.float32)
            o.so_tap_global_pool(b, C, _fp(xs[i]), _fp(pool), 0)
            mid = np.zeros(se, np.float32)
            o.so_tap_fully_connect(3 * C, se, _fp(w1), _fp(b1), _fp(pool), _fp(mid), act)
            exc = np.zeros(2 * C, np.float32)
            o.so_tap_fully_connect(se, 2 * C, _fp(w2), _fp(b2), _fp(mid), _fp(exc), 0)
            exp_gate = np.concatenate([1.0 / (1.0 + np.exp(-exc[:C].astype(np.float64))), exc[C:]])
            assert np.abs(gate[i] - exp_gate).max() <= 1e-4 * max(1.0, np.abs(exp_gate).max()), (bsz, i, "gate")
            # the whole unit
            ref = xs[i].copy()
            o.so_tap_se_unit(b, C, se, _fp(w1), _fp(b1), _fp(w2), _fp(b2), _fp(ref), _fp(rs[i]) if rs else None, act)
            got = y[off:off + C * S].reshape(C, S)
            off += C * S
            scale = max(1.0, float(np.abs(ref).max()))
            tol = (2e-3 if fp16 else 2e-5) * scale
            assert np.isfinite(got).all()
            assert np.abs(got - ref).max() <= tol, (bsz, i, act, float(np.abs(got - ref).max()), tol)


@pytest.mark.parametrize("fp16", [False, True], ids=["fp32", "fp16"])
@pytest.mark.parametrize("act", range(8))
def test_head_tail_kernel(act, fp16):
    lib, o = _lib.hip(), oracle()
    rng = np.random.default_rng(200 + act)
    for bsz, Cp, Cv in ((BOARDS[act % len(BOARDS)], 24, 24), (BOARDS[(act + 2) % len(BOARDS)], 32, 48), ([19, 13], 48, 32)):
        n, prob_ch, pass_outs, misc_outs, B2 = len(bsz), 5, 5, 15, 361
        pcs = [r16(rng.standard_normal((Cp, b * b)).astype(np.float32), fp16) for b in bsz]
        vcs = [r16(rng.standard_normal((Cv, b * b)).astype(np.float32), fp16) for b in bsz]
        shapes = [(Cp, 3 * Cp), (Cp,), (pass_outs, Cp), (pass_outs,), (3 * Cv, 3 * Cv), (3 * Cv,), (misc_outs, 3 * Cv), (misc_outs,),
                  (prob_ch, Cp), (prob_ch,), (Cv,), (1,)]
        ws = [(rng.standard_normal(s) / np.sqrt(s[-1] if len(s) > 1 else 4)).astype(np.float32) for s in shapes]
        warr = (FP * 12)(*[_fp(w) for w in ws])
        pcat = np.concatenate([p.ravel() for p in pcs])
        vcat = np.concatenate([v.ravel() for v in vcs])
        prob = np.zeros((n, prob_ch, B2), np.float32)
        pas = np.zeros((n, pass_outs), np.float32)
        misc = np.zeros((n, misc_outs), np.float32)
        own = np.zeros((n, B2), np.float32)
        bs_arr = np.asarray(bsz, np.int32)
        lib.sayuri_hip_test_head_tail.argtypes = [ctypes.c_int] * 3 + [_lib.c_int_p] + [ctypes.c_int] * 7 + [FP, FP, ctypes.POINTER(FP)] + [FP] * 4
        rc = lib.sayuri_hip_test_head_tail(0, int(fp16), n, bs_arr.ctypes.data_as(_lib.c_int_p), 19, Cp, Cv, prob_ch, pass_outs, misc_outs, act,
                                           _fp(pcat), _fp(vcat), warr, _fp(prob), _fp(pas), _fp(misc), _fp(own))
        assert rc == 0, lib.sayuri_hip_last_error().decode()
        for i, b in enumerate(bsz):
            S = b * b
            e_prob, e_pass = np.zeros((prob_ch, S), np.float32), np.zeros(pass_outs, np.float32)
            e_own, e_misc = np.zeros(S, np.float32), np.zeros(misc_outs, np.float32)
            pc = pcs[i].copy()
            o.so_tap_head_tail(b, Cp, Cv, prob_ch, pass_outs, misc_outs, act, _fp(pc), _fp(vcs[i]), *[_fp(w) for w in ws],
                               _fp(e_prob), _fp(e_pass), _fp(e_own), _fp(e_misc))
            tol = 2e-4
            got_prob = prob[i].reshape(prob_ch, 19, 19)[:, :b, :b].reshape(prob_ch, S)
            got_own = own[i].reshape(19, 19)[:b, :b].ravel()
            assert np.abs(got_prob - e_prob).max() <= tol * max(1.0, np.abs(e_prob).max()), (bsz, i, "prob")
            assert np.abs(got_own - e_own).max() <= tol * max(1.0, np.abs(e_own).max()), (bsz, i, "own")
            assert np.abs(pas[i] - e_pass).max() <= tol * max(1.0, np.abs(e_pass).max()), (bsz, i, "pass")
            assert np.abs(misc[i] - e_misc).max() <= tol * max(1.0, np.abs(e_misc).max()), (bsz, i, "misc")
            # off-board cells of a smaller sample stay 0 in the NN grid
            mask = np.ones((19, 19), bool)
            mask[:b, :b] = False
            assert not prob[i].reshape(prob_ch, 19, 19)[:, mask].any() and not own[i].reshape(19, 19)[mask].any()


def conv3x3_f64(x, w, bias, b):
    """float64 direct 3x3 convolution of one sample: x [C][b*b], w [K][C][3][3] -> [K][b*b]"""
    C, K = x.shape[0], w.shape[0]
    xp = np.zeros((C, b + 2, b + 2), np.float64)
    xp[:, 1:-1, 1:-1] = x.reshape(C, b, b)
    y = np.zeros((K, b, b), np.float64)
    for dy in range(3):
        for dx in range(3):
            y += np.einsum("kc,cyx->kyx", w[:, :, dy, dx].astype(np.float64), xp[:, dy:dy + b, dx:dx + b], optimize=True)
    return (y + bias.astype(np.float64)[:, None, None]).reshape(K, b * b)


def se_pool_f64(x, bs):
    """GlobalPooling<false> (se_unit.cc:9-40) of x [C][bs*bs] in float64: (mean, mean * (bs - 14) / 10, max) -> [3C]"""
    x = np.asarray(x, np.float64)
    mean = x.sum(axis=1) / float(bs * bs)
    return np.concatenate([mean, mean * ((bs - 14.0) / 10.0), x.max(axis=1)])


def se_gate_f64(pool, w1, b1, w2, b2, act):
    """squeeze FC with `act`, excite FC: pooled [3C] -> (sigmoid(gamma) [C], beta [C]), float64"""
    mid = act_np(np.asarray(w1, np.float64) @ pool + np.asarray(b1, np.float64), act)
    exc = np.asarray(w2, np.float64) @ mid + np.asarray(b2, np.float64)
    C = exc.shape[0] // 2
    return 1.0 / (1.0 + np.exp(-exc[:C])), exc[C:]


def se_apply_f64(x, res, gamma, beta, act):
    v = gamma[:, None] * np.asarray(x, np.float64) + beta[:, None]
    if res is not None:
        v = v + np.asarray(res, np.float64)
    return act_np(v, act)


def se_unit_f64(x, res, w1, b1, w2, b2, bs, act):
    """SEUnit::Forward (se_unit.cc:70-128) on x [C][bs*bs] in float64 throughout: pool = (mean, mean * (bs-14)/10, max),
    squeeze FC with `act`, excite FC, act(sigmoid(gamma) * x + beta + res).  w1 [se][3C], w2 [2C][se]; res or None."""
    gamma, beta = se_gate_f64(se_pool_f64(x, bs), w1, b1, w2, b2, act)
    return se_apply_f64(x, res, gamma, beta, act)


# ---- inputs of the split-channel SE convolution tests.  With x ~ N(0, 1) per pixel a channel's mean is ~ 1 / sqrt(npix) and
# the unit's gates sit near 0.5: a wrong mean row of the squeeze image would move nothing.  So the convolution gets a bias
# of O(1) per channel (pooled means of O(1) that differ by channel), and the two FCs are scaled to pre-activations of O(1)
# (gates spread over ~0.1 .. 0.9).  tests/test_sx_reference_cpu.py proves on these very draws that the unit's terms matter.
SX_TOL = 3e-3


class SxTrunk:
    """x, w, bias, res of one C -> C 3x3 layer over the boards `bsz` (x, w, res rounded to fp16 as the kernel sees them), and
    the float64 convolution of each sample, computed once on demand."""

    def __init__(self, seed, bsz, C):
        rng = np.random.default_rng([seed, C] + list(bsz))
        self.bsz, self.C = list(bsz), C
        self.xs = [r16(rng.standard_normal((C, b * b)).astype(np.float32), True) for b in bsz]
        self.rs = [r16(rng.standard_normal((C, b * b)).astype(np.float32), True) for b in bsz]
        self.w = r16((rng.standard_normal((C, C, 3, 3)) / np.sqrt(9 * C)).astype(np.float32), True)
        self.bias = rng.standard_normal(C).astype(np.float32)
        self._conv = {}

    def conv(self, i):
        if i not in self._conv:
            self._conv[i] = conv3x3_f64(self.xs[i], self.w, self.bias, self.bsz[i])
            self._conv[i].setflags(write=False)
        return self._conv[i]


@functools.lru_cache(maxsize=None)
def sx_trunk(seed, bsz, C):
    return SxTrunk(seed, bsz, C)


@functools.lru_cache(maxsize=None)
def sx_fc(seed, C, se):
    """w1 [se][3C], b1 [se], w2 [2C][se], b2 [2C] of the unit"""
    rng = np.random.default_rng([seed, C, se, 77])
    w1 = (rng.standard_normal((se, 3 * C)) / np.sqrt(3 * C)).astype(np.float32)
    b1 = (rng.standard_normal(se) * 0.5).astype(np.float32)
    w2 = (rng.standard_normal((2 * C, se)) / np.sqrt(se)).astype(np.float32)
    b2 = (rng.standard_normal(2 * C) * 0.5).astype(np.float32)
    return w1, b1, w2, b2


def sx_reference(T, fc, i, act, with_res):
    return se_unit_f64(T.conv(i), T.rs[i] if with_res else None, *fc, T.bsz[i], act)


@pytest.mark.parametrize("via_tower", [0, 1], ids=["per-layer kernel", "tower kernel"])
@pytest.mark.parametrize("act", range(8))
def test_conv_with_se_unit_inside(act, via_tower):
    """conv_board_se_kernel / the SE body of the persistent tower kernel at kernel level: float64 convolution followed by
    the oracle's SEUnit::Forward tap (se_unit.cc:70-128) on it.  Boards 2..19, C = 96 / 128 / 256, se = 24 / 32 / 64,
    one sample per tile (fused) and several samples per tile (the tap must report the fallback)."""
    lib, o = _lib.hip(), oracle()
    rng = np.random.default_rng(300 + act)
    lib.sayuri_hip_test_conv_se.argtypes = [ctypes.c_int] * 2 + [_lib.c_int_p] + [ctypes.c_int] * 5 + [FP] * 9
    cases = [([19, 19, 19], 256, 64, True), ([19] * 2, 128, 32, False), ([19, 17, 16, 15, 14], 128, 24, True), ([19], 96, 24, True)]
    # small boards one per batch (a batch of several small boards shares a tile: checked below)
    cases += [([b], 128, 32, bool(b & 1)) for b in (2, 3, 5, 9, 13)][act % 5:act % 5 + 2]
    for bsz, C, se, with_res in cases:
        n = len(bsz)
        xs = [r16(rng.standard_normal((C, b * b)).astype(np.float32), True) for b in bsz]
        rs = [r16(rng.standard_normal((C, b * b)).astype(np.float32), True) for b in bsz] if with_res else None
        w = r16((rng.standard_normal((C, C, 3, 3)) / np.sqrt(9 * C)).astype(np.float32), True)
        bias = (rng.standard_normal(C) * 0.1).astype(np.float32)
        w1 = (rng.standard_normal((se, 3 * C)) / np.sqrt(3 * C)).astype(np.float32)
        b1 = (rng.standard_normal(se) * 0.1).astype(np.float32)
        w2 = (rng.standard_normal((2 * C, se)) / np.sqrt(se)).astype(np.float32)
        b2 = (rng.standard_normal(2 * C) * 0.1).astype(np.float32)
        xcat = np.concatenate([x.ravel() for x in xs])
        rcat = np.concatenate([r.ravel() for r in rs]) if rs else None
        y = np.zeros_like(xcat)
        bs_arr = np.asarray(bsz, np.int32)
        rc = lib.sayuri_hip_test_conv_se(0, n, bs_arr.ctypes.data_as(_lib.c_int_p), 19, C, se, act, via_tower, _fp(xcat), _fp(w), _fp(bias),
                                         _fp(rcat) if rs else None, _fp(w1), _fp(b1), _fp(w2), _fp(b2), _fp(y))
        if C % 128:  # no board kernel for this channel count (the engine runs such layers on conv_mfma + the separate SE kernels)
            assert rc == 1
            continue
        assert rc == 0, (bsz, C, rc, lib.sayuri_hip_last_error().decode())
        off = 0
        for i, b in enumerate(bsz):
            S = b * b
            ref = conv3x3_f64(xs[i], w, bias, b).astype(np.float32)
            ref = np.ascontiguousarray(ref)
            o.so_tap_se_unit(b, C, se, _fp(w1), _fp(b1), _fp(w2), _fp(b2), _fp(ref), _fp(rs[i]) if rs else None, act)
            got = y[off:off + C * S].reshape(C, S)
            off += C * S
            scale = max(1.0, float(np.abs(ref).max()))
            assert np.isfinite(got).all()
            # fp16 store + fp16 FC weights: 3e-3 of the output scale
            assert np.abs(got - ref).max() <= 3e-3 * scale, (bsz, i, C, act, float(np.abs(got - ref).max()), scale)
    # several samples in one tile: the fused kernel does not apply, the tap says so (the engine runs conv + se_pool / se_fc / se_scale)
    bs_arr = np.asarray([9, 9, 9, 9], np.int32)
    dummy = np.zeros(4 * 128 * 81, np.float32)
    w = np.zeros((128, 128, 3, 3), np.float32)
    z = np.zeros(3 * 128 * 32 + 512, np.float32)
    rc = lib.sayuri_hip_test_conv_se(0, 4, bs_arr.ctypes.data_as(_lib.c_int_p), 19, 128, 32, act, via_tower, _fp(dummy), _fp(w), _fp(z), None,
                                     _fp(z), _fp(z), _fp(z), _fp(z), _fp(dummy.copy()))
    assert rc == 1


@pytest.mark.parametrize("act", range(8))
def test_head_board_kernel(act):
    """head_board_kernel at kernel level: the two 1x1 head convolutions in float64 (on the fp16-rounded trunk), rounded to
    nothing, then the oracle's head-tail tap (blas_forward_pipe.cc:449-580).  Boards 2..19, C = 128 / 256, Cp / Cv =
    24 / 32 / 48."""
    lib, o = _lib.hip(), oracle()
    rng = np.random.default_rng(400 + act)
    lib.sayuri_hip_test_head_board.argtypes = [ctypes.c_int] * 2 + [_lib.c_int_p] + [ctypes.c_int] * 8 + [FP] * 5 + [ctypes.POINTER(FP)] + [FP] * 4
    for bsz, C, Cp, Cv in ((BOARDS[act % len(BOARDS)], 128, 24, 24), (BOARDS[(act + 2) % len(BOARDS)], 256, 32, 32), ([19, 13, 2], 256, 32, 48),
                           ([19, 5], 128, 48, 32)):
        n, prob_ch, pass_outs, misc_outs, B2 = len(bsz), 5, 5, 15, 361
        ts = [r16(rng.standard_normal((C, b * b)).astype(np.float32), True) for b in bsz]
        p_w = r16((rng.standard_normal((Cp, C)) / np.sqrt(C)).astype(np.float32), True)
        v_w = r16((rng.standard_normal((Cv, C)) / np.sqrt(C)).astype(np.float32), True)
        p_b = (rng.standard_normal(Cp) * 0.1).astype(np.float32)
        v_b = (rng.standard_normal(Cv) * 0.1).astype(np.float32)
        shapes = [(Cp, 3 * Cp), (Cp,), (pass_outs, Cp), (pass_outs,), (3 * Cv, 3 * Cv), (3 * Cv,), (misc_outs, 3 * Cv), (misc_outs,),
                  (prob_ch, Cp), (prob_ch,), (Cv,), (1,)]
        ws = [(rng.standard_normal(s) / np.sqrt(s[-1] if len(s) > 1 else 4)).astype(np.float32) for s in shapes]
        ws[8] = r16(ws[8], True)   # the per-pixel weights are an fp16 MFMA image in the kernel
        ws[10] = r16(ws[10], True)
        warr = (FP * 12)(*[_fp(w) for w in ws])
        tcat = np.concatenate([t.ravel() for t in ts])
        prob = np.zeros((n, prob_ch, B2), np.float32)
        pas = np.zeros((n, pass_outs), np.float32)
        misc = np.zeros((n, misc_outs), np.float32)
        own = np.zeros((n, B2), np.float32)
        bs_arr = np.asarray(bsz, np.int32)
        rc = lib.sayuri_hip_test_head_board(0, n, bs_arr.ctypes.data_as(_lib.c_int_p), 19, C, Cp, Cv, prob_ch, pass_outs, misc_outs, act,
                                            _fp(tcat), _fp(p_w), _fp(p_b), _fp(v_w), _fp(v_b), warr, _fp(prob), _fp(pas), _fp(misc), _fp(own))
        assert rc == 0, (bsz, C, Cp, Cv, rc, lib.sayuri_hip_last_error().decode())
        for i, b in enumerate(bsz):
            S = b * b
            from test_gpu_layers import act_np
            pc = act_np(p_w.astype(np.float64) @ ts[i].astype(np.float64) + p_b[:, None], act).astype(np.float32)
            vc = act_np(v_w.astype(np.float64) @ ts[i].astype(np.float64) + v_b[:, None], act).astype(np.float32)
            pc, vc = np.ascontiguousarray(pc), np.ascontiguousarray(vc)
            e_prob, e_pass = np.zeros((prob_ch, S), np.float32), np.zeros(pass_outs, np.float32)
            e_own, e_misc = np.zeros(S, np.float32), np.zeros(misc_outs, np.float32)
            o.so_tap_head_tail(b, Cp, Cv, prob_ch, pass_outs, misc_outs, act, _fp(pc), _fp(vc), *[_fp(w) for w in ws],
                               _fp(e_prob), _fp(e_pass), _fp(e_own), _fp(e_misc))
            # the head planes stay in fp32 registers; the per-pixel product runs on fp16-rounded planes: 2e-3 of the scale
            tol = 2e-3
            got_prob = prob[i].reshape(prob_ch, 19, 19)[:, :b, :b].reshape(prob_ch, S)
            got_own = own[i].reshape(19, 19)[:b, :b].ravel()
            assert np.abs(got_prob - e_prob).max() <= tol * max(1.0, np.abs(e_prob).max()), (bsz, i, "prob", float(np.abs(got_prob - e_prob).max()))
            assert np.abs(got_own - e_own).max() <= tol * max(1.0, np.abs(e_own).max()), (bsz, i, "own")
            assert np.abs(pas[i] - e_pass).max() <= tol * max(1.0, np.abs(e_pass).max()), (bsz, i, "pass")
            assert np.abs(misc[i] - e_misc).max() <= tol * max(1.0, np.abs(e_misc).max()), (bsz, i, "misc")
            mask = np.ones((19, 19), bool)
            mask[:b, :b] = False
            assert not prob[i].reshape(prob_ch, 19, 19)[:, mask].any() and not own[i].reshape(19, 19)[mask].any()


# ------------------------------------------------------------------ conv_board_sx_kernel (conv_board_sx.h) at layer level
KIND_BOARD_SX = 5
SX_STANDARD = (19,) * 5 + (13,) * 5 + (9,) * 6  # 10 tiles: a second group of 8 with empty places, partial tiles of 13 and of 9


def sx_lib():
    lib = _lib.hip()
    lib.sayuri_hip_test_conv_sx.argtypes = [ctypes.c_int] * 2 + [_lib.c_int_p] + [ctypes.c_int] * 4 + [FP] * 9
    return lib


def sx_call(bsz, C, se, act, xs, rs, w, bias, fc, max_board=19):
    """One launch of the tap.  y starts as NaN on the host (and in the tap's device buffer): what comes back finite was written.
    -> (return code, [y of each sample [C][b*b]])"""
    lib = sx_lib()
    xcat = np.concatenate([x.ravel() for x in xs])
    rcat = np.concatenate([r.ravel() for r in rs]) if rs is not None else None
    y = np.full(xcat.shape, np.nan, np.float32)
    bs_arr = np.asarray(bsz, np.int32)
    rc = lib.sayuri_hip_test_conv_sx(0, len(bsz), bs_arr.ctypes.data_as(_lib.c_int_p), max_board, C, se, act, _fp(xcat), _fp(w), _fp(bias),
                                     _fp(rcat) if rcat is not None else None, *[_fp(a) for a in fc], _fp(y))
    outs, off = [], 0
    for b in bsz:
        outs.append(y[off:off + C * b * b].reshape(C, b * b))
        off += C * b * b
    return rc, outs


def sx_run(seed, bsz, C, se, act, with_res, kts, check=None):
    """The layer of sx_trunk(seed, bsz, C) / sx_fc(seed, C, se) through the tap: it must run, on `kts` channel tiles per board
    tile; every output finite; the samples `check` (default: all) within SX_TOL of conv3x3_f64 + se_unit_f64."""
    T, fc = sx_trunk(seed, tuple(bsz), C), sx_fc(seed, C, se)
    rc, outs = sx_call(T.bsz, C, se, act, T.xs, T.rs if with_res else None, T.w, T.bias, fc)
    lib = sx_lib()
    assert rc == 0, (bsz, C, se, rc, lib.sayuri_hip_last_error().decode())
    assert lib.sayuri_hip_test_last_conv_kind() == KIND_BOARD_SX
    ran_kts = lib.sayuri_hip_test_last_sx_kts()
    print(f"conv_board_sx C={C} se={se} act={act} res={int(with_res)} boards={list(bsz)}: kts={ran_kts}")
    assert ran_kts == kts, (C, ran_kts, kts)
    for i, got in enumerate(outs):
        assert np.isfinite(got).all(), (bsz, C, se, act, i, "an output nobody wrote, or a non-finite one")
    for i in (range(len(bsz)) if check is None else check):
        ref = sx_reference(T, fc, i, act, with_res)
        tol = SX_TOL * max(1.0, float(np.abs(ref).max()))
        err = float(np.abs(outs[i] - ref).max())
        print(f"  sample {i} ({T.bsz[i]}x{T.bsz[i]}): err {err:.5f}, tol {tol:.5f}")
        assert err <= tol, (bsz, C, se, act, with_res, i, err, tol)
    return outs


@pytest.mark.parametrize("with_res", [True, False], ids=["res", "nores"])
def test_sx_standard_layer_more_than_8_tiles(with_res):
    """C = 384, se = 96 on 10 tiles: 5 of 19x19, 13x13 as (2, 2, 1), 9x9 as (4, 2) -- the 9x9 tiles are the second group of 8
    (block index >= 8 kts), whose other six places are empty.  Checked: the first and last sample of every tile kind."""
    check = (0, 4, 5, 6, 8, 9, 10, 13, 14, 15)
    sx_run(1, SX_STANDARD, 384, 96, 5, with_res, 3, check)


@pytest.mark.parametrize("bsz", [(10,) * 4 + (11,) * 3 + (12,) * 3, (14, 15, 16, 17, 18)], ids=["10-11-12", "14..18"])
def test_sx_three_per_tile_and_alone_in_a_tile(bsz):
    """10x10 and 11x11 are the only sizes with three samples per tile (3 x 11x11 = 507 of the 512 halo positions); 14..18 sit
    alone in a tile, each with its own eighth length ceil(npix / 8)."""
    sx_run(2, bsz, 384, 96, 5, True, 3)


@pytest.mark.parametrize("with_res", [True, False], ids=["res", "nores"])
@pytest.mark.parametrize("act", range(8))
def test_sx_activations(act, with_res):
    """Every activation in mid = activate(...) and in the epilogue's switch (the trunk and its float64 convolution are shared)."""
    sx_run(3, (13, 13, 9, 9, 9, 19), 384, 48, act, with_res, 3)


@pytest.mark.parametrize("C,se,kts", [(256, 96, 2), (512, 64, 4)], ids=["kts2", "kts4"])
def test_sx_channel_tile_counts(C, se, kts):
    """Two and four sibling workgroups per board tile.  (C = 256 reaches this kernel in the engine when the one-workgroup
    images of make_se_images do not fit, se >= 72; se = 64 at kts = 4 fills the whole `red` area, parts * se = 2048.)"""
    sx_run(4, (19, 13, 13, 9, 9, 9, 9), C, se, 5, True, kts)


def test_sx_pad_channels():
    """C = 360 in a 384-row image: channels 360..383 of the third channel tile are padding (zero weight rows, zero image rows)."""
    sx_run(5, (19, 11, 11, 11), 360, 96, 5, True, 3)


@pytest.mark.parametrize("se", [100, 64, 20, 4])
def test_sx_se_width_edges(se):
    """se = 100: the two images fill SxLds::stage_bytes to the byte (51200 + 53248); 64: quads = 16, parts * se = 2048; 20: quads
    = 5 does not divide 512; 4: quads = 1."""
    sx_run(6, (13, 13, 9), 384, se, 5, True, 3)


def test_sx_refusals():
    """Shapes the form does not apply to return 1 -- never a launch, never an error: a board of which more than four fit a tile,
    one channel tile, an SE width whose images do not fit the stage area (104) or that is no multiple of 4 (6)."""
    lib = sx_lib()
    for bsz, C, se in (((9, 9, 8), 384, 96), ((19, 5), 384, 96), ((19, 9), 128, 32), ((13, 9), 384, 104), ((13, 9), 384, 6)):
        T = sx_trunk(7, bsz, C)
        rng = np.random.default_rng(se)
        fc = [rng.standard_normal(s).astype(np.float32) for s in ((se, 3 * C), (se,), (2 * C, se), (2 * C,))]
        rc, outs = sx_call(T.bsz, C, se, 5, T.xs, T.rs, T.w, T.bias, fc)
        assert rc == 1, (bsz, C, se, rc, lib.sayuri_hip_last_error().decode())
        assert lib.sayuri_hip_test_last_sx_kts() == 0
        assert all(np.isnan(o).all() for o in outs)  # nothing was written


@pytest.mark.parametrize("bs,full", [(9, 4), (11, 3)], ids=["9x9", "11x11"])
def test_sx_position_independence_on_bits(bs, full):
    """A sample's result is a function of the sample alone (README): one board gives the same BITS alone, first and last in a
    full tile of its size, in a partial tile, and inside a 10-tile batch (the standard one for 9x9; for 11x11 the same batch
    with seven 11x11 in place of the 13x13: tiles of 3, 3 and 1)."""
    C, se, act = 384, 96, 5
    big = SX_STANDARD if bs == 9 else (19,) * 5 + (11,) * 7 + (9,) * 6
    T, fc = sx_trunk(8, big, C), sx_fc(8, C, se)
    pool = [i for i, b in enumerate(big) if b == bs]  # the samples of this size: the probe and its fillers
    probe, fill = pool[1], [pool[0]] + pool[2:]

    def run(order):
        rc, outs = sx_call([T.bsz[i] for i in order], C, se, act, [T.xs[i] for i in order], [T.rs[i] for i in order], T.w, T.bias, fc)
        assert rc == 0, (order, rc, sx_lib().sayuri_hip_last_error().decode())
        assert sx_lib().sayuri_hip_test_last_sx_kts() == 3
        got = outs[order.index(probe)]
        assert np.isfinite(got).all()
        return got

    alone = run([probe])
    ref = sx_reference(T, fc, probe, act, True)
    assert np.abs(alone - ref).max() <= SX_TOL * max(1.0, float(np.abs(ref).max()))
    situations = {
        "first in a full tile": [probe] + fill[:full - 1],
        "last in a full tile": fill[:full - 1] + [probe],
        "in a partial tile": [fill[0], probe],
        "behind a full tile, alone in the next": fill[:full] + [probe],
        "inside the 10-tile batch": list(range(len(big))),
    }
    for name, order in situations.items():
        np.testing.assert_array_equal(run(order), alone, err_msg=name)
