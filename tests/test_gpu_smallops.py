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
in registers, fp16 FC images, fp16 store.

The *_pooled_statistics cases at the end run the one-workgroup SE kernels (both forms of the unit: staged images, FCs from L2),
se_pool / se_fc / se_scale and both head kernels on inputs that make every pooled statistic visible, against se_unit_f64 and
head_tail_f64, at the tolerances above; tests/test_se_head_reference_cpu.py holds the float64 references and the inputs to
account.  Measured on an MI355X, worst error / tolerance: convolution + unit 0.18 (staged) and 0.15 (from L2), per-layer and
tower alike; se_pool / se_fc / se_scale 0.24 (fp16), 0.03 (fp32), gate 0.01; head_board 0.41; head_tail < 0.01."""
import ctypes
import functools

import numpy as np
import pytest

from _oracle import PortNet
from sayuri_amd import _lib
from test_gpu_layers import act_np

pytestmark = pytest.mark.gpu

FP = ctypes.POINTER(ctypes.c_float)


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
        rc = lib.sayuri_hip_test_se_unit(0, int(fp16), n, bs_arr.ctypes.data_as(_lib.c_int_p), 19, C, se, act, _lib.fp(xcat),
                                         _lib.fp(rcat) if rs else None, _lib.fp(w1), _lib.fp(b1), _lib.fp(w2), _lib.fp(b2), _lib.fp(y), _lib.fp(gate))
        assert rc == 0, lib.sayuri_hip_last_error().decode()
        off = 0
        for i, b in enumerate(bsz):
            S = b * b
            # GlobalPooling<false> + both FullyConnects -> the gate
            pool = np.zeros(3 * C, np.float32)
            o.so_tap_global_pool(b, C, _lib.fp(xs[i]), _lib.fp(pool), 0)
            mid = np.zeros(se, np.float32)
            o.so_tap_fully_connect(3 * C, se, _lib.fp(w1), _lib.fp(b1), _lib.fp(pool), _lib.fp(mid), act)
            exc = np.zeros(2 * C, np.float32)
            o.so_tap_fully_connect(se, 2 * C, _lib.fp(w2), _lib.fp(b2), _lib.fp(mid), _lib.fp(exc), 0)
            exp_gate = np.concatenate([1.0 / (1.0 + np.exp(-exc[:C].astype(np.float64))), exc[C:]])
            assert np.abs(gate[i] - exp_gate).max() <= 1e-4 * max(1.0, np.abs(exp_gate).max()), (bsz, i, "gate")
            # the whole unit
            ref = xs[i].copy()
            o.so_tap_se_unit(b, C, se, _lib.fp(w1), _lib.fp(b1), _lib.fp(w2), _lib.fp(b2), _lib.fp(ref), _lib.fp(rs[i]) if rs else None, act)
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
        warr = (FP * 12)(*[_lib.fp(w) for w in ws])
        pcat = np.concatenate([p.ravel() for p in pcs])
        vcat = np.concatenate([v.ravel() for v in vcs])
        prob = np.zeros((n, prob_ch, B2), np.float32)
        pas = np.zeros((n, pass_outs), np.float32)
        misc = np.zeros((n, misc_outs), np.float32)
        own = np.zeros((n, B2), np.float32)
        bs_arr = np.asarray(bsz, np.int32)
        rc = lib.sayuri_hip_test_head_tail(0, int(fp16), n, bs_arr.ctypes.data_as(_lib.c_int_p), 19, Cp, Cv, prob_ch, pass_outs, misc_outs, act,
                                           _lib.fp(pcat), _lib.fp(vcat), warr, _lib.fp(prob), _lib.fp(pas), _lib.fp(misc), _lib.fp(own))
        assert rc == 0, lib.sayuri_hip_last_error().decode()
        for i, b in enumerate(bsz):
            S = b * b
            e_prob, e_pass = np.zeros((prob_ch, S), np.float32), np.zeros(pass_outs, np.float32)
            e_own, e_misc = np.zeros(S, np.float32), np.zeros(misc_outs, np.float32)
            pc = pcs[i].copy()
            o.so_tap_head_tail(b, Cp, Cv, prob_ch, pass_outs, misc_outs, act, _lib.fp(pc), _lib.fp(vcs[i]), *[_lib.fp(w) for w in ws],
                               _lib.fp(e_prob), _lib.fp(e_pass), _lib.fp(e_own), _lib.fp(e_misc))
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
        rc = lib.sayuri_hip_test_conv_se(0, n, bs_arr.ctypes.data_as(_lib.c_int_p), 19, C, se, act, via_tower, _lib.fp(xcat), _lib.fp(w), _lib.fp(bias),
                                         _lib.fp(rcat) if rs else None, _lib.fp(w1), _lib.fp(b1), _lib.fp(w2), _lib.fp(b2), _lib.fp(y))
        if C % 128:  # no board kernel for this channel count (the engine runs such layers on conv_mfma + the separate SE kernels)
            assert rc == 1
            continue
        assert rc == 0, (bsz, C, rc, lib.sayuri_hip_last_error().decode())
        off = 0
        for i, b in enumerate(bsz):
            S = b * b
            ref = conv3x3_f64(xs[i], w, bias, b).astype(np.float32)
            ref = np.ascontiguousarray(ref)
            o.so_tap_se_unit(b, C, se, _lib.fp(w1), _lib.fp(b1), _lib.fp(w2), _lib.fp(b2), _lib.fp(ref), _lib.fp(rs[i]) if rs else None, act)
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
    rc = lib.sayuri_hip_test_conv_se(0, 4, bs_arr.ctypes.data_as(_lib.c_int_p), 19, 128, 32, act, via_tower, _lib.fp(dummy), _lib.fp(w), _lib.fp(z), None,
                                     _lib.fp(z), _lib.fp(z), _lib.fp(z), _lib.fp(z), _lib.fp(dummy.copy()))
    assert rc == 1


@pytest.mark.parametrize("act", range(8))
def test_head_board_kernel(act):
    """head_board_kernel at kernel level: the two 1x1 head convolutions in float64 (on the fp16-rounded trunk), rounded to
    nothing, then the oracle's head-tail tap (blas_forward_pipe.cc:449-580).  Boards 2..19, C = 128 / 256, Cp / Cv =
    24 / 32 / 48."""
    lib, o = _lib.hip(), oracle()
    rng = np.random.default_rng(400 + act)
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
        warr = (FP * 12)(*[_lib.fp(w) for w in ws])
        tcat = np.concatenate([t.ravel() for t in ts])
        prob = np.zeros((n, prob_ch, B2), np.float32)
        pas = np.zeros((n, pass_outs), np.float32)
        misc = np.zeros((n, misc_outs), np.float32)
        own = np.zeros((n, B2), np.float32)
        bs_arr = np.asarray(bsz, np.int32)
        rc = lib.sayuri_hip_test_head_board(0, n, bs_arr.ctypes.data_as(_lib.c_int_p), 19, C, Cp, Cv, prob_ch, pass_outs, misc_outs, act,
                                            _lib.fp(tcat), _lib.fp(p_w), _lib.fp(p_b), _lib.fp(v_w), _lib.fp(v_b), warr, _lib.fp(prob), _lib.fp(pas), _lib.fp(misc), _lib.fp(own))
        assert rc == 0, (bsz, C, Cp, Cv, rc, lib.sayuri_hip_last_error().decode())
        for i, b in enumerate(bsz):
            S = b * b
            from test_gpu_layers import act_np
            pc = act_np(p_w.astype(np.float64) @ ts[i].astype(np.float64) + p_b[:, None], act).astype(np.float32)
            vc = act_np(v_w.astype(np.float64) @ ts[i].astype(np.float64) + v_b[:, None], act).astype(np.float32)
            pc, vc = np.ascontiguousarray(pc), np.ascontiguousarray(vc)
            e_prob, e_pass = np.zeros((prob_ch, S), np.float32), np.zeros(pass_outs, np.float32)
            e_own, e_misc = np.zeros(S, np.float32), np.zeros(misc_outs, np.float32)
            o.so_tap_head_tail(b, Cp, Cv, prob_ch, pass_outs, misc_outs, act, _lib.fp(pc), _lib.fp(vc), *[_lib.fp(w) for w in ws],
                               _lib.fp(e_prob), _lib.fp(e_pass), _lib.fp(e_own), _lib.fp(e_misc))
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
    return _lib.hip()


def sx_call(bsz, C, se, act, xs, rs, w, bias, fc, max_board=19):
    """One launch of the tap.  y starts as NaN on the host (and in the tap's device buffer): what comes back finite was written.
    -> (return code, [y of each sample [C][b*b]])"""
    lib = sx_lib()
    xcat = np.concatenate([x.ravel() for x in xs])
    rcat = np.concatenate([r.ravel() for r in rs]) if rs is not None else None
    y = np.full(xcat.shape, np.nan, np.float32)
    bs_arr = np.asarray(bsz, np.int32)
    rc = lib.sayuri_hip_test_conv_sx(0, len(bsz), bs_arr.ctypes.data_as(_lib.c_int_p), max_board, C, se, act, _lib.fp(xcat), _lib.fp(w), _lib.fp(bias),
                                     _lib.fp(rcat) if rcat is not None else None, *[_lib.fp(a) for a in fc], _lib.fp(y))
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


# ====================================================================================================================
# Pooled statistics of the one-workgroup SE kernels and of the heads.
#
# With x ~ N(0, 1) the tests above cannot see a wrong pooled statistic: a channel mean is ~ 1 / sqrt(npix), a single pixel
# moves it by 1 / npix, the maximum is never negative.  The cases below draw inputs on which each statistic carries weight and
# compare with float64 references (conv3x3_f64 + se_unit_f64, head_tail_f64).  tests/test_se_head_reference_cpu.py pins
# head_tail_f64 to the oracle's tap and proves, on these very draws, that every listed defect of the pooling moves the
# reference by >= 4x the tolerance used here, and that the staged kernel's fp16 images cost <= half of it.
#
#   spread draws  the sx_trunk / sx_fc recipe: pooled means of O(1) that differ by channel, gates over ~0.1 .. 0.9.
#   probe draws   what random data cannot show -- one pixel too few or too many, a maximum that sees an empty cell.  The input
#                 is small noise with one spike per channel at a boundary pixel of the kernels' pixel partitions (by channel
#                 group, probe_pixels), the convolution passes it on (identity centre tap + a small remainder), one channel
#                 group sits at a negative level so that its true maximum is negative, and the FCs are probes: a hidden unit
#                 reads the mean or the maximum of ONE channel group and the next FC carries it to that group with a known gain.
PROBE_NOISE = 0.05
PROBE_GROUPS = 8  # channel c belongs to group c % 8: 0..5 spike at probe_pixels(bs)[g], 6 the negative level, 7 noise alone (the unit: a level of 1)
PROBE_NEG = 6
PROBE_B1 = 2.0    # the hidden probes sit at 2 + gain * statistic: every activation has slope ~1 there


def probe_pixels(bs):
    """pixel 0, the last pixel, the first pixel of the last 16-pixel column tile, the end of the first row, the start of the
    last row, the first pixel of the second wave column (conv_board.h: column tiles (ncols + 1) / 2 .. of the tile)"""
    npix = bs * bs
    ncols = (npix + 15) // 16
    return (0, npix - 1, 16 * ((npix - 1) // 16), bs - 1, npix - bs, min(npix - 1, 16 * ((ncols + 1) // 2)))


def probe_amp(bs):
    """height of the spike: 8 on 9x9 and larger; lower on the smallest boards, where one pixel is a large share of the mean
    (a spike of 8 over 4 pixels would carry the output scale, which the tolerance is relative to, to ~40)"""
    return 8.0 if bs >= 9 else max(1.0, 8.0 * bs * bs / 81.0)


def probe_planes(rng, C, bs, level=None):
    """[C][bs*bs] float64: noise, the spike of each channel's group, `level` added to the channels of the negative group"""
    x = PROBE_NOISE * rng.standard_normal((C, bs * bs))
    g = np.arange(C) % PROBE_GROUPS
    for k, p in enumerate(probe_pixels(bs)):
        x[g == k, p] += probe_amp(bs)
    if level is not None:
        x[g == PROBE_NEG] += level
    return x


def probe_fc(C, outs, rows):
    """[outs][3C] float32 probe rows over a (mean, scaled mean, max) vector, and their bias: row k reads one statistic of one
    channel group, rows[k] = (group, "mean" | "scaled" | "max", gain); the gain is divided over the group's channels; the other
    rows are 0"""
    w, b = np.zeros((outs, 3 * C), np.float32), np.zeros(outs, np.float32)
    g = np.arange(C) % PROBE_GROUPS
    for k, (group, kind, gain) in enumerate(rows):
        sel = np.flatnonzero(g == group)
        w[k, ("mean", "scaled", "max").index(kind) * C + sel] = gain / len(sel)
        b[k] = PROBE_B1
    return w, b


class SeProbe:
    """SxTrunk's counterpart of the probe draws (same attributes)."""

    def __init__(self, seed, bsz, C):
        rng = np.random.default_rng([seed, C, 11] + list(bsz))
        self.bsz, self.C = list(bsz), C
        self.xs = [r16(probe_planes(rng, C, b).astype(np.float32), True) for b in bsz]
        self.rs = [r16((0.25 * rng.standard_normal((C, b * b))).astype(np.float32), True) for b in bsz]
        w = 0.02 * rng.standard_normal((C, C, 3, 3)) / np.sqrt(9 * C)
        w[np.arange(C), np.arange(C), 1, 1] += 1.0
        self.w = r16(w.astype(np.float32), True)
        self.bias = np.choose(np.arange(C) % PROBE_GROUPS, [0.0] * 6 + [-2.0, 1.0]).astype(np.float32)
        self._conv = {}

    conv = SxTrunk.conv


# The unit's probes: (channel group, statistic, squeeze gain, group whose beta shows it, excite gain) -- all powers of two, exact
# in the fp16 images.  Spike groups: mean -> beta 4 * 4 (a pixel of 8 in 361 moves beta by 0.35), maximum -> beta 1/4 * 1/2 (a lost
# spike of 8 moves it by 1).  The negative group's maximum (-1.9) shows in the level group's beta, 1/2 * 1 (a 0 in its place: 0.95):
# its own channels sit at -2, where ReLU and HardSwish would hide any beta.  The level group (conv bias 1: a mean of 1): mean
# 2 * 2 (divided by 384 on 19x19: 0.24), scaled mean 1 * 2 (a neighbour size's factor, or none on 13x13 / 15x15: 0.2).  Separate
# gains: with one gain for all, either "pixel 0 twice" drowns or the output scale, which the tolerance follows, blows up.
PROBE_LEVEL = 7
SE_PROBES = ([(g, "mean", 4.0, g, 4.0) for g in range(6)] + [(g, "max", 0.25, g, 0.5) for g in range(6)] +
             [(PROBE_NEG, "max", 0.5, PROBE_LEVEL, 1.0), (PROBE_LEVEL, "mean", 2.0, PROBE_LEVEL, 2.0), (PROBE_LEVEL, "scaled", 1.0, PROBE_LEVEL, 2.0)])


@functools.lru_cache(maxsize=None)
def se_probe_fc(seed, C, se):
    """w1, b1, w2, b2 of the probe unit (SE_PROBES); gamma from its bias alone"""
    rng = np.random.default_rng([seed, C, se, 78])
    w1, b1 = probe_fc(C, se, [p[:3] for p in SE_PROBES])
    w2, b2 = np.zeros((2 * C, se), np.float32), np.zeros(2 * C, np.float32)
    b2[:C] = (rng.standard_normal(C) * 0.5).astype(np.float32)
    g = np.arange(C) % PROBE_GROUPS
    for k, p in enumerate(SE_PROBES):
        w2[C + np.flatnonzero(g == p[3]), k] = p[4]
    b2[C:] = -PROBE_B1 * w2[C:].sum(axis=1)  # the probes' resting level taken out again
    b2[C + np.flatnonzero(g == PROBE_LEVEL)] += 4.0  # keeps the level group's output above 0 on every board size (ReLU)
    return w1, b1, w2, b2


@functools.lru_cache(maxsize=None)
def se_inputs(draw, seed, bsz, C, se):
    """(trunk, (w1, b1, w2, b2)) of one layer of the pooled-statistics cases; draw = "spread" | "probe" """
    if draw == "spread":
        return sx_trunk(seed, tuple(bsz), C), sx_fc(seed, C, se)
    assert draw == "probe"
    return SeProbe(seed, tuple(bsz), C), se_probe_fc(seed, C, se)


# The cases: (C, se) whose images make_se_images stages, and two it refuses (the FCs then read fp32 weights from L2: C = 256, se = 128
# is what the engine meets; at C = 128 the images fit far beyond the usual widths, and the L2 form's thread layout needs 512 % (se / 4) == 0).
SE_SEED = 41
SE_LAYERS = ((256, 64), (128, 32))
SE_L2_LAYERS = ((256, 128), (128, 256))
SE_BATCHES = ((19, 19), (19, 18, 17, 16, 15, 14), (2,), (3,), (5,), (9,), (13,))  # one sample per tile
SE_ACT_BATCH = (19, 15)
SE_L2_BATCHES = ((19, 17, 14), (9,))
SE_UNIT_BATCHES = ((19, 16, 14), (9, 9, 9, 13, 13, 2))  # se_pool / se_fc / se_scale: any batch
SE_STAGED, SE_FROM_L2 = 1, 2  # sayuri_hip_test_last_se_form


def se_case_batches(C, se, act):
    """the batches of test_conv_se_pooled_statistics at this layer and activation (none: no such case)"""
    if (C, se) in SE_L2_LAYERS:
        return SE_L2_BATCHES if act == 5 else ()
    return (SE_BATCHES if act in (5, 0) else ()) + ((SE_ACT_BATCH,) if (C, se) == (128, 32) else ())


SE_CASES = [(C, se, act) for C, se in SE_LAYERS + SE_L2_LAYERS for act in (5, 0, 1, 2, 3, 4, 6, 7) if se_case_batches(C, se, act)]
SE_CASE_IDS = [f"C{c}se{s}act{a}" for c, s, a in SE_CASES]


def se_unit_x(T, i, fp16):
    """the unit's input of the separate kernels' cases: the trunk's convolution as the engine would have stored it"""
    return r16(T.conv(i).astype(np.float32), fp16)


def zero_scaled_mean(w, C):
    """a valid but different weight set: the columns of the scaled-mean third of a (mean, scaled mean, third) FC zeroed"""
    w = w.copy()
    w[:, C:2 * C] = 0.0
    return w


# ---- the heads: float64 restatement of so_tap_head_tail (oracle/sayuri_oracle.c; reference blas_forward_pipe.cc:496-580), in
# pieces a test can replace.  weights12 as in sayuri_hip_test_head_tail.
def head_pool_f64(x, bs, value_head):
    """GlobalPooling<false/true> (se_unit.cc:9-68) of x [C][bs*bs]: (mean, mean * (bs-14)/10, max | mean * ((bs-14)^2/100 - 0.1))"""
    x = np.asarray(x, np.float64)
    mean = x.sum(axis=1) / float(bs * bs)
    d = bs - 14.0
    return np.concatenate([mean, mean * (d / 10.0), mean * (d * d / 100.0 - 0.1) if value_head else x.max(axis=1)])


def head_inter_f64(pool, w, b, act):
    return act_np(np.asarray(w, np.float64) @ pool + np.asarray(b, np.float64), act)


def head_pixel_f64(planes, w, b):
    """a 1x1 convolution with bias over planes [C][S]: w [K][C] -> [K][S]"""
    return np.asarray(w, np.float64) @ planes + np.asarray(b, np.float64)[:, None]


def head_tail_f64(pc, vc, ws, bs, act, ppool=None, vpool=None, spatial_bias=True):
    """-> (prob [prob_ch][S], pass, own [S], misc) from the activated head planes pc [Cp][S], vc [Cv][S].  ppool / vpool: a
    pooled vector to use in place of the sample's own; spatial_bias=False leaves p_inter's output off the policy planes."""
    p_inter_w, p_inter_b, pass_w, pass_b, v_inter_w, v_inter_b, v_misc_w, v_misc_b, prob_w, prob_b, own_w, own_b = ws
    pc, vc = np.asarray(pc, np.float64), np.asarray(vc, np.float64)
    pinter = head_inter_f64(head_pool_f64(pc, bs, False) if ppool is None else ppool, p_inter_w, p_inter_b, act)
    prob = head_pixel_f64(pc + pinter[:, None] if spatial_bias else pc, prob_w, prob_b)
    pas = head_inter_f64(pinter, pass_w, pass_b, 0)
    vinter = head_inter_f64(head_pool_f64(vc, bs, True) if vpool is None else vpool, v_inter_w, v_inter_b, act)
    own = head_pixel_f64(vc, np.asarray(own_w, np.float64).reshape(1, -1), own_b)[0]
    misc = head_inter_f64(vinter, v_misc_w, v_misc_b, 0)
    return prob, pas, own, misc


HEAD_OUTS = ("prob", "pass", "own", "misc")
HEAD_SEED = 43
HEAD_BOARDS = (19, 14, 13, 9, 2)
HEAD_PAIRS = ((32, 32), (24, 48))
HEAD_DIMS = dict(prob_ch=5, pass_outs=5, misc_outs=15)
# probe gains of the heads: p_inter / v_inter rows as probe_fc; the statistic reaches pass / misc through the random second FC
HEAD_PROBES = [(g, "mean", 32.0) for g in range(6)] + [(g, "max", 0.25) for g in range(6)] + [(PROBE_NEG, "max", 2.0)]


def head_weights(draw, rng, Cp, Cv):
    """weights12.  spread: the recipe of the tests above with biases of 0.5 N(0, 1); probe: p_inter / v_inter are probe rows."""
    d = HEAD_DIMS
    shapes = [(Cp, 3 * Cp), (Cp,), (d["pass_outs"], Cp), (d["pass_outs"],), (3 * Cv, 3 * Cv), (3 * Cv,), (d["misc_outs"], 3 * Cv), (d["misc_outs"],),
              (d["prob_ch"], Cp), (d["prob_ch"],), (Cv,), (1,)]
    ws = [(rng.standard_normal(s) / np.sqrt(s[-1]) if len(s) > 1 else 0.5 * rng.standard_normal(s)).astype(np.float32) for s in shapes]
    if draw == "probe":
        ws[0], ws[1] = probe_fc(Cp, Cp, HEAD_PROBES)
        ws[4], ws[5] = probe_fc(Cv, 3 * Cv, HEAD_PROBES[:6])
    ws[8], ws[10] = r16(ws[8], True), r16(ws[10], True)  # head_board_kernel holds the per-pixel weights as an fp16 image
    return ws


class HeadDraw:
    """Inputs of the head kernels over the boards `bsz`.  C = 0: the activated head planes themselves (head_tail_kernel), rounded
    to fp16 where the kernel stores them so; C > 0: a trunk and the two 1x1 head convolutions in front (head_board_kernel), the
    planes are their float64 result.  planes(i, act) -> (pc, vc) of sample i, computed once."""

    def __init__(self, draw, seed, bsz, Cp, Cv, C=0, fp16=True):
        rng = np.random.default_rng([seed, Cp, Cv, C, int(draw == "probe")] + list(bsz))
        self.bsz, self.Cp, self.Cv, self.C = list(bsz), Cp, Cv, C
        self.ws = head_weights(draw, rng, Cp, Cv)
        self._planes = {}
        if C == 0:
            if draw == "spread":
                mk = lambda ch, b: rng.standard_normal((ch, b * b)) + rng.standard_normal((ch, 1))
                self.pcs, self.vcs = [mk(Cp, b) for b in bsz], [mk(Cv, b) for b in bsz]
            else:
                self.pcs = [probe_planes(rng, Cp, b, level=-2.0) for b in bsz]
                self.vcs = [probe_planes(rng, Cv, b) for b in bsz]
            self.pcs = [r16(p.astype(np.float32), fp16) for p in self.pcs]
            self.vcs = [r16(v.astype(np.float32), fp16) for v in self.vcs]
            return
        if draw == "spread":
            self.ts = [rng.standard_normal((C, b * b)) for b in bsz]
            p_w, v_w = rng.standard_normal((Cp, C)) / np.sqrt(C), rng.standard_normal((Cv, C)) / np.sqrt(C)
            self.p_b, self.v_b = rng.standard_normal(Cp).astype(np.float32), rng.standard_normal(Cv).astype(np.float32)
        else:
            # trunk channel j carries the spike of policy channel j, channel Cp + j that of value channel j; dominant rows pass them on
            self.ts = [PROBE_NOISE * rng.standard_normal((C, b * b)) for b in bsz]
            for t, b in zip(self.ts, bsz):
                t[:Cp] = probe_planes(rng, Cp, b)
                t[Cp:Cp + Cv] = probe_planes(rng, Cv, b)
            p_w, v_w = 0.02 * rng.standard_normal((Cp, C)) / np.sqrt(C), 0.02 * rng.standard_normal((Cv, C)) / np.sqrt(C)
            p_w[np.arange(Cp), np.arange(Cp)] += 1.0
            v_w[np.arange(Cv), Cp + np.arange(Cv)] += 1.0
            # the negative group rests where Mish is lowest (-0.31 at -1.2); the identity keeps -1.2
            self.p_b = np.where(np.arange(Cp) % PROBE_GROUPS == PROBE_NEG, -1.2, 0.0).astype(np.float32)
            self.v_b = np.zeros(Cv, np.float32)
        self.ts = [r16(t.astype(np.float32), True) for t in self.ts]
        self.p_w, self.v_w = r16(p_w.astype(np.float32), True), r16(v_w.astype(np.float32), True)

    def planes(self, i, act):
        if self.C == 0:
            return self.pcs[i], self.vcs[i]
        if (i, act) not in self._planes:
            t = self.ts[i].astype(np.float64)
            self._planes[i, act] = (act_np(self.p_w.astype(np.float64) @ t + self.p_b[:, None], act),
                                    act_np(self.v_w.astype(np.float64) @ t + self.v_b[:, None], act))
        return self._planes[i, act]

    def reference(self, i, act, **kw):
        return head_tail_f64(*self.planes(i, act), self.ws, self.bsz[i], act, **kw)


@functools.lru_cache(maxsize=None)
def head_inputs(draw, seed, bsz, Cp, Cv, C=0, fp16=True):
    return HeadDraw(draw, seed, tuple(bsz), Cp, Cv, C, fp16)


def head_ratio(a, b, ref, tol):
    """largest |a - b| over the four outputs, each in units of its own tolerance tol * max(1, |ref|max)"""
    return max(float(np.abs(np.asarray(x) - y).max()) / (tol * max(1.0, float(np.abs(r).max()))) for x, y, r in zip(a, b, ref))


# ------------------------------------------------------------------------------------------------ the GPU cases
def conv_se_call(T, fc, C, se, act, via_tower, with_res=True):
    """one launch of sayuri_hip_test_conv_se -> (return code, [y of each sample [C][b*b]]); y starts as NaN on the host"""
    lib = _lib.hip()
    xcat = np.concatenate([x.ravel() for x in T.xs])
    rcat = np.concatenate([r.ravel() for r in T.rs]) if with_res else None
    y = np.full(xcat.shape, np.nan, np.float32)
    bs_arr = np.asarray(T.bsz, np.int32)
    rc = lib.sayuri_hip_test_conv_se(0, len(T.bsz), bs_arr.ctypes.data_as(_lib.c_int_p), 19, C, se, act, via_tower, _lib.fp(xcat), _lib.fp(T.w), _lib.fp(T.bias),
                                     _lib.fp(rcat) if with_res else None, *[_lib.fp(np.ascontiguousarray(a)) for a in fc], _lib.fp(y))
    outs, off = [], 0
    for b in T.bsz:
        outs.append(y[off:off + C * b * b].reshape(C, b * b))
        off += C * b * b
    return rc, outs


def conv_se_run(draw, bsz, C, se, act, via_tower, with_res=True):
    """The layer of se_inputs(draw, SE_SEED, bsz, C, se) through the tap: it must run, in the form the layer's SE width asks for;
    every sample within SX_TOL of conv3x3_f64 + se_unit_f64.  -> the worst error / tolerance"""
    lib = _lib.hip()
    T, fc = se_inputs(draw, SE_SEED, tuple(bsz), C, se)
    rc, outs = conv_se_call(T, fc, C, se, act, via_tower, with_res)
    assert rc == 0, (draw, bsz, C, se, via_tower, rc, lib.sayuri_hip_last_error().decode())
    form = lib.sayuri_hip_test_last_se_form()
    assert form == (SE_FROM_L2 if (C, se) in SE_L2_LAYERS else SE_STAGED), (C, se, form)
    worst = 0.0
    for i, got in enumerate(outs):
        ref = sx_reference(T, fc, i, act, with_res)
        tol = SX_TOL * max(1.0, float(np.abs(ref).max()))
        assert np.isfinite(got).all(), (draw, bsz, C, se, act, i)
        err = float(np.abs(got - ref).max())
        worst = max(worst, err / tol)
        assert err <= tol, (draw, bsz, C, se, act, via_tower, i, err, tol)
    print(f"conv + SE unit {draw} C={C} se={se} act={act} {'tower' if via_tower else 'per-layer'} form={form} boards={list(bsz)}: worst error {worst:.2f} x tol")
    return worst


@pytest.mark.parametrize("via_tower", [0, 1], ids=["per-layer kernel", "tower kernel"])
@pytest.mark.parametrize("draw", ["spread", "probe"])
@pytest.mark.parametrize("C,se,act", SE_CASES, ids=SE_CASE_IDS)
def test_conv_se_pooled_statistics(C, se, act, draw, via_tower):
    """conv_board_se_kernel / the tower's SE stage on inputs that show every pooled statistic (see above), staged images
    (C = 256 / se = 64, C = 128 / se = 32) and FCs from L2 (se = 128 / 256): samples alone in a tile of 19x19 .. 14x14 and of
    2x2 .. 13x13 at activations 5 and 0, all eight activations on one small batch.  The tap reports which form ran."""
    for bsz in se_case_batches(C, se, act):
        conv_se_run(draw, bsz, C, se, act, via_tower)


@pytest.mark.parametrize("via_tower", [0, 1], ids=["per-layer kernel", "tower kernel"])
@pytest.mark.parametrize("C,se", [(256, 64), (256, 128)], ids=["staged", "from-L2"])
def test_conv_se_test_can_fail(C, se, via_tower):
    """The real kernel on a valid but different weight set -- w1 with its scaled-mean columns zeroed -- is >= 4x the tolerance away
    from the unmutated reference on every sample but the 14x14 one, where the term is 0 (and which stays within the tolerance):
    neither fp16 path washes the term out."""
    lib = _lib.hip()
    bsz, act = (19, 18, 17, 16, 15, 14), 5
    T, fc = se_inputs("spread", SE_SEED, bsz, C, se)
    rc, outs = conv_se_call(T, (zero_scaled_mean(fc[0], C),) + fc[1:], C, se, act, via_tower)
    assert rc == 0, (C, se, rc, lib.sayuri_hip_last_error().decode())
    for i, bs in enumerate(bsz):
        ref = sx_reference(T, fc, i, act, True)
        ratio = float(np.abs(outs[i] - ref).max()) / (SX_TOL * max(1.0, float(np.abs(ref).max())))
        print(f"conv + SE unit C={C} se={se} {'tower' if via_tower else 'per-layer'} without the scaled-mean columns, {bs}x{bs}: {ratio:.1f} x tol")
        assert ratio <= 1.0 if bs == 14 else ratio >= 4.0, (C, se, via_tower, bs, ratio)


def se_unit_call(fp16, bsz, C, se, act, xs, rs, fc):
    """one run of se_pool / se_fc / se_scale -> (return code, [y of each sample], gate [n][2C])"""
    lib = _lib.hip()
    xcat = np.concatenate([x.ravel() for x in xs])
    rcat = np.concatenate([r.ravel() for r in rs])
    y = np.full(xcat.shape, np.nan, np.float32)
    gate = np.zeros((len(bsz), 2 * C), np.float32)
    bs_arr = np.asarray(bsz, np.int32)
    rc = lib.sayuri_hip_test_se_unit(0, int(fp16), len(bsz), bs_arr.ctypes.data_as(_lib.c_int_p), 19, C, se, act, _lib.fp(xcat), _lib.fp(rcat),
                                     *[_lib.fp(np.ascontiguousarray(a)) for a in fc], _lib.fp(y), _lib.fp(gate))
    outs, off = [], 0
    for b in bsz:
        outs.append(y[off:off + C * b * b].reshape(C, b * b))
        off += C * b * b
    return rc, outs, gate


@pytest.mark.parametrize("fp16", [False, True], ids=["fp32", "fp16"])
@pytest.mark.parametrize("draw", ["spread", "probe"])
@pytest.mark.parametrize("act", [5, 0])
def test_se_unit_kernels_pooled_statistics(act, draw, fp16):
    """se_pool / se_fc / se_scale on the same two draws (the unit's input is the trunk's convolution, rounded as the engine stores
    it), against se_unit_f64: 2e-3 / 2e-5 of the output scale, the gate read out at 1e-4.  One batch of large boards, one where
    several small boards follow each other."""
    lib = _lib.hip()
    for C, se in SE_LAYERS:
        for bsz in SE_UNIT_BATCHES:
            T, fc = se_inputs(draw, SE_SEED, bsz, C, se)
            xs = [se_unit_x(T, i, fp16) for i in range(len(bsz))]
            rc, outs, gate = se_unit_call(fp16, bsz, C, se, act, xs, T.rs, fc)
            assert rc == 0, lib.sayuri_hip_last_error().decode()
            worst = worst_gate = 0.0
            for i, bs in enumerate(bsz):
                gamma, beta = se_gate_f64(se_pool_f64(xs[i], bs), *fc, act)
                exp_gate = np.concatenate([gamma, beta])
                gerr = float(np.abs(gate[i] - exp_gate).max()) / (1e-4 * max(1.0, float(np.abs(exp_gate).max())))
                ref = se_apply_f64(xs[i], T.rs[i], gamma, beta, act)
                tol = (2e-3 if fp16 else 2e-5) * max(1.0, float(np.abs(ref).max()))
                assert np.isfinite(outs[i]).all()
                err = float(np.abs(outs[i] - ref).max())
                worst, worst_gate = max(worst, err / tol), max(worst_gate, gerr)
                assert gerr <= 1.0, (draw, bsz, C, i, "gate", gerr)
                assert err <= tol, (draw, bsz, C, se, act, fp16, i, err, tol)
            print(f"SE kernels {draw} {'fp16' if fp16 else 'fp32'} C={C} se={se} act={act} boards={list(bsz)}: worst error {worst:.2f} x tol, "
                  f"gate {worst_gate:.2f} x 1e-4")


@pytest.mark.parametrize("fp16", [False, True], ids=["fp32", "fp16"])
def test_se_unit_kernels_test_can_fail(fp16):
    """as test_conv_se_test_can_fail, for the separate kernels"""
    lib = _lib.hip()
    C, se, act, bsz = 128, 32, 5, (19, 16, 14)
    T, fc = se_inputs("spread", SE_SEED, bsz, C, se)
    xs = [se_unit_x(T, i, fp16) for i in range(len(bsz))]
    rc, outs, _ = se_unit_call(fp16, bsz, C, se, act, xs, T.rs, (zero_scaled_mean(fc[0], C),) + fc[1:])
    assert rc == 0, lib.sayuri_hip_last_error().decode()
    for i, bs in enumerate(bsz):
        ref = se_unit_f64(xs[i], T.rs[i], *fc, bs, act)
        ratio = float(np.abs(outs[i] - ref).max()) / ((2e-3 if fp16 else 2e-5) * max(1.0, float(np.abs(ref).max())))
        print(f"SE kernels {'fp16' if fp16 else 'fp32'} without the scaled-mean columns, {bs}x{bs}: {ratio:.1f} x tol")
        assert ratio <= 1.0 if bs == 14 else ratio >= 4.0, (fp16, bs, ratio)


def head_call(H, act, fp16=True):
    """head_tail_kernel on H's planes (H.C == 0) or head_board_kernel on its trunk -> (return code, prob, pass, own, misc), the
    per-pixel outputs cut to each sample's board; asserts that the off-board cells of the NN grid stayed 0"""
    lib = _lib.hip()
    d, n, B2 = HEAD_DIMS, len(H.bsz), 361
    warr = (FP * 12)(*[_lib.fp(w) for w in H.ws])
    prob, own = np.zeros((n, d["prob_ch"], B2), np.float32), np.zeros((n, B2), np.float32)
    pas, misc = np.zeros((n, d["pass_outs"]), np.float32), np.zeros((n, d["misc_outs"]), np.float32)
    bs_arr = np.asarray(H.bsz, np.int32)
    if H.C == 0:
        pcat, vcat = np.concatenate([p.ravel() for p in H.pcs]), np.concatenate([v.ravel() for v in H.vcs])
        rc = lib.sayuri_hip_test_head_tail(0, int(fp16), n, bs_arr.ctypes.data_as(_lib.c_int_p), 19, H.Cp, H.Cv, d["prob_ch"], d["pass_outs"],
                                           d["misc_outs"], act, _lib.fp(pcat), _lib.fp(vcat), warr, _lib.fp(prob), _lib.fp(pas), _lib.fp(misc), _lib.fp(own))
    else:
        tcat = np.concatenate([t.ravel() for t in H.ts])
        rc = lib.sayuri_hip_test_head_board(0, n, bs_arr.ctypes.data_as(_lib.c_int_p), 19, H.C, H.Cp, H.Cv, d["prob_ch"], d["pass_outs"], d["misc_outs"],
                                            act, _lib.fp(tcat), _lib.fp(H.p_w), _lib.fp(H.p_b), _lib.fp(H.v_w), _lib.fp(H.v_b), warr, _lib.fp(prob), _lib.fp(pas), _lib.fp(misc), _lib.fp(own))
    outs = []
    for i, b in enumerate(H.bsz):
        mask = np.ones((19, 19), bool)
        mask[:b, :b] = False
        assert not prob[i].reshape(-1, 19, 19)[:, mask].any() and not own[i].reshape(19, 19)[mask].any()
        outs.append((prob[i].reshape(-1, 19, 19)[:, :b, :b].reshape(-1, b * b), pas[i], own[i].reshape(19, 19)[:b, :b].ravel(), misc[i]))
    return rc, outs


def head_run(draw, Cp, Cv, C, act, fp16, tol):
    lib = _lib.hip()
    H = head_inputs(draw, HEAD_SEED, HEAD_BOARDS, Cp, Cv, C, fp16)
    rc, outs = head_call(H, act, fp16)
    assert rc == 0, (draw, Cp, Cv, C, rc, lib.sayuri_hip_last_error().decode())
    worst = 0.0
    for i, bs in enumerate(H.bsz):
        ref = H.reference(i, act)
        for name, got, r in zip(HEAD_OUTS, outs[i], ref):
            assert np.isfinite(got).all()
            ratio = float(np.abs(got - r).max()) / (tol * max(1.0, float(np.abs(r).max())))
            worst = max(worst, ratio)
            assert ratio <= 1.0, (draw, Cp, Cv, C, act, fp16, i, bs, name, ratio)
    print(f"{'head_board' if C else 'head_tail'} {draw} C={C} Cp={Cp} Cv={Cv} act={act} {'fp16' if fp16 else 'fp32'}: worst error {worst:.2f} x tol")


@pytest.mark.parametrize("fp16", [False, True], ids=["fp32", "fp16"])
@pytest.mark.parametrize("draw", ["spread", "probe"])
@pytest.mark.parametrize("act", [5, 0])
def test_head_tail_kernel_pooled_statistics(act, draw, fp16):
    """head_tail_kernel against head_tail_f64 at 2e-4, boards 19 / 14 / 13 / 9 / 2 in one batch, on planes whose pooled statistics
    each carry weight (spread) and with spikes at the pooling's boundary pixels behind probe FCs (probe)."""
    for Cp, Cv in HEAD_PAIRS:
        head_run(draw, Cp, Cv, 0, act, fp16, 2e-4)


@pytest.mark.parametrize("C", [128, 256])
@pytest.mark.parametrize("draw", ["spread", "probe"])
@pytest.mark.parametrize("act", [5, 0])
def test_head_board_kernel_pooled_statistics(act, draw, C):
    """head_board_kernel against the float64 head convolutions + head_tail_f64 at 2e-3, same boards: its pooling runs over 384 pixel
    slots in 24 column tiles, of which a board uses a prefix."""
    for Cp, Cv in HEAD_PAIRS:
        head_run(draw, Cp, Cv, C, act, True, 2e-3)


@pytest.mark.parametrize("C", [0, 256], ids=["head_tail", "head_board"])
def test_head_kernels_test_can_fail(C):
    """The real kernels on p_inter with its scaled-mean columns zeroed are >= 4x the tolerance away from the unmutated reference
    on every sample but the 14x14 one (which stays within it)."""
    import copy
    lib = _lib.hip()
    Cp, Cv, act, tol = 32, 32, 5, 2e-3 if C else 2e-4
    H = head_inputs("spread", HEAD_SEED, HEAD_BOARDS, Cp, Cv, C, True)
    M = copy.copy(H)
    M.ws = [zero_scaled_mean(H.ws[0], Cp)] + H.ws[1:]
    rc, outs = head_call(M, act)
    assert rc == 0, (C, rc, lib.sayuri_hip_last_error().decode())
    for i, bs in enumerate(H.bsz):
        ref = H.reference(i, act)
        ratio = head_ratio(outs[i], ref, ref, tol)
        print(f"{'head_board' if C else 'head_tail'} without p_inter's scaled-mean columns, {bs}x{bs}: {ratio:.1f} x tol")
        assert ratio <= 1.0 if bs == 14 else ratio >= 4.0, (C, bs, ratio)
