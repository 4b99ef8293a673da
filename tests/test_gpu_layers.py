"""Layer-level parity of the HIP kernels (through the conv tap of _taps.py) against a
float64 numpy restatement of the direct convolution the CPU oracle computes, conv_ref of _kref.py
(reference src/neural/blas/convolution.h:41-125, convolution.cc:27-62, biases.cc:14-77).

fp32 mode: fp32 MFMA is an exact fmaf chain -> abs tolerance 2e-5 on O(1) outputs.
fp16 mode: inputs/weights rounded to fp16, fp32 accumulate, fp16 store -> tolerance
4e-3 * max|y| (half has 11 significant bits; K <= 2304 products of O(1)*O(0.03))."""
import numpy as np
import pytest

import _taps
from _cases import BOARD_CASES, CASES
from _kref import conv_ref
from _taps import KIND_BOARD

pytestmark = pytest.mark.gpu


def run_case(fp16, bsz, cin, cout, k, depthwise=False, act=5, with_res=True, post=False, seed=0, max_board=19, kind=None):
    rng = np.random.default_rng(seed)
    xc = cout if depthwise else cin
    xs = [rng.standard_normal((xc, b * b)).astype(np.float32) for b in bsz]
    wshape = (cout, 1, k, k) if depthwise else (cout, cin, k, k)
    fan = k * k * (1 if depthwise else cin)
    w = (rng.standard_normal(wshape) / np.sqrt(fan)).astype(np.float32)
    bias = (rng.standard_normal(cout) * 0.1).astype(np.float32)
    res = [rng.standard_normal((cout, b * b)).astype(np.float32) for b in bsz] if with_res else None
    if fp16:  # the kernel sees fp16-rounded operands; give the reference the same
        xs_r = [x.astype(np.float16).astype(np.float64) for x in xs]
        w_r = w.astype(np.float16).astype(np.float64) if not depthwise else w.astype(np.float64)
        res_r = [r.astype(np.float16).astype(np.float64) for r in res] if res else None
    else:
        xs_r, w_r = [x.astype(np.float64) for x in xs], w.astype(np.float64)
        res_r = [r.astype(np.float64) for r in res] if res else None
    ref = conv_ref(xs_r, bsz, w_r, bias.astype(np.float64), res_r, k, depthwise, act, post)
    t = _taps.ok(_taps.conv(fp16, bsz, cin, cout, k, act, xs, w, bias, res, depthwise, post, max_board))
    worst = 0.0
    scale = max(float(np.abs(r).max()) for r in ref)
    for got, exp in zip(t.outs, ref):
        assert np.isfinite(got).all()
        worst = max(worst, float(np.abs(got - exp).max()))
    tol = 4e-3 * scale if fp16 else 2e-5 * max(scale, 1.0)
    assert worst <= tol, (worst, tol, scale)
    if kind is not None:
        assert t.kind == kind, "the layer ran on another kernel family than the test is about"
    return worst


@pytest.mark.parametrize("fp16", [False, True], ids=["fp32", "fp16"])
@pytest.mark.parametrize("case", CASES, ids=[f"{c[1]}x{c[2]}k{c[3]}n{len(c[0])}b{min(c[0])}" for c in CASES])
def test_conv_mfma(case, fp16):
    bsz, cin, cout, k = case
    run_case(fp16, bsz, cin, cout, k, act=5, with_res=True, seed=cin + cout)


@pytest.mark.parametrize("fp16", [False, True], ids=["fp32", "fp16"])
@pytest.mark.parametrize("act", range(8))
def test_conv_epilogue_variants(act, fp16):
    run_case(fp16, [19, 9], 32, 32, 3, act=act, with_res=False, seed=act)
    run_case(fp16, [19, 9], 32, 32, 3, act=act, with_res=True, seed=act + 10)


@pytest.mark.parametrize("case", BOARD_CASES, ids=[f"{c[1]}x{c[2]}n{len(c[0])}b{min(c[0])}" for c in BOARD_CASES])
def test_conv_board(case):
    bsz, cin, cout = case
    run_case(True, bsz, cin, cout, 3, act=5, with_res=True, seed=cin + cout, kind=KIND_BOARD)
    run_case(True, bsz, cin, cout, 3, act=0, with_res=False, seed=cin + cout + 1, kind=KIND_BOARD)


@pytest.mark.parametrize("act", range(8))
def test_conv_board_activations(act):
    run_case(True, [19, 19], 64, 128, 3, act=act, with_res=True, seed=40 + act, kind=KIND_BOARD)
    run_case(True, [13, 13, 13], 64, 192, 3, act=act, with_res=False, seed=50 + act, kind=KIND_BOARD)


def test_conv_board_batch256():
    """Full bench geometry (256 x 19x19 = 256 board tiles = one workgroup per CU): a subset of samples against the float64
    reference, and sample independence -- permuting the batch permutes the outputs bit for bit."""
    rng = np.random.default_rng(17)
    n, cin, cout = 256, 64, 256
    x = rng.standard_normal((n, cin, 361)).astype(np.float32)
    w = (rng.standard_normal((cout, cin, 3, 3)) / np.sqrt(9 * cin)).astype(np.float32)
    bias = (rng.standard_normal(cout) * 0.1).astype(np.float32)

    def run(xx):
        r = _taps.ok(_taps.conv(True, [19] * n, cin, cout, 3, 5, xx, w, bias))
        assert r.kind == KIND_BOARD
        return np.stack(r.outs)

    y = run(x)
    w16 = w.astype(np.float16).astype(np.float64)
    for i in (0, 1, 99, 100, 177, 255):
        ref = conv_ref([x[i].astype(np.float16).astype(np.float64)], [19], w16, bias.astype(np.float64), None, 3, False, 5,
                       False)[0]
        assert np.abs(y[i] - ref).max() <= 4e-3 * np.abs(ref).max()
    perm = rng.permutation(n)
    np.testing.assert_array_equal(run(x[perm]), y[perm])


@pytest.mark.parametrize("fp16", [False, True], ids=["fp32", "fp16"])
@pytest.mark.parametrize("k", [3, 5, 7])
def test_depthwise(k, fp16):
    run_case(fp16, [19, 9, 13], 1, 48, k, depthwise=True, act=5, with_res=True, post=True, seed=k)
    run_case(fp16, [19, 7], 1, 32, k, depthwise=True, act=1, with_res=False, seed=k + 1)
    run_case(fp16, [2, 3, 5], 1, 48, k, depthwise=True, act=5, with_res=True, post=True, seed=k + 2)  # boards smaller than the 5x5 and 7x7 kernels
    run_case(fp16, [2, 3, 5], 1, 40, k, depthwise=True, act=1, with_res=False, seed=k + 3)


def test_conv_batch256_tile_seams():
    """Full bench geometry (256 x 19x19): every pixel tile seam / sample crossing is exercised;
    checked through linearity in the input (conv(a*x) = a*conv(x) with identity act, no bias)
    and against the float64 reference on a subset of samples."""
    rng = np.random.default_rng(5)
    n, cin, cout = 256, 32, 32
    x = rng.standard_normal((n, cin, 361)).astype(np.float32)
    w = (rng.standard_normal((cout, cin, 3, 3)) / np.sqrt(9 * cin)).astype(np.float32)
    y = np.stack(_taps.ok(_taps.conv(False, [19] * n, cin, cout, 3, 0, x, w, None)).outs)
    for i in (0, 1, 100, 177, 255):
        ref = conv_ref([x[i].astype(np.float64)], [19], w.astype(np.float64), None, None, 3, False, 0, False)[0]
        assert np.abs(y[i] - ref).max() < 2e-5
    # samples are independent: permuting the batch permutes the outputs
    perm = rng.permutation(n)
    y2 = np.stack(_taps.ok(_taps.conv(False, [19] * n, cin, cout, 3, 0, x[perm], w, None)).outs)
    np.testing.assert_array_equal(y2, y[perm])


@pytest.mark.parametrize("env", [("SAYURI_CONV", "glds"), ("SAYURI_CONV", "v0")], ids=lambda e: f"{e[0]}={e[1]}")
def test_conv_kernel_variants(env):
    """The A/B switch of the fp16 3x3 kernels (glds: tiles across samples instead of one workgroup per board; v0: the
    generic register-staged kernel) is read once per process, so each runs the fp16 layer cases in a process of its own."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    e = dict(os.environ, **{env[0]: env[1]})
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.join(root, "tests", "test_gpu_layers.py"), "-x", "-q", "-k",
                        "(test_conv_mfma or test_conv_epilogue_variants or test_conv_batch256) and not fp32"],
                       env=e, cwd=root, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
