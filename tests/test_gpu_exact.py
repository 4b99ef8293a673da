"""Exact-arithmetic parity of the convolution kernels: conv_mfma_kernel (fp32 and fp16), conv_board_kernel, conv_split_kernel,
depthwise_kernel, the convolution inside conv_board_se_kernel / the tower's SE stage / conv_board_sx_kernel, the persistent
conv_tower_kernel with its generated epilogue, and -- in child processes -- conv_glds_kernel and the generic fp16 kernel on the
board shapes.  No tolerance: every output has one correct value and must have it.

The principle.  x, w, bias and the residual are integers (more generally: w and bias integers, x and the residual multiples of
2^-q).  For an output let A = sum |w x| + |bias| + |res|.  If A * 2^q < 2^24, every partial sum any kernel can form -- in any
order, in any MFMA, with any split of the channels -- is a multiple of 2^-q below 2^24 * 2^-q and therefore exact in fp32: the
accumulator holds the exact sum S.  The kernels' contract (fp16 operands, fp32 accumulate, bias and residual added in fp32, ONE
round-to-nearest-even fp16 store) then leaves exactly one result, float16(act(S)) for act = identity / ReLU, which is what
np.float64(S).astype(np.float16) gives.  exact_layer computes it and asserts the regime itself (A * 2^q < 2^24, |S| < 65504), so
a case outside it cannot run.  Values are compared with ==, so that -0 equals +0.  The other six activations are no exact
functions: test_gpu_act_sweep.py puts every finite fp16 value through each kernel's epilogue for all eight.

Two draws.  unit: x in [-2, 2], w in {-1, 0, 1}, bias in [-8, 8], residual in [-16, 16] -- every output is itself an fp16 value,
nothing rounds: the tier for "every product of every tap, channel and pixel lands in the right place".  wide: x in [-16, 16], w
in [-8, 8] -- outputs run past 2048 and 4096, so the store rounds (exact ties and non-ties): the tier for the store's rounding
and for any fp16 intermediate.  The wide tier runs where it rounds enough to mean something (tests/test_exact_reference_cpu.py
holds every wide case to >= 1 % outputs that are no fp16 value, ties and non-ties both present): the 256 / 384 / 512-channel
layers.  At the generic kernel's own shapes (32 .. 96 channels, 1x1) and in the depthwise kernel it hardly rounds, so they get
the unit tier; the generic fp16 kernel's store is reached at 256 -> 256 and 384 -> 384 by the SAYURI_CONV=v0 child.

Every case asserts the kernel family (the kind a conv tap of _taps.py reports), the SE form or the tower's report it is about.  The
can-fail cases run the REAL kernels on w with one entry changed by 1 against the unchanged reference: the outputs that differ
must be exactly those the integer arithmetic predicts (one output channel, the pixels whose shifted input is not 0), by exactly
the predicted amount.  tests/test_exact_reference_cpu.py pins exact_layer to conv_ref, proves every case list of this module to
be inside the exact regime, and shows that a dropped product, a store that rounds toward zero, a convolution rounded before
the residual and fp16 partial sums per chunk are each seen.

The SE kernels are reached through a unit whose gate is the identity: both FCs zero, the excite bias +32 for gamma (the
kernels' 1.0f / (1.0f + exp(-32)) is exactly 1.0f: test_se_gate_is_exactly_one reads it back from se_fc) and small integers for
beta, so y = act(conv + bias + beta + res) is again exact.  The depthwise kernel has one residual order, act(conv + bias) + res
(post_residual = 1); with post_residual = 0 the layer has no residual.  In a tower run every layer is checked from what the
previous layer really wrote (integers, since it was exact); a layer with a compiled-epilogue activation (HardSwish) is left out
of the check, and its successor is checked from the multiples of 2^-12 it wrote (q = 12).

Run on an MI355X: all 203 cases of this module pass with zero differing values, each on the family, SE form or tower report it
asserts; se_fc's gate at gamma = 32 is exactly 1.0f (fp32 and fp16 engine, C = 128 / 256 / 384), and the three fused SE kernels
are exact behind it, so no kernel's case had to be left out; every can-fail case moved exactly the predicted outputs (522 .. 1174
of them per changed weight) by the predicted amount; both fallback children pass.  No defect was found.  Wall time of the
module: 14 s, 6 s of it the two child processes.

The reference (exact_layer and its kin) is in _kref.py, the draws and case lists in _cases.py.
"""
import copy
import os
import subprocess
import sys

import numpy as np
import pytest

import _taps
from _cases import (BOARD_EXACT, CAN_FAIL, CAN_FAIL_TAPS, CAN_FAIL_TOWER, DEPTHWISE_EXACT, GENERIC_EXACT, RES_MAX, SE_EXACT, SPLIT_EXACT, SX_EXACT,
                    TOWER_CASES, TOWER_WIDTHS, case_id, exact_run_layer, layer_reference, se_identity_fc, se_reference, split_strips, tower_draw,
                    tower_spec)
from _kref import act_np, assert_exact, assert_localised, mutated, predicted_change
from _taps import KIND_BOARD, KIND_BOARD_SX, KIND_DEPTHWISE, KIND_GENERIC, KIND_GLDS, KIND_SPLIT, SE_FROM_L2, SE_STAGED, tower_run

pytestmark = pytest.mark.gpu

# the kernel family a child process of test_exact_cases_on_the_fallback_kernels expects of the fp16 3x3 board shapes
VARIANT_KIND = os.environ.get("SAYURI_EXACT_VARIANT_KIND")


# ------------------------------------------------------------------------------------------------ the taps
def tap_conv(c, xs, w, bias, res):
    """one launch of the conv tap -> ([y of every sample], the kernel family that ran)"""
    t = _taps.ok(_taps.conv(c.fp16, c.bsz, c.cin, c.cout, c.k, c.act, xs, w, bias, res, c.depthwise, c.post), c)
    return t.outs, t.kind


def tap_split(c, xs, w, bias, res, strips):
    t = _taps.ok(_taps.conv_split(c.bsz, c.cin, c.cout, c.act, xs, w, bias, res, strips), c, strips)
    return t.outs, t.kind


def board_shape_kind(c):
    """the family an fp16 3x3 board shape must run on: the board kernel, or -- in a child process of a fallback variant -- the
    variant's kernel (asserted where every variant has one: 256 weight rows), never the board kernel"""
    if VARIANT_KIND is None:
        return (KIND_BOARD,)
    return (int(VARIANT_KIND),) if c.cout == 256 else (KIND_GENERIC, int(VARIANT_KIND))


# ------------------------------------------------------------------------------------------------ the GPU cases
@pytest.mark.parametrize("c", GENERIC_EXACT, ids=case_id)
def test_generic_kernel_exact(c):
    """conv_mfma_kernel, fp32 and fp16, 3x3 and 1x1: mixed boards with tiles crossing samples, 43 and 48 input channels (padded
    chunks), 72 and 96 output channels, boards of 2x2 .. 5x5"""
    (xs, w, bias, res), exp = layer_reference(c)
    got, kind = tap_conv(c, xs, w, bias, res)
    assert kind == KIND_GENERIC, (c, kind)
    assert_exact(got, exp, c)


@pytest.mark.parametrize("c", BOARD_EXACT, ids=case_id)
def test_board_shapes_exact(c):
    """conv_board_kernel on every entry of BOARD_CASES (one, two, four, seven boards per tile, mixed sizes, a batch of one, the
    43-channel input convolution, two channel tiles), both tiers at 256 -> 256 and 384 -> 384"""
    (xs, w, bias, res), exp = layer_reference(c)
    got, kind = tap_conv(c, xs, w, bias, res)
    assert kind in board_shape_kind(c), (c, kind, VARIANT_KIND)
    assert_exact(got, exp, c)


@pytest.mark.parametrize("c", SPLIT_EXACT, ids=case_id)
def test_split_kernel_exact(c):
    """conv_split_kernel at every forced split: one strip, two, one per row of the largest board, the engine's choice"""
    (xs, w, bias, res), exp = layer_reference(c)
    for strips in split_strips(c.bsz):
        got, kind = tap_split(c, xs, w, bias, res, strips)
        assert kind == KIND_SPLIT, (c, strips, kind)
        assert_exact(got, exp, (c, "strips", strips))


@pytest.mark.parametrize("fp16", [False, True], ids=["fp32", "fp16"])
@pytest.mark.parametrize("k", [3, 5, 7])
def test_depthwise_kernel_exact(k, fp16):
    """depthwise_kernel: 48 and 40 channels (40: a channel stride of 64 with 24 pad channels), boards down to 2x2 under a 7x7
    kernel, with the residual behind the activation and without one"""
    cases = [c for c in DEPTHWISE_EXACT if c.k == k and c.fp16 == fp16]
    assert len(cases) == 8
    for c in cases:
        (xs, w, bias, res), exp = layer_reference(c)
        got, kind = tap_conv(c, xs, w, bias, res)
        assert kind == KIND_DEPTHWISE, (c, kind)
        assert_exact(got, exp, c)


@pytest.mark.parametrize("fp16", [False, True], ids=["fp32", "fp16"])
@pytest.mark.parametrize("C,se", [(256, 64), (128, 32), (384, 96)])
def test_se_gate_is_exactly_one(C, se, fp16):
    """What the SE cases below rest on, read back from se_pool / se_fc / se_scale: with both FCs zero the gate is sigmoid(32),
    which the kernels' 1.0f / (1.0f + exp(-32)) must give as exactly 1.0f, beta comes back as given, and the unit is
    act(x + beta + res) exactly."""
    bsz = (19, 9, 2)
    fc, beta = se_identity_fc(C, se, 7)
    rng = np.random.default_rng([7, C, se])
    xs = [rng.integers(-200, 201, (C, b * b)).astype(np.float32) for b in bsz]
    rs = [rng.integers(-RES_MAX, RES_MAX + 1, (C, b * b)).astype(np.float32) for b in bsz]
    for act in (0, 1):
        t = _taps.ok(_taps.se_unit(fp16, bsz, C, se, act, xs, rs, fc))
        gate = t.gate
        print(f"se_fc C={C} se={se} {'fp16' if fp16 else 'fp32'} act={act}: gate at gamma = 32 in [{gate[:, :C].min()!r}, {gate[:, :C].max()!r}]")
        assert np.array_equal(gate[:, :C], np.ones((len(bsz), C), np.float32)), "sigmoid(32) is not exactly 1.0f"
        assert np.array_equal(gate[:, C:], np.tile(beta, (len(bsz), 1)))
        exp = [act_np(x.astype(np.float64) + beta[:, None] + r, act).astype(np.float32) for x, r in zip(xs, rs)]
        assert_exact(t.outs, exp, ("se unit", C, se, fp16, act))


@pytest.mark.parametrize("via_tower", [0, 1], ids=["per-layer kernel", "tower kernel"])
@pytest.mark.parametrize("c", SE_EXACT, ids=case_id)
def test_convolution_inside_the_se_kernels_exact(c, via_tower):
    """conv_board_se_kernel and the tower's SE stage (staged FC images: C = 256 / se = 64, C = 128 / se = 32; FCs from L2: se = 128)
    behind an identity gate: y = act(conv + bias + beta + res)"""
    (xs, w, bias, res), fc, exp = se_reference(c)
    t = _taps.ok(_taps.conv_se(c.bsz, c.C, c.se, c.act, xs, w, bias, res, fc, via_tower), c, via_tower)
    assert t.form == (SE_FROM_L2 if (c.C, c.se) == (256, 128) else SE_STAGED), (c, t.form)
    assert_exact(t.outs, exp, (c, "via_tower", via_tower))


@pytest.mark.parametrize("c", SX_EXACT, ids=case_id)
def test_convolution_inside_the_split_channel_se_kernel_exact(c):
    """conv_board_sx_kernel on three and four channel tiles per board tile, one to three samples per tile, behind an identity gate"""
    (xs, w, bias, res), fc, exp = se_reference(c)
    t = _taps.ok(_taps.conv_sx(c.bsz, c.C, c.se, c.act, xs, w, bias, res, fc), c)
    assert t.kind == KIND_BOARD_SX
    assert t.kts == c.C // 128
    assert_exact(t.outs, exp, c)


def tower_report(tc, spec, chain):
    """(layers, layers on the generated epilogue, hand-over links): a link out of every layer without residual whose successor has
    the same weight geometry (not out of a 43-channel input convolution)"""
    links = sum(1 for l in range(spec.L - 1) if spec.res_from[l] < 0 and not (l == 0 and spec.cin0 != spec.C))
    return spec.L, tc.gen, links if chain else 0


@pytest.mark.parametrize("tc", TOWER_CASES, ids=lambda tc: tc.name)
@pytest.mark.parametrize("C", TOWER_WIDTHS)
def test_tower_run_exact(C, tc):
    """conv_tower_kernel, one launch per run: the generated epilogue (ReLU, identity; one board of 19x19 per tile) and the compiled
    one inside a run (shared tiles, mixed sizes), the 43-channel input convolution first, a HardSwish layer in the middle.  Every
    exact layer against exact_layer on what its predecessor really wrote; without the weight hand-over the same values."""
    spec, D = tower_spec(tc, C), tower_draw(tc, C)
    t = _taps.ok(tower_run(spec, D, chain=1), spec)
    outs = t.outs
    assert t.report == tower_report(tc, spec, 1), (spec, t.report)
    for l in range(spec.L):
        for i in range(len(spec.bsz)):
            assert np.isfinite(outs[l][i]).all(), (spec, "layer", l, "sample", i, "an output nobody wrote")
    for l in range(spec.L):
        if l not in tc.skip:
            assert_exact(outs[l], exact_run_layer(spec, D, outs, l), (spec, "layer", l))
    t = tower_run(spec, D, chain=0)
    assert t.rc == 0 and t.report == tower_report(tc, spec, 0), (spec, t.rc, t.report)
    for l in range(spec.L):
        assert_exact(t.outs[l], outs[l], (spec, "layer", l, "without the weight hand-over"))


@pytest.mark.parametrize("name,c,kc", CAN_FAIL, ids=[f[0] for f in CAN_FAIL])
def test_one_changed_weight_is_seen_and_localised(name, c, kc):
    """The real board, split and generic fp16 kernels on w with ONE entry changed by 1, against the unchanged reference."""
    (xs, w, bias, _), exp = layer_reference(c)
    for kr, kcol in CAN_FAIL_TAPS:
        w2 = mutated(w, *kc, kr, kcol)
        if name.startswith("split"):
            got, kind = tap_split(c, xs, w2, bias, None, 2)
            assert kind == KIND_SPLIT
        else:
            got, kind = tap_conv(c, xs, w2, bias, None)
            assert kind == (KIND_BOARD if name.startswith("board") else KIND_GENERIC), (name, kind)
        n = assert_localised(got, exp, predicted_change(xs, c.bsz, c.cout, *kc, kr, kcol), (name, kc, kr, kcol))
        print(f"{name}: w[{kc[0]}][{kc[1]}][{kr}][{kcol}] + 1 moved exactly the {n} predicted outputs")


@pytest.mark.parametrize("C", TOWER_WIDTHS)
def test_one_changed_weight_is_seen_and_localised_in_a_tower_run(C):
    """the same for a one-layer run of the persistent tower kernel (generated epilogue)"""
    tc = CAN_FAIL_TOWER
    spec, D = tower_spec(tc, C), tower_draw(tc, C)
    exp = exact_run_layer(spec, D, [], 0)
    for kr, kcol in CAN_FAIL_TAPS:
        M = copy.copy(D)
        M.ws = [mutated(D.ws[0], C - 1, C - 1, kr, kcol)]
        t = tower_run(spec, M, chain=1)
        outs = t.outs
        assert t.rc == 0 and t.report == (1, 1, 0), (t.rc, t.report)
        n = assert_localised(outs[0], exp, predicted_change(D.xs, spec.bsz, C, C - 1, C - 1, kr, kcol), ("tower", C, kr, kcol))
        print(f"tower C={C}: w[{C - 1}][{C - 1}][{kr}][{kcol}] + 1 moved exactly the {n} predicted outputs")


@pytest.mark.parametrize("env,kind", [("glds", KIND_GLDS), ("v0", KIND_GENERIC)], ids=["SAYURI_CONV=glds", "SAYURI_CONV=v0"])
def test_exact_cases_on_the_fallback_kernels(env, kind):
    """The A/B switch of the fp16 3x3 kernels is read once per process: conv_glds_kernel (tiles across samples) and the generic
    register-staged kernel run the generic and the board-shape cases of this module in a process of their own, which asserts the
    variant's family on every 256 -> 256 layer and that no layer took the board kernel."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    e = dict(os.environ, SAYURI_CONV=env, SAYURI_EXACT_VARIANT_KIND=str(kind))
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.join(root, "tests", "test_gpu_exact.py"), "-x", "-q", "-k",
                        "test_generic_kernel_exact or test_board_shapes_exact"], env=e, cwd=root, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert " passed" in r.stdout and "skipped" not in r.stdout, r.stdout[-1000:]
