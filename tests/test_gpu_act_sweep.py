"""Every activation epilogue over the whole fp16 range: the compiled epilogue of conv_board_kernel, conv_split_kernel, conv_glds_kernel
and the generic fp16 kernel (child processes), conv_mfma_kernel<float>, conv_pw_kernel, conv_dw_kernel<3> and depthwise_kernel, the
persistent tower's generated and compiled epilogues, se_scale_kernel / se_unit_kernel, conv_board_se_kernel, the tower's SE stage and
conv_board_sx_kernel -- all eight activations each.  test_gpu_exact.py holds the same kernels to one value for the identity and ReLU
on small integers; here the six transcendental activations get a bound that a wrong constant, edge, guard or store cannot meet.

The principle.  An identity convolution delivers any chosen value exactly: the weights are a channel permutation pi in the centre tap
(w[c][pi(c)][centre] = 1, all else 0, bias 0), so the accumulator holds x[pi(c)] -- every other product is 0 * finite.  One layer of
at least 92 416 pre-activations carries all 63 488 finite fp16 values (both zeros, every subnormal), the rest of the slots repeat the
activations' edges and their fp16 neighbours (0, +-3, 20, +-11.09, +-65504), shuffled with a fixed seed (_cases.sweep_values).  Each
route runs three times per activation: without residual; with a residual that is another permutation of the same sweep (sums
cancel, leave the fp16 grid, overflow); with a small residual (z = x + res fills |z| < 32 off the grid).  The fp32 routes add fp32
points next to 0, +-3, 20 and at +-87.3, +-88.8, +-104 where fp32 exp under- and overflows.

The reference is _kref.act_f64 on the exact float64 z = x[pi] + res (depthwise order: act(x) + res).  The bound of an fp16 store:
    |got - ref| <= ulp16(ref) / 2 + K 2^-24 max(1, |z|, |ref|)        (an fp32 store: the second term alone)
the one round-to-nearest store plus the fp32 evaluation, whose error is absolute in shape (Mish's 1 - 2r, GELU's 1 - 2 / (e + 1), ELU's
exp - 1 cancel: the restated Mish is 16 subnormal ulps off at x = -16.6, yet 1.0 x 2^-24 |x|).  K = 8: the numpy-float32 restatement of
common.h's formulas is at most 3.34 (SELU) such units off over all fp16 values (test_act_sweep_reference_cpu.py recomputes the table);
numpy's exp2 and division are correctly rounded where v_exp_f32 and v_rcp_f32 are good to 1 ulp, so the transcendental part may
double, and the fp32 rounding of x + res adds at most 1.1: 2 x 3.34 + 1.1 < 8.  K was fixed before any GPU run.  Identity and ReLU
have no bound: got == float16(act(z)) value for value (the sum of two fp16 values rounded to fp32 and then to fp16 is float16 of the
exact sum).  No output may be NaN; +-inf only if |ref| + bound >= 65520, and required if |ref| - bound >= 65520.

Every case asserts the kernel family, the SE form or the tower report it is about, and the bit identities the code and DESIGN.md
claim are asserted on the sweep's raw outputs: split == board, tower (generated and compiled epilogue in a run) == board, pw ==
generic fp16 1x1, conv_dw == depthwise_kernel, se_unit under SAYURI_SE_ONE=1 == three launches.

Run on an MI355X: all 162 cases pass, each on the family, SE form or tower report it asserts, and every bit identity holds on every
activation and residual mode.  The identity sweep comes back value for value on every route, all 2046 fp16 subnormals included: the
MFMA path does not flush them, so nothing is excluded from the draw.  No kernel defect was found.  Wall time of the module: 10.5 s,
3.7 s of it the two child processes.  Worst observed |got - ref| / bound per route and activation, over the three residual modes,
and behind the slash how much of K the finite outputs use ((|got - ref| - the store's half ulp) / (2^-24 max(1, |z|, |ref|)); for an
fp32 store that is the whole error, and the 1.00 of the fp32 identity is the one rounding of x + res).  With an fp16 store the first
figure is the store's own half ulp (0.999 of the bound wherever a value sits next to a tie).  A record, no input to the bound:
  conv_board_kernel 128 ch and conv_split_kernel (same bits): elu 0.999/0.60, selu 0.999/1.32, gelu 0.999/1.35, mish 0.999/1.49,
      swish 0.999/0.96, hardswish 0.999/0.57
  conv_board_kernel 192 ch: elu 0.999/0.60, selu 0.999/1.26, gelu 0.999/1.27, mish 0.999/1.39, swish 0.999/1.01, hardswish
      0.999/0.32
  conv_board_kernel 256 ch, conv_glds_kernel, generic fp16 3x3 (three kernels, same figures): elu 0.999/0.59, selu 0.999/1.26,
      gelu 0.999/1.31, mish 0.999/1.30, swish 0.999/0.99, hardswish 0.999/0.57
  conv_mfma_kernel<float> 3x3: identity 0/1.00, relu 0/1.00, elu 0.132/1.06, selu 0.326/2.61, gelu 0.311/2.49, mish 0.301/2.41,
      swish 0.346/2.77, hardswish 0.320/2.56
  conv_mfma_kernel<float> 1x1: identity 0/1.00, relu 0/1.00, elu 0.134/1.07, selu 0.321/2.57, gelu 0.328/2.62, mish 0.303/2.42,
      swish 0.328/2.62, hardswish 0.300/2.40
  conv_pw_kernel and generic fp16 1x1 (same bits): elu 0.999/0.60, selu 0.999/1.49, gelu 0.999/1.46, mish 0.999/1.29, swish
      0.999/0.99, hardswish 0.999/0.30
  conv_dw_kernel<3> and depthwise_kernel fp16 (same bits): elu 0.999/0.70, selu 0.999/1.31, gelu 0.999/1.21, mish 0.999/1.11,
      swish 0.999/1.13, hardswish 0.999/0.46
  depthwise_kernel fp32: identity 0/1.00, relu 0/1.00, elu 0.208/1.66, selu 0.411/3.28, gelu 0.235/1.88, mish 0.259/2.07, swish
      0.268/2.14, hardswish 0.187/1.50
  tower C=256: generated mish 0.999/1.35; compiled elu 0.999/0.63, selu 0.999/1.07, gelu 0.999/1.25, swish 0.999/0.99, hardswish
      0.999/0.56
  tower C=128: generated mish 0.999/1.29; compiled elu 0.999/0.60, selu 0.999/1.07, gelu 0.999/1.16, swish 0.999/0.99, hardswish
      0.999/0.22
  se_scale / se_unit_kernel fp16: elu 0.999/0.60, selu 0.999/1.07, gelu 0.999/1.18, mish 0.999/1.30, swish 0.999/0.96, hardswish
      0.999/0.27
  se_scale / se_unit_kernel fp32: identity 0/1.00, relu 0/1.00, elu 0.152/1.22, selu 0.327/2.62, gelu 0.321/2.57, mish
      0.285/2.28, swish 0.326/2.60, hardswish 0.302/2.42
  conv_board_se_kernel and the tower's SE stage (same figures) C=256 se=64 and se=128: elu 0.999/0.58, selu 0.999/1.35, gelu
      0.999/1.46, mish 0.999/1.39, swish 0.999/1.23, hardswish 0.999/0.22
  the same, C=128 se=32: elu 0.999/0.62, selu 0.999/1.37, gelu 0.999/1.27, mish 0.999/1.48, swish 0.999/0.99, hardswish 0.999/0.74
  conv_board_sx_kernel C=384 se=96: elu 0.999/0.59, selu 0.999/0.96, gelu 0.999/1.27, mish 0.999/1.41, swish 0.999/1.07,
      hardswish 0.999/0.69
Identity and ReLU are equal value for value everywhere (0 / 0 where not listed).  The reference, bound and predicate are in _kref.py, the
draws in _cases.py; test_act_sweep_reference_cpu.py shows on the CPU that the predicate can fail.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import _taps
from _cases import RunSpec, perm_weights, se_identity_fc, sweep_inputs, sweep_perm
from _kref import ACT_NAMES, act_f64, act_sweep_bad, act_units_used
from _taps import KIND_BOARD, KIND_BOARD_SX, KIND_DEPTHWISE, KIND_GENERIC, KIND_GLDS, KIND_SPLIT, SE_FROM_L2, SE_STAGED
from sayuri_amd import hipraw

pytestmark = pytest.mark.gpu

KIND_PW, KIND_DW_LDS = 6, 7   # what the last-conv-kind reader says after the pointwise / the LDS depthwise tap
MODES = ("none", "sweep", "small")
ACTS = list(range(8))
GENERATED = (0, 1, 5)   # the activations the tower's generated epilogue covers
NORMALS_ONLY = False    # DESIGN.md, "Activation sweep": whether the MFMA path keeps fp16-subnormal operands
# the kernel family a child process of test_sweep_on_the_fallback_kernels expects of the 256 -> 256 board shape
VARIANT_KIND = os.environ.get("SAYURI_ACT_SWEEP_VARIANT_KIND")


def flat(planes):
    return np.concatenate([np.asarray(p).ravel() for p in planes])


def inputs(bsz, C, mode, seed=0, f32=False):
    return sweep_inputs(tuple(bsz), C, mode, seed, NORMALS_ONLY, f32)


def z_of(xs, res, pi):
    """the exact float64 argument of the activation behind a permutation convolution: x[pi] + res, flat in the outputs' order"""
    z = flat([x[pi] for x in xs]).astype(np.float64)
    return z if res is None else z + flat(res).astype(np.float64)


def check(route, act, mode, outs, z, store16=True, post_res=None):
    """the sweep's predicate on one launch's outputs; prints how much of the bound was used"""
    got = flat(outs)
    post_res = None if post_res is None else flat(post_res)
    bad, ratio = act_sweep_bad(got, z, act, store16, post_res)
    print(f"[act-sweep] {route} | {ACT_NAMES[act]} | {mode}: worst |got - ref| / bound = {float(ratio.max()):.3f}, "
          f"of K {act_units_used(got, z, act, store16, post_res):.2f}, {got.size} values, {int(np.isinf(got).sum())} inf")
    if bad.any():
        ref = act_f64(z, act) + (0.0 if post_res is None else post_res)
        first = [(float(z[i]), float(got[i]), float(ref[i])) for i in np.flatnonzero(bad)[:8]]
        raise AssertionError((route, ACT_NAMES[act], mode, int(bad.sum()), "values outside the bound; the first (z, got, ref):", first))


def same_bits(a, b):
    bits = lambda v: np.ascontiguousarray(v, np.float32).view(np.uint32)
    return len(a) == len(b) and all(np.array_equal(bits(x), bits(y)) for x, y in zip(a, b))


def act_id(a):
    return ACT_NAMES[a]


# ------------------------------------------------------------------------------------------------ 3x3 board shapes
BOARD_SHAPES = {"c128": (128, (19, 19)),   # the split kernel's shape
                "c192": (192, (19, 19)),   # an odd row-tile count per wave: the lone tile's 4-wide store
                "c256": (256, (19,))}      # residual pieces that go to registers


def board_layer(C, bsz, act, mode):
    xs, res = inputs(bsz, C, mode, seed=C)
    pi = sweep_perm(C, C)
    t = _taps.ok(_taps.conv(True, bsz, C, C, 3, act, xs, perm_weights(pi, 3), None, res), C, act, mode)
    return xs, res, pi, t


@pytest.mark.parametrize("act", ACTS, ids=act_id)
@pytest.mark.parametrize("shape", list(BOARD_SHAPES))
def test_compiled_epilogue_of_the_board_kernel(shape, act):
    """conv_board_kernel -- in a child process of a fallback variant, the variant's kernel on the 256 -> 256 shape"""
    C, bsz = BOARD_SHAPES[shape]
    for mode in MODES:
        xs, res, pi, t = board_layer(C, bsz, act, mode)
        if VARIANT_KIND is None:
            assert t.kind == KIND_BOARD, (shape, t.kind)
        elif C == 256:
            assert t.kind == int(VARIANT_KIND), (shape, t.kind, VARIANT_KIND)
        else:
            assert t.kind != KIND_BOARD, (shape, t.kind)
        check(f"conv tap kind {t.kind} {shape}", act, mode, t.outs, z_of(xs, res, pi))


@pytest.mark.parametrize("act", ACTS, ids=act_id)
def test_split_kernel(act):
    """conv_split_kernel at one strip, two, one per row and the engine's choice: the bound, and the board kernel's bits"""
    C, bsz = BOARD_SHAPES["c128"]
    for mode in MODES:
        xs, res, pi, board = board_layer(C, bsz, act, mode)
        assert board.kind == KIND_BOARD
        z = z_of(xs, res, pi)
        for strips in (1, 2, 19, 0):
            t = _taps.ok(_taps.conv_split(bsz, C, C, act, xs, perm_weights(pi, 3), None, res, strips), act, mode, strips)
            assert t.kind == KIND_SPLIT, (strips, t.kind)
            check(f"conv_split strips {strips}", act, mode, t.outs, z)
            assert same_bits(t.outs, board.outs), (act, mode, strips, "split != board")


@pytest.mark.parametrize("env,kind", [("glds", KIND_GLDS), ("v0", KIND_GENERIC)], ids=["SAYURI_CONV=glds", "SAYURI_CONV=v0"])
def test_sweep_on_the_fallback_kernels(env, kind):
    """conv_glds_kernel and the generic register-staged fp16 kernel: the A/B switch is read once per process, so the 256 -> 256 case of
    test_compiled_epilogue_of_the_board_kernel runs in a process of its own, which asserts the variant's family"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    e = dict(os.environ, SAYURI_CONV=env, SAYURI_ACT_SWEEP_VARIANT_KIND=str(kind))
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.join(root, "tests", "test_gpu_act_sweep.py"), "-x", "-q", "-s", "-k",
                        "test_compiled_epilogue_of_the_board_kernel and c256"], env=e, cwd=root, capture_output=True, text=True, timeout=600)
    print("\n".join(line for line in r.stdout.splitlines() if line.startswith("[act-sweep]")))
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert "8 passed" in r.stdout and "skipped" not in r.stdout, r.stdout[-1000:]


# ------------------------------------------------------------------------------------------------ fp32, pointwise, depthwise
@pytest.mark.parametrize("act", ACTS, ids=act_id)
@pytest.mark.parametrize("k", [3, 1])
def test_generic_fp32_kernel(k, act):
    """conv_mfma_kernel<float>: the fp16-grid values and the fp32 points, an fp32 store"""
    C, bsz = 128, (19, 19)
    pi = sweep_perm(C, 32 + k)
    for mode in MODES:
        xs, res = inputs(bsz, C, mode, seed=32 + k, f32=True)
        t = _taps.ok(_taps.conv(False, bsz, C, C, k, act, xs, perm_weights(pi, k), None, res), k, act, mode)
        assert t.kind == KIND_GENERIC, t.kind
        check(f"conv_mfma<float> {k}x{k}", act, mode, t.outs, z_of(xs, res, pi), store16=False)


@pytest.mark.parametrize("act", ACTS, ids=act_id)
def test_pointwise_kernel(act):
    """conv_pw_kernel at the engine's cut and at two pieces: the bound, and the generic fp16 1x1 kernel's bits"""
    C, bsz = 128, (19, 19)
    pi = sweep_perm(C, 41)
    w = perm_weights(pi, 1)
    for mode in MODES:
        xs, res = inputs(bsz, C, mode, seed=41)
        z = z_of(xs, res, pi)
        gen = _taps.ok(_taps.conv(True, bsz, C, C, 1, act, xs, w, None, res), act, mode)
        assert gen.kind == KIND_GENERIC, gen.kind
        check("generic fp16 1x1", act, mode, gen.outs, z)
        for pieces in (0, 2):
            t = _taps.ok(_taps.Conv(*hipraw.conv_pw_layer(list(bsz), C, C, act, xs, w, None, res, pieces)), act, mode, pieces)
            assert t.kind == KIND_PW, t.kind
            check(f"conv_pw pieces {pieces}", act, mode, t.outs, z)
            assert same_bits(t.outs, gen.outs), (act, mode, pieces, "pw != generic fp16 1x1")


@pytest.mark.parametrize("act", ACTS, ids=act_id)
@pytest.mark.parametrize("bsz", [(19,), (9, 13, 19)], ids=["b19", "b9-13-19"])
def test_depthwise_kernels(bsz, act):
    """conv_dw_kernel<3> and depthwise_kernel (fp16 and fp32), centre tap 1: act(x) + res, the residual behind the activation"""
    C = 256
    pi = sweep_perm(C, 0, identity=True)
    w = perm_weights(pi, 3, depthwise=True)
    for mode in MODES:
        xs, res = inputs(bsz, C, mode, seed=51)
        z = z_of(xs, None, pi)
        lds = _taps.ok(_taps.Conv(*hipraw.conv_dw_layer(list(bsz), C, 3, act, xs, w, None, res)), act, mode)
        assert lds.kind == KIND_DW_LDS, lds.kind
        check("conv_dw<3>", act, mode, lds.outs, z, post_res=res)
        old = _taps.ok(_taps.conv(True, bsz, 1, C, 3, act, xs, w, None, res, depthwise=True, post=res is not None), act, mode)
        assert old.kind == KIND_DEPTHWISE, old.kind
        check("depthwise_kernel fp16", act, mode, old.outs, z, post_res=res)
        assert same_bits(lds.outs, old.outs), (act, mode, "conv_dw != depthwise_kernel")
        xf, rf = inputs(bsz, C, mode, seed=51, f32=True)
        t = _taps.ok(_taps.conv(False, bsz, 1, C, 3, act, xf, w, None, rf, depthwise=True, post=rf is not None), act, mode)
        assert t.kind == KIND_DEPTHWISE, t.kind
        check("depthwise_kernel fp32", act, mode, t.outs, z_of(xf, None, pi), store16=False, post_res=rf)


# ------------------------------------------------------------------------------------------------ the persistent tower
class RunData:
    def __init__(self, xs, ws, C):
        self.xs, self.ws, self.bias, self.fc = xs, ws, np.zeros((len(ws), C), np.float32), None


@pytest.mark.parametrize("act", ACTS, ids=act_id)
@pytest.mark.parametrize("C", [256, 128])
def test_tower_epilogues(C, act):
    """conv_tower_kernel, two layers in one launch, one 19x19 board per tile: layer 0 is a permutation under the identity, the checked
    layer 1 a second permutation under `act` with the run's input as residual, so the two addends differ.  Mish, ReLU and the
    identity run on the generated epilogue (the report says two row-order layers), the other five on the compiled one inside the
    run (one).  The bound, and the board kernel's bits on the same operands."""
    bsz = (19, 19)
    p0, p1 = sweep_perm(C, 61), sweep_perm(C, 62)
    ws = [perm_weights(p0, 3), perm_weights(p1, 3)]
    for mode in MODES:
        # "small": the run's input is the small draw itself, so z = s[pi] + s fills |z| < 32 off the grid
        xs = inputs(bsz, C, "small", seed=60 + C)[1] if mode == "small" else inputs(bsz, C, "none", seed=60 + C)[0]
        with_res = mode != "none"
        spec = RunSpec(bsz, C, (0, act), (-1, 0 if with_res else -1), seed=0)
        t = _taps.ok(_taps.tower_run(spec, RunData(xs, ws, C), chain=1), spec)
        assert t.report == (2, 1 + int(act in GENERATED), 1), (spec, t.report)
        check(f"tower C={C} layer 0", 0, mode, t.outs[0], z_of(xs, None, p0))
        mid = [x[p0] for x in xs]
        res = xs if with_res else None
        check(f"tower C={C} {'generated' if act in GENERATED else 'compiled'} epilogue", act, mode, t.outs[1], z_of(mid, res, p1))
        board = _taps.ok(_taps.conv(True, bsz, C, C, 3, act, t.outs[0], ws[1], None, res), spec)
        assert board.kind == KIND_BOARD
        assert same_bits(t.outs[1], board.outs), (C, act, mode, "tower != board")


# ------------------------------------------------------------------------------------------------ the SE kernels
def identity_gate(C, se):
    """both FCs zero, gamma = 32 (the kernels' sigmoid gives exactly 1.0f: test_gpu_exact.py reads it back), beta = 0"""
    fc, _ = se_identity_fc(C, se, 0)
    b2 = fc[3].copy()
    b2[C:] = 0.0
    return fc[:3] + (b2,)


@pytest.mark.parametrize("act", ACTS, ids=act_id)
@pytest.mark.parametrize("fp16", [True, False], ids=["fp16", "fp32"])
def test_se_scale_and_se_unit_kernels(fp16, act, monkeypatch):
    """se_pool / se_fc / se_scale and, under SAYURI_SE_ONE=1, se_unit_kernel behind an identity gate: y = act(x + res); same bits"""
    C, se, bsz = 128, 32, (19, 19)
    fc = identity_gate(C, se)
    pi = np.arange(C)
    for mode in MODES:
        xs, res = inputs(bsz, C, mode, seed=71, f32=not fp16)
        z = z_of(xs, res, pi)
        outs = {}
        for one in (False, True):
            if one:
                monkeypatch.setenv("SAYURI_SE_ONE", "1")
            else:
                monkeypatch.delenv("SAYURI_SE_ONE", raising=False)
            try:
                t = _taps.ok(_taps.se_unit(fp16, bsz, C, se, act, xs, res, fc), act, mode, one)
            finally:
                monkeypatch.delenv("SAYURI_SE_ONE", raising=False)
            assert np.array_equal(t.gate[:, :C], np.ones((len(bsz), C), np.float32)) and not t.gate[:, C:].any(), "the gate is not the identity"
            check(f"se unit {'fp16' if fp16 else 'fp32'} {'one launch' if one else 'three launches'}", act, mode, t.outs, z, store16=fp16)
            outs[one] = t.outs
        assert same_bits(outs[True], outs[False]), (fp16, act, mode, "se_unit under the switch != three launches")


SE_SHAPES = [(256, 64, (19,)), (128, 32, (19, 19)), (256, 128, (19,))]


@pytest.mark.parametrize("act", ACTS, ids=act_id)
@pytest.mark.parametrize("via_tower", [0, 1], ids=["per-layer kernel", "tower kernel"])
@pytest.mark.parametrize("C,se,bsz", SE_SHAPES, ids=[f"C{c}se{s}" for c, s, _ in SE_SHAPES])
def test_fused_se_kernels(C, se, bsz, via_tower, act):
    """conv_board_se_kernel and the tower's SE stage behind an identity gate, FC images staged and read from L2"""
    fc = identity_gate(C, se)
    pi = sweep_perm(C, 81)
    for mode in MODES:
        xs, res = inputs(bsz, C, mode, seed=81)
        t = _taps.ok(_taps.conv_se(bsz, C, se, act, xs, perm_weights(pi, 3), None, res, fc, via_tower), C, se, act, mode, via_tower)
        assert t.form == (SE_FROM_L2 if (C, se) == (256, 128) else SE_STAGED), (C, se, t.form)
        check(f"conv_se C={C} se={se} {'tower' if via_tower else 'per-layer'}", act, mode, t.outs, z_of(xs, res, pi))


@pytest.mark.parametrize("act", ACTS, ids=act_id)
def test_split_channel_se_kernel(act):
    """conv_board_sx_kernel on three channel tiles per board tile behind an identity gate"""
    C, se, bsz = 384, 96, (19, 19)
    fc = identity_gate(C, se)
    pi = sweep_perm(C, 91)
    for mode in MODES:
        xs, res = inputs(bsz, C, mode, seed=91)
        t = _taps.ok(_taps.conv_sx(bsz, C, se, act, xs, perm_weights(pi, 3), None, res, fc), act, mode)
        assert t.kind == KIND_BOARD_SX and t.kts == 3, (t.kind, t.kts)
        check("conv_sx C=384 se=96", act, mode, t.outs, z_of(xs, res, pi))
