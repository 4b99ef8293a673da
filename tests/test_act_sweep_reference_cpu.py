"""What test_gpu_act_sweep.py rests on, without a GPU: the float64 reference act_f64, the sweep draw, the bound and its constant
K, and that the bound is not vacuous -- every planted mistake of an epilogue puts values outside it, while the suite's old bound
(4e-3 * max|y| on N(0, 1) pre-activations) lets nearly all of them pass.

The K table.  act_f32_emu (_kref.py) restates common.h's activate() in numpy float32.  Over the 63 488 finite fp16 values the worst
|emu - ref| / (2^-24 max(1, |x|, |ref|)) is: identity 0, ReLU 0, ELU 1.90, SELU 3.34, GELU 1.61, Mish 1.55, Swish 1.87, HardSwish 0.59
(ELU and SELU with __expf stated as numpy's float32 exp; stated as exp2(x * log2e) they give 1.21 and 2.62).  Every entry is asserted
<= 3.5, and with K = 8 the restatement has no value outside the bound, with and without a residual.

Planted mistakes, values outside the bound among the 63 488 (the store rounds to nearest unless said otherwise): HardSwish edge at 2.5
255, / 6 as * 0.1667 4754, SELU alpha 1.67 25 547, GELU coefficient 0.0455 3481, erf-form GELU 3448, Mish guard at 2 1065, exp2
without log2(e) in Swish 24 458 and in ELU 18 916, a store rounding toward zero 6681 .. 18 537 per transcendental activation.  Each
is asserted >= 100.  SELU scale 1.0507 for 1.05070098 is a relative mistake of 15.6 * 2^-24, forty times smaller than the store's
half ulp, so it shows only where it flips a rounding: 18 of the 63 488 grid values, 87 over the three residual modes of the 128-channel
case, 194 over the three modes of the 128- and the 192-channel board cases together, which is where its floor of 100 is asserted.

The old bound.  On 92 416 N(0, 1) fp16 pre-activations, in units of 4e-3 * max|y|: / 6 as * 0.1667 0.09, SELU alpha 0.21, SELU scale 0.09,
GELU coefficient 0.08, erf-form GELU 0.08, a store toward zero <= 1 for all six -- all pass.  Four do not stay inside it where the
data reaches them: HardSwish edge at 2.5 11.9 (a step of 0.21 on the 0.6 % of N(0, 1) that falls in [2.5, 3)), Mish guard at 2 3.2,
exp2 without log2(e) in Swish 11.2 and in ELU 7.7.  LOOSE_SEES lists those four and the test asserts the list."""
import numpy as np
import pytest

from _cases import (F16_FINITE, F32_POINTS, SWEEP_EDGES, SWEEP_MODES, perm_weights, sweep_edge_bits, sweep_inputs, sweep_perm, sweep_small,
                    sweep_values)
from _kref import (ACT_DEFECTS, ACT_K, ACT_NAMES, act_bound, act_f32_emu, act_f64, act_np, act_sweep_bad, conv_ref, f16_store_toward_zero, ulp16)

GRID = F16_FINITE.view(np.float16).astype(np.float32)
K_TABLE = {0: 0.0, 1: 0.0, 2: 1.90, 3: 3.34, 4: 1.61, 5: 1.55, 6: 1.87, 7: 0.59}
DEFECT_ACT = {"hswish_edge_2.5": 7, "hswish_times_0.1667": 7, "selu_alpha_1.67": 3, "selu_scale_1.0507": 3, "gelu_coef_0.0455": 4, "gelu_erf": 4,
              "mish_guard_2": 5, "swish_no_log2e": 6, "elu_no_log2e": 2}
LOOSE_SEES = {"swish_no_log2e", "elu_no_log2e", "hswish_edge_2.5", "mish_guard_2"}   # the planted mistakes the old bound does see


def store16(a):
    with np.errstate(over="ignore"):
        return np.asarray(a, np.float32).astype(np.float16).astype(np.float64)


def flat(planes):
    return np.concatenate([p.ravel() for p in planes])


def mode_z(bsz, C, mode):
    """(the fp32 sum a kernel forms, the exact float64 z) of one residual mode of a sweep case"""
    xs, res = sweep_inputs(bsz, C, mode)
    x = flat(xs)
    if res is None:
        return x, x.astype(np.float64)
    r = flat(res)
    return x + r, x.astype(np.float64) + r.astype(np.float64)


# ---------------------------------------------------------------------------------------------------------------- the reference
@pytest.mark.parametrize("act", range(8), ids=ACT_NAMES)
def test_act_f64_agrees_with_act_np_and_has_its_limits(act):
    z = np.concatenate([np.linspace(-30, 30, 24001), GRID[np.abs(GRID) <= 30].astype(np.float64)])
    a, b = act_f64(z, act), act_np(z, act)
    assert np.all(np.abs(a - b) <= 1e-12 * np.abs(b)), (act, "relative agreement on |z| <= 30")
    far = np.array([-1.4e5, -65504.0, -800.0, -100.0, -31.0, 31.0, 100.0, 800.0, 65504.0, 1.4e5])
    lim = {0: far, 1: np.maximum(far, 0), 2: np.where(far > 0, far, -1.0), 3: np.where(far > 0, 1.05070098 * far, -1.05070098 * 1.67326324),
           4: np.maximum(far, 0), 5: np.maximum(far, 0), 6: np.maximum(far, 0), 7: np.maximum(far, 0)}[act]
    got = act_f64(far, act)
    assert np.isfinite(got).all()
    assert np.all(np.abs(got - lim) <= 1e-11 * np.maximum(1.0, np.abs(lim))), (act, got - lim)


def test_act_f64_keeps_the_negative_tails_act_np_loses():
    """Mish at -16.6 is -1.0e-6 (x e^x to first order); the restated kernel formula is 16 subnormal fp16 ulps away from it there, yet
    only 1.0 x 2^-24 |x|: 1 - 2r cancels, the error is absolute.  So the bound cannot be one in ulps.  The tails past 709 stay finite."""
    x = float(np.float16(-16.6))
    true = float(act_f64(x, 5))
    assert abs(true - x * np.exp(x)) <= 1e-6 * abs(true) and -1.1e-6 < true < -9.8e-7
    emu = float(act_f32_emu(np.float32(x), 5))
    assert abs(emu - true) / float(ulp16(true)) > 15
    assert abs(emu - true) <= 1.1 * 2.0 ** -24 * abs(x)
    assert not act_sweep_bad(np.array([emu]), np.array([x]), 5)[0].any()
    for act in (5, 6):
        assert float(act_f64(-800.0, act)) == 0.0 and float(act_f64(800.0, act)) == 800.0
    with np.errstate(over="ignore", invalid="ignore"):
        assert not np.isfinite(act_np(np.array([800.0]), 5)).all() or float(act_np(np.array([-800.0]), 6)[0]) == 0.0


@pytest.mark.parametrize("act", range(8), ids=ACT_NAMES)
def test_act_f64_against_the_oracle(act):
    """The CPU oracle's own activations, reached through its fully-connected tap with zero weights: y = act(bias), in fp32 with libm --
    2e-5 of the scale, the project's fp32 bound, over the fp16 grid where the oracle's float forms stay finite (|z| <= 80) and the
    fp32 points below that"""
    from _oracle import PortNet
    from sayuri_amd._lib import fp
    z = np.ascontiguousarray(np.concatenate([GRID[np.abs(GRID) <= 80.0], F32_POINTS[np.abs(F32_POINTS) <= 80.0]]))
    y, w, x = np.full(z.shape, np.nan, np.float32), np.zeros(z.shape, np.float32), np.zeros(1, np.float32)
    PortNet.lib().so_tap_fully_connect(1, len(z), fp(w), fp(z), fp(x), fp(y), act)
    ref = act_f64(z, act)
    assert np.isfinite(y).all()
    assert np.all(np.abs(y - ref) <= 2e-5 * np.maximum(1.0, np.abs(ref))), (act, float(np.abs(y - ref).max()))


def test_ulp16():
    for v, u in ((0.0, 2.0 ** -24), (2.0 ** -15, 2.0 ** -24), (2.0 ** -14, 2.0 ** -24), (1.0, 2.0 ** -10), (1.999, 2.0 ** -10), (2.0, 2.0 ** -9),
                 (-2048.0, 2.0), (65504.0, 32.0), (1.0e5, 32.0)):
        assert float(ulp16(v)) == u, (v, float(ulp16(v)), u)
    pos = np.arange(0x0001, 0x7C00, dtype=np.uint16).view(np.float16).astype(np.float64)
    assert np.array_equal(ulp16(pos[:-1]), np.diff(pos))


# ---------------------------------------------------------------------------------------------------------------- the draw
def test_sweep_draw_holds_every_finite_fp16_value_and_every_edge():
    n = 128 * 2 * 361
    v = sweep_values(n, 0)
    assert v.shape == (n,) and v.dtype == np.float32 and not v.flags.writeable
    bits = v.astype(np.float16).view(np.uint16)
    assert np.array_equal(bits.view(np.float16).astype(np.float32), v), "every value is an fp16 value"
    assert np.array_equal(np.unique(bits), np.sort(F16_FINITE)) and len(F16_FINITE) == 63488
    edges = np.array(SWEEP_EDGES, np.float16).view(np.uint16)
    for e in edges.tolist():
        for nb in (e - 1, e, e + 1):   # the neighbour of 0 below is the other zero's first subnormal, which the other zero brings
            if (nb & 0x7FFF) < 0x7C00 and 0 <= nb and nb != 0x7FFF:
                assert (bits == nb).sum() >= 2, ("an edge or its neighbour is not repeated", hex(nb))
    assert set(sweep_edge_bits().tolist()) <= set(bits.tolist())
    assert np.array_equal(v, sweep_values.__wrapped__(n, 0)), "the same draw for the same seed"
    assert not np.array_equal(v, sweep_values(n, 1000)) and np.array_equal(np.sort(v), np.sort(sweep_values(n, 1000)))
    nz = sweep_values(n, 0, normals_only=True).astype(np.float16).view(np.uint16)
    assert len(np.unique(nz)) == 61442 and not (((nz & 0x7FFF) < 0x0400) & ((nz & 0x7FFF) != 0)).any()
    f = sweep_values(n, 0, f32_points=True)
    assert all((f == p).any() for p in F32_POINTS) and len(np.unique(f.view(np.uint32))) > 63488
    s = sweep_small(n, 0)
    assert float(np.abs(s).max()) <= 16.0 and np.array_equal(s.astype(np.float16).astype(np.float32), s)


def test_residual_modes_cancel_overflow_and_leave_the_grid():
    x32, z = mode_z((19, 19), 128, "sweep")
    assert (z == 0).sum() > 0 and (np.abs(z) >= 65520).sum() > 100
    assert (store16(z).astype(np.float64) != z).sum() > 10000, "sums off the fp16 grid"
    assert np.array_equal(x32.astype(np.float64), z) or float(np.abs(x32 - z).max()) <= 2.0 ** -24 * 131008
    _, zs = mode_z((19, 19), 128, "small")
    band = zs[np.abs(zs) < 32]
    assert len(band) > 60000 and (store16(band) != band).sum() > 10000
    # the sum of two fp16 values rounded to fp32 and then to fp16 is float16 of the exact sum: identity and ReLU have one value
    for mode in SWEEP_MODES[1:]:
        s32, s64 = mode_z((19, 19), 128, mode)
        with np.errstate(over="ignore"):
            assert np.array_equal(s32.astype(np.float16), s64.astype(np.float16))


def test_permutation_weights_deliver_x_of_pi():
    C, bsz = 128, (19, 19)
    pi = sweep_perm(C, 0)
    assert sorted(pi.tolist()) == list(range(C)) and not np.array_equal(pi, np.arange(C))
    xs, res = sweep_inputs(bsz, C, "sweep")
    w = perm_weights(pi, 3)
    assert w.sum() == C and np.array_equal(np.nonzero(w)[1], pi) and set(np.nonzero(w)[2]) == {1} == set(np.nonzero(w)[3])
    y = conv_ref([x.astype(np.float64) for x in xs], bsz, w, None, None, 3, False, 0, False)
    for yy, x in zip(y, xs):
        assert np.array_equal(yy, x[pi].astype(np.float64))
    wd = perm_weights(np.arange(8), 3, depthwise=True)
    yd = conv_ref([xs[0][:8].astype(np.float64)], (19,), wd, None, None, 3, True, 0, True)
    assert np.array_equal(yd[0], xs[0][:8].astype(np.float64))


# ---------------------------------------------------------------------------------------------------------------- K and the bound
def test_k_table():
    for act in range(8):
        ref = act_f64(GRID, act)
        emu = act_f32_emu(GRID, act).astype(np.float64)
        worst = float((np.abs(emu - ref) / (2.0 ** -24 * np.maximum(1.0, np.maximum(np.abs(GRID), np.abs(ref))))).max())
        print(f"{ACT_NAMES[act]}: worst |emu - ref| / (2^-24 max(1, |x|, |ref|)) = {worst:.2f}")
        assert worst <= 3.5 and abs(worst - K_TABLE[act]) <= 0.011, (act, worst)
        assert ACT_K >= 2 * worst + 1.1


@pytest.mark.parametrize("mode", SWEEP_MODES)
@pytest.mark.parametrize("act", range(8), ids=ACT_NAMES)
def test_restatement_is_inside_the_bound(act, mode):
    z32, z = mode_z((19, 19), 128, mode)
    bad, ratio = act_sweep_bad(store16(act_f32_emu(z32, act)), z, act)
    print(f"{ACT_NAMES[act]} {mode}: worst |emu - ref| / bound = {float(ratio.max()):.3f}")
    assert not bad.any(), (act, mode, int(bad.sum()), z[bad][:8])
    bad32, _ = act_sweep_bad(act_f32_emu(z32, act), z, act, store16=False)
    assert not bad32.any(), (act, mode, "fp32 store", int(bad32.sum()), z[bad32][:8])


def test_fp32_points_are_inside_the_bound():
    for act in range(8):
        bad, _ = act_sweep_bad(act_f32_emu(F32_POINTS, act), F32_POINTS, act, store16=False)
        assert not bad.any(), (act, F32_POINTS[bad])


# ---------------------------------------------------------------------------------------------------------------- planted mistakes
@pytest.mark.parametrize("defect", ACT_DEFECTS)
def test_planted_mistake_leaves_the_bound(defect):
    act = DEFECT_ACT[defect]
    if defect == "selu_scale_1.0507":   # see the module docstring: its floor holds over the modes of the two board cases
        n = 0
        for C in (128, 192):
            for mode in SWEEP_MODES:
                z32, z = mode_z((19, 19), C, mode)
                n += int(act_sweep_bad(store16(act_f32_emu(z32, act, defect)), z, act)[0].sum())
    else:
        n = int(act_sweep_bad(store16(act_f32_emu(GRID, act, defect)), GRID, act)[0].sum())
    print(f"{defect}: {n} values outside the bound")
    assert n >= 100, (defect, n)


@pytest.mark.parametrize("act", range(2, 8), ids=ACT_NAMES[2:])
def test_store_rounding_toward_zero_leaves_the_bound(act):
    n = int(act_sweep_bad(f16_store_toward_zero(act_f32_emu(GRID, act)), GRID, act)[0].sum())
    print(f"{ACT_NAMES[act]}: a store toward zero puts {n} values outside the bound")
    assert n >= 100, (act, n)
    # and identity / ReLU see it through equality on the sums off the grid
    z32, z = mode_z((19, 19), 128, "sweep")
    assert int(act_sweep_bad(f16_store_toward_zero(act_f32_emu(z32, 1)), z, 1)[0].sum()) >= 100


def test_f16_store_toward_zero():
    a = np.array([1.0, 1.0 + 2.0 ** -11, 1.0 + 2.0 ** -10 - 2.0 ** -20, -1.0 - 2.0 ** -11 - 2.0 ** -20, 70000.0, -70000.0, 2.0 ** -25 * 1.5, 0.0], np.float32)
    assert f16_store_toward_zero(a).tolist() == [1.0, 1.0, 1.0, -1.0, 65504.0, -65504.0, 0.0, 0.0]


def test_the_old_bound_passes_the_planted_mistakes():
    """4e-3 * max|y| on N(0, 1) fp16 pre-activations, as test_gpu_layers.py and its kin hold the six activations"""
    x = np.random.default_rng(5).standard_normal(92416).astype(np.float16).astype(np.float32)
    seen = set()
    for defect in ACT_DEFECTS:
        act = DEFECT_ACT[defect]
        ref = act_f64(x, act)
        err = float(np.abs(store16(act_f32_emu(x, act, defect)) - ref).max()) / (4e-3 * float(np.abs(ref).max()))
        print(f"{defect}: {err:.2f} x the old bound")
        if err > 1.0:
            seen.add(defect)
    assert seen == LOOSE_SEES, seen
    for act in range(2, 8):
        ref = act_f64(x, act)
        assert float(np.abs(f16_store_toward_zero(act_f32_emu(x, act)) - ref).max()) <= 4e-3 * float(np.abs(ref).max())


# ---------------------------------------------------------------------------------------------------------------- overflow
def test_overflow_predicate():
    z = np.array([65504.0, 62000.0, 63000.0, 70000.0, -70000.0, 100.0])
    for act in (3, 6):
        ref = act_f64(z, act)
        good = store16(ref)
        assert np.isinf(good).sum() >= 1
        assert not act_sweep_bad(good, z, act)[0].any(), (act, good)
        sat = np.clip(good, -65504.0, 65504.0)
        bad = act_sweep_bad(sat, z, act)[0]
        assert np.array_equal(bad, np.isinf(good)), "a saturating store: 65504 where inf is due"
        early = np.where(np.abs(ref) > 60000, np.copysign(np.inf, ref), good)
        assert act_sweep_bad(early, z, act)[0].sum() >= 1, "inf where the reference is far inside the range"
        nan = good.copy()
        nan[-1] = np.nan
        assert act_sweep_bad(nan, z, act)[0][-1]
        flipped = np.where(np.isinf(good), -good, good)
        assert np.array_equal(act_sweep_bad(flipped, z, act)[0], np.isinf(good))
    for act in (0, 1):   # exactly where float16(z) overflows
        good = store16(act_f64(z, act))
        assert not act_sweep_bad(good, z, act)[0].any()
        assert act_sweep_bad(np.clip(good, -65504.0, 65504.0), z, act)[0].sum() == np.isinf(good).sum() > 0
    # the tie itself: 65520 stores as inf, 65519.99 as 65504; the bound lets a transcendental kernel land on either side of it
    edge = np.array([65519.0, 65521.0])
    assert store16(edge).tolist() == [65504.0, np.inf]
    b = act_bound(edge, edge)
    assert np.all(edge + b >= 65520) and np.all(edge - b < 65520)
