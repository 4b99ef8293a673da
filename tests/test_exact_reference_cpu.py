"""What makes tests/test_gpu_exact.py trustworthy, checked without a GPU.

1. The reference.  exact_conv / exact_layer give conv_ref's result (_kref.py: the float64 restatement of the oracle's
   direct convolution) EXACTLY on small integer cases: k = 1, 3, 5, 7, depthwise, mixed boards down to 2x2, both residual orders.
2. The regime.  Every case of every case list the GPU module runs is inside the exact regime (exact_layer's own assertions: A * 2^q
   < 2^24, |S| < 65504).  In the unit tier every expected output is its own fp16 rounding; every wide-tier case has >= 1 % outputs
   that are no fp16 value, exact ties and non-ties both present, >= 0.5 % non-ties at the 256- and 384-channel shapes.  The tower
   runs are followed layer by layer as a correct kernel would write them; their last layer rounds too.  The can-fail cases'
   prediction (predicted_change) is the difference of the two references.  These are conditions on the inputs: a draw that
   misses them is changed, not the condition.
3. Mutants of the reference, compared with assert_exact's predicate: (a) one product dropped at a corner pixel differs at exactly
   one output of a unit-tier case; (b) an fp16 store that rounds toward zero, (c) the convolution rounded to fp16 before the
   residual is added (on the cases that have a residual: without one it is no mutant), (d) every 32-channel chunk's partial sum
   rounded to fp16 before it is accumulated -- each differs on every wide-tier case.
4. The gap.  On run_case's own N(0, 1) draw at ([19] * 2, 256 -> 256, seed 512, identity, residual) the mutants (a), (b) and (c) of the
   float64 reference stay inside run_case's bound 4e-3 * max|ref|: what the tolerance tests cannot see."""
import numpy as np
import pytest

from _cases import (BOARD_CASES, BOARD_EXACT, CAN_FAIL, CAN_FAIL_TAPS, CAN_FAIL_TOWER, case_id, DEPTHWISE_EXACT, draw_conv, EPILOGUES, exact_draw,
                    exact_run_layer, GENERIC_EXACT, layer_io, layer_reference, SE_EXACT, se_identity_fc, se_reference, SeCase, SPLIT_EXACT,
                    split_strips, SX_EXACT, TIERS, TOWER_CASES, tower_draw, tower_spec, TOWER_WIDTHS, WIDE_CHANNELS)
from _kref import act_np, assert_exact, assert_localised, conv_ref, exact_conv, exact_diff, exact_layer, mutated, predicted_change, quantum_bits


def f16(v):
    return np.asarray(v, np.float64).astype(np.float16).astype(np.float64)


def rtz16(v):
    """an fp16 store that rounds toward zero"""
    v = np.asarray(v, np.float64)
    h = v.astype(np.float16)
    h = np.where(np.abs(h.astype(np.float64)) > np.abs(v), np.nextafter(h, np.float16(0)), h)
    return h.astype(np.float64)


def rounding_shares(vs):
    """of the exact values `vs`: (share that is no fp16 value, share that is an exact tie between two, share that is neither)"""
    v = np.concatenate([np.asarray(a, np.float64).ravel() for a in vs])
    h = f16(v)
    inexact = h != v
    ulp = 2.0 ** (np.floor(np.log2(np.abs(v[inexact]))) - 10)
    ties = int(np.count_nonzero(2.0 * np.abs(v[inexact] - h[inexact]) == ulp))
    return inexact.mean(), ties / v.size, (int(inexact.sum()) - ties) / v.size


# ---------------------------------------------------------------------------------------------------- 1. the reference
@pytest.mark.parametrize("k,depthwise", [(1, False), (3, False), (5, True), (7, True), (3, True), (5, False), (7, False)])
@pytest.mark.parametrize("post", [False, True], ids=["res-then-act", "act-then-res"])
def test_exact_layer_is_conv_ref(k, depthwise, post):
    bsz, cin, cout = (2, 5, 3, 9, 2), 37, 24
    for tier in TIERS:
        xs, w, bias, res = exact_draw(tier, bsz, cin, cout, k, depthwise, 3)
        for act in (0, 1):
            for r in (res, None):
                exp = conv_ref([x.astype(np.float64) for x in xs], list(bsz), w.astype(np.float64), bias.astype(np.float64),
                               [a.astype(np.float64) for a in r] if r else None, k, depthwise, act, post)
                for i, b in enumerate(bsz):
                    got = exact_layer(xs[i], w, bias, r[i] if r else None, b, k, depthwise, act, post=post, store=None)
                    assert np.array_equal(got, exp[i]), (tier, k, depthwise, act, post, i)
                    stored = exact_layer(xs[i], w, bias, r[i] if r else None, b, k, depthwise, act, post=post)
                    assert np.array_equal(stored, exp[i].astype(np.float16).astype(np.float32))


def test_exact_layer_refuses_what_is_outside_the_regime():
    xs, w, bias, res = exact_draw("wide", (5,), 32, 8, 3, False, 1)
    with pytest.raises(AssertionError):
        exact_layer(xs[0] * 4096, w, bias, None, 5, 3, False, 0)  # A >= 2^24
    with pytest.raises(AssertionError):
        exact_layer(xs[0] * 64, w, bias, None, 5, 3, False, 0)  # an output past 65504
    with pytest.raises(AssertionError):
        exact_layer(xs[0] + 2.0 ** -20, w * 256, bias, None, 5, 3, False, 0)  # sums of multiples of 2^-20 that fp32 cannot hold
    with pytest.raises(AssertionError):
        exact_layer(xs[0], w, bias, None, 5, 3, False, 5)  # Mish is no exact function
    exact_layer(xs[0] / 4096, w, bias, res[0], 5, 3, False, 1)  # multiples of 2^-12 of this size are inside


def test_the_predicate_sees_one_value_and_takes_minus_zero_for_zero():
    exp = [np.zeros((3, 4), np.float32), np.ones((3, 9), np.float32)]
    got = [e.copy() for e in exp]
    got[0][1, 2] = -0.0
    assert exact_diff(got, exp) == []
    assert_exact(got, exp, "equal")
    got[1][2, 7] = np.nextafter(np.float32(1), np.float32(2))
    assert [b[:3] for b in exact_diff(got, exp)] == [(1, 2, 7)]
    with pytest.raises(AssertionError):
        assert_exact(got, exp, "one ulp")
    got[1][2, 7] = np.nan
    with pytest.raises(AssertionError):
        assert_exact(got, exp, "not written")


# ---------------------------------------------------------------------------------------------------- 2. the regime
def exact_values(c):
    """the exact outputs of a Case or SeCase before the store, float64, one array per sample (exact_layer asserts the regime)"""
    return se_reference(c, store=None)[2] if isinstance(c, SeCase) else layer_reference(c, store=None)[1]


LAYER_LISTS = {"generic": GENERIC_EXACT, "board": BOARD_EXACT, "split": SPLIT_EXACT, "depthwise": DEPTHWISE_EXACT, "se": SE_EXACT,
               "sx": SX_EXACT, "can-fail": [f[1] for f in CAN_FAIL]}


@pytest.mark.parametrize("name", list(LAYER_LISTS))
def test_every_layer_case_is_inside_the_exact_regime(name):
    cases = LAYER_LISTS[name]
    assert cases and len(set(cases)) == len(cases)
    for c in cases:
        vs = exact_values(c)
        if c.tier == "unit":
            assert all(np.array_equal(f16(v), v) for v in vs), (c, "a unit-tier output is no fp16 value")
            continue
        inexact, ties, others = rounding_shares(vs)
        channels = c.C if isinstance(c, SeCase) else c.cin
        print(f"{case_id(c)}: max|y| {max(float(np.abs(v).max()) for v in vs):.0f}, no fp16 value {100 * inexact:.1f} %, ties {100 * ties:.1f} %, "
              f"non-ties {100 * others:.1f} %")
        assert inexact >= 0.01 and ties > 0 and others > 0, (c, inexact, ties, others)
        assert channels in WIDE_CHANNELS and others >= 0.005, (c, others)


def test_the_lists_hold_what_the_module_says():
    """every shape, tier, type and epilogue the module's docstrings speak of is in the lists"""
    assert {(c.fp16, c.k) for c in GENERIC_EXACT} == {(False, 1), (True, 1), (False, 3), (True, 3)}
    assert {(c.act, c.with_res) for c in GENERIC_EXACT} == set(EPILOGUES) and len(GENERIC_EXACT) == 5 * 2 * 4
    assert {(c.bsz, c.cin, c.cout) for c in BOARD_EXACT} == {(tuple(b), ci, co) for b, ci, co in BOARD_CASES}
    assert {(c.cin, c.cout) for c in BOARD_EXACT if c.tier == "wide"} == {(256, 256), (384, 384)}
    assert sum(c.tier == "wide" for c in BOARD_EXACT) == 4 * 2
    assert {(c.act, c.with_res) for c in BOARD_EXACT + SPLIT_EXACT + SE_EXACT + SX_EXACT} == {(0, False), (1, True)}
    assert all(split_strips(c.bsz) == (1, 2, max(c.bsz), 0) for c in SPLIT_EXACT)
    assert {(c.k, c.fp16, c.cout, c.post, c.act) for c in DEPTHWISE_EXACT} == {(k, f, C, p, a) for k in (3, 5, 7) for f in (False, True) for C in (48, 40)
                                                                                 for p in (False, True) for a in (0, 1)}
    assert all(c.bsz == (19, 9, 2, 3, 5) and c.with_res == c.post for c in DEPTHWISE_EXACT)
    assert {(c.C, c.se) for c in SE_EXACT} == {(256, 64), (128, 32), (256, 128)} and {c.bsz for c in SE_EXACT} == {(19, 19), (14,), (9,)}
    assert {(c.C, c.se) for c in SX_EXACT} == {(384, 96), (512, 64)} and (10,) * 4 + (11,) * 3 + (12,) * 3 in {c.bsz for c in SX_EXACT}
    assert {tc.bsz for tc in TOWER_CASES} == {(19, 19, 19), (13,) * 5, (2, 3, 5, 19)}
    assert any(tc.first43 for tc in TOWER_CASES) and any(tc.skip for tc in TOWER_CASES)
    for _, c, (k, cc) in CAN_FAIL:
        assert (c.tier, c.act, c.with_res) == ("unit", 0, False) and cc == c.cin - 1 and cc // 32 == (c.cin - 1) // 32 and k < c.cout


def follow_run(tc, C):
    """the run as a kernel that keeps its contract writes it -> (spec, draw, outs[layer][sample], the exact layers' values before the store)"""
    spec, D = tower_spec(tc, C), tower_draw(tc, C)
    outs, values = [], {}
    for l in range(spec.L):
        if l in tc.skip:  # the compiled epilogue's function in float64, stored as fp16
            xin, res = layer_io(spec, D, outs, l)
            outs.append([f16(act_np(exact_conv(xin[i], D.ws[l], b, 3, False)[0] + D.bias[l][:, None].astype(np.float64) +
                                      (res[i] if res is not None else 0.0), spec.acts[l])).astype(np.float32) for i, b in enumerate(spec.bsz)])
            continue
        values[l] = exact_run_layer(spec, D, outs, l, store=None)
        outs.append([v.astype(np.float16).astype(np.float32) for v in values[l]])
    return spec, D, outs, values


@pytest.mark.parametrize("tc", TOWER_CASES, ids=lambda tc: tc.name)
@pytest.mark.parametrize("C", TOWER_WIDTHS)
def test_every_tower_run_is_inside_the_exact_regime(C, tc):
    spec, D, outs, values = follow_run(tc, C)
    assert set(values) == set(range(spec.L)) - set(tc.skip)
    assert all(spec.acts[l] in (0, 1) for l in values) and all(spec.acts[l] not in (0, 1, 5) for l in tc.skip)
    last = values[spec.L - 1]
    inexact, ties, others = rounding_shares(last)
    print(f"tower {tc.name} C={C}: layer {spec.L - 1} max|y| {max(float(np.abs(v).max()) for v in last):.1f}, no fp16 value {100 * inexact:.1f} % "
          f"(ties {100 * ties:.1f} %, non-ties {100 * others:.1f} %), operands in units of 2^-{quantum_bits(*outs[spec.L - 2])}")
    assert inexact >= 0.01 and ties > 0 and others > 0, (tc, C, "the last layer of a run rounds on its own")
    if tc.skip:
        assert quantum_bits(*outs[tc.skip[0]]) > 0, "the layer behind the compiled epilogue reads no fractions: the case shows nothing"


@pytest.mark.parametrize("name,c,kc", CAN_FAIL, ids=[f[0] for f in CAN_FAIL])
def test_the_can_fail_prediction_is_the_difference_of_the_references(name, c, kc):
    (xs, w, bias, _), exp = layer_reference(c)
    for kr, kcol in CAN_FAIL_TAPS:
        w2 = mutated(w, *kc, kr, kcol)
        delta = predicted_change(xs, c.bsz, c.cout, *kc, kr, kcol)
        moved = [exact_layer(xs[i], w2, bias, None, b, 3, False, 0) for i, b in enumerate(c.bsz)]  # inside the regime, too
        assert assert_localised(moved, exp, delta, name) > 0
        with pytest.raises(AssertionError):
            assert_localised(exp, exp, delta, name)  # a kernel that lost the product
        elsewhere = predicted_change(xs, c.bsz, c.cout, kc[0], kc[1] - 1, kr, kcol)
        with pytest.raises(AssertionError):
            assert_localised(moved, exp, elsewhere, name)  # ... or read a neighbouring channel


@pytest.mark.parametrize("C", TOWER_WIDTHS)
def test_the_tower_can_fail_case_is_inside_the_exact_regime(C):
    tc = CAN_FAIL_TOWER
    spec, D = tower_spec(tc, C), tower_draw(tc, C)
    exp = exact_run_layer(spec, D, [], 0)
    assert all(np.array_equal(f16(e), e) for e in exp)
    for kr, kcol in CAN_FAIL_TAPS:
        w2 = mutated(D.ws[0], C - 1, C - 1, kr, kcol)
        moved = [exact_layer(D.xs[i], w2, D.bias[0], None, b, 3, False, 0) for i, b in enumerate(spec.bsz)]
        assert assert_localised(moved, exp, predicted_change(D.xs, spec.bsz, C, C - 1, C - 1, kr, kcol), "tower") > 0


# ---------------------------------------------------------------------------------------------------- 3. mutants of the reference
def operands(c):
    """(xs, w, bias with an SE unit's beta in it, res | None, act, [exact_conv of every sample]) of a Case or SeCase"""
    if isinstance(c, SeCase):
        (xs, w, bias, res), conv = draw_conv(c.tier, c.bsz, c.C, c.C, 3, False, c.seed)
        bias = bias + se_identity_fc(c.C, c.se, c.seed)[1]
    else:
        (xs, w, bias, res), conv = draw_conv(c.tier, c.bsz, c.cin, c.cout, c.k, c.depthwise, c.seed)
    return xs, w, bias.astype(np.float64), res if c.with_res else None, c.act, conv


def store_toward_zero(conv, r, act):
    return rtz16(act_np(conv + r, act))


def conv_rounded_before_residual(conv, r, act):
    return f16(act_np(f16(conv) + r, act))


WIDE_CASES = [c for cases in LAYER_LISTS.values() for c in cases if c.tier == "wide"]


@pytest.mark.parametrize("c", WIDE_CASES, ids=case_id)
def test_rounding_mutants_differ_on_every_wide_case(c):
    xs, w, bias, res, act, convs = operands(c)
    correct, toward_zero, early, chunked = [], [], [], []
    for i, b in enumerate(c.bsz):
        r = res[i].astype(np.float64) if res else 0.0
        conv = convs[i][0] + bias[:, None]
        correct.append(f16(act_np(conv + r, act)))
        toward_zero.append(store_toward_zero(conv, r, act))
        early.append(conv_rounded_before_residual(conv, r, act))
        parts = sum(f16(exact_conv(xs[i][c0:c0 + 32], w[:, c0:c0 + 32], b, 3, False)[0]) for c0 in range(0, w.shape[1], 32))
        chunked.append(f16(act_np(parts + bias[:, None] + r, act)))
    n = sum(a.size for a in correct)
    seen = {name: len(exact_diff(m, correct)) for name, m in (("store toward zero", toward_zero), ("conv rounded before the residual", early),
                                                                 ("fp16 partial sums per chunk", chunked))}
    print(f"{case_id(c)}: of {n} outputs differ " + ", ".join(f"{k}: {v}" for k, v in seen.items()))
    assert seen["store toward zero"] > 0 and seen["fp16 partial sums per chunk"] > 0, (c, seen)
    if res:
        assert seen["conv rounded before the residual"] > 0, (c, seen)
    else:
        assert seen["conv rounded before the residual"] == 0  # without a residual it is the contract itself


@pytest.mark.parametrize("c", [BOARD_EXACT[0], GENERIC_EXACT[1], SPLIT_EXACT[2], SE_EXACT[0]], ids=case_id)
def test_one_dropped_corner_product_differs_at_exactly_one_output(c):
    assert c.tier == "unit"
    xs, w, bias, res, act, _ = operands(c)
    i, b = len(c.bsz) - 1, c.bsz[-1]
    exp = exact_values(c)
    for pixel, (kr, kcol) in ((0, (1, 1)), (b * b - 1, (0, 0)), (b - 1, (2, 0))):  # three corners, a tap that is on the board there
        src = pixel + (kr - 1) * b + (kcol - 1)
        prod = w[:, :, kr, kcol] * xs[i][:, src][None, :]
        ks, cs = np.nonzero((prod != 0) & ((exp[i][:, pixel] > 0) | (act == 0))[:, None])  # (under ReLU: an output that is not cut off)
        k, ch = int(ks[-1]), int(cs[-1])
        mutant = [e.copy() for e in exp]
        pre = exp[i][k, pixel] if act == 0 or exp[i][k, pixel] > 0 else None
        mutant[i][k, pixel] = act_np(np.float64(pre - prod[k, ch]), act)
        bad = exact_diff([f16(m) for m in mutant], [f16(e) for e in exp])
        assert [x[:3] for x in bad] == [(i, k, pixel)], (c, pixel, bad)


# ---------------------------------------------------------------------------------------------------- 4. the gap
def test_the_tolerance_tests_cannot_see_these_mutants():
    """run_case(True, [19] * 2, 256, 256, 3, act=0, with_res=True, seed=512) as test_gpu_layers.py draws it"""
    rng = np.random.default_rng(512)
    bsz, C = [19, 19], 256
    xs = [rng.standard_normal((C, b * b)).astype(np.float32) for b in bsz]
    w = (rng.standard_normal((C, C, 3, 3)) / np.sqrt(9 * C)).astype(np.float32)
    bias = (rng.standard_normal(C) * 0.1).astype(np.float32).astype(np.float64)
    res = [rng.standard_normal((C, b * b)).astype(np.float32) for b in bsz]
    xs, w, res = [f16(x) for x in xs], f16(w), [f16(r) for r in res]
    conv = [exact_conv(x, w, b, 3, False)[0] + bias[:, None] for x, b in zip(xs, bsz)]
    ref = [c + r for c, r in zip(conv, res)]
    bound = 4e-3 * max(float(np.abs(r).max()) for r in ref)
    worst = lambda ms: max(float(np.abs(m - r).max()) for m, r in zip(ms, ref))
    products = np.abs(w[:, :, 1, 1] * xs[0][:, 0][None, :])  # every product the centre tap adds at the corner pixel 0 of sample 0
    k, ch = 7, C - 1
    rows = {"a correct round-to-nearest store": worst([f16(r) for r in ref]),
            f"(a) the product w[{k}][{ch}][1][1] x[{ch}][0] dropped": float(products[k, ch]),
            "(b) a store that rounds toward zero": worst([rtz16(r) for r in ref]),
            "(c) the convolution rounded to fp16 before the residual": worst([f16(f16(c) + r) for c, r in zip(conv, res)])}
    print(f"scale {bound / 4e-3:.3f}, bound {bound:.5f}; median corner product {float(np.median(products)):.5f}, "
          f"{100 * float((products <= bound).mean()):.1f} % of them inside the bound")
    for name, err in rows.items():
        print(f"  {name}: {err:.5f} = {err / bound:.2f} x bound")
        assert err <= bound, (name, err, bound)
    assert rows["(a) the product w[7][255][1][1] x[255][0] dropped"] > 0
    assert (products <= bound).mean() >= 0.5
    assert rows["(b) a store that rounds toward zero"] > rows["a correct round-to-nearest store"]
