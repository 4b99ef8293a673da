"""The yardsticks of the pooled-statistics cases of tests/test_gpu_smallops.py (conv_board_se_kernel and the tower's SE stage,
se_pool / se_fc / se_scale, head_tail_kernel, head_board_kernel), checked without a GPU.

1. head_tail_f64, the float64 restatement of the head tail the GPU tests compare with, against the oracle's so_tap_head_tail
   (the C restatement of blas_forward_pipe.cc:496-580 that the whole-network goldens pin): boards 2 / 9 / 13 / 14 / 19, all
   eight activations, two channel pairs, 2e-5 * scale -- the project's fp32 bound.  (se_unit_f64 is pinned the same way by
   tests/test_sx_reference_cpu.py.)
2. The inputs make the GPU tests sensitive.  On the very generators they use (se_inputs / head_inputs, spread and probe draws)
   every way the pooling could be subtly wrong moves the float64 reference by at least 4x the tolerance of the GPU test that
   uses the generator -- on every sample the defect touches.  Each defect is held to that bar on the draw that is made for it
   (SE_SEEN_BY / HEAD_SEEN_BY: a mean of O(1) shows a wrong factor or divisor, a spike at a boundary pixel shows a pixel lost
   or counted twice, a negative level shows a maximum that saw a 0); the ratio on the other draw is printed too.
   Named exemptions, where the reference itself makes the defect no defect: at 14x14 the scaled-mean factor is 0, so dropping the
   term changes nothing; a divisor that equals the board's npix is the right one; a wave column without pixels (boards of at most
   16 pixels) has no partial to lose.
3. An emulation of the staged kernel's rounding -- the folded squeeze image W_mean + (bs-14)/10 W_scaled, the excite image and the
   output in fp16, everything else float64 -- stays within half the GPU tolerance of the reference on every case, so a correct
   kernel keeps as much again for its accumulation order."""
import numpy as np
import pytest

from _oracle import PortNet
from sayuri_amd._lib import fp
from _cases import (HEAD_BOARDS, HEAD_DIMS, head_inputs, HEAD_PAIRS, HEAD_SEED, se_case_batches, SE_CASE_IDS, SE_CASES, se_inputs, SE_LAYERS, SE_SEED,
                    SE_UNIT_BATCHES, se_unit_x, SX_TOL)
from _kref import head_pool_f64, head_ratio, head_tail_f64, se_apply_f64, se_gate_f64, se_pool_f64

BAR = 4.0


@pytest.mark.parametrize("act", range(8))
def test_head_tail_f64_matches_the_oracle(act):
    o = PortNet.lib()
    d = HEAD_DIMS
    for draw in ("spread", "probe"):
        for Cp, Cv in ((32, 32), (24, 48)):
            H = head_inputs(draw, 950 + act, (2, 9, 13, 14, 19), Cp, Cv, 0, False)
            for i, bs in enumerate(H.bsz):
                S = bs * bs
                pc, vc = H.planes(i, act)
                got = head_tail_f64(pc, vc, H.ws, bs, act)
                e_prob, e_pass = np.zeros((d["prob_ch"], S), np.float32), np.zeros(d["pass_outs"], np.float32)
                e_own, e_misc = np.zeros(S, np.float32), np.zeros(d["misc_outs"], np.float32)
                o.so_tap_head_tail(bs, Cp, Cv, d["prob_ch"], d["pass_outs"], d["misc_outs"], act, fp(pc.copy()), fp(vc), *[fp(w) for w in H.ws],
                                   fp(e_prob), fp(e_pass), fp(e_own), fp(e_misc))
                for name, g, e in zip(("prob", "pass", "own", "misc"), got, (e_prob, e_pass, e_own, e_misc)):
                    scale = max(1.0, float(np.abs(e).max()))
                    err = float(np.abs(g - e).max())
                    assert np.isfinite(g).all()
                    assert err <= 2e-5 * scale, (draw, Cp, Cv, bs, act, name, err, scale)


# ------------------------------------------------------------------------------------------------ defects of a pooled vector
def pooled(x, bs, third, keep=None, twice=None, div=None, size=None, scaled=True, zero_cell=False):
    """(mean, scaled mean, third) of x [C][npix] with a defect: only the pixels `keep` pooled; pixel `twice` summed twice; the sum
    divided by `div`; the factors of board size `size`; no scaled-mean term; a maximum that also saw a 0.
    third: "max" | "moment" (the value head's mean * ((bs-14)^2 / 100 - 0.1))"""
    x = np.asarray(x, np.float64)
    npix = bs * bs
    xs = x if keep is None else x[:, keep]
    s = xs.sum(axis=1) + (x[:, twice] if twice is not None else 0.0)
    mean = s / float(npix if div is None else div)
    d = (bs if size is None else size) - 14.0
    if third == "moment":
        t = mean * (d * d / 100.0 - 0.1)
    else:
        t = xs.max(axis=1, initial=-5000.0)
        if zero_cell:
            t = np.maximum(t, 0.0)
    return np.concatenate([mean, mean * (d / 10.0) if scaled else 0.0 * mean, t])


def pixel_defects(bs, third):
    """name -> keyword arguments of pooled(), or None where the reference makes it no defect (the named exemptions)"""
    npix = bs * bs
    every = np.arange(npix)
    last_tile = 16 * ((npix - 1) // 16)
    nj0 = ((npix + 15) // 16 + 1) // 2  # column tiles of the first wave column (conv_board.h)
    D = {
        "a: factor of size bs-1": dict(size=bs - 1),
        "a: factor of size bs+1": dict(size=bs + 1),
        "b: scaled-mean term dropped": dict(scaled=False) if bs != 14 else None,
        "d: last pixel not pooled": dict(keep=every[:-1]),
        "e: pixel 0 counted twice": dict(twice=0),
        "f: last column tile missing": dict(keep=every[:last_tile]),
        "f: first pixel of the last column tile missing": dict(keep=every[every != last_tile]),
        "h: first wave column's partial missing": dict(keep=every[16 * nj0:]),
        "h: second wave column's partial missing": dict(keep=every[:16 * nj0]) if npix > 16 * nj0 else None,
    }
    for div in (361, 384, 512):
        D[f"c: sum divided by {div}"] = dict(div=div) if div != npix else None
    if third == "max":
        D["g: a maximum that sees a 0"] = dict(zero_cell=True)
    return D


# ------------------------------------------------------------------------------------------------ the SE unit
# the draw that is held to the bar for each defect (by the defect's letter)
SE_SEEN_BY = {"a": "probe", "b": "probe", "c": "probe", "h": "spread", "i": "spread", "j": "spread", "d": "probe", "e": "probe", "f": "probe", "g": "probe"}


def se_sensitivity(draw, C, se, act, bsz, rel_tol, x_of=lambda T, i: T.conv(i)):
    """-> [(defect, sample, board size, ratio)] of every defect of the unit on one batch of the GPU cases; rel_tol: that GPU test's
    tolerance relative to max(1, |ref|max); x_of(T, i): the unit's input there"""
    T, fc = se_inputs(draw, SE_SEED, bsz, C, se)
    n = len(bsz)
    xs = [x_of(T, i) for i in range(n)]
    pools = [se_pool_f64(xs[i], T.bsz[i]) for i in range(n)]
    gates = [se_gate_f64(pools[i], *fc, act) for i in range(n)]
    ref = [se_apply_f64(xs[i], T.rs[i], *gates[i], act) for i in range(n)]
    out = []
    for i, bs in enumerate(T.bsz):
        tol = rel_tol * max(1.0, float(np.abs(ref[i]).max()))
        x, nxt = xs[i], (i + 1) % n

        def from_pool(pool):
            return se_apply_f64(x, T.rs[i], *se_gate_f64(pool, *fc, act), act)

        variants = {}
        for name, kw in pixel_defects(bs, "max").items():
            variants[name] = None if kw is None else from_pool(pooled(x, bs, "max", **kw))
        if n > 1 and not (bsz[nxt] == bs and draw == "probe"):  # (probe draws: two boards of one size pool alike by construction)
            variants["i: the next sample's gate"] = se_apply_f64(x, T.rs[i], *gates[nxt], act)
            pool = pools[i].copy()
            pool[2 * C:] = pools[nxt][2 * C:]
            variants["i: the next sample's maximum"] = from_pool(pool)
        variants["j: beta dropped"] = se_apply_f64(x, T.rs[i], gates[i][0], 0.0 * gates[i][1], act)
        for name, v in variants.items():
            out.append((name, i, bs, None if v is None else float(np.abs(v - ref[i]).max()) / tol))
    return out


def report(tag, draw, seen_by, rows):
    """print every ratio; -> the (defect, sample) pairs below the bar among the defects this draw is held to"""
    low = []
    for name, i, bs, ratio in rows:
        held = seen_by[name[0]] == draw
        if ratio is None:
            print(f"{tag} {draw} sample {i} ({bs}x{bs}) {name}: exempt, no defect on this board")
            continue
        print(f"{tag} {draw} sample {i} ({bs}x{bs}) {name}: {ratio:.1f} x tol{'' if held else '  (not held to the bar on this draw)'}")
        if held and not ratio >= BAR:
            low.append((name, i, bs, round(ratio, 2)))
    return low


@pytest.mark.parametrize("draw", ["spread", "probe"])
@pytest.mark.parametrize("C,se,act", SE_CASES, ids=SE_CASE_IDS)
def test_se_inputs_expose_wrong_pooled_statistics(C, se, act, draw):
    """The cases of test_conv_se_pooled_statistics, batch by batch, at its 3e-3 * max(1, |ref|max)."""
    low = []
    with np.errstate(over="ignore"):  # a pool of no pixels at all has the maximum -5000
        for bsz in se_case_batches(C, se, act):
            low += report(f"C={C} se={se} act={act} boards={list(bsz)}", draw, SE_SEEN_BY, se_sensitivity(draw, C, se, act, bsz, SX_TOL))
    assert not low, low


@pytest.mark.parametrize("draw", ["spread", "probe"])
@pytest.mark.parametrize("act", [5, 0])
def test_se_unit_kernel_inputs_expose_wrong_pooled_statistics(act, draw):
    """The cases of test_se_unit_kernels_pooled_statistics at the fp16 engine's 2e-3 (the fp32 engine's 2e-5 is 100x as sharp on
    inputs that differ by the fp16 rounding of x alone)."""
    low = []
    with np.errstate(over="ignore"):
        for C, se in SE_LAYERS:
            for bsz in SE_UNIT_BATCHES:
                low += report(f"SE kernels C={C} se={se} act={act} boards={list(bsz)}", draw, SE_SEEN_BY,
                              se_sensitivity(draw, C, se, act, bsz, 2e-3, lambda T, i: se_unit_x(T, i, True)))
    assert not low, low


def test_mutated_weight_cases_are_far_enough_in_float64():
    """test_conv_se_test_can_fail / test_se_unit_kernels_test_can_fail ask a correct kernel, on w1 without its scaled-mean columns,
    for >= 4x the tolerance from the unmutated reference: in float64 the distance is >= 5x, which leaves the kernel its own 1x."""
    cases = [(256, 64, (19, 18, 17, 16, 15, 14), SX_TOL, None), (256, 128, (19, 18, 17, 16, 15, 14), SX_TOL, None), (128, 32, (19, 16, 14), 2e-3, True)]
    for C, se, bsz, rel_tol, fp16 in cases:
        x_of = (lambda T, i: T.conv(i)) if fp16 is None else (lambda T, i: se_unit_x(T, i, True))
        for name, i, bs, ratio in se_sensitivity("spread", C, se, 5, bsz, rel_tol, x_of):
            if name[0] == "b" and ratio is not None:
                print(f"C={C} se={se} boards={list(bsz)} sample {i} ({bs}x{bs}) {name}: {ratio:.1f} x tol")
                assert ratio >= 5.0, (C, se, bsz, i, ratio)


def test_every_defect_is_held_to_the_bar_somewhere():
    assert set(SE_SEEN_BY) == set("abcdefghij")
    assert {k[0] for k in pixel_defects(19, "max")} | {"i", "j"} == set(SE_SEEN_BY)


def staged_emulation(T, fc, i, act):
    """the staged kernel's rounding: folded squeeze image, excite image and output in fp16, the rest float64"""
    w1, b1, w2, b2 = fc
    C, bs = T.C, T.bsz[i]
    h = lambda a: np.asarray(a, np.float32).astype(np.float16).astype(np.float64)
    sc = np.float32((np.float32(bs) - np.float32(14.0)) / np.float32(10.0))
    folded = h(w1[:, :C] + sc * w1[:, C:2 * C])  # fp32 arithmetic, as make_se_images does it
    x = T.conv(i)
    pool = se_pool_f64(x, bs)
    w1e = np.concatenate([folded, np.zeros((w1.shape[0], C)), h(w1[:, 2 * C:])], axis=1)
    gamma, beta = se_gate_f64(pool, w1e, b1, h(w2), b2, act)
    return h(se_apply_f64(x, T.rs[i], gamma, beta, act))


STAGED_CASES = [c for c in SE_CASES if c[:2] in SE_LAYERS]


@pytest.mark.parametrize("draw", ["spread", "probe"])
@pytest.mark.parametrize("C,se,act", STAGED_CASES, ids=[f"C{c}se{s}act{a}" for c, s, a in STAGED_CASES])
def test_se_inputs_leave_room_for_the_fp16_images(C, se, act, draw):
    for bsz in se_case_batches(C, se, act):
        T, fc = se_inputs(draw, SE_SEED, bsz, C, se)
        for i, bs in enumerate(T.bsz):
            ref = se_apply_f64(T.conv(i), T.rs[i], *se_gate_f64(se_pool_f64(T.conv(i), bs), *fc, act), act)
            d = float(np.abs(staged_emulation(T, fc, i, act) - ref).max()) / (SX_TOL * max(1.0, float(np.abs(ref).max())))
            print(f"C={C} se={se} act={act} {draw} boards={list(bsz)} sample {i} ({bs}x{bs}): emulated rounding {d:.2f} x tol")
            assert d <= 0.5, (draw, C, se, act, bsz, i, d)


# ------------------------------------------------------------------------------------------------ the heads
HEAD_SEEN_BY = {"a": "spread", "b": "spread", "c": "spread", "t": "spread", "s": "spread", "n": "spread", "d": "probe", "e": "probe", "g": "probe"}
HEAD_POLICY = ("a", "b", "c", "d", "e", "g")  # (b) is what test_head_kernels_test_can_fail passes the kernels
HEAD_VALUE = ("a", "c", "d", "e")


def head_sensitivity(H, act, tol):
    """-> [(defect, sample, board size, ratio)]: the largest deviation over the four outputs in units of each one's tolerance"""
    n = len(H.bsz)
    out = []
    for i, bs in enumerate(H.bsz):
        pc, vc = H.planes(i, act)
        ref = H.reference(i, act)
        variants = {}
        for name, kw in pixel_defects(bs, "max").items():
            if name[0] in HEAD_POLICY:
                variants[name + " (policy)"] = None if kw is None else H.reference(i, act, ppool=pooled(pc, bs, "max", **kw))
        for name, kw in pixel_defects(bs, "moment").items():
            if name[0] in HEAD_VALUE:
                variants[name + " (value)"] = None if kw is None else H.reference(i, act, vpool=pooled(vc, bs, "moment", **kw))
        variants["t: the value pooling's third term is the maximum"] = H.reference(i, act, vpool=pooled(vc, bs, "max"))
        variants["t: the policy pooling's third term is the value head's"] = H.reference(i, act, ppool=pooled(pc, bs, "moment"))
        variants["s: spatial bias not added to the policy planes"] = H.reference(i, act, spatial_bias=False)
        nxt = (i + 1) % n
        pn, vn = H.planes(nxt, act)
        variants["n: the next sample's policy pool"] = H.reference(i, act, ppool=head_pool_f64(pn, H.bsz[nxt], False))
        variants["n: the next sample's value pool"] = H.reference(i, act, vpool=head_pool_f64(vn, H.bsz[nxt], True))
        for name, v in variants.items():
            out.append((name, i, bs, None if v is None else head_ratio(v, ref, ref, tol)))
    return out


@pytest.mark.parametrize("act", [5, 0])
@pytest.mark.parametrize("Cp,Cv", HEAD_PAIRS, ids=[f"Cp{p}Cv{v}" for p, v in HEAD_PAIRS])
@pytest.mark.parametrize("C,tol", [(0, 2e-4), (128, 2e-3), (256, 2e-3)], ids=["head_tail", "head_board-C128", "head_board-C256"])
@pytest.mark.parametrize("draw", ["spread", "probe"])
def test_head_inputs_expose_wrong_pooled_statistics(draw, C, tol, Cp, Cv, act):
    """head_tail_kernel's generator (the planes themselves) at its 2e-4, head_board_kernel's (a trunk behind the head
    convolutions) at its 2e-3, each relative to max(1, |ref|max) of the output it shows in."""
    H = head_inputs(draw, HEAD_SEED, HEAD_BOARDS, Cp, Cv, C, True)
    low = report(f"C={C} Cp={Cp} Cv={Cv} act={act}", draw, HEAD_SEEN_BY, head_sensitivity(H, act, tol))
    assert not low, low
