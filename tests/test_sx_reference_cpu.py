"""The yardstick of the split-channel SE convolution tests (test_gpu_smallops.py test_sx_*), checked without a GPU.

1. se_unit_f64, the float64 restatement of SEUnit::Forward the GPU tests compare with, against the oracle's so_tap_se_unit
   (the C restatement of se_unit.cc:70-128 that the whole-network goldens pin): boards 2 / 9 / 11 / 13 / 19, all eight
   activations, 2e-5 * scale -- the project's fp32 bound.
2. The inputs of those tests make them sensitive: on the very generator they use (sx_trunk / sx_fc), the ways
   conv_board_sx_kernel could be subtly wrong each move the result by at least 4x the GPU tolerance
   (3e-3 * max(1, |ref|max)) -- on every sample the defect touches, not just somewhere."""
import numpy as np
import pytest

from _oracle import PortNet
from sayuri_amd._lib import fp
from _cases import SX_TOL, sx_fc, sx_reference, sx_trunk
from _kref import se_apply_f64, se_gate_f64, se_pool_f64, se_unit_f64


@pytest.mark.parametrize("act", range(8))
def test_se_unit_f64_matches_the_oracle(act):
    o = PortNet.lib()
    rng = np.random.default_rng(900 + act)
    for bs in (2, 9, 11, 13, 19):
        for C, se, with_res in ((96, 24, True), (40, 12, False)):
            S = bs * bs
            x = (rng.standard_normal((C, S)) + rng.standard_normal((C, 1))).astype(np.float32)  # channel means of O(1)
            res = rng.standard_normal((C, S)).astype(np.float32) if with_res else None
            w1 = (rng.standard_normal((se, 3 * C)) / np.sqrt(3 * C)).astype(np.float32)
            b1 = (rng.standard_normal(se) * 0.5).astype(np.float32)
            w2 = (rng.standard_normal((2 * C, se)) / np.sqrt(se)).astype(np.float32)
            b2 = (rng.standard_normal(2 * C) * 0.5).astype(np.float32)
            got = se_unit_f64(x, res, w1, b1, w2, b2, bs, act)
            exp = x.copy()
            o.so_tap_se_unit(bs, C, se, fp(w1), fp(b1), fp(w2), fp(b2), fp(exp), fp(res) if with_res else None, act)
            scale = max(1.0, float(np.abs(exp).max()))
            err = float(np.abs(got - exp).max())
            assert np.isfinite(got).all()
            assert err <= 2e-5 * scale, (bs, C, act, err, scale)


# (C, se, act) of the GPU cases: the standard layer, the activation cases' width, both other channel-tile counts, the SE-width edges
SENSITIVITY_CASES = [(384, 96, 5), (384, 48, 1), (384, 48, 0), (256, 96, 5), (512, 64, 5), (384, 100, 5), (384, 20, 5), (384, 4, 5), (360, 96, 5)]
SENS_BOARDS = (13, 13, 9, 9)  # two samples that share a tile, of each of two sizes


@pytest.mark.parametrize("C,se,act", SENSITIVITY_CASES, ids=[f"C{c}se{s}act{a}" for c, s, a in SENSITIVITY_CASES])
def test_sx_inputs_expose_a_wrong_se_unit(C, se, act):
    T, fc = sx_trunk(31, SENS_BOARDS, C), sx_fc(31, C, se)
    w1, b1, w2, b2 = fc
    n = len(SENS_BOARDS)
    other = {13: 9, 9: 13}
    mate = [1, 0, 3, 2]  # the neighbour in the shared tile
    ref = [sx_reference(T, fc, i, act, True) for i in range(n)]
    tol = [SX_TOL * max(1.0, float(np.abs(r).max())) for r in ref]
    gates = [se_gate_f64(se_pool_f64(T.conv(i), T.bsz[i]), *fc, act) for i in range(n)]

    def from_pool(i, pool):
        return se_apply_f64(T.conv(i), T.rs[i], *se_gate_f64(pool, *fc, act), act)

    def a_other_sizes_mean_factor(i):
        bs, x = T.bsz[i], T.conv(i)
        pool = se_pool_f64(x, bs)
        pool[C:2 * C] = pool[:C] * ((other[bs] - 14.0) / 10.0)
        return from_pool(i, pool)

    def b_other_sizes_pixel_count(i):
        bs, x = T.bsz[i], T.conv(i)
        mean = x.sum(axis=1) / float(other[bs] ** 2)
        return from_pool(i, np.concatenate([mean, mean * ((bs - 14.0) / 10.0), x.max(axis=1)]))

    def c_neighbours_maximum(i):
        pool = se_pool_f64(T.conv(i), T.bsz[i])
        pool[2 * C:] = T.conv(mate[i]).max(axis=1)
        return from_pool(i, pool)

    def d_neighbours_gate(i):
        return se_apply_f64(T.conv(i), T.rs[i], *gates[mate[i]], act)

    def e_an_eighth_not_pooled(i):
        bs, x = T.bsz[i], T.conv(i)
        per = (bs * bs + 7) // 8
        keep = np.ones(bs * bs, bool)
        keep[3 * per:4 * per] = False
        mean = x[:, keep].sum(axis=1) / float(bs * bs)
        return from_pool(i, np.concatenate([mean, mean * ((bs - 14.0) / 10.0), x[:, keep].max(axis=1)]))

    def f_a_siblings_partial_missing(i):
        pool = se_pool_f64(T.conv(i), T.bsz[i])
        c = np.arange(128, min(C, 256))  # channel tile 1
        pool[np.concatenate([c, C + c, 2 * C + c])] = 0.0
        return from_pool(i, pool)

    for variant in (a_other_sizes_mean_factor, b_other_sizes_pixel_count, c_neighbours_maximum, d_neighbours_gate, e_an_eighth_not_pooled,
                    f_a_siblings_partial_missing):
        for i in range(n):
            d = float(np.abs(variant(i) - ref[i]).max())
            print(f"C={C} se={se} act={act} {variant.__name__} sample {i} ({T.bsz[i]}x{T.bsz[i]}): differs by {d:.4f} = {d / tol[i]:.1f} x tol")
            assert d >= 4 * tol[i], (variant.__name__, i, d, tol[i])
