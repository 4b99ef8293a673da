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
a case outside it cannot run.  Values are compared with ==, so that -0 equals +0.

Two draws.  unit: x in [-2, 2], w in {-1, 0, 1}, bias in [-8, 8], residual in [-16, 16] -- every output is itself an fp16 value,
nothing rounds: the tier for "every product of every tap, channel and pixel lands in the right place".  wide: x in [-16, 16], w
in [-8, 8] -- outputs run past 2048 and 4096, so the store rounds (exact ties and non-ties): the tier for the store's rounding
and for any fp16 intermediate.  The wide tier runs where it rounds enough to mean something (tests/test_exact_reference_cpu.py
holds every wide case to >= 1 % outputs that are no fp16 value, ties and non-ties both present): the 256 / 384 / 512-channel
layers.  At the generic kernel's own shapes (32 .. 96 channels, 1x1) and in the depthwise kernel it hardly rounds, so they get
the unit tier; the generic fp16 kernel's store is reached at 256 -> 256 and 384 -> 384 by the SAYURI_CONV=v0 child.

Every case asserts the kernel family (sayuri_hip_test_last_conv_kind), the SE form or the tower's report it is about.  The
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
"""
import collections
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

from sayuri_amd import _lib
from test_gpu_layers import BOARD_CASES, CASES, KIND_BOARD, act_np
from test_gpu_latency import KIND_SPLIT, LAYER_SHAPES
from test_gpu_smallops import KIND_BOARD_SX, SE_FROM_L2, SE_STAGED
from test_gpu_tower_run import BLOCK3, RunSpec, layer_io, split, tower_run

pytestmark = pytest.mark.gpu

KIND_GENERIC, KIND_GLDS, KIND_DEPTHWISE = 0, 1, 3
MAX_BOARD = 19
TIERS = {"unit": (2, 1), "wide": (16, 8)}  # |x|, |w| at most
BIAS_MAX, RES_MAX = 8, 16
# the kernel family a child process of test_exact_cases_on_the_fallback_kernels expects of the fp16 3x3 board shapes
VARIANT_KIND = os.environ.get("SAYURI_EXACT_VARIANT_KIND")


# ------------------------------------------------------------------------------------------------ draws and the reference
def exact_draw(tier, bsz, cin, cout, k, depthwise, seed):
    """-> (xs [sample] = [cin][b*b], w [cout][cin | 1][k][k], bias [cout], res [sample] = [cout][b*b]), float32 integers of `tier`"""
    xa, wa = TIERS[tier]
    rng = np.random.default_rng([seed, xa, cin, cout, k, int(depthwise)] + list(bsz))
    xc = cout if depthwise else cin
    xs = [rng.integers(-xa, xa + 1, (xc, b * b)).astype(np.float32) for b in bsz]
    w = rng.integers(-wa, wa + 1, (cout, 1 if depthwise else cin, k, k)).astype(np.float32)
    bias = rng.integers(-BIAS_MAX, BIAS_MAX + 1, cout).astype(np.float32)
    res = [rng.integers(-RES_MAX, RES_MAX + 1, (cout, b * b)).astype(np.float32) for b in bsz]
    return xs, w, bias, res


def quantum_bits(*arrays):
    """the smallest q with every value of `arrays` a multiple of 2^-q (0: integers)"""
    for q in range(25):
        if all(a is None or np.array_equal(np.rint(np.asarray(a, np.float64) * 2.0 ** q), np.asarray(a, np.float64) * 2.0 ** q) for a in arrays):
            return q
    raise AssertionError("an operand is no multiple of 2^-24")


def exact_conv(x, w, bs, k, depthwise):
    """The k x k convolution of one sample as k*k matrix products in float64, which holds these sums exactly: x [C][bs*bs], w
    [K][C | 1][k][k] -> (sum w x, sum |w x|), each [K][bs*bs]"""
    x, w64 = np.asarray(x, np.float64), np.asarray(w, np.float64)
    C, K, pad = x.shape[0], w64.shape[0], k // 2
    xp = np.zeros((C, bs + 2 * pad, bs + 2 * pad), np.float64)
    xp[:, pad:pad + bs, pad:pad + bs] = x.reshape(C, bs, bs)
    wa = np.abs(w64)
    S, A = np.zeros((K, bs * bs), np.float64), np.zeros((K, bs * bs), np.float64)
    for dy in range(k):
        for dx in range(k):
            patch = np.ascontiguousarray(xp[:, dy:dy + bs, dx:dx + bs]).reshape(C, bs * bs)
            if depthwise:
                S += w64[:, 0, dy, dx][:, None] * patch
                A += wa[:, 0, dy, dx][:, None] * np.abs(patch)
            else:
                S += np.matmul(np.ascontiguousarray(w64[:, :, dy, dx]), patch)
                A += np.matmul(np.ascontiguousarray(wa[:, :, dy, dx]), np.abs(patch))
    return S, A


def exact_layer(x, w, bias, res, bs, k, depthwise, act, post=False, beta=None, store=np.float16, conv=None):
    """The one correct output of a layer on operands of the exact regime: x [C][bs*bs], w, bias [K] or None, res [K][bs*bs] or None
    -> float16(act(conv + bias + beta + res)) as float32, [K][bs*bs]; post: act(conv + bias) + res (the depthwise kernel's order);
    beta: a second per-channel addend (an SE unit's); store=np.float32: the fp32 kernels' store; store=None: the exact value
    before the store, float64; conv: exact_conv(x, w, bs, k, depthwise) where the caller has it already.  Asserts the regime: act
    is the identity or ReLU, w / bias / beta are integers, A * 2^q < 2^24, |S| < 65504."""
    assert act in (0, 1), "only the identity and ReLU are exact functions"
    assert quantum_bits(w, bias, beta) == 0, "weights and biases are integers"
    q = quantum_bits(x, res)
    S, A = exact_conv(x, w, bs, k, depthwise) if conv is None else conv
    for addend in (bias, beta):
        if addend is not None:
            S = S + np.asarray(addend, np.float64)[:, None]
            A = A + np.abs(np.asarray(addend, np.float64))[:, None]
    r = np.asarray(res, np.float64) if res is not None else 0.0
    A = A + np.abs(r)
    assert float(A.max()) * 2.0 ** q < 2.0 ** 24, ("outside the exact regime: sum |w x| + |bias| + |res| =", float(A.max()), "in units of 2^-%d" % q)
    v = act_np(S, act) + r if post else act_np(S + r, act)
    assert max(float(np.abs(S + r).max()), float(np.abs(v).max())) < 65504.0, "an output leaves the fp16 range"
    return v if store is None else v.astype(store).astype(np.float32)


def exact_diff(got, exp):
    """the predicate of assert_exact: [(sample, channel, pixel, got, exp)] of every value that differs (== on values: -0 equals +0)"""
    bad = []
    for i, (g, e) in enumerate(zip(got, exp)):
        for c, p in zip(*np.nonzero(np.asarray(g) != np.asarray(e))):
            bad.append((i, int(c), int(p), float(g[c, p]), float(e[c, p])))
    return bad


def assert_exact(got, exp, what):
    """every sample's output finite and equal to the reference, value for value"""
    assert len(got) == len(exp), what
    for i, g in enumerate(got):
        assert g.shape == exp[i].shape and np.isfinite(g).all(), (what, "sample", i, "an output nobody wrote, or a non-finite one")
    bad = exact_diff(got, exp)
    assert not bad, (what, len(bad), "values differ; the first (sample, channel, pixel, got, exp):", bad[:8])


# ------------------------------------------------------------------------------------------------ the cases
Case = collections.namedtuple("Case", "tier fp16 bsz cin cout k depthwise act with_res post seed")
SeCase = collections.namedtuple("SeCase", "tier bsz C se act with_res seed")
EPILOGUES = ((0, False), (1, True), (1, False), (0, True))  # activation, with residual


def case_id(c):
    if isinstance(c, SeCase):
        return f"{c.tier}-C{c.C}se{c.se}n{len(c.bsz)}b{min(c.bsz)}act{c.act}res{int(c.with_res)}"
    return (f"{c.tier}-{'fp16' if c.fp16 else 'fp32'}-{c.cin}x{c.cout}k{c.k}{'dw' if c.depthwise else ''}n{len(c.bsz)}b{min(c.bsz)}"
            f"act{c.act}res{int(c.with_res)}{'post' if c.post else ''}")


# the generic kernel's own shapes (kind 0 in fp32 and in fp16: no board or LDS-DMA kernel has these channel tiles, or k = 1)
GENERIC_SHAPES = [CASES[2], CASES[3], CASES[8], CASES[7], CASES[10]]
assert [s[1:] for s in GENERIC_SHAPES] == [(32, 64, 3), (43, 96, 3), (48, 72, 1), (256, 32, 1), (32, 32, 3)]
GENERIC_EXACT = [Case("unit", fp16, tuple(bsz), cin, cout, k, False, act, with_res, False, 10 + j)
                 for j, (bsz, cin, cout, k) in enumerate(GENERIC_SHAPES) for fp16 in (False, True) for act, with_res in EPILOGUES]

WIDE_CHANNELS = (256, 384, 512)  # where the wide draw rounds enough (tests/test_exact_reference_cpu.py)
BOARD_EXACT = [Case(tier, True, tuple(bsz), cin, cout, 3, False, act, with_res, False, 30 + j)
               for j, (bsz, cin, cout) in enumerate(BOARD_CASES) for tier in ("unit", "wide") if tier == "unit" or (cin in WIDE_CHANNELS and cin == cout)
               for act, with_res in EPILOGUES[:2]]

SPLIT_SHAPES = [LAYER_SHAPES[5], LAYER_SHAPES[6]]
assert [s[1:] for s in SPLIT_SHAPES] == [(256, 256), (43, 128)]
SPLIT_EXACT = ([Case("unit", True, tuple(bsz), cin, cout, 3, False, act, with_res, False, 50 + j)
                for j, (bsz, cin, cout) in enumerate(SPLIT_SHAPES) for act, with_res in EPILOGUES[:2]] +
               [Case("wide", True, (19,), 256, 256, 3, False, act, with_res, False, 52) for act, with_res in EPILOGUES[:2]])


def split_strips(bsz):
    return (1, 2, max(bsz), 0)


DEPTHWISE_BOARDS = (19, 9, 2, 3, 5)  # the last three are smaller than the 5 x 5 and 7 x 7 kernels
# post_residual = 1: act(conv + bias) + res.  The kernel has no residual in front of the activation (the tap passes none on when
# post_residual = 0), so those cases have no residual.
DEPTHWISE_EXACT = [Case("unit", fp16, DEPTHWISE_BOARDS, 1, C, k, True, act, bool(post), bool(post), 60 + k)
                   for k in (3, 5, 7) for fp16 in (False, True) for C in (48, 40) for post in (0, 1) for act in (0, 1)]

SE_BOARDS = ((19, 19), (14,), (9,))
SE_EXACT = [SeCase(tier, bsz, C, se, act, with_res, 70 + j)
            for j, (C, se) in enumerate(((256, 64), (128, 32), (256, 128))) for bsz in SE_BOARDS
            for tier in ("unit", "wide") if tier == "unit" or C in WIDE_CHANNELS for act, with_res in EPILOGUES[:2]]
SX_BOARDS = SE_BOARDS + ((10,) * 4 + (11,) * 3 + (12,) * 3,)
SX_EXACT = [SeCase(tier, bsz, C, se, act, with_res, 80 + j)
            for j, (C, se) in enumerate(((384, 96), (512, 64))) for bsz in SX_BOARDS for tier in ("unit", "wide") for act, with_res in EPILOGUES[:2]]


@functools.lru_cache(maxsize=2)
def draw_conv(tier, bsz, cin, cout, k, depthwise, seed):
    """(exact_draw, [exact_conv of every sample]): the cases of one shape share the draw and its convolution"""
    draw = exact_draw(tier, bsz, cin, cout, k, depthwise, seed)
    return draw, [exact_conv(draw[0][i], draw[1], b, k, depthwise) for i, b in enumerate(bsz)]


def layer_reference(c, store=np.float16):
    """((xs, w, bias, res | None), [the exact output of every sample]) of a Case"""
    (xs, w, bias, res), conv = draw_conv(c.tier, c.bsz, c.cin, c.cout, c.k, c.depthwise, c.seed)
    res = res if c.with_res else None
    exp = [exact_layer(xs[i], w, bias, res[i] if res else None, b, c.k, c.depthwise, c.act, post=c.post, conv=conv[i],
                       store=store if c.fp16 or store is None else np.float32) for i, b in enumerate(c.bsz)]
    return (xs, w, bias, res), exp


def se_identity_fc(C, se, seed):
    """The SE unit whose gate is the identity: w1 [se][3C] = 0, b1 = 0, w2 [2C][se] = 0, b2 = (+32 for gamma, small integers for beta)"""
    beta = np.random.default_rng([seed, C, se, 99]).integers(-4, 5, C).astype(np.float32)
    fc = (np.zeros((se, 3 * C), np.float32), np.zeros(se, np.float32), np.zeros((2 * C, se), np.float32),
          np.concatenate([np.full(C, 32.0, np.float32), beta]))
    return fc, beta


def se_reference(c, store=np.float16):
    """((xs, w, bias, res | None), fc, [the exact output of every sample]) of an SeCase"""
    (xs, w, bias, res), conv = draw_conv(c.tier, c.bsz, c.C, c.C, 3, False, c.seed)
    res = res if c.with_res else None
    fc, beta = se_identity_fc(c.C, c.se, c.seed)
    exp = [exact_layer(xs[i], w, bias, res[i] if res else None, b, 3, False, c.act, beta=beta, conv=conv[i], store=store) for i, b in enumerate(c.bsz)]
    return (xs, w, bias, res), fc, exp


# ---- tower runs: layer 0 dense unit weights on the unit draw's x, later layers unit weights at a density that keeps three
# layers inside the regime (about 144 non-zero weights per output: |y| grows by ~12 per layer, so layer 2 runs to ~4e4 and
# rounds on its own).  The run around a compiled-epilogue layer is sparse from the start (about 4 weights per output in layers 0
# and 1), so that what HardSwish writes -- multiples of 2^-12 -- stays below 2^12 in sum.
HSWISH = 7
TOWER_BOARDS = ((19, 19, 19), (13,) * 5, (2, 3, 5, 19))
TowerCase = collections.namedtuple("TowerCase", "name bsz acts res_from first43 sparse skip gen")
TOWER_CASES = ([TowerCase(f"{name}-{'x'.join(map(str, sorted(set(bsz))))}", bsz, acts, BLOCK3, False, False, (), 3 if bsz == TOWER_BOARDS[0] else 0)
                for bsz in TOWER_BOARDS for name, acts in (("relu", (1, 1, 1)), ("identity", (0, 0, 0)))] +
               [TowerCase(f"input43-{'x'.join(map(str, sorted(set(bsz))))}", bsz, (1, 0, 1), (-1, -1, 1), True, False, (), 3 if bsz == TOWER_BOARDS[0] else 0)
                for bsz in (TOWER_BOARDS[0], TOWER_BOARDS[2])] +
               [TowerCase(f"hardswish-middle-{'x'.join(map(str, sorted(set(bsz))))}", bsz, (1, HSWISH, 0), BLOCK3, False, True, (1,), 2 if bsz == TOWER_BOARDS[0] else 0)
                for bsz in TOWER_BOARDS[:2]])
TOWER_WIDTHS = (256, 128)


def tower_spec(tc, C):
    return RunSpec(tc.bsz, C, tc.acts, tc.res_from, cin0=43 if tc.first43 else None, seed=90)


class ExactRunDraw:
    """x of every sample, w and bias of every layer, as tower_run takes them"""

    def __init__(self, spec, sparse):
        rng = np.random.default_rng([spec.seed, spec.C, spec.cin0, spec.L, int(sparse)] + list(spec.bsz))
        self.xs = [rng.integers(-2, 3, (spec.cin0, b * b)).astype(np.float32) for b in spec.bsz]
        self.ws = []
        for l in range(spec.L):
            cin = spec.cin0 if l == 0 else spec.C
            density = 1.0 if l == 0 and not sparse else (4.0 if sparse and l < 2 else 144.0) / (9 * cin)
            w = rng.integers(0, 2, (spec.C, cin, 3, 3)) * 2 - 1
            self.ws.append((w * (rng.random(w.shape) < density)).astype(np.float32))
        self.bias = rng.integers(-BIAS_MAX, BIAS_MAX + 1, (spec.L, spec.C)).astype(np.float32)
        self.fc = None


@functools.lru_cache(maxsize=4)
def tower_draw(tc, C):
    return ExactRunDraw(tower_spec(tc, C), tc.sparse)


def exact_run_layer(spec, D, outs, l, store=np.float16):
    """layer l's exact outputs from what layer l - 1 wrote (`outs`) -> [sample]"""
    xin, res = layer_io(spec, D, outs, l)
    return [exact_layer(xin[i], D.ws[l], D.bias[l], res[i] if res is not None else None, b, 3, False, spec.acts[l], store=store)
            for i, b in enumerate(spec.bsz)]


# ---- can-fail: (name, shape ..., the changed weight (k, c), in the last 32-channel chunk -- c = 42 is the last real channel of a
# 43-channel input convolution in front of its padding).  Unit tier, identity, no residual.
CAN_FAIL = [("board", Case("unit", True, (19, 19), 384, 384, 3, False, 0, False, False, 101), (383, 383)),
            ("board-input43", Case("unit", True, (19,) * 4, 43, 256, 3, False, 0, False, False, 102), (255, 42)),
            ("split", Case("unit", True, (13, 9, 9, 19, 13, 9), 43, 128, 3, False, 0, False, False, 103), (64, 42)),
            ("generic", Case("unit", True, (9, 13, 19, 7, 19), 32, 64, 3, False, 0, False, False, 104), (63, 31)),
            ("generic-input43", Case("unit", True, (19,) * 4, 43, 96, 3, False, 0, False, False, 105), (95, 42))]
CAN_FAIL_TAPS = ((1, 1), (0, 2))  # an interior tap and a corner tap
CAN_FAIL_TOWER = TowerCase("one-layer", (19, 19, 19), (0,), (-1,), False, False, (), 1)


def mutated(w, k, c, kr, kc):
    """w with the one entry changed by 1 (still a small integer)"""
    w2 = w.copy()
    w2[k, c, kr, kc] += 1.0
    return w2


def predicted_change(xs, bsz, cout, k, c, kr, kc):
    """what adding 1 to w[k][c][kr][kc] adds to every sample's 3x3 convolution: channel k only, the input channel c shifted by the tap"""
    out = []
    for x, b in zip(xs, bsz):
        xp = np.zeros((b + 2, b + 2), np.float64)
        xp[1:-1, 1:-1] = np.asarray(x[c], np.float64).reshape(b, b)
        d = np.zeros((cout, b * b), np.float64)
        d[k] = xp[kr:kr + b, kc:kc + b].ravel()
        out.append(d)
    return out


def assert_localised(got, exp, delta, what):
    """the real kernel on the changed weight against the UNCHANGED reference: it differs exactly where, and by what, the integer
    arithmetic says"""
    n_pred = sum(int(np.count_nonzero(d)) for d in delta)
    assert n_pred > 0, (what, "the changed weight meets no non-zero input")
    for i, (g, e, d) in enumerate(zip(got, exp, delta)):
        assert np.isfinite(g).all(), (what, "sample", i)
        wrong = np.nonzero((g != e) != (d != 0))
        assert wrong[0].size == 0, (what, "sample", i, wrong[0].size, "outputs differ where none was predicted, or do not where one was; the first (channel, pixel):",
                                    list(zip(*wrong))[:8])
        assert np.array_equal(g.astype(np.float64) - e, d), (what, "sample", i, "an output moved by another amount than the input under the tap")
    return n_pred


# ------------------------------------------------------------------------------------------------ the taps
def cat(arrs):
    return np.concatenate([np.ascontiguousarray(a, np.float32).ravel() for a in arrs])


def tap_conv(c, xs, w, bias, res):
    """one launch of sayuri_hip_test_conv -> ([y of every sample], the kernel family that ran)"""
    lib = _lib.hip()
    y = np.full(sum(c.cout * b * b for b in c.bsz), np.nan, np.float32)
    rc = lib.sayuri_hip_test_conv(0, int(c.fp16), len(c.bsz), _lib.ip(np.asarray(c.bsz, np.int32)), MAX_BOARD, c.cin, c.cout, c.k, int(c.depthwise), c.act,
                                  int(c.post), _lib.fp(cat(xs)), _lib.fp(np.ascontiguousarray(w).ravel()), _lib.fp(bias), _lib.fp(cat(res)) if res else None,
                                  _lib.fp(y))
    assert rc == 0, (c, rc, lib.sayuri_hip_last_error().decode())
    return split(y, c.bsz, c.cout), lib.sayuri_hip_test_last_conv_kind()


def tap_split(c, xs, w, bias, res, strips):
    lib = _lib.hip()
    y = np.full(sum(c.cout * b * b for b in c.bsz), np.nan, np.float32)
    rc = lib.sayuri_hip_test_conv_split(0, len(c.bsz), _lib.ip(np.asarray(c.bsz, np.int32)), MAX_BOARD, c.cin, c.cout, c.act, _lib.fp(cat(xs)),
                                        _lib.fp(np.ascontiguousarray(w).ravel()), _lib.fp(bias), _lib.fp(cat(res)) if res else None, _lib.fp(y), 0, strips)
    assert rc == 0, (c, strips, rc, lib.sayuri_hip_last_error().decode())
    return split(y, c.bsz, c.cout), lib.sayuri_hip_test_last_conv_kind()


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
    lib = _lib.hip()
    bsz = (19, 9, 2)
    fc, beta = se_identity_fc(C, se, 7)
    rng = np.random.default_rng([7, C, se])
    xs = [rng.integers(-200, 201, (C, b * b)).astype(np.float32) for b in bsz]
    rs = [rng.integers(-RES_MAX, RES_MAX + 1, (C, b * b)).astype(np.float32) for b in bsz]
    for act in (0, 1):
        y = np.full(sum(C * b * b for b in bsz), np.nan, np.float32)
        gate = np.full((len(bsz), 2 * C), np.nan, np.float32)
        rc = lib.sayuri_hip_test_se_unit(0, int(fp16), len(bsz), _lib.ip(np.asarray(bsz, np.int32)), MAX_BOARD, C, se, act, _lib.fp(cat(xs)), _lib.fp(cat(rs)),
                                         *[_lib.fp(a) for a in fc], _lib.fp(y), _lib.fp(gate))
        assert rc == 0, lib.sayuri_hip_last_error().decode()
        print(f"se_fc C={C} se={se} {'fp16' if fp16 else 'fp32'} act={act}: gate at gamma = 32 in [{gate[:, :C].min()!r}, {gate[:, :C].max()!r}]")
        assert np.array_equal(gate[:, :C], np.ones((len(bsz), C), np.float32)), "sigmoid(32) is not exactly 1.0f"
        assert np.array_equal(gate[:, C:], np.tile(beta, (len(bsz), 1)))
        exp = [act_np(x.astype(np.float64) + beta[:, None] + r, act).astype(np.float32) for x, r in zip(xs, rs)]
        assert_exact(split(y, bsz, C), exp, ("se unit", C, se, fp16, act))


@pytest.mark.parametrize("via_tower", [0, 1], ids=["per-layer kernel", "tower kernel"])
@pytest.mark.parametrize("c", SE_EXACT, ids=case_id)
def test_convolution_inside_the_se_kernels_exact(c, via_tower):
    """conv_board_se_kernel and the tower's SE stage (staged FC images: C = 256 / se = 64, C = 128 / se = 32; FCs from L2: se = 128)
    behind an identity gate: y = act(conv + bias + beta + res)"""
    lib = _lib.hip()
    (xs, w, bias, res), fc, exp = se_reference(c)
    y = np.full(sum(c.C * b * b for b in c.bsz), np.nan, np.float32)
    rc = lib.sayuri_hip_test_conv_se(0, len(c.bsz), _lib.ip(np.asarray(c.bsz, np.int32)), MAX_BOARD, c.C, c.se, c.act, via_tower, _lib.fp(cat(xs)),
                                     _lib.fp(np.ascontiguousarray(w).ravel()), _lib.fp(bias), _lib.fp(cat(res)) if res else None, *[_lib.fp(a) for a in fc], _lib.fp(y))
    assert rc == 0, (c, via_tower, rc, lib.sayuri_hip_last_error().decode())
    form = lib.sayuri_hip_test_last_se_form()
    assert form == (SE_FROM_L2 if (c.C, c.se) == (256, 128) else SE_STAGED), (c, form)
    assert_exact(split(y, c.bsz, c.C), exp, (c, "via_tower", via_tower))


@pytest.mark.parametrize("c", SX_EXACT, ids=case_id)
def test_convolution_inside_the_split_channel_se_kernel_exact(c):
    """conv_board_sx_kernel on three and four channel tiles per board tile, one to three samples per tile, behind an identity gate"""
    lib = _lib.hip()
    (xs, w, bias, res), fc, exp = se_reference(c)
    y = np.full(sum(c.C * b * b for b in c.bsz), np.nan, np.float32)
    rc = lib.sayuri_hip_test_conv_sx(0, len(c.bsz), _lib.ip(np.asarray(c.bsz, np.int32)), MAX_BOARD, c.C, c.se, c.act, _lib.fp(cat(xs)),
                                     _lib.fp(np.ascontiguousarray(w).ravel()), _lib.fp(bias), _lib.fp(cat(res)) if res else None, *[_lib.fp(a) for a in fc], _lib.fp(y))
    assert rc == 0, (c, rc, lib.sayuri_hip_last_error().decode())
    assert lib.sayuri_hip_test_last_conv_kind() == KIND_BOARD_SX
    assert lib.sayuri_hip_test_last_sx_kts() == c.C // 128
    assert_exact(split(y, c.bsz, c.C), exp, c)


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
    lib = _lib.hip()
    spec, D = tower_spec(tc, C), tower_draw(tc, C)
    rc, outs, report, _ = tower_run(spec, D, chain=1)
    assert rc == 0, (spec, rc, lib.sayuri_hip_last_error().decode())
    assert report == tower_report(tc, spec, 1), (spec, report)
    for l in range(spec.L):
        for i in range(len(spec.bsz)):
            assert np.isfinite(outs[l][i]).all(), (spec, "layer", l, "sample", i, "an output nobody wrote")
    for l in range(spec.L):
        if l not in tc.skip:
            assert_exact(outs[l], exact_run_layer(spec, D, outs, l), (spec, "layer", l))
    rc, plain, report, _ = tower_run(spec, D, chain=0)
    assert rc == 0 and report == tower_report(tc, spec, 0), (spec, rc, report)
    for l in range(spec.L):
        assert_exact(plain[l], outs[l], (spec, "layer", l, "without the weight hand-over"))


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
    import copy
    tc = CAN_FAIL_TOWER
    spec, D = tower_spec(tc, C), tower_draw(tc, C)
    exp = exact_run_layer(spec, D, [], 0)
    for kr, kcol in CAN_FAIL_TAPS:
        M = copy.copy(D)
        M.ws = [mutated(D.ws[0], C - 1, C - 1, kr, kcol)]
        rc, outs, report, _ = tower_run(spec, M, chain=1)
        assert rc == 0 and report == (1, 1, 0), (rc, report)
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
