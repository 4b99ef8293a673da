"""Run-level parity of the persistent tower launch (conv_tower.h) at both widths, through the tap sayuri_hip_test_tower_run:
a run of 1..8 board convolutions as ONE launch -- the body conv_tower_kernel<4> / <2>, the seam tower_seam.py writes between two
layers (table stepping, rebuilt entry registers, the weight hand-over) and the generated epilogue (Mish / ReLU / identity, with
and without residual, every board size's branch), which no single-layer tap reaches.  The tap hands back EVERY layer's output,
so each layer l of a run is checked on its own, for every sample:

  bits     against sayuri_hip_test_conv -- conv_board_kernel, the compiled epilogue, one launch -- on the run's OWN layer l-1
           output with the same residual and activation (the SE layer: sayuri_hip_test_conv_se's per-layer kernel): the generated
           epilogue, the seam and the hand-over promise to change no bit;
  float64  against a float64 direct convolution of the run's own layer l-1 output, at the single-layer bounds of the project:
           4e-3 * max|ref| for a plain layer (test_gpu_layers.py), SX_TOL * max(1, max|ref|) with se_unit_f64 for the SE layer
           (test_gpu_smallops.py).  Step by step every layer stays at the single-layer bound, and a layer that read stale input
           across the seam is still caught: its reference is computed from what the previous layer really wrote.

Every output must be finite (every layer's buffer starts as fp16 NaN), and the tap's report (layers, layers in row order = on
the generated epilogue, hand-over links) must equal what the case is about.  Inputs are fp16-exact draws: N(0, 1) activations,
weights N(0, 1 / fan-in), bias 0.1 N(0, 1), the SE unit's FCs as sx_fc draws them.  tests/test_tower_run_reference_cpu.py pins
the float64 convolution used here to conv_ref and shows that the can-fail case's bar is no artefact of the draw.

Measured on an MI355X (every bits check exact, every report as expected), worst float64 error / tolerance: generated epilogue
on boards 2..19 0.11 (Mish) and 0.12 (ReLU, identity) at both widths; several workgroups 0.12; compiled epilogue in a run 0.11;
index tables 0.11; input convolution first 0.11; SE layer in a run 0.14 (C = 256, se = 64), 0.15 (C = 128, se = 32), 0.12 (from
L2); eight layers 0.09.  The can-fail case lands 130 .. 263 x the tolerance away."""
import functools

import numpy as np
import pytest

from sayuri_amd import _lib
from test_gpu_layers import BOARD_CASES, KIND_BOARD, act_np
from test_gpu_smallops import SE_FROM_L2, SE_STAGED, SX_TOL, r16, se_unit_f64, sx_fc

pytestmark = pytest.mark.gpu

PLAIN_TOL = 4e-3  # times max|ref|: test_gpu_layers.py, fp16
MAX_BOARD = 19



def conv3x3_taps_f64(x, w64, bias, b):
    """float64 direct 3x3 convolution of one sample as nine matrix products: x [C][b*b], w64 [K][C][3][3] float64 -> [K][b*b]"""
    C, K = x.shape[0], w64.shape[0]
    xp = np.zeros((C, b + 2, b + 2), np.float64)
    xp[:, 1:-1, 1:-1] = np.asarray(x, np.float64).reshape(C, b, b)
    y = np.zeros((K, b * b), np.float64)
    for dy in range(3):
        for dx in range(3):
            y += np.matmul(np.ascontiguousarray(w64[:, :, dy, dx]), np.ascontiguousarray(xp[:, dy:dy + b, dx:dx + b]).reshape(C, b * b))
    return y + np.asarray(bias, np.float64)[:, None]


class RunSpec:
    """One run: boards, width, the first layer's input channels, per layer activation and residual source (-1 none, 0 the run's
    input, k the output of layer k-1), the SE layer (index, SE width) or None."""

    def __init__(self, bsz, C, acts, res_from, cin0=None, se=None, seed=0):
        self.bsz, self.C, self.acts, self.res_from = tuple(bsz), C, tuple(acts), tuple(res_from)
        self.cin0 = C if cin0 is None else cin0
        self.se, self.seed = se, seed
        self.L = len(self.acts)
        assert len(self.res_from) == self.L

    def __repr__(self):
        return f"run(C={self.C} cin0={self.cin0} boards={list(self.bsz)} acts={self.acts} res={self.res_from} se={self.se})"


class RunDraw:
    """x of every sample, w and bias of every layer (x, w fp16-exact), the SE unit's FCs"""

    def __init__(self, bsz, C, cin0, L, se, seed):
        rng = np.random.default_rng([seed, C, cin0, L] + list(bsz))
        self.xs = [r16(rng.standard_normal((cin0, b * b)).astype(np.float32), True) for b in bsz]
        self.ws = []
        for l in range(L):
            cin = cin0 if l == 0 else C
            self.ws.append(r16((rng.standard_normal((C, cin, 3, 3)) / np.sqrt(9 * cin)).astype(np.float32), True))
        self.bias = (rng.standard_normal((L, C)) * 0.1).astype(np.float32)
        self.fc = sx_fc(seed, C, se[1]) if se else None
        self._w64 = {}

    def w64(self, l):
        if l not in self._w64:
            self._w64[l] = self.ws[l].astype(np.float64)
        return self._w64[l]


@functools.lru_cache(maxsize=8)
def _draw(bsz, C, cin0, L, se, seed):
    return RunDraw(bsz, C, cin0, L, se, seed)


def run_draw(spec):
    return _draw(spec.bsz, spec.C, spec.cin0, spec.L, spec.se, spec.seed)


def split(flat, bsz, C):
    outs, off = [], 0
    for b in bsz:
        outs.append(flat[off:off + C * b * b].reshape(C, b * b))
        off += C * b * b
    return outs


def tower_run(spec, D, chain=1):
    """one launch of the tap -> (return code, outs[layer][sample] = [C][b*b], (layers, row-order layers, links), SE form)"""
    lib = _lib.hip()
    n, C, L = len(spec.bsz), spec.C, spec.L
    per = C * sum(b * b for b in spec.bsz)
    y = np.full(L * per, np.nan, np.float32)
    xcat = np.concatenate([x.ravel() for x in D.xs])
    wcat = np.concatenate([w.ravel() for w in D.ws])
    fc = [np.ascontiguousarray(a) for a in D.fc] if spec.se else [None] * 4
    rc = lib.sayuri_hip_test_tower_run(0, n, _lib.ip(np.asarray(spec.bsz, np.int32)), MAX_BOARD, C, spec.cin0, L, _lib.ip(np.asarray(spec.acts, np.int32)),
                                       _lib.ip(np.asarray(spec.res_from, np.int32)), _lib.fp(wcat), _lib.fp(np.ascontiguousarray(D.bias)),
                                       spec.se[0] if spec.se else -1, spec.se[1] if spec.se else 0, *[_lib.fp(a) if a is not None else None for a in fc],
                                       chain, _lib.fp(xcat), _lib.fp(y))
    report = np.zeros(3, np.int32)
    assert lib.sayuri_hip_test_last_tower_run(_lib.ip(report)) == 0
    form = lib.sayuri_hip_test_last_se_form()
    return rc, [split(y[l * per:(l + 1) * per], spec.bsz, C) for l in range(L)], tuple(int(v) for v in report), form


def layer_io(spec, D, outs, l):
    """what layer l of the run read: (input of every sample, residual of every sample or None)"""
    xin = D.xs if l == 0 else outs[l - 1]
    r = spec.res_from[l]
    return xin, None if r < 0 else (D.xs if r == 0 else outs[r - 1])


def per_layer_kernel(spec, D, l, xin, res):
    """layer l as ONE launch of the per-layer board kernel (compiled epilogue) on the same input -> [sample] = [C][b*b]"""
    lib = _lib.hip()
    n, C = len(spec.bsz), spec.C
    cin = spec.cin0 if l == 0 else C
    xcat = np.concatenate([np.ascontiguousarray(x, np.float32).ravel() for x in xin])
    rcat = np.concatenate([np.ascontiguousarray(r, np.float32).ravel() for r in res]) if res is not None else None
    y = np.full(C * sum(b * b for b in spec.bsz), np.nan, np.float32)
    bs_arr = np.asarray(spec.bsz, np.int32)
    w, bias = np.ascontiguousarray(D.ws[l]), np.ascontiguousarray(D.bias[l])
    if spec.se and spec.se[0] == l:
        rc = lib.sayuri_hip_test_conv_se(0, n, _lib.ip(bs_arr), MAX_BOARD, C, spec.se[1], spec.acts[l], 0, _lib.fp(xcat), _lib.fp(w), _lib.fp(bias),
                                         _lib.fp(rcat) if res is not None else None, *[_lib.fp(np.ascontiguousarray(a)) for a in D.fc], _lib.fp(y))
        assert rc == 0, (spec, l, rc, lib.sayuri_hip_last_error().decode())
    else:
        rc = lib.sayuri_hip_test_conv(0, 1, n, _lib.ip(bs_arr), MAX_BOARD, cin, C, 3, 0, spec.acts[l], 0, _lib.fp(xcat), _lib.fp(w), _lib.fp(bias),
                                      _lib.fp(rcat) if res is not None else None, _lib.fp(y))
        assert rc == 0, (spec, l, rc, lib.sayuri_hip_last_error().decode())
        assert lib.sayuri_hip_test_last_conv_kind() == KIND_BOARD, "the bits reference is the board kernel"
    return split(y, spec.bsz, C)


def layer_f64(spec, D, l, i, x, res, w64=None):
    """(float64 reference of layer l on sample i given its input x and residual, its tolerance)"""
    b = spec.bsz[i]
    conv = conv3x3_taps_f64(x, D.w64(l) if w64 is None else w64, D.bias[l], b)
    if spec.se and spec.se[0] == l:
        ref = se_unit_f64(conv, res, *D.fc, b, spec.acts[l])
        return ref, SX_TOL * max(1.0, float(np.abs(ref).max()))
    ref = act_np(conv + (np.asarray(res, np.float64) if res is not None else 0.0), spec.acts[l])
    return ref, PLAIN_TOL * float(np.abs(ref).max())


def check_run(spec, row_order, links, chain=1, bits=True):
    """The run through the tap: the report as expected, every layer's output finite, bit-equal to the per-layer kernel and within
    the single-layer float64 bound, for every sample.  -> (outs, worst error / tolerance)"""
    lib = _lib.hip()
    D = run_draw(spec)
    rc, outs, report, form = tower_run(spec, D, chain)
    assert rc == 0, (spec, rc, lib.sayuri_hip_last_error().decode())
    assert report == (spec.L, row_order, links), (spec, chain, report)
    if spec.se:
        assert form == (SE_FROM_L2 if (spec.C, spec.se[1]) == (256, 128) else SE_STAGED), (spec, form)
    worst = 0.0
    for l in range(spec.L):
        for i in range(len(spec.bsz)):
            assert np.isfinite(outs[l][i]).all(), (spec, "layer", l, "sample", i, "an output nobody wrote")
    for l in range(spec.L):
        xin, res = layer_io(spec, D, outs, l)
        if bits:
            exp = per_layer_kernel(spec, D, l, xin, res)
            for i in range(len(spec.bsz)):
                bad = int((exp[i] != outs[l][i]).sum())
                assert bad == 0, (spec, "layer", l, "sample", i, bad, "values differ from the per-layer kernel's",
                                  float(np.abs(exp[i] - outs[l][i]).max()))
        for i in range(len(spec.bsz)):
            ref, tol = layer_f64(spec, D, l, i, xin[i], res[i] if res is not None else None)
            err = float(np.abs(outs[l][i] - ref).max())
            worst = max(worst, err / tol)
            assert err <= tol, (spec, "layer", l, "sample", i, err, tol)
    print(f"tower {spec} chain={chain} report={report}: worst error {worst:.2f} x tol")
    return outs, worst


def check_unchained(spec, row_order, outs):
    """the same run without the weight hand-over: no link, the same bits"""
    rc, plain, report, _ = tower_run(spec, run_draw(spec), chain=0)
    assert rc == 0 and report == (spec.L, row_order, 0), (spec, rc, report)
    for l in range(spec.L):
        for i in range(len(spec.bsz)):
            assert np.array_equal(plain[l][i], outs[l][i], equal_nan=True), (spec, "layer", l, "sample", i, "the hand-over changed bits")


BLOCK3 = (-1, 0, 1)  # layer 1 adds the run's input, layer 2 the output of layer 0: one hand-over (0 -> 1), one refused (1 has a residual)


@pytest.mark.parametrize("act", [5, 1, 0], ids=["mish", "relu", "identity"])
@pytest.mark.parametrize("C", [256, 128])
def test_generated_epilogue_on_every_board_size(C, act):
    """Cases a and e: one board of every size 2..19 -- every rung of the generated epilogue's wait ladder, nj == 0 for the second
    wave column of 2x2..4x4, residual pieces in LDS and in registers --, three layers with and without residual, at both widths
    and the three activations the generated text covers; with and without the weight hand-over."""
    worst = 0.0
    for b in range(2, 20):
        spec = RunSpec([b], C, (act,) * 3, BLOCK3, seed=100 + b)
        outs, w = check_run(spec, row_order=3, links=1)
        check_unchained(spec, 3, outs)
        worst = max(worst, w)
    print(f"generated epilogue C={C} act={act}, boards 2..19: worst error {worst:.2f} x tol")


@pytest.mark.parametrize("bsz", [(19,) * 3, (14,) * 3], ids=["19x3", "14x3"])
@pytest.mark.parametrize("C", [256, 128])
def test_computed_table_entries_with_several_workgroups(C, bsz):
    """Case b: several one-sample tiles -- the generated epilogue's sample offset is workgroup id x slot stride."""
    check_run(RunSpec(bsz, C, (5,) * 3, BLOCK3, seed=200), row_order=3, links=1)


@pytest.mark.parametrize("act", [2, 3, 4, 6, 7])
@pytest.mark.parametrize("C", [256, 128])
def test_compiled_epilogue_inside_a_run(C, act):
    """Case c: the activations the generated epilogue does not cover keep the compiled one, also inside a run."""
    check_run(RunSpec((19, 19), C, (act,) * 3, BLOCK3, seed=300 + act), row_order=0, links=1)


SHARED_TILES = [(13,) * 5, (9,) * 9, (7,) * 13, (2, 2, 2), tuple(BOARD_CASES[5][0])]


@pytest.mark.parametrize("bsz", SHARED_TILES, ids=["13x5", "9x9", "7x13", "2x3", "mixed"])
@pytest.mark.parametrize("C", [256, 128])
def test_index_tables_inside_a_run(C, bsz):
    """Case c: several samples per tile and a mixed batch read the index tables and take the compiled epilogue (Mish too)."""
    check_run(RunSpec(bsz, C, (5,) * 3, BLOCK3, seed=400), row_order=0, links=1)


@pytest.mark.parametrize("cin0", [43, 96])
@pytest.mark.parametrize("C", [256, 128])
def test_input_convolution_as_first_layer(C, cin0):
    """Cases d and e: the input convolution (43 planes: two chunks; 96: three) as a run's first layer, then a residual block on its
    output.  No hand-over out of layer 0 (another weight geometry, an odd chunk count), one from layer 1 to layer 2."""
    spec = RunSpec((19, 19), C, (5,) * 3, (-1, -1, 1), cin0=cin0, seed=500)
    outs, _ = check_run(spec, row_order=3, links=1)
    check_unchained(spec, 3, outs)


@pytest.mark.parametrize("bsz", [(19, 19), (9,)], ids=["19x2", "9"])
@pytest.mark.parametrize("C,se", [(256, 64), (128, 32), (256, 128)], ids=["C256se64", "C128se32", "C256se128-from-L2"])
def test_seam_after_an_se_stage(C, se, bsz):
    """Case f: plain layer, SE layer with the run's input as residual, plain layer -- the hand-over INTO the SE layer, the seam
    behind its stage (staged FC images and FCs from L2), at both widths."""
    check_run(RunSpec(bsz, C, (5,) * 3, (-1, 0, -1), se=(1, se), seed=600), row_order=3, links=1)


RES_BLOCKS8 = (-1, 0, -1, 2, -1, 4, -1, 6)  # four residual blocks: conv, conv + the block's input


def blocks_spec(C):
    return RunSpec((19, 19), C, (5,) * 8, RES_BLOCKS8, seed=700)


@pytest.mark.parametrize("C", [256, 128])
def test_eight_layers_as_four_residual_blocks(C):
    """Case g: the table stepped over eight elements, a hand-over into every block's second layer and none out of it."""
    check_run(blocks_spec(C), row_order=8, links=4)


SWAP = {2: 3, 3: 2}
CAN_FAIL_BAR = 4.0  # times the tolerance: the bar of the project's can-fail cases


@pytest.mark.parametrize("C", [256, 128])
def test_run_test_can_fail(C):
    """Case g's float64 check with the reference given layer 2's and layer 3's weights swapped: both layers land >= 4x the
    tolerance away on every sample (tests/test_tower_run_reference_cpu.py: the two references differ by far more on this draw)."""
    spec = blocks_spec(C)
    D = run_draw(spec)
    rc, outs, report, _ = tower_run(spec, D)
    assert rc == 0 and report == (8, 8, 4), (rc, report)
    for l, other in SWAP.items():
        xin, res = layer_io(spec, D, outs, l)
        for i in range(len(spec.bsz)):
            ref, tol = layer_f64(spec, D, l, i, xin[i], res[i] if res is not None else None, w64=D.w64(other))
            ratio = float(np.abs(outs[l][i] - ref).max()) / tol
            print(f"tower C={C} layer {l} against the reference with layer {other}'s weights, sample {i}: {ratio:.0f} x tol")
            assert ratio >= CAN_FAIL_BAR, (C, l, i, ratio)


def test_tap_refuses_what_it_cannot_run():
    """bad arguments are refused with a message before anything is launched, and the report says nothing ran"""
    lib = _lib.hip()
    for spec, what in ((RunSpec((19,), 192, (5,), (-1,)), "128 or 256"), (RunSpec((19,), 128, (5,) * 9, (-1,) * 9), "1 to 8"),
                       (RunSpec((19,), 128, (5, 5), (-1, 2)), "earlier layer"), (RunSpec((19,), 128, (5, 5), (-1, 0), cin0=43), "channels"),
                       (RunSpec((9, 9), 128, (5,), (-1,), se=(0, 32)), "one sample per tile")):
        rc, _, report, _ = tower_run(spec, RunDraw(spec.bsz, spec.C, spec.cin0, spec.L, spec.se, 1))
        assert rc == -1 and what in lib.sayuri_hip_last_error().decode(), (spec, rc, lib.sayuri_hip_last_error().decode())
        assert report == (0, 0, 0)
