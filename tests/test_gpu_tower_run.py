"""Run-level parity of the persistent tower launch (conv_tower.h) at both widths, through the tower_run tap of _taps.py:
a run of 1..8 board convolutions as ONE launch -- the body conv_tower_kernel<4> / <2>, the seam tower_seam.py writes between two
layers (table stepping, rebuilt entry registers, the weight hand-over) and the generated epilogue (Mish / ReLU / identity, with
and without residual, every board size's branch), which no single-layer tap reaches.  The tap hands back EVERY layer's output,
so each layer l of a run is checked on its own, for every sample:

  bits     against the conv tap -- conv_board_kernel, the compiled epilogue, one launch -- on the run's OWN layer l-1
           output with the same residual and activation (the SE layer: the conv_se tap's per-layer kernel): the generated
           epilogue, the seam and the hand-over promise to change no bit;
  float64  against a float64 direct convolution of the run's own layer l-1 output, at the single-layer bounds of the project:
           4e-3 * max|ref| for a plain layer (test_gpu_layers.py), SX_TOL * max(1, max|ref|) with se_unit_f64 for the SE layer
           (test_gpu_smallops.py).  Step by step every layer stays at the single-layer bound, and a layer that read stale input
           across the seam is still caught: its reference is computed from what the previous layer really wrote.

Every output must be finite (every layer's buffer starts as fp16 NaN), and the tap's report (layers, layers in row order = on
the generated epilogue, hand-over links) must equal what the case is about.  Inputs are fp16-exact draws: N(0, 1) activations,
weights N(0, 1 / fan-in), bias 0.1 N(0, 1), the SE unit's FCs as sx_fc draws them (RunDraw of _cases.py).  tests/test_tower_run_reference_cpu.py pins
the float64 convolution used here to conv_ref and shows that the can-fail case's bar is no artefact of the draw.

Measured on an MI355X (every bits check exact, every report as expected), worst float64 error / tolerance: generated epilogue
on boards 2..19 0.11 (Mish) and 0.12 (ReLU, identity) at both widths; several workgroups 0.12; compiled epilogue in a run 0.11;
index tables 0.11; input convolution first 0.11; SE layer in a run 0.14 (C = 256, se = 64), 0.15 (C = 128, se = 32), 0.12 (from
L2); eight layers 0.09.  The can-fail case lands 130 .. 263 x the tolerance away."""
import numpy as np
import pytest

import _taps
from _cases import BLOCK3, BOARD_CASES, CAN_FAIL_BAR, SWAP, RunDraw, RunSpec, blocks_spec, layer_f64, layer_io, run_draw
from _taps import KIND_BOARD, SE_FROM_L2, SE_STAGED, tower_run

pytestmark = pytest.mark.gpu


def per_layer_kernel(spec, D, l, xin, res):
    """layer l as ONE launch of the per-layer board kernel (compiled epilogue) on the same input -> [sample] = [C][b*b]"""
    if spec.se and spec.se[0] == l:
        return _taps.ok(_taps.conv_se(spec.bsz, spec.C, spec.se[1], spec.acts[l], xin, D.ws[l], D.bias[l], res, D.fc), spec, l).outs
    t = _taps.ok(_taps.conv(True, spec.bsz, spec.cin0 if l == 0 else spec.C, spec.C, 3, spec.acts[l], xin, D.ws[l], D.bias[l], res), spec, l)
    assert t.kind == KIND_BOARD, "the bits reference is the board kernel"
    return t.outs


def check_run(spec, row_order, links, chain=1, bits=True):
    """The run through the tap: the report as expected, every layer's output finite, bit-equal to the per-layer kernel and within
    the single-layer float64 bound, for every sample.  -> (outs, worst error / tolerance)"""
    D = run_draw(spec)
    t = _taps.ok(tower_run(spec, D, chain), spec)
    outs = t.outs
    assert t.report == (spec.L, row_order, links), (spec, chain, t.report)
    if spec.se:
        assert t.form == (SE_FROM_L2 if (spec.C, spec.se[1]) == (256, 128) else SE_STAGED), (spec, t.form)
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
    print(f"tower {spec} chain={chain} report={t.report}: worst error {worst:.2f} x tol")
    return outs, worst


def check_unchained(spec, row_order, outs):
    """the same run without the weight hand-over: no link, the same bits"""
    t = tower_run(spec, run_draw(spec), chain=0)
    assert t.rc == 0 and t.report == (spec.L, row_order, 0), (spec, t.rc, t.report)
    for l in range(spec.L):
        for i in range(len(spec.bsz)):
            assert np.array_equal(t.outs[l][i], outs[l][i], equal_nan=True), (spec, "layer", l, "sample", i, "the hand-over changed bits")


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


@pytest.mark.parametrize("C", [256, 128])
def test_eight_layers_as_four_residual_blocks(C):
    """Case g: the table stepped over eight elements, a hand-over into every block's second layer and none out of it."""
    check_run(blocks_spec(C), row_order=8, links=4)


@pytest.mark.parametrize("C", [256, 128])
def test_run_test_can_fail(C):
    """Case g's float64 check with the reference given layer 2's and layer 3's weights swapped: both layers land >= 4x the
    tolerance away on every sample (tests/test_tower_run_reference_cpu.py: the two references differ by far more on this draw)."""
    spec = blocks_spec(C)
    D = run_draw(spec)
    t = tower_run(spec, D)
    outs = t.outs
    assert t.rc == 0 and t.report == (8, 8, 4), (t.rc, t.report)
    for l, other in SWAP.items():
        xin, res = layer_io(spec, D, outs, l)
        for i in range(len(spec.bsz)):
            ref, tol = layer_f64(spec, D, l, i, xin[i], res[i] if res is not None else None, w64=D.w64(other))
            ratio = float(np.abs(outs[l][i] - ref).max()) / tol
            print(f"tower C={C} layer {l} against the reference with layer {other}'s weights, sample {i}: {ratio:.0f} x tol")
            assert ratio >= CAN_FAIL_BAR, (C, l, i, ratio)


def test_tap_refuses_what_it_cannot_run():
    """bad arguments are refused with a message before anything is launched, and the report says nothing ran"""
    for spec, what in ((RunSpec((19,), 192, (5,), (-1,)), "128 or 256"), (RunSpec((19,), 128, (5,) * 9, (-1,) * 9), "1 to 8"),
                       (RunSpec((19,), 128, (5, 5), (-1, 2)), "earlier layer"), (RunSpec((19,), 128, (5, 5), (-1, 0), cin0=43), "channels"),
                       (RunSpec((9, 9), 128, (5,), (-1,), se=(0, 32)), "one sample per tile")):
        t = tower_run(spec, RunDraw(spec.bsz, spec.C, spec.cin0, spec.L, spec.se, 1))
        assert t.rc == -1 and what in _taps.last_error(), (spec, t.rc, _taps.last_error())
        assert t.report == (0, 0, 0)
