"""The yardstick of the run-level tower tests (test_gpu_tower_run.py), checked without a GPU.

1. conv3x3_f64 of _kref.py, the float64 convolution as nine matrix products that every kernel test uses, against conv_ref of
   _kref.py (the float64 restatement of the oracle's direct convolution) on small cases: 1e-12 * scale, both are
   float64 sums of the same products in another order.
2. The can-fail case of the GPU module (the eight-layer run checked against a reference that was given layer 2's and layer 3's
   weights swapped) on the very draw it uses: with every layer's output rounded to fp16 as the kernel stores it, the float64
   reference with the right weights and the one with the swapped weights differ by at least 4x the GPU tolerance
   (4e-3 * max|ref|) on every sample of both layers -- the bar is not an artefact of the draw."""
import numpy as np
import pytest

from _cases import CAN_FAIL_BAR, SWAP, blocks_spec, layer_f64, layer_io, run_draw
from _kref import conv3x3_f64, conv_ref, r16


@pytest.mark.parametrize("bs,cin,cout", [(2, 40, 24), (5, 33, 64), (19, 16, 8)])
def test_conv3x3_taps_f64_matches_conv_ref(bs, cin, cout):
    rng = np.random.default_rng([11, bs, cin, cout])
    x = rng.standard_normal((cin, bs * bs))
    w = rng.standard_normal((cout, cin, 3, 3)) / np.sqrt(9 * cin)
    bias = rng.standard_normal(cout)
    exp = conv_ref([x], [bs], w, bias, None, 3, False, 0, False)[0]
    got = conv3x3_f64(x, w, bias, bs)
    assert got.shape == exp.shape
    assert np.abs(got - exp).max() <= 1e-12 * max(1.0, float(np.abs(exp).max()))


@pytest.mark.parametrize("C", [256, 128])
def test_swapped_weights_move_the_reference_past_the_bar(C):
    spec = blocks_spec(C)
    D = run_draw(spec)
    n = len(spec.bsz)
    outs = []  # the run in float64 with every layer's output rounded to fp16, as far as the swapped layers
    for l in range(max(SWAP) + 1):
        xin, res = layer_io(spec, D, outs, l)
        refs = [layer_f64(spec, D, l, i, xin[i], res[i] if res is not None else None) for i in range(n)]
        if l in SWAP:
            for i in range(n):
                ref, tol = refs[i]
                swapped, tol_s = layer_f64(spec, D, l, i, xin[i], res[i] if res is not None else None, w64=D.w64(SWAP[l]))
                d = float(np.abs(ref - swapped).max())
                print(f"C={C} layer {l} sample {i}: the references differ by {d:.3f} = {d / max(tol, tol_s):.0f} x tol")
                assert d >= CAN_FAIL_BAR * max(tol, tol_s), (C, l, i, d, tol, tol_s)
        outs.append([r16(ref.astype(np.float32), True) for ref, _ in refs])
