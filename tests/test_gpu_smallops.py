"""Kernel-level parity of the non-GEMM kernels -- se_pool / se_fc / se_scale and head_tail (csrc/hip/small_ops.h) --
against the CPU oracle's restatements of the reference layers they replace:
GlobalPooling<false/true> (src/neural/blas/se_unit.cc:9-68), FullyConnect (fullyconnect.cc:7-19), SEUnit::Forward
(se_unit.cc:70-128) and the head tail of BlasForwardPipe::Forward (blas_forward_pipe.cc:496-580), through the oracle's
layer taps (oracle/sayuri_oracle.c so_tap_*).  Board sizes 2..19, mixed batches, all eight activations.

fp32 engine: abs <= 2e-5 * scale.  fp16 engine: the kernels see fp16-rounded activations (the oracle is given the same
rounded values) and store fp16 -> 2e-3 * scale on activations, 1e-4 on the fp32 outputs of the heads / gates.

The convolutions with the SE unit inside: conv_board_se_kernel / the tower's SE stage against a float64 convolution + the
oracle's unit (test_conv_with_se_unit_inside), and the split-channel form conv_board_sx_kernel (conv_board_sx.h, test_sx_*)
against a float64 convolution + se_unit_f64 -- a float64 restatement of the unit that tests/test_sx_reference_cpu.py pins to
the oracle's -- on inputs drawn so that the unit matters (sx_trunk / sx_fc: the same CPU module proves that a wrong mean
term, a wrong pixel count, a neighbour's maximum or gate, a missing eighth of the pool and a missing sibling partial each
move the result by >= 4x the tolerance).  3e-3 * max(1, |ref|max), as for the one-workgroup form: fp32 accumulators gated
in registers, fp16 FC images, fp16 store.

The *_pooled_statistics cases at the end run the one-workgroup SE kernels (both forms of the unit: staged images, FCs from L2),
se_pool / se_fc / se_scale and both head kernels on inputs that make every pooled statistic visible, against se_unit_f64 and
head_tail_f64, at the tolerances above; tests/test_se_head_reference_cpu.py holds the float64 references and the inputs to
account.  Measured on an MI355X, worst error / tolerance: convolution + unit 0.18 (staged) and 0.15 (from L2), per-layer and
tower alike; se_pool / se_fc / se_scale 0.24 (fp16), 0.03 (fp32), gate 0.01; head_board 0.41; head_tail < 0.01."""
import numpy as np
import pytest

import _taps
from _cases import (HEAD_BOARDS, HEAD_PAIRS, HEAD_SEED, SE_CASE_IDS, SE_CASES, SE_L2_LAYERS, SE_LAYERS, SE_SEED, SE_UNIT_BATCHES, SX_TOL, head_inputs,
                    se_case_batches, se_inputs, se_unit_x, sx_fc, sx_reference, sx_trunk)
from _kref import act_np, conv3x3_f64, head_ratio, r16, se_apply_f64, se_gate_f64, se_pool_f64, se_unit_f64
from _oracle import PortNet
from _taps import KIND_BOARD_SX, SE_FROM_L2, SE_STAGED
from sayuri_amd import _lib

pytestmark = pytest.mark.gpu

oracle = PortNet.lib
HEAD_OUTS = ("prob", "pass", "own", "misc")
BOARDS = [[19], [9, 13, 19], [2, 3, 5, 7, 19, 4], [19] * 5, [13, 13, 9, 9, 9, 19, 6]]


@pytest.mark.parametrize("fp16", [False, True], ids=["fp32", "fp16"])
@pytest.mark.parametrize("act", range(8))
def test_se_unit_kernels(act, fp16):
    o = oracle()
    rng = np.random.default_rng(100 + act)
    for bsz, C, se, with_res in ((BOARDS[act % len(BOARDS)], 64, 16, True), (BOARDS[(act + 1) % len(BOARDS)], 96, 24, False),
                                 ([19, 9], 256, 64, True)):
        xs = [r16(rng.standard_normal((C, b * b)).astype(np.float32), fp16) for b in bsz]
        rs = [r16(rng.standard_normal((C, b * b)).astype(np.float32), fp16) for b in bsz] if with_res else None
        w1 = (rng.standard_normal((se, 3 * C)) / np.sqrt(3 * C)).astype(np.float32)
        b1 = (rng.standard_normal(se) * 0.1).astype(np.float32)
        w2 = (rng.standard_normal((2 * C, se)) / np.sqrt(se)).astype(np.float32)
        b2 = (rng.standard_normal(2 * C) * 0.1).astype(np.float32)
        t = _taps.ok(_taps.se_unit(fp16, bsz, C, se, act, xs, rs, (w1, b1, w2, b2)))
        for i, b in enumerate(bsz):
            # GlobalPooling<false> + both FullyConnects -> the gate
            pool = np.zeros(3 * C, np.float32)
            o.so_tap_global_pool(b, C, _lib.fp(xs[i]), _lib.fp(pool), 0)
            mid = np.zeros(se, np.float32)
            o.so_tap_fully_connect(3 * C, se, _lib.fp(w1), _lib.fp(b1), _lib.fp(pool), _lib.fp(mid), act)
            exc = np.zeros(2 * C, np.float32)
            o.so_tap_fully_connect(se, 2 * C, _lib.fp(w2), _lib.fp(b2), _lib.fp(mid), _lib.fp(exc), 0)
            exp_gate = np.concatenate([1.0 / (1.0 + np.exp(-exc[:C].astype(np.float64))), exc[C:]])
            assert np.abs(t.gate[i] - exp_gate).max() <= 1e-4 * max(1.0, np.abs(exp_gate).max()), (bsz, i, "gate")
            # the whole unit
            ref = xs[i].copy()
            o.so_tap_se_unit(b, C, se, _lib.fp(w1), _lib.fp(b1), _lib.fp(w2), _lib.fp(b2), _lib.fp(ref), _lib.fp(rs[i]) if rs else None, act)
            got = t.outs[i]
            scale = max(1.0, float(np.abs(ref).max()))
            tol = (2e-3 if fp16 else 2e-5) * scale
            assert np.isfinite(got).all()
            assert np.abs(got - ref).max() <= tol, (bsz, i, act, float(np.abs(got - ref).max()), tol)


def oracle_head_tail(o, b, Cp, Cv, act, pc, vc, ws, prob_ch=5, pass_outs=5, misc_outs=15):
    """the oracle's head tail on the activated head planes of one sample -> (prob [prob_ch][b*b], pass, own [b*b], misc)"""
    S = b * b
    e_prob, e_pass = np.zeros((prob_ch, S), np.float32), np.zeros(pass_outs, np.float32)
    e_own, e_misc = np.zeros(S, np.float32), np.zeros(misc_outs, np.float32)
    o.so_tap_head_tail(b, Cp, Cv, prob_ch, pass_outs, misc_outs, act, _lib.fp(pc), _lib.fp(vc), *[_lib.fp(w) for w in ws],
                       _lib.fp(e_prob), _lib.fp(e_pass), _lib.fp(e_own), _lib.fp(e_misc))
    return e_prob, e_pass, e_own, e_misc


def assert_heads(got, exp, tol, what):
    for name, g, e in zip(HEAD_OUTS, got, exp):
        assert np.abs(g - e).max() <= tol * max(1.0, np.abs(e).max()), what + (name, float(np.abs(g - e).max()))


@pytest.mark.parametrize("fp16", [False, True], ids=["fp32", "fp16"])
@pytest.mark.parametrize("act", range(8))
def test_head_tail_kernel(act, fp16):
    o = oracle()
    rng = np.random.default_rng(200 + act)
    for bsz, Cp, Cv in ((BOARDS[act % len(BOARDS)], 24, 24), (BOARDS[(act + 2) % len(BOARDS)], 32, 48), ([19, 13], 48, 32)):
        prob_ch, pass_outs, misc_outs = 5, 5, 15
        pcs = [r16(rng.standard_normal((Cp, b * b)).astype(np.float32), fp16) for b in bsz]
        vcs = [r16(rng.standard_normal((Cv, b * b)).astype(np.float32), fp16) for b in bsz]
        shapes = [(Cp, 3 * Cp), (Cp,), (pass_outs, Cp), (pass_outs,), (3 * Cv, 3 * Cv), (3 * Cv,), (misc_outs, 3 * Cv), (misc_outs,),
                  (prob_ch, Cp), (prob_ch,), (Cv,), (1,)]
        ws = [(rng.standard_normal(s) / np.sqrt(s[-1] if len(s) > 1 else 4)).astype(np.float32) for s in shapes]
        outs = _taps.head_boards(_taps.ok(_taps.head_tail(fp16, bsz, Cp, Cv, act, pcs, vcs, ws)), bsz)  # off-board cells of a smaller sample stay 0
        for i, b in enumerate(bsz):
            assert_heads(outs[i], oracle_head_tail(o, b, Cp, Cv, act, pcs[i].copy(), vcs[i], ws), 2e-4, (bsz, i))


@pytest.mark.parametrize("via_tower", [0, 1], ids=["per-layer kernel", "tower kernel"])
@pytest.mark.parametrize("act", range(8))
def test_conv_with_se_unit_inside(act, via_tower):
    """conv_board_se_kernel / the SE body of the persistent tower kernel at kernel level: float64 convolution followed by
    the oracle's SEUnit::Forward tap (se_unit.cc:70-128) on it.  Boards 2..19, C = 96 / 128 / 256, se = 24 / 32 / 64,
    one sample per tile (fused) and several samples per tile (the tap must report the fallback)."""
    o = oracle()
    rng = np.random.default_rng(300 + act)
    cases = [([19, 19, 19], 256, 64, True), ([19] * 2, 128, 32, False), ([19, 17, 16, 15, 14], 128, 24, True), ([19], 96, 24, True)]
    # small boards one per batch (a batch of several small boards shares a tile: checked below)
    cases += [([b], 128, 32, bool(b & 1)) for b in (2, 3, 5, 9, 13)][act % 5:act % 5 + 2]
    for bsz, C, se, with_res in cases:
        xs = [r16(rng.standard_normal((C, b * b)).astype(np.float32), True) for b in bsz]
        rs = [r16(rng.standard_normal((C, b * b)).astype(np.float32), True) for b in bsz] if with_res else None
        w = r16((rng.standard_normal((C, C, 3, 3)) / np.sqrt(9 * C)).astype(np.float32), True)
        bias = (rng.standard_normal(C) * 0.1).astype(np.float32)
        w1 = (rng.standard_normal((se, 3 * C)) / np.sqrt(3 * C)).astype(np.float32)
        b1 = (rng.standard_normal(se) * 0.1).astype(np.float32)
        w2 = (rng.standard_normal((2 * C, se)) / np.sqrt(se)).astype(np.float32)
        b2 = (rng.standard_normal(2 * C) * 0.1).astype(np.float32)
        t = _taps.conv_se(bsz, C, se, act, xs, w, bias, rs, (w1, b1, w2, b2), via_tower)
        if C % 128:  # no board kernel for this channel count (the engine runs such layers on conv_mfma + the separate SE kernels)
            assert t.rc == 1
            continue
        _taps.ok(t, bsz, C)
        for i, b in enumerate(bsz):
            ref = conv3x3_f64(xs[i], w, bias, b).astype(np.float32)
            ref = np.ascontiguousarray(ref)
            o.so_tap_se_unit(b, C, se, _lib.fp(w1), _lib.fp(b1), _lib.fp(w2), _lib.fp(b2), _lib.fp(ref), _lib.fp(rs[i]) if rs else None, act)
            got = t.outs[i]
            scale = max(1.0, float(np.abs(ref).max()))
            assert np.isfinite(got).all()
            # fp16 store + fp16 FC weights: 3e-3 of the output scale
            assert np.abs(got - ref).max() <= 3e-3 * scale, (bsz, i, C, act, float(np.abs(got - ref).max()), scale)
    # several samples in one tile: the fused kernel does not apply, the tap says so (the engine runs conv + se_pool / se_fc / se_scale)
    z = np.zeros(3 * 128 * 32 + 512, np.float32)
    assert _taps.conv_se([9] * 4, 128, 32, act, [np.zeros((128, 81), np.float32)] * 4, np.zeros((128, 128, 3, 3), np.float32), z, None, (z,) * 4,
                         via_tower).rc == 1


@pytest.mark.parametrize("via_tower", [0, 1], ids=["per-layer kernel", "tower kernel"])
def test_conv_se_tap_says_that_an_se_width_of_zero_does_not_apply(via_tower):
    """se_size = 0 has no form of the SE stage (se_l2_form_ok's guard stands in front of the divisions by se / 4): the tap
    returns 1 in front of any upload of the layer or launch, reports form 0, and a normal call afterwards (se = 32) gives
    the bits of the same call before it."""
    rng = np.random.default_rng(77)
    C, se, bsz = 128, 32, [19]
    xs = [rng.standard_normal((C, 361)).astype(np.float32)]
    w = (rng.standard_normal((C, C, 3, 3)) / np.sqrt(9 * C)).astype(np.float32)
    bias = (rng.standard_normal(C) * 0.1).astype(np.float32)
    fc = ((rng.standard_normal((se, 3 * C)) / np.sqrt(3 * C)).astype(np.float32), (rng.standard_normal(se) * 0.1).astype(np.float32),
          (rng.standard_normal((2 * C, se)) / np.sqrt(se)).astype(np.float32), (rng.standard_normal(2 * C) * 0.1).astype(np.float32))
    before = _taps.ok(_taps.conv_se(bsz, C, se, 5, xs, w, bias, None, fc, via_tower), via_tower)
    assert before.form != 0
    one = np.zeros(1, np.float32)
    t = _taps.conv_se(bsz, C, 0, 5, xs, w, bias, None, (one,) * 4, via_tower)
    assert t.rc == 1 and t.form == 0, (t.rc, t.form)
    after = _taps.ok(_taps.conv_se(bsz, C, se, 5, xs, w, bias, None, fc, via_tower), via_tower)
    assert after.form == before.form and np.array_equal(after.outs[0].view(np.uint32), before.outs[0].view(np.uint32))


@pytest.mark.parametrize("act", range(8))
def test_head_board_kernel(act):
    """head_board_kernel at kernel level: the two 1x1 head convolutions in float64 (on the fp16-rounded trunk), rounded to
    nothing, then the oracle's head-tail tap (blas_forward_pipe.cc:449-580).  Boards 2..19, C = 128 / 256, Cp / Cv =
    24 / 32 / 48."""
    o = oracle()
    rng = np.random.default_rng(400 + act)
    for bsz, C, Cp, Cv in ((BOARDS[act % len(BOARDS)], 128, 24, 24), (BOARDS[(act + 2) % len(BOARDS)], 256, 32, 32), ([19, 13, 2], 256, 32, 48),
                           ([19, 5], 128, 48, 32)):
        prob_ch, pass_outs, misc_outs = 5, 5, 15
        ts = [r16(rng.standard_normal((C, b * b)).astype(np.float32), True) for b in bsz]
        p_w = r16((rng.standard_normal((Cp, C)) / np.sqrt(C)).astype(np.float32), True)
        v_w = r16((rng.standard_normal((Cv, C)) / np.sqrt(C)).astype(np.float32), True)
        p_b = (rng.standard_normal(Cp) * 0.1).astype(np.float32)
        v_b = (rng.standard_normal(Cv) * 0.1).astype(np.float32)
        shapes = [(Cp, 3 * Cp), (Cp,), (pass_outs, Cp), (pass_outs,), (3 * Cv, 3 * Cv), (3 * Cv,), (misc_outs, 3 * Cv), (misc_outs,),
                  (prob_ch, Cp), (prob_ch,), (Cv,), (1,)]
        ws = [(rng.standard_normal(s) / np.sqrt(s[-1] if len(s) > 1 else 4)).astype(np.float32) for s in shapes]
        ws[8] = r16(ws[8], True)   # the per-pixel weights are an fp16 MFMA image in the kernel
        ws[10] = r16(ws[10], True)
        outs = _taps.head_boards(_taps.ok(_taps.head_board(bsz, C, Cp, Cv, act, ts, p_w, p_b, v_w, v_b, ws), bsz, C, Cp, Cv), bsz)
        for i, b in enumerate(bsz):
            pc = act_np(p_w.astype(np.float64) @ ts[i].astype(np.float64) + p_b[:, None], act).astype(np.float32)
            vc = act_np(v_w.astype(np.float64) @ ts[i].astype(np.float64) + v_b[:, None], act).astype(np.float32)
            pc, vc = np.ascontiguousarray(pc), np.ascontiguousarray(vc)
            # the head planes stay in fp32 registers; the per-pixel product runs on fp16-rounded planes: 2e-3 of the scale
            assert_heads(outs[i], oracle_head_tail(o, b, Cp, Cv, act, pc, vc, ws), 2e-3, (bsz, i))


# ------------------------------------------------------------------ conv_board_sx_kernel (conv_board_sx.h) at layer level
SX_STANDARD = (19,) * 5 + (13,) * 5 + (9,) * 6  # 10 tiles: a second group of 8 with empty places, partial tiles of 13 and of 9


def sx_run(seed, bsz, C, se, act, with_res, kts, check=None):
    """The layer of sx_trunk(seed, bsz, C) / sx_fc(seed, C, se) through the tap: it must run, on `kts` channel tiles per board
    tile; every output finite; the samples `check` (default: all) within SX_TOL of conv3x3_f64 + se_unit_f64."""
    T, fc = sx_trunk(seed, tuple(bsz), C), sx_fc(seed, C, se)
    t = _taps.ok(_taps.conv_sx(T.bsz, C, se, act, T.xs, T.w, T.bias, T.rs if with_res else None, fc), bsz, C, se)
    outs = t.outs
    assert t.kind == KIND_BOARD_SX
    print(f"conv_board_sx C={C} se={se} act={act} res={int(with_res)} boards={list(bsz)}: kts={t.kts}")
    assert t.kts == kts, (C, t.kts, kts)
    for i, got in enumerate(outs):
        assert np.isfinite(got).all(), (bsz, C, se, act, i, "an output nobody wrote, or a non-finite one")
    for i in (range(len(bsz)) if check is None else check):
        ref = sx_reference(T, fc, i, act, with_res)
        tol = SX_TOL * max(1.0, float(np.abs(ref).max()))
        err = float(np.abs(outs[i] - ref).max())
        print(f"  sample {i} ({T.bsz[i]}x{T.bsz[i]}): err {err:.5f}, tol {tol:.5f}")
        assert err <= tol, (bsz, C, se, act, with_res, i, err, tol)
    return outs


@pytest.mark.parametrize("with_res", [True, False], ids=["res", "nores"])
def test_sx_standard_layer_more_than_8_tiles(with_res):
    """C = 384, se = 96 on 10 tiles: 5 of 19x19, 13x13 as (2, 2, 1), 9x9 as (4, 2) -- the 9x9 tiles are the second group of 8
    (block index >= 8 kts), whose other six places are empty.  Checked: the first and last sample of every tile kind."""
    check = (0, 4, 5, 6, 8, 9, 10, 13, 14, 15)
    sx_run(1, SX_STANDARD, 384, 96, 5, with_res, 3, check)


@pytest.mark.parametrize("bsz", [(10,) * 4 + (11,) * 3 + (12,) * 3, (14, 15, 16, 17, 18)], ids=["10-11-12", "14..18"])
def test_sx_three_per_tile_and_alone_in_a_tile(bsz):
    """10x10 and 11x11 are the only sizes with three samples per tile (3 x 11x11 = 507 of the 512 halo positions); 14..18 sit
    alone in a tile, each with its own eighth length ceil(npix / 8)."""
    sx_run(2, bsz, 384, 96, 5, True, 3)


@pytest.mark.parametrize("with_res", [True, False], ids=["res", "nores"])
@pytest.mark.parametrize("act", range(8))
def test_sx_activations(act, with_res):
    """Every activation in mid = activate(...) and in the epilogue's switch (the trunk and its float64 convolution are shared)."""
    sx_run(3, (13, 13, 9, 9, 9, 19), 384, 48, act, with_res, 3)


@pytest.mark.parametrize("C,se,kts", [(256, 96, 2), (512, 64, 4)], ids=["kts2", "kts4"])
def test_sx_channel_tile_counts(C, se, kts):
    """Two and four sibling workgroups per board tile.  (C = 256 reaches this kernel in the engine when the one-workgroup
    images of make_se_images do not fit, se >= 72; se = 64 at kts = 4 fills the whole `red` area, parts * se = 2048.)"""
    sx_run(4, (19, 13, 13, 9, 9, 9, 9), C, se, 5, True, kts)


def test_sx_pad_channels():
    """C = 360 in a 384-row image: channels 360..383 of the third channel tile are padding (zero weight rows, zero image rows)."""
    sx_run(5, (19, 11, 11, 11), 360, 96, 5, True, 3)


@pytest.mark.parametrize("se", [100, 64, 20, 4])
def test_sx_se_width_edges(se):
    """se = 100: the two images fill SxLds::stage_bytes to the byte (51200 + 53248); 64: quads = 16, parts * se = 2048; 20: quads
    = 5 does not divide 512; 4: quads = 1."""
    sx_run(6, (13, 13, 9), 384, se, 5, True, 3)


def test_sx_refusals():
    """Shapes the form does not apply to return 1 -- never a launch, never an error: a board of which more than four fit a tile,
    one channel tile, an SE width whose images do not fit the stage area (104) or that is no multiple of 4 (6)."""
    for bsz, C, se in (((9, 9, 8), 384, 96), ((19, 5), 384, 96), ((19, 9), 128, 32), ((13, 9), 384, 104), ((13, 9), 384, 6)):
        T = sx_trunk(7, bsz, C)
        rng = np.random.default_rng(se)
        fc = [rng.standard_normal(s).astype(np.float32) for s in ((se, 3 * C), (se,), (2 * C, se), (2 * C,))]
        t = _taps.conv_sx(T.bsz, C, se, 5, T.xs, T.w, T.bias, T.rs, fc)
        assert t.rc == 1, (bsz, C, se, t.rc, _taps.last_error())
        assert t.kts == 0
        assert all(np.isnan(o).all() for o in t.outs)  # nothing was written


@pytest.mark.parametrize("bs,full", [(9, 4), (11, 3)], ids=["9x9", "11x11"])
def test_sx_position_independence_on_bits(bs, full):
    """A sample's result is a function of the sample alone (README): one board gives the same BITS alone, first and last in a
    full tile of its size, in a partial tile, and inside a 10-tile batch (the standard one for 9x9; for 11x11 the same batch
    with seven 11x11 in place of the 13x13: tiles of 3, 3 and 1)."""
    C, se, act = 384, 96, 5
    big = SX_STANDARD if bs == 9 else (19,) * 5 + (11,) * 7 + (9,) * 6
    T, fc = sx_trunk(8, big, C), sx_fc(8, C, se)
    pool = [i for i, b in enumerate(big) if b == bs]  # the samples of this size: the probe and its fillers
    probe, fill = pool[1], [pool[0]] + pool[2:]

    def run(order):
        t = _taps.ok(_taps.conv_sx([T.bsz[i] for i in order], C, se, act, [T.xs[i] for i in order], T.w, T.bias, [T.rs[i] for i in order], fc), order)
        assert t.kts == 3
        got = t.outs[order.index(probe)]
        assert np.isfinite(got).all()
        return got

    alone = run([probe])
    ref = sx_reference(T, fc, probe, act, True)
    assert np.abs(alone - ref).max() <= SX_TOL * max(1.0, float(np.abs(ref).max()))
    situations = {
        "first in a full tile": [probe] + fill[:full - 1],
        "last in a full tile": fill[:full - 1] + [probe],
        "in a partial tile": [fill[0], probe],
        "behind a full tile, alone in the next": fill[:full] + [probe],
        "inside the 10-tile batch": list(range(len(big))),
    }
    for name, order in situations.items():
        np.testing.assert_array_equal(run(order), alone, err_msg=name)


# ====================================================================================================================
# Pooled statistics of the one-workgroup SE kernels and of the heads, on the spread and probe draws of _cases.py (se_inputs,
# head_inputs), against float64 references (conv3x3_f64 + se_unit_f64, head_tail_f64).
def zero_scaled_mean(w, C):
    """a valid but different weight set: the columns of the scaled-mean third of a (mean, scaled mean, third) FC zeroed"""
    w = w.copy()
    w[:, C:2 * C] = 0.0
    return w


def conv_se_tap(T, fc, C, se, act, via_tower, with_res=True):
    return _taps.conv_se(T.bsz, C, se, act, T.xs, T.w, T.bias, T.rs if with_res else None, fc, via_tower)


def conv_se_run(draw, bsz, C, se, act, via_tower, with_res=True):
    """The layer of se_inputs(draw, SE_SEED, bsz, C, se) through the tap: it must run, in the form the layer's SE width asks for;
    every sample within SX_TOL of conv3x3_f64 + se_unit_f64.  -> the worst error / tolerance"""
    T, fc = se_inputs(draw, SE_SEED, tuple(bsz), C, se)
    t = _taps.ok(conv_se_tap(T, fc, C, se, act, via_tower, with_res), draw, bsz, C, se, via_tower)
    form = t.form
    assert form == (SE_FROM_L2 if (C, se) in SE_L2_LAYERS else SE_STAGED), (C, se, form)
    worst = 0.0
    for i, got in enumerate(t.outs):
        ref = sx_reference(T, fc, i, act, with_res)
        tol = SX_TOL * max(1.0, float(np.abs(ref).max()))
        assert np.isfinite(got).all(), (draw, bsz, C, se, act, i)
        err = float(np.abs(got - ref).max())
        worst = max(worst, err / tol)
        assert err <= tol, (draw, bsz, C, se, act, via_tower, i, err, tol)
    print(f"conv + SE unit {draw} C={C} se={se} act={act} {'tower' if via_tower else 'per-layer'} form={form} boards={list(bsz)}: worst error {worst:.2f} x tol")
    return worst


@pytest.mark.parametrize("via_tower", [0, 1], ids=["per-layer kernel", "tower kernel"])
@pytest.mark.parametrize("draw", ["spread", "probe"])
@pytest.mark.parametrize("C,se,act", SE_CASES, ids=SE_CASE_IDS)
def test_conv_se_pooled_statistics(C, se, act, draw, via_tower):
    """conv_board_se_kernel / the tower's SE stage on inputs that show every pooled statistic (_cases.py), staged images
    (C = 256 / se = 64, C = 128 / se = 32) and FCs from L2 (se = 128 / 256): samples alone in a tile of 19x19 .. 14x14 and of
    2x2 .. 13x13 at activations 5 and 0, all eight activations on one small batch.  The tap reports which form ran."""
    for bsz in se_case_batches(C, se, act):
        conv_se_run(draw, bsz, C, se, act, via_tower)


@pytest.mark.parametrize("via_tower", [0, 1], ids=["per-layer kernel", "tower kernel"])
@pytest.mark.parametrize("C,se", [(256, 64), (256, 128)], ids=["staged", "from-L2"])
def test_conv_se_test_can_fail(C, se, via_tower):
    """The real kernel on a valid but different weight set -- w1 with its scaled-mean columns zeroed -- is >= 4x the tolerance away
    from the unmutated reference on every sample but the 14x14 one, where the term is 0 (and which stays within the tolerance):
    neither fp16 path washes the term out."""
    bsz, act = (19, 18, 17, 16, 15, 14), 5
    T, fc = se_inputs("spread", SE_SEED, bsz, C, se)
    outs = _taps.ok(conv_se_tap(T, (zero_scaled_mean(fc[0], C),) + fc[1:], C, se, act, via_tower), C, se).outs
    for i, bs in enumerate(bsz):
        ref = sx_reference(T, fc, i, act, True)
        ratio = float(np.abs(outs[i] - ref).max()) / (SX_TOL * max(1.0, float(np.abs(ref).max())))
        print(f"conv + SE unit C={C} se={se} {'tower' if via_tower else 'per-layer'} without the scaled-mean columns, {bs}x{bs}: {ratio:.1f} x tol")
        assert ratio <= 1.0 if bs == 14 else ratio >= 4.0, (C, se, via_tower, bs, ratio)


@pytest.mark.parametrize("fp16", [False, True], ids=["fp32", "fp16"])
@pytest.mark.parametrize("draw", ["spread", "probe"])
@pytest.mark.parametrize("act", [5, 0])
def test_se_unit_kernels_pooled_statistics(act, draw, fp16):
    """se_pool / se_fc / se_scale on the same two draws (the unit's input is the trunk's convolution, rounded as the engine stores
    it), against se_unit_f64: 2e-3 / 2e-5 of the output scale, the gate read out at 1e-4.  One batch of large boards, one where
    several small boards follow each other."""
    for C, se in SE_LAYERS:
        for bsz in SE_UNIT_BATCHES:
            T, fc = se_inputs(draw, SE_SEED, bsz, C, se)
            xs = [se_unit_x(T, i, fp16) for i in range(len(bsz))]
            t = _taps.ok(_taps.se_unit(fp16, bsz, C, se, act, xs, T.rs, fc))
            outs, gate = t.outs, t.gate
            worst = worst_gate = 0.0
            for i, bs in enumerate(bsz):
                gamma, beta = se_gate_f64(se_pool_f64(xs[i], bs), *fc, act)
                exp_gate = np.concatenate([gamma, beta])
                gerr = float(np.abs(gate[i] - exp_gate).max()) / (1e-4 * max(1.0, float(np.abs(exp_gate).max())))
                ref = se_apply_f64(xs[i], T.rs[i], gamma, beta, act)
                tol = (2e-3 if fp16 else 2e-5) * max(1.0, float(np.abs(ref).max()))
                assert np.isfinite(outs[i]).all()
                err = float(np.abs(outs[i] - ref).max())
                worst, worst_gate = max(worst, err / tol), max(worst_gate, gerr)
                assert gerr <= 1.0, (draw, bsz, C, i, "gate", gerr)
                assert err <= tol, (draw, bsz, C, se, act, fp16, i, err, tol)
            print(f"SE kernels {draw} {'fp16' if fp16 else 'fp32'} C={C} se={se} act={act} boards={list(bsz)}: worst error {worst:.2f} x tol, "
                  f"gate {worst_gate:.2f} x 1e-4")


@pytest.mark.parametrize("fp16", [False, True], ids=["fp32", "fp16"])
def test_se_unit_kernels_test_can_fail(fp16):
    """as test_conv_se_test_can_fail, for the separate kernels"""
    C, se, act, bsz = 128, 32, 5, (19, 16, 14)
    T, fc = se_inputs("spread", SE_SEED, bsz, C, se)
    xs = [se_unit_x(T, i, fp16) for i in range(len(bsz))]
    outs = _taps.ok(_taps.se_unit(fp16, bsz, C, se, act, xs, T.rs, (zero_scaled_mean(fc[0], C),) + fc[1:])).outs
    for i, bs in enumerate(bsz):
        ref = se_unit_f64(xs[i], T.rs[i], *fc, bs, act)
        ratio = float(np.abs(outs[i] - ref).max()) / ((2e-3 if fp16 else 2e-5) * max(1.0, float(np.abs(ref).max())))
        print(f"SE kernels {'fp16' if fp16 else 'fp32'} without the scaled-mean columns, {bs}x{bs}: {ratio:.1f} x tol")
        assert ratio <= 1.0 if bs == 14 else ratio >= 4.0, (fp16, bs, ratio)


def head_call(H, act, fp16=True):
    """head_tail_kernel on H's planes (H.C == 0) or head_board_kernel on its trunk -> [(prob, pass, own, misc) of each sample], the
    per-pixel outputs cut to the sample's board"""
    if H.C == 0:
        t = _taps.head_tail(fp16, H.bsz, H.Cp, H.Cv, act, H.pcs, H.vcs, H.ws)
    else:
        t = _taps.head_board(H.bsz, H.C, H.Cp, H.Cv, act, H.ts, H.p_w, H.p_b, H.v_w, H.v_b, H.ws)
    return _taps.head_boards(_taps.ok(t, H.C, H.Cp, H.Cv), H.bsz)


def head_run(draw, Cp, Cv, C, act, fp16, tol):
    H = head_inputs(draw, HEAD_SEED, HEAD_BOARDS, Cp, Cv, C, fp16)
    outs = head_call(H, act, fp16)
    worst = 0.0
    for i, bs in enumerate(H.bsz):
        ref = H.reference(i, act)
        for name, got, r in zip(HEAD_OUTS, outs[i], ref):
            assert np.isfinite(got).all()
            ratio = float(np.abs(got - r).max()) / (tol * max(1.0, float(np.abs(r).max())))
            worst = max(worst, ratio)
            assert ratio <= 1.0, (draw, Cp, Cv, C, act, fp16, i, bs, name, ratio)
    print(f"{'head_board' if C else 'head_tail'} {draw} C={C} Cp={Cp} Cv={Cv} act={act} {'fp16' if fp16 else 'fp32'}: worst error {worst:.2f} x tol")


@pytest.mark.parametrize("fp16", [False, True], ids=["fp32", "fp16"])
@pytest.mark.parametrize("draw", ["spread", "probe"])
@pytest.mark.parametrize("act", [5, 0])
def test_head_tail_kernel_pooled_statistics(act, draw, fp16):
    """head_tail_kernel against head_tail_f64 at 2e-4, boards 19 / 14 / 13 / 9 / 2 in one batch, on planes whose pooled statistics
    each carry weight (spread) and with spikes at the pooling's boundary pixels behind probe FCs (probe)."""
    for Cp, Cv in HEAD_PAIRS:
        head_run(draw, Cp, Cv, 0, act, fp16, 2e-4)


@pytest.mark.parametrize("C", [128, 256])
@pytest.mark.parametrize("draw", ["spread", "probe"])
@pytest.mark.parametrize("act", [5, 0])
def test_head_board_kernel_pooled_statistics(act, draw, C):
    """head_board_kernel against the float64 head convolutions + head_tail_f64 at 2e-3, same boards: its pooling runs over 384 pixel
    slots in 24 column tiles, of which a board uses a prefix."""
    for Cp, Cv in HEAD_PAIRS:
        head_run(draw, Cp, Cv, C, act, True, 2e-3)


@pytest.mark.parametrize("C", [0, 256], ids=["head_tail", "head_board"])
def test_head_kernels_test_can_fail(C):
    """The real kernels on p_inter with its scaled-mean columns zeroed are >= 4x the tolerance away from the unmutated reference
    on every sample but the 14x14 one (which stays within it)."""
    import copy
    Cp, Cv, act, tol = 32, 32, 5, 2e-3 if C else 2e-4
    H = head_inputs("spread", HEAD_SEED, HEAD_BOARDS, Cp, Cv, C, True)
    M = copy.copy(H)
    M.ws = [zero_scaled_mean(H.ws[0], Cp)] + H.ws[1:]
    outs = head_call(M, act)
    for i, bs in enumerate(H.bsz):
        ref = H.reference(i, act)
        ratio = head_ratio(outs[i], ref, ref, tol)
        print(f"{'head_board' if C else 'head_tail'} without p_inter's scaled-mean columns, {bs}x{bs}: {ratio:.1f} x tol")
        assert ratio <= 1.0 if bs == 14 else ratio >= 4.0, (C, bs, ratio)
