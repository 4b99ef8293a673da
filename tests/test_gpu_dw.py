"""The depthwise convolutions of mixer blocks and the RepLK policy head on conv_dw.h (include/sayuri_hip.h: the conv_dw layer tap,
sayuri_hip_dw_plan, sayuri_hip_last_dw_launches; switches SAYURI_DW, SAYURI_DW_STRIPS).

conv_dw_kernel does depthwise_kernel<f16>'s arithmetic per output element (zero start, taps in row-major order with the taps outside
the board skipped, one fused multiply-add each, then bias, activate(), the residual behind it, one rounding), so the checks are on
BITS, against code that existed before the feature:
  layer level  the conv_dw tap == the conv tap with depthwise=1 (depthwise_kernel, kind 3), for every forced cut
  whole net    a context == a context created under SAYURI_DW=0, default and latency contexts alike
and, independently of the old kernel, against the float64 direct convolution (test_gpu_layers.py's bound) and the exact-arithmetic
reference of _kref.py (equality).  The tap returns the channels below C; what the kernel stores in the pad channels [C, cs) of its
NaN-pre-set buffer is read back bit for bit (hipraw.conv_dw_pad_bits) next to what depthwise_kernel stores there on the same operands.
"""
import functools
import os

import numpy as np
import pytest

import _cases
import _taps
from _golden import Golden
from _kref import assert_exact, conv_ref, exact_layer
from _oracle import PortNet
from _pipes import MAXB, Pinned, Pool, check, device_ms, fp16_tol, grid_of, make_pipe_under, within_oracle
from _taps import KIND_DEPTHWISE
from sayuri_amd import _lib, hipraw
from sayuri_amd import weights as W
from sayuri_amd.pipe import hip_forward_raw

pytestmark = pytest.mark.gpu

B = 19
DW_SWITCHES = ("SAYURI_DW", "SAYURI_DW_STRIPS")
OUTS = ("prob", "pass", "misc", "own")
KIND_DW_LDS = 7  # what the last-conv-kind reader says after the conv_dw tap


make_pipe = functools.partial(make_pipe_under, DW_SWITCHES, batch=64)  # this feature's two switches exactly as `env` says


def conv_dw(bsz, C, k, act, xs, w, bias, res=None, strips=0, max_board=_taps.MAX_BOARD, fp16=True):
    """the fp16 depthwise layer on conv_dw.h (the tap's one Python caller is hipraw.conv_dw_layer); a result as _taps.conv gives it"""
    return _taps.Conv(*hipraw.conv_dw_layer(bsz, C, k, act, xs, w, bias, res, strips, max_board, fp16))


def old_kernel(bsz, C, k, act, xs, w, bias, res=None):
    """the same layer on depthwise_kernel: the yardstick"""
    t = _taps.ok(_taps.conv(True, bsz, 1, C, k, act, xs, w, bias, res, depthwise=True, post=res is not None))
    assert t.kind == KIND_DEPTHWISE, "the yardstick is depthwise_kernel"
    return t


def _layer_tensors(bsz, C, k, with_res, seed):
    rng = np.random.default_rng(seed)
    xs = [rng.standard_normal((C, b * b)).astype(np.float32) for b in bsz]
    w = (rng.standard_normal((C, 1, k, k)) / k).astype(np.float32)
    bias = (rng.standard_normal(C) * 0.1).astype(np.float32)
    res = [rng.standard_normal((C, b * b)).astype(np.float32) for b in bsz] if with_res else None
    return xs, w, bias, res


def cuts_of(bsz):
    """the plan's own cut, 1, 2 and 5 strips, one strip per row -- those a batch's largest board has rows for (more are refused)"""
    return sorted({s for s in (0, 1, 2, 5, max(bsz)) if s <= max(bsz)})


# ---------------------------------------------------------------------------------------------------------------- 1. layer level
DW_CHANNELS = [32, 40, 48, 64, 256, 384]  # strides 32, 64 (40, 48 and 64 true channels), 256, 384
DW_BOARDS = [[2], [3] * 7, [5, 2, 3], [19], [9, 13, 19, 7, 19], [19] * 3]


@pytest.mark.parametrize("C", DW_CHANNELS)
@pytest.mark.parametrize("k", [3, 5, 7])
def test_depthwise_lds_kernel_has_the_old_kernels_bits(k, C):
    """Channel strides of 32 (one 32-channel slice), 64 (40, 48 and 64 true channels), 256 and 384 (four and six 64-channel slices);
    boards smaller than the kernel, a full board, a mixed batch, several full boards; with and without the residual behind the
    activation.  Every cut -- the engine's, 1, 2, 5 strips, one strip per row -- gives depthwise_kernel's fp16 outputs; nothing
    inside a board stays NaN, and the pad channels of 40 and 48 true channels (24 and 16 of a stride of 64) hold depthwise_kernel's
    zeros."""
    for j, bsz in enumerate(DW_BOARDS):
        for with_res in (False, True):
            act = 5 if with_res else 1
            xs, w, bias, res = _layer_tensors(bsz, C, k, with_res, seed=1000 * k + C + 11 * j + with_res)
            old = old_kernel(bsz, C, k, act, xs, w, bias, res)
            for strips in cuts_of(bsz):
                t = _taps.ok(conv_dw(bsz, C, k, act, xs, w, bias, res, strips), bsz, strips)
                assert t.kind == KIND_DW_LDS
                for y, yo in zip(t.outs, old.outs):
                    assert not np.isnan(y).any(), (k, C, bsz, strips, "an element of a board was not written")
                    assert np.array_equal(y, yo), (k, C, bsz, strips, with_res, float(np.abs(y - yo).max()))
                # channels [C, cs) of every board pixel: depthwise_kernel's bits, which are +0 -- the buffer started as NaN
                pad, pad_old = hipraw.conv_dw_pad_bits(0), hipraw.conv_dw_pad_bits(1)
                assert pad.size == pad_old.size == sum(b * b for b in bsz) * (-C % 32), (k, C, bsz, strips)
                assert np.array_equal(pad, pad_old) and not pad.any(), (k, C, bsz, strips, "pad channels", np.unique(pad)[:8])


def test_depthwise_lds_kernel_every_activation_with_and_without_residual():
    bsz = [19, 13]
    for act in range(8):
        for with_res in (True, False):
            xs, w, bias, res = _layer_tensors(bsz, 64, 7, with_res, seed=500 + 2 * act + with_res)
            old = old_kernel(bsz, 64, 7, act, xs, w, bias, res)
            t = _taps.ok(conv_dw(bsz, 64, 7, act, xs, w, bias, res))
            assert t.kind == KIND_DW_LDS
            for y, yo in zip(t.outs, old.outs):
                assert not np.isnan(y).any()
                assert np.array_equal(y, yo), (act, with_res)


# ---------------------------------------------------------------------------------------------------------------- 2. not the old kernel
@pytest.mark.parametrize("k", [3, 5, 7])
def test_depthwise_lds_kernel_within_the_float64_bound(k):
    """test_gpu_layers.py's bound (4e-3 of the reference's scale) against the float64 direct convolution on the fp16-rounded
    operands: 96 channels (three 32-channel slices), a mixed batch cut into 3 strips, the residual behind a mish."""
    bsz, C, act = [19, 9, 13, 5], 96, 5
    xs, w, bias, res = _layer_tensors(bsz, C, k, True, seed=40 + k)
    t = _taps.ok(conv_dw(bsz, C, k, act, xs, w, bias, res, strips=3))
    r16 = lambda a: a.astype(np.float16).astype(np.float64)
    ref = conv_ref([r16(x) for x in xs], bsz, w.astype(np.float64), bias.astype(np.float64), [r16(r) for r in res], k, True, act, True)
    scale = max(float(np.abs(r).max()) for r in ref)
    for got, exp in zip(t.outs, ref):
        assert float(np.abs(got - exp).max()) <= 4e-3 * scale


@pytest.mark.parametrize("k", [3, 5, 7])
def test_depthwise_lds_kernel_is_exact_on_small_integers(k):
    """_cases.exact_draw's unit tier: every product and sum is an integer fp32 holds exactly, so the one correct fp16 output
    (_kref.exact_layer, act(conv + bias) + res) is demanded value for value -- boards smaller than the kernel among them, 40 true
    channels in a stride of 64, the engine's cut and one strip per row."""
    bsz, C = _cases.DEPTHWISE_BOARDS, 40
    xs, w, bias, res = _cases.exact_draw("unit", bsz, 1, C, k, True, seed=60 + k)
    for act, with_res in ((1, True), (0, False)):
        r = res if with_res else None
        exp = [exact_layer(xs[i], w, bias, r[i] if r else None, b, k, True, act, post=True) for i, b in enumerate(bsz)]
        for strips in (0, max(bsz)):
            t = _taps.ok(conv_dw(list(bsz), C, k, act, xs, w, bias, r, strips))
            assert_exact(t.outs, exp, (k, act, with_res, strips))


# ---------------------------------------------------------------------------------------------------------------- 3. refusals
def test_depthwise_tap_refuses_what_the_route_does_not_cover():
    bsz = [19, 9]
    xs, w, bias, res = _layer_tensors(bsz, 64, 7, True, seed=77)
    before = _taps.ok(conv_dw(bsz, 64, 7, 5, xs, w, bias, res))
    x = [np.zeros((64, 361), np.float32)]
    for k in (9, 4, 2):
        assert conv_dw([19], 64, k, 0, x, np.zeros(64 * k * k, np.float32), None).rc == -1 and f"k = {k}" in _taps.last_error()
    assert conv_dw([19], 64, 7, 0, x, np.zeros(64 * 49, np.float32), None, fp16=False).rc == -1 and "fp32" in _taps.last_error()
    assert conv_dw([19], 64, 7, 0, x, np.zeros(64 * 49, np.float32), None, strips=20).rc == -1 and "more than the 19 rows" in _taps.last_error()
    after = _taps.ok(conv_dw(bsz, 64, 7, 5, xs, w, bias, res))
    for a, b in zip(before.outs, after.outs):
        assert np.array_equal(a, b)


def test_a_context_says_once_that_a_forced_cut_was_refused(tmp_weights_dir, capfd):
    """SAYURI_DW_STRIPS=20 on 19x19 boards: dw_plan refuses, the layers keep depthwise_kernel (0 launches, the old kernel's bits) and
    the context says so on stderr, once."""
    path = net_path("mixer64", tmp_weights_dir)
    sizes = [19, 9]
    gr = grid_of(W.synthetic_planes(2, sizes, seed=4), sizes)
    off, forced = make_pipe(path, {"SAYURI_DW": "0"}, batch=16), make_pipe(path, {"SAYURI_DW": "1", "SAYURI_DW_STRIPS": "20"}, batch=16)
    try:
        a = hip_forward_raw(off.ctx(0), gr, sizes, B)
        capfd.readouterr()
        b = hip_forward_raw(forced.ctx(0), gr, sizes, B)
        b = hip_forward_raw(forced.ctx(0), gr, sizes, B)
        err = capfd.readouterr().err
        assert _lib.hip().sayuri_hip_last_dw_launches(forced.ctx(0)) == 0
        assert err.count("SAYURI_DW_STRIPS=20") == 1 and "more than the 19 rows" in err and "keeps depthwise_kernel" in err, err
        for x, y in zip(a, b):
            assert np.array_equal(x, y)
    finally:
        off.Destroy()
        forced.Destroy()


# ---------------------------------------------------------------------------------------------------------------- 4. whole networks
def _mixer(channels, ffn, n=2):
    return W.NetSpec(channels, [W.BlockSpec("MixerBlock", se=bool(i % 2), ffn_channels=ffn) for i in range(n)], 32, 32)


NETS = {  # name -> spec
    "mixer64": lambda: _mixer(64, 96),
    "mixer256": lambda: _mixer(256, 384),
    "res64-replk": lambda: W.NetSpec(64, [W.BlockSpec("ResidualBlock"), W.BlockSpec("ResidualBlock", se=True)], 32, 32, policy_head="RepLK"),
    "mixer10_256": lambda: W.NetSpec(256, [W.BlockSpec("MixerBlock", se=(i % 3 == 2), ffn_channels=384) for i in range(10)], 32, 32),
}
BATCHES = [[19], [9], [19] * 5, [19, 9, 13, 9, 19, 13, 9, 9, 19, 13, 7, 19, 9, 13, 16]]


def net_path(name, workdir):
    path = os.path.join(workdir, f"dw_{name}.bin")
    if not os.path.exists(path):
        W.write_weights(path, NETS[name](), seed=35)
    return path


@pytest.mark.parametrize("name", ["mixer64", "mixer256", "res64-replk"])
def test_network_has_the_bits_of_the_old_kernel_in_both_kinds_of_context(name, tmp_weights_dir):
    """SAYURI_DW=0, the default and SAYURI_DW=1 with three forced strips give identical outputs; the first launched no conv_dw, the
    last did; in both kinds of context two positions per batch are within fp16_tol of the CPU oracle."""
    path = net_path(name, tmp_weights_dir)
    lib, net = _lib.hip(), PortNet(path)
    planes = [W.synthetic_planes(len(sizes), sizes, seed=6300 + k) for k, sizes in enumerate(BATCHES)]
    oracle = [{i: net.forward_raw(pl[i], sizes[i]) for i in {0, len(sizes) - 1}} for sizes, pl in zip(BATCHES, planes)]  # once, for both contexts
    for latency in (False, True):
        off, rule = make_pipe(path, {"SAYURI_DW": "0"}, latency=latency), make_pipe(path, latency=latency)
        forced = make_pipe(path, {"SAYURI_DW": "1", "SAYURI_DW_STRIPS": "3"}, latency=latency)
        try:
            assert lib.sayuri_hip_latency_state(forced.ctx(0)) == int(latency)
            for sizes, pl, exp in zip(BATCHES, planes, oracle):
                gr = grid_of(pl, sizes)
                a = hip_forward_raw(off.ctx(0), gr, sizes, B)
                assert lib.sayuri_hip_last_dw_launches(off.ctx(0)) == 0
                b = hip_forward_raw(rule.ctx(0), gr, sizes, B)
                c = hip_forward_raw(forced.ctx(0), gr, sizes, B)
                assert lib.sayuri_hip_last_dw_launches(forced.ctx(0)) > 0, (name, latency, sizes)
                assert np.abs(a[0]).max() > 0
                for x, y, z, what in zip(a, b, c, OUTS):
                    assert np.array_equal(x, y), (name, latency, sizes, what, "rule", float(np.abs(x - y).max()))
                    assert np.array_equal(x, z), (name, latency, sizes, what, "forced", float(np.abs(x - z).max()))
                for i, e in exp.items():
                    within_oracle(e, a, i, sizes[i], (name, latency, sizes, "SAYURI_DW=0"))
                    within_oracle(e, c, i, sizes[i], (name, latency, sizes, "SAYURI_DW=1"))
        finally:
            off.Destroy()
            rule.Destroy()
            forced.Destroy()


@pytest.mark.parametrize("latency", [False, True], ids=["default", "latency"])
def test_a_position_does_not_depend_on_its_batch_mates(latency, tmp_weights_dir):
    """a 9x9, a 13x13 and a 19x19 probe alone and inside shuffled mixed batches -- the cut changes with the batch --, SAYURI_DW=1"""
    path = net_path("mixer256", tmp_weights_dir)
    probes = {bs: W.synthetic_planes(1, bs, seed=4300 + bs)[0] for bs in (9, 13, 19)}
    rng = np.random.default_rng(78)
    pipe = make_pipe(path, {"SAYURI_DW": "1"}, latency=latency)
    try:
        ctx = pipe.ctx(0)
        for bs, probe in probes.items():
            alone = [np.array(t[0]) for t in hip_forward_raw(ctx, grid_of([probe], [bs]), [bs], B)]
            assert np.abs(alone[0]).max() > 0 and _lib.hip().sayuri_hip_last_dw_launches(ctx) > 0
            for k, sizes in enumerate([[19] * 5 + [9] * 7 + [13] * 3, [9] * 40, [13] * 9 + [7] * 6 + [19] * 2 + [9] * 21 + [16] * 3]):
                sizes = list(sizes)
                rng.shuffle(sizes)
                at = int(rng.integers(0, len(sizes) + 1))
                sizes.insert(at, bs)
                planes = W.synthetic_planes(len(sizes), sizes, seed=910 + 10 * bs + k)
                planes[at] = probe
                got = [np.array(t[at]) for t in hip_forward_raw(ctx, grid_of(planes, sizes), sizes, B)]
                for a, b, what in zip(alone, got, OUTS):
                    assert np.array_equal(a, b), (latency, bs, k, what, float(np.abs(a - b).max()))
    finally:
        pipe.Destroy()


def test_two_tickets_in_flight_give_the_solo_bits(tmp_weights_dir):
    path = net_path("mixer256", tmp_weights_dir)
    pool = Pool()
    rng = np.random.default_rng(12)
    pipe = make_pipe(path, {"SAYURI_DW": "1"}, batch=MAXB)
    pinned = Pinned()
    try:
        ctx = pipe.ctx(0)
        idxs = [pool.draw(rng, 3, "mixed"), pool.draw(rng, 11, "wild")]
        solo = [hip_forward_raw(ctx, pool.grid[i], pool.bsz[i], B) for i in idxs]
        assert _lib.hip().sayuri_hip_last_dw_launches(ctx) > 0
        tick = [pinned.submit(ctx, 0, pool, idxs[0], False), pinned.submit(ctx, 1, pool, idxs[1], False)]
        for r in range(6):
            i = r & 1
            got = pinned.wait(ctx, i, tick[i], len(idxs[i]))
            for a, b in zip(solo[i], got):
                assert np.array_equal(a, b), r
            if r < 4:
                tick[i] = pinned.submit(ctx, i, pool, idxs[i], False)
    finally:
        pinned.close()
        pipe.Destroy()


# ---------------------------------------------------------------------------------------------------------------- 5. no effect elsewhere
def test_networks_without_a_depthwise_layer_launch_no_conv_dw(tmp_weights_dir):
    from test_gpu_pw import net_path as pw_net_path
    paths = [Golden("net_20b256", tmp_weights_dir).weights_path, Golden("net_6b96", tmp_weights_dir).weights_path,
             pw_net_path("nested256-mish", tmp_weights_dir)]
    sizes = [19, 9]
    gr = grid_of(W.synthetic_planes(2, sizes, seed=3), sizes)
    for path in paths:
        for latency in (False, True):
            pipe = make_pipe(path, {"SAYURI_DW": "1"}, latency=latency, batch=16)
            try:
                hip_forward_raw(pipe.ctx(0), gr, sizes, B)
                assert _lib.hip().sayuri_hip_last_dw_launches(pipe.ctx(0)) == 0, (path, latency)
            finally:
                pipe.Destroy()


@pytest.mark.parametrize("env", [None, {"SAYURI_DW": "0"}, {"SAYURI_DW": "1"}], ids=["default", "dw0", "dw1"])
def test_tiny_all_still_matches_its_golden(env, tmp_weights_dir):
    """a 7x7 and a 5x5 mixer block on 16 channels and a RepLK head on 8, all in a stride of 32: the pad channels are the kernel's zeros"""
    g = Golden("tiny_all", tmp_weights_dir)
    cases = [(g.planes(c), c["board_size"], c["offset"], g.expected(c)) for c in g.cases if c.get("winograd", 1) == 1]
    pipe = make_pipe(g.weights_path, env, batch=16)
    try:
        check(pipe, cases, fp16_tol, "tiny_all-dw")
        sizes = [19, 9]
        hip_forward_raw(pipe.ctx(0), grid_of(W.synthetic_planes(2, sizes, seed=3), sizes), sizes, B)
        n = _lib.hip().sayuri_hip_last_dw_launches(pipe.ctx(0))
        assert (n == 0) if env == {"SAYURI_DW": "0"} else (n == 3), (env, n)
    finally:
        pipe.Destroy()


# ---------------------------------------------------------------------------------------------------------------- 6. the rule, speed
def test_the_routing_rule_has_its_boundary_where_design_md_puts_it(tmp_weights_dir):
    """engine_plan.h, dw_pays: every measured row wins (DESIGN.md Kernel 1j), so the rule takes conv_dw.h wherever the kernel applies
    and the boundary is the kernel's own: the fp16 engine and k = 3, 5, 7.  A network of a 7x7 and a 9x9 mixer block launches conv_dw
    once per forward at 1, 32 and 256 boards, under the rule and under SAYURI_DW=1 alike -- the 9x9 layer keeps depthwise_kernel --,
    never under SAYURI_DW=0 and never in the fp32 engine.  Same bits on both sides."""
    path = os.path.join(tmp_weights_dir, "dw_mixer64_k7_k9.bin")
    if not os.path.exists(path):
        W.write_weights(path, W.NetSpec(64, [W.BlockSpec("MixerBlock", ffn_channels=96, kernel_size=7),
                                             W.BlockSpec("MixerBlock", ffn_channels=96, kernel_size=9)], 32, 32), seed=36)
    lib = _lib.hip()
    pipes = {"off": make_pipe(path, {"SAYURI_DW": "0"}, batch=256), "rule": make_pipe(path, batch=256),
             "everywhere": make_pipe(path, {"SAYURI_DW": "1"}, batch=256), "fp32": make_pipe(path, batch=256, fp16=False)}
    want = {"off": 0, "rule": 1, "everywhere": 1, "fp32": 0}
    try:
        full = grid_of(W.synthetic_planes(256, [19] * 256, seed=9), [19] * 256)
        for n in (1, 32, 256):
            outs = {}
            for k, p in pipes.items():
                outs[k] = hip_forward_raw(p.ctx(0), full[:n], [19] * n, B)
                assert lib.sayuri_hip_last_dw_launches(p.ctx(0)) == want[k], (k, n)
            for x, y, z, what in zip(outs["off"], outs["rule"], outs["everywhere"], OUTS):
                assert np.array_equal(x, y) and np.array_equal(x, z), (n, what)
    finally:
        for p in pipes.values():
            p.Destroy()


@pytest.mark.parametrize("n", [256, 32])
def test_depthwise_route_is_no_slower_than_the_old_kernel(n, tmp_weights_dir, capsys):
    """Ten mixer blocks at 256 channels (feed-forward 384, 7x7), n boards of 19x19, default context.  Three contexts in one process,
    interleaved: SAYURI_DW=0 (the parent commit's kernel), SAYURI_DW=0 again, the default.  The gate: default <= first =0 arm x
    (1 + s), s = the relative difference of the two =0 arms in this same run -- no ratio is fixed in advance.  The default arm must
    have launched conv_dw.  This test's own run on an MI355X printed (ms per forward; DESIGN.md Kernel 1j):
    [dw] mixer10_256, 256 x 19x19, default context, device ms per forward: SAYURI_DW=0 4.9702 / 4.9354 (spread 0.0070), default 3.6424 (ratio 0.7328, conv_dw launches 10)
    [dw] mixer10_256, 32 x 19x19, default context, device ms per forward: SAYURI_DW=0 0.7302 / 0.7289 (spread 0.0018), default 0.5962 (ratio 0.8164, conv_dw launches 10)"""
    sizes = [19] * n
    path = net_path("mixer10_256", tmp_weights_dir)
    gr = grid_of(W.synthetic_planes(n, sizes, seed=1), sizes)
    pipes = {"off": make_pipe(path, {"SAYURI_DW": "0"}, batch=256), "off2": make_pipe(path, {"SAYURI_DW": "0"}, batch=256),
             "on": make_pipe(path, batch=256)}
    try:
        t = device_ms(pipes, gr, sizes)
        launches = _lib.hip().sayuri_hip_last_dw_launches(pipes["on"].ctx(0))
        s = abs(t["off"] - t["off2"]) / t["off"]
        with capsys.disabled():
            print(f"\n[dw] mixer10_256, {n} x 19x19, default context, device ms per forward: SAYURI_DW=0 {t['off']:.4f} / {t['off2']:.4f} "
                  f"(spread {s:.4f}), default {t['on']:.4f} (ratio {t['on'] / t['off']:.4f}, conv_dw launches {launches})")
        assert _lib.hip().sayuri_hip_last_dw_launches(pipes["off"].ctx(0)) == 0
        assert launches > 0, "a feature that does not route this batch has no purpose"
        assert t["on"] <= t["off"] * (1 + s), (n, t)
    finally:
        for p in pipes.values():
            p.Destroy()
