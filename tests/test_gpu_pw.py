"""The tower's 1x1 convolutions of bottleneck-family networks on conv_pw.h (include/sayuri_hip.h: the conv_pw layer tap,
sayuri_hip_pw_plan, sayuri_hip_last_pw_launches; switches SAYURI_PW, SAYURI_PW_PIECES).

conv_pw_kernel accumulates as the generic kernel does for fp16 1x1 layers (zero start, 32-channel chunks ascending, one MFMA per
chunk and tile, then bias, residual, activate(), one rounding), so the checks are on BITS, against code that existed before the
feature:
  layer level  the conv_pw tap == the conv tap (generic kernel, kind 0), for every forced cut
  whole net    a context == a context created under SAYURI_PW=0, default and latency contexts alike
The tolerance checks (float64 direct convolution, the CPU oracle) reuse conv_ref of _kref.py, fp16_tol of _pipes.py and the bound of
test_gpu_layers.py.
"""
import functools
import os

import numpy as np
import pytest

import _taps
from _golden import Golden
from _kref import conv_ref
from _oracle import PortNet
from _pipes import MAXB, Pinned, Pool, device_ms, grid_of, make_pipe_under, within_oracle
from _taps import KIND_GENERIC
from sayuri_amd import _lib, hipraw
from sayuri_amd import weights as W
from sayuri_amd.pipe import hip_forward_packed_raw, hip_forward_raw

pytestmark = pytest.mark.gpu

B = 19
PW_SWITCHES = ("SAYURI_PW", "SAYURI_PW_PIECES")
OUTS = ("prob", "pass", "misc", "own")


make_pipe = functools.partial(make_pipe_under, PW_SWITCHES, batch=64)  # this feature's two switches exactly as `env` says


KIND_PW = 6  # what the last-conv-kind reader says after the pointwise tap


def conv_pw(bsz, cin, cout, act, xs, w, bias, res=None, pieces=0, max_board=_taps.MAX_BOARD):
    """the fp16 1x1 layer on conv_pw.h (the tap's one Python caller is hipraw.conv_pw_layer); a result as _taps.conv gives it"""
    return _taps.Conv(*hipraw.conv_pw_layer(bsz, cin, cout, act, xs, w, bias, res, pieces, max_board))


def _layer_tensors(bsz, cin, cout, with_res, seed):
    rng = np.random.default_rng(seed)
    xs = [rng.standard_normal((cin, b * b)).astype(np.float32) for b in bsz]
    w = (rng.standard_normal((cout, cin, 1, 1)) / np.sqrt(cin)).astype(np.float32)
    bias = (rng.standard_normal(cout) * 0.1).astype(np.float32)
    res = [rng.standard_normal((cout, b * b)).astype(np.float32) for b in bsz] if with_res else None
    return xs, w, bias, res


def _f64_bound_holds(outs, bsz, xs, w, bias, res, act):
    """the yardstick against the float64 direct convolution on the fp16-rounded operands: test_gpu_layers.py's bound"""
    ref = conv_ref([x.astype(np.float16).astype(np.float64) for x in xs], bsz, w.astype(np.float16).astype(np.float64), bias.astype(np.float64),
                   [r.astype(np.float16).astype(np.float64) for r in res] if res else None, 1, False, act, False)
    scale = max(float(np.abs(r).max()) for r in ref)
    for got, exp in zip(outs, ref):
        assert float(np.abs(got - exp).max()) <= 4e-3 * scale


# ---------------------------------------------------------------------------------------------------------------- 1. layer level
PW_SHAPES = [(32, 64), (96, 64), (256, 128), (128, 256), (384, 192), (192, 384)]
PW_BOARDS = [[2], [19], [9, 13, 19, 7, 19], [3] * 7, [19] * 3]


@pytest.mark.parametrize("cin,cout", PW_SHAPES, ids=[f"{a}x{b}" for a, b in PW_SHAPES])
def test_pointwise_kernel_has_the_generic_kernels_bits(cin, cout):
    """One chunk, an odd number of chunks, both directions of both production widths (three and six channel tiles); boards of 4
    pixels (less than a column tile), 22 tiles + 9 pixels, mixed, many tiny, several full.  Every cut -- the engine's, 1, 2, 5 pieces,
    one piece per column tile -- gives the generic kernel's fp16 outputs; nothing inside a board stays NaN."""
    for k, bsz in enumerate(PW_BOARDS):
        act, with_res = (5, True) if k % 2 == 0 else (1, False)
        xs, w, bias, res = _layer_tensors(bsz, cin, cout, with_res, seed=cin + cout + 11 * k)
        gen = _taps.ok(_taps.conv(True, bsz, cin, cout, 1, act, xs, w, bias, res))
        assert gen.kind == KIND_GENERIC, "the yardstick is the generic kernel"
        for pieces in (0, 1, 2, 5, (max(bsz) ** 2 + 15) // 16):
            t = _taps.ok(conv_pw(bsz, cin, cout, act, xs, w, bias, res, pieces))
            assert t.kind == KIND_PW
            for y, yg in zip(t.outs, gen.outs):
                assert not np.isnan(y).any(), (bsz, pieces, "an element of a board was not written")
                assert np.array_equal(y, yg), (cin, cout, bsz, pieces, float(np.abs(y - yg).max()))
        if (cin, cout) in ((256, 128), (192, 384)) and k == 2:
            _f64_bound_holds(gen.outs, bsz, xs, w, bias, res, act)


def test_pointwise_kernel_every_activation_with_and_without_residual():
    bsz = [19, 13]
    for act in range(8):
        for with_res in (True, False):
            xs, w, bias, res = _layer_tensors(bsz, 64, 128, with_res, seed=500 + 2 * act + with_res)
            gen = _taps.ok(_taps.conv(True, bsz, 64, 128, 1, act, xs, w, bias, res))
            assert gen.kind == KIND_GENERIC
            t = _taps.ok(conv_pw(bsz, 64, 128, act, xs, w, bias, res))
            assert t.kind == KIND_PW
            for y, yg in zip(t.outs, gen.outs):
                assert not np.isnan(y).any()
                assert np.array_equal(y, yg), (act, with_res)


# ---------------------------------------------------------------------------------------------------------------- 2. refusals
def test_pointwise_tap_refuses_what_the_route_does_not_cover():
    xs, w, bias, res = _layer_tensors([19, 9], 64, 128, True, seed=77)
    before = _taps.ok(conv_pw([19, 9], 64, 128, 5, xs, w, bias, res))
    x = [np.zeros((64, 361), np.float32)]
    assert conv_pw([19], 64, 96, 0, x, np.zeros(96 * 64, np.float32), None).rc == -1 and "64-channel" in _taps.last_error()
    x = [np.zeros((48, 361), np.float32)]
    assert conv_pw([19], 48, 64, 0, x, np.zeros(64 * 48, np.float32), None).rc == -1 and "32-channel" in _taps.last_error()
    # one piece of a 25x25 board is 40 column tiles: wider than the kernel holds (the engine's own choice cuts it in two)
    x = [np.zeros((64, 625), np.float32)]
    assert conv_pw([25], 64, 64, 0, x, np.zeros(64 * 64, np.float32), None, pieces=1, max_board=25).rc == -1 and "column tiles" in _taps.last_error()
    assert conv_pw([25], 64, 64, 0, x, np.zeros(64 * 64, np.float32), None, pieces=0, max_board=25).rc == 0
    after = _taps.ok(conv_pw([19, 9], 64, 128, 5, xs, w, bias, res))
    for a, b in zip(before.outs, after.outs):
        assert np.array_equal(a, b)


# ---------------------------------------------------------------------------------------------------------------- 3. whole networks
def _blocks(kind, inner=None, ffn=None):
    return [W.BlockSpec(kind, se=False, bottleneck_channels=inner, ffn_channels=ffn), W.BlockSpec(kind, se=True, bottleneck_channels=inner, ffn_channels=ffn)]


NETS = {  # name -> (channels, blocks, activation)
    "nested128-mish": (128, _blocks("NestedBottleneckBlock", 64), "mish"),
    "nested128-relu": (128, _blocks("NestedBottleneckBlock", 64), "relu"),
    "nested256-mish": (256, _blocks("NestedBottleneckBlock", 128), "mish"),
    "nested384-relu": (384, _blocks("NestedBottleneckBlock", 192), "relu"),
    "bottleneck256-relu": (256, _blocks("BottleneckBlock", 128), "relu"),
    "mixer128-mish": (128, _blocks("MixerBlock", ffn=192), "mish"),
}
BATCHES = [[19], [9], [19] * 5, [19, 9, 13, 9, 19, 13, 9, 9, 19, 13, 7, 19, 9, 13, 16]]  # the last: test_gpu_latency.py's BATCHES[3]


def net_path(name, workdir, nblocks=None):
    """the synthetic network `name` (nblocks: the first block kind repeated so often, every third with SE), written once"""
    channels, blocks, act = NETS[name]
    if nblocks:
        blocks = [W.BlockSpec(blocks[0].kind, se=(i % 3 == 2), bottleneck_channels=blocks[0].bottleneck_channels, ffn_channels=blocks[0].ffn_channels)
                  for i in range(nblocks)]
    path = os.path.join(workdir, f"pw_{name}_{len(blocks)}.bin")
    if not os.path.exists(path):
        W.write_weights(path, W.NetSpec(channels, blocks, 32, 32, activation=act), seed=33)
    return path


@pytest.mark.parametrize("name", list(NETS))
def test_network_has_the_bits_of_the_generic_kernel_in_both_kinds_of_context(name, tmp_weights_dir):
    """Two blocks (the second with SE) of every block kind with tower 1x1 layers, at the widths these networks have.  SAYURI_PW=0
    and the default give identical outputs; the default arm really launched conv_pw, the other none; in both kinds of context two
    positions per batch are within fp16_tol of the CPU oracle."""
    path = net_path(name, tmp_weights_dir)
    lib, net = _lib.hip(), PortNet(path)
    planes = [W.synthetic_planes(len(sizes), sizes, seed=6100 + k) for k, sizes in enumerate(BATCHES)]
    oracle = [{i: net.forward_raw(pl[i], sizes[i]) for i in {0, len(sizes) - 1}} for sizes, pl in zip(BATCHES, planes)]  # once, for both contexts
    for latency in (False, True):
        off, on = make_pipe(path, {"SAYURI_PW": "0"}, latency=latency), make_pipe(path, latency=latency)
        try:
            assert lib.sayuri_hip_latency_state(on.ctx(0)) == int(latency)
            for sizes, pl, exp in zip(BATCHES, planes, oracle):
                gr = grid_of(pl, sizes)
                a = hip_forward_raw(off.ctx(0), gr, sizes, B)
                assert lib.sayuri_hip_last_pw_launches(off.ctx(0)) == 0
                b = hip_forward_raw(on.ctx(0), gr, sizes, B)
                assert lib.sayuri_hip_last_pw_launches(on.ctx(0)) > 0, (name, latency, sizes)
                assert np.abs(a[0]).max() > 0
                for x, y, what in zip(a, b, OUTS):
                    assert np.array_equal(x, y), (name, latency, sizes, what, float(np.abs(x - y).max()))
                for i, e in exp.items():
                    within_oracle(e, b, i, sizes[i], (name, latency, sizes))
        finally:
            off.Destroy()
            on.Destroy()


@pytest.mark.parametrize("name", ["net_20b256", "net_6b96", "tiny_all"])
def test_no_network_of_the_existing_suite_takes_the_new_route(name, tmp_weights_dir):
    g = Golden(name, tmp_weights_dir)
    for latency in (False, True):
        pipe = make_pipe(g.weights_path, latency=latency, batch=16)
        try:
            sizes = [19, 9]
            hip_forward_raw(pipe.ctx(0), grid_of(W.synthetic_planes(2, sizes, seed=3), sizes), sizes, B)
            assert _lib.hip().sayuri_hip_last_pw_launches(pipe.ctx(0)) == 0, (name, latency)
        finally:
            pipe.Destroy()


# ---------------------------------------------------------------------------------------------------------------- 4. batch mates, tickets
@pytest.mark.parametrize("latency", [False, True], ids=["default", "latency"])
def test_a_position_does_not_depend_on_its_batch_mates_or_on_the_cut(latency, tmp_weights_dir):
    """test_gpu_latency.py's construction on the 256 / 128 nested network: a 9x9, a 13x13 and a 19x19 probe alone and inside four
    shuffled mixed batches -- the cut changes with the batch size --, and under SAYURI_PW_PIECES = 1, 2, 4."""
    path = net_path("nested256-mish", tmp_weights_dir)
    probes = {bs: W.synthetic_planes(1, bs, seed=4200 + bs)[0] for bs in (9, 13, 19)}
    rng = np.random.default_rng(77)
    alone = {}
    pipe = make_pipe(path, latency=latency)
    try:
        ctx = pipe.ctx(0)
        for bs, probe in probes.items():
            alone[bs] = [np.array(t[0]) for t in hip_forward_raw(ctx, grid_of([probe], [bs]), [bs], B)]
            assert np.abs(alone[bs][0]).max() > 0 and _lib.hip().sayuri_hip_last_pw_launches(ctx) > 0
            mates = [[19] * 5 + [9] * 7 + [13] * 3, [9] * 40, [19] * 30 + [13] * 3 + [9] * 2, [13] * 9 + [7] * 6 + [19] * 2 + [9] * 21 + [16] * 3]
            for k, sizes in enumerate(mates):
                sizes = list(sizes)
                rng.shuffle(sizes)
                at = int(rng.integers(0, len(sizes) + 1))
                sizes.insert(at, bs)
                planes = W.synthetic_planes(len(sizes), sizes, seed=900 + 10 * bs + k)
                planes[at] = probe
                got = [np.array(t[at]) for t in hip_forward_raw(ctx, grid_of(planes, sizes), sizes, B)]
                for a, b, what in zip(alone[bs], got, OUTS):
                    assert np.array_equal(a, b), (latency, bs, k, what, float(np.abs(a - b).max()))
    finally:
        pipe.Destroy()
    for pieces in (1, 2, 4):
        pipe = make_pipe(path, {"SAYURI_PW_PIECES": str(pieces)}, latency=latency)
        try:
            for bs, probe in probes.items():
                got = [np.array(t[0]) for t in hip_forward_raw(pipe.ctx(0), grid_of([probe], [bs]), [bs], B)]
                assert _lib.hip().sayuri_hip_last_pw_launches(pipe.ctx(0)) > 0
                for a, b, what in zip(alone[bs], got, OUTS):
                    assert np.array_equal(a, b), (latency, "pieces", pieces, bs, what)
        finally:
            pipe.Destroy()


@pytest.mark.parametrize("latency", [False, True], ids=["default", "latency"])
def test_packed_planes_and_two_tickets_on_the_nested_network(latency, tmp_weights_dir):
    """submit_packed gives the submit bits, and two tickets in flight (different batches, six rounds) give the solo bits."""
    path = net_path("nested256-mish", tmp_weights_dir)
    pool = Pool()
    rng = np.random.default_rng(11)
    pipe = make_pipe(path, latency=latency, batch=MAXB)
    pinned = Pinned()
    try:
        ctx = pipe.ctx(0)
        idxs = [pool.draw(rng, 3, "mixed"), pool.draw(rng, 11, "wild")]
        solo = [hip_forward_raw(ctx, pool.grid[i], pool.bsz[i], B) for i in idxs]
        assert _lib.hip().sayuri_hip_last_pw_launches(ctx) > 0
        for i, s in zip(idxs, solo):
            for a, b in zip(s, hip_forward_packed_raw(ctx, pool.rec[i], 37, pool.bsz[i], B)):
                assert np.array_equal(a, b)
        for packed in (False, True):
            tick = [pinned.submit(ctx, 0, pool, idxs[0], packed), pinned.submit(ctx, 1, pool, idxs[1], packed)]
            for r in range(6):
                i = r & 1
                got = pinned.wait(ctx, i, tick[i], len(idxs[i]))
                for a, b in zip(solo[i], got):
                    assert np.array_equal(a, b), (latency, packed, r)
                if r < 4:
                    tick[i] = pinned.submit(ctx, i, pool, idxs[i], packed)
    finally:
        pinned.close()
        pipe.Destroy()


# ---------------------------------------------------------------------------------------------------------------- 5. speed
def test_the_routing_rule_has_its_boundary_where_design_md_puts_it(tmp_weights_dir):
    """engine_plan.h, pw_pays: a tower 1x1 takes conv_pw.h when the piece rule gives a sample at least three pieces, 768 / (samples
    x channel tiles) >= 3, i.e. samples x channel tiles <= 256.  On the two-block 256 / 128 nested network (PRE_BTL: two channel
    tiles, POST_BTL: four) both layers of a block take it up to 64 boards, only PRE_BTL up to 128, none beyond; SAYURI_PW=1 takes it
    everywhere.  Same bits on both sides."""
    path = net_path("nested256-mish", tmp_weights_dir)
    lib = _lib.hip()
    rule, everywhere = make_pipe(path, batch=256), make_pipe(path, {"SAYURI_PW": "1"}, batch=256)
    try:
        full = grid_of(W.synthetic_planes(256, [19] * 256, seed=8), [19] * 256)
        for n, launches in ((64, 4), (65, 2), (128, 2), (129, 0), (256, 0)):
            sizes, gr = [19] * n, full[:n]
            a = hip_forward_raw(rule.ctx(0), gr, sizes, B)
            assert lib.sayuri_hip_last_pw_launches(rule.ctx(0)) == launches, (n, launches)
            b = hip_forward_raw(everywhere.ctx(0), gr, sizes, B)
            assert lib.sayuri_hip_last_pw_launches(everywhere.ctx(0)) == 4, n
            for x, y, what in zip(a, b, OUTS):
                assert np.array_equal(x, y), (n, what)
    finally:
        rule.Destroy()
        everywhere.Destroy()


SPEED_CASES = [("latency-1x19", True, [19]), ("default-64x19", False, [19] * 64)]


@pytest.mark.parametrize("label,latency,sizes", SPEED_CASES, ids=[c[0] for c in SPEED_CASES])
def test_pointwise_route_is_no_slower_than_the_generic_kernel(label, latency, sizes, tmp_weights_dir, capsys):
    """The 10-block 256 / 128 nested network.  Three contexts in one process, interleaved: SAYURI_PW=0 (the parent commit's kernel),
    SAYURI_PW=0 again, the default.  The gate: default <= first =0 arm x (1 + s), s = the relative difference of the two =0 arms in
    this same run -- no ratio is fixed in advance.  This test's own run on an MI355X printed (ms per forward; DESIGN.md Kernel 1i,
    profiles/r12_pw_conv.json): one 19x19 board, latency context 0.7999 / 0.8001 (spread 0.0003), default 0.4790, ratio 0.599;
    64 boards, default context 1.5747 / 1.5839 (spread 0.0058), default 1.3927, ratio 0.884; 20 conv_pw launches in both."""
    path = net_path("nested256-mish", tmp_weights_dir, nblocks=10)
    gr = grid_of(W.synthetic_planes(len(sizes), sizes, seed=1), sizes)
    pipes = {"off": make_pipe(path, {"SAYURI_PW": "0"}, latency=latency), "off2": make_pipe(path, {"SAYURI_PW": "0"}, latency=latency),
             "on": make_pipe(path, latency=latency)}
    try:
        t = device_ms(pipes, gr, sizes)
        launches = _lib.hip().sayuri_hip_last_pw_launches(pipes["on"].ctx(0))
        s = abs(t["off"] - t["off2"]) / t["off"]
        with capsys.disabled():
            print(f"\n[pw] nested 10b 256/128, {label}, device ms per forward: SAYURI_PW=0 {t['off']:.4f} / {t['off2']:.4f} (spread {s:.4f}), "
                  f"default {t['on']:.4f} (ratio {t['on'] / t['off']:.4f}, conv_pw launches {launches})")
        assert _lib.hip().sayuri_hip_last_pw_launches(pipes["off"].ctx(0)) == 0
        assert t["on"] <= t["off"] * (1 + s), (label, t)
    finally:
        for p in pipes.values():
            p.Destroy()
