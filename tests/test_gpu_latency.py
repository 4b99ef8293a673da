"""The latency context (include/sayuri_hip.h: sayuri_hip_create_ex with SAYURI_HIP_LATENCY; csrc/hip/conv_split.h): every fp16 3x3
tower convolution cut into many small workgroups, for the batches of 1 to 16 positions of a playing engine.

The split kernel accumulates in the board kernel's K order (32-channel chunk, kernel row, tap; bias first) and shares its
epilogue arithmetic, so the checks are on BITS, against code that existed before the feature:
  layer level  the conv_split tap == the conv tap (board kernel, kind 2), for every forced split
  whole net    a latency context == a default context created under SAYURI_SE_FUSED=0 SAYURI_SE_SPLIT=0 SAYURI_TOWER=0
The tolerance checks (float64 direct convolution, the goldens) reuse conv_ref of _kref.py, check / fp16_tol of _pipes.py and the bounds
of test_gpu_layers.py / test_gpu_net.py.
"""
import ctypes
import functools

import numpy as np
import pytest

import _pipes
import _taps
from _cases import LAYER_SHAPES
from _golden import Golden
from _kref import conv_ref
from _pipes import MAXB, Pinned, Pool, check, fp16_tol, grid_of, wrong_samples
from _taps import KIND_BOARD, KIND_SPLIT
from golden_specs import FIXTURES
from sayuri_amd import _lib
from sayuri_amd import weights as W
from sayuri_amd.pipe import hip_forward_packed_raw, hip_forward_raw

pytestmark = pytest.mark.gpu

B = 19
SEPARATE = {"SAYURI_SE_FUSED": "0", "SAYURI_SE_SPLIT": "0", "SAYURI_TOWER": "0"}
make_pipe = functools.partial(_pipes.make_pipe, batch=64)  # the batch of this module's pipes where a test names none


# ---------------------------------------------------------------------------------------------------------------- 1. layer level
VARIANTS = [  # act, with residual
    (5, True), (5, False), (1, True), (0, False), (0, True), (1, False),
]


def _layer_tensors(bsz, cin, cout, with_res, seed):
    rng = np.random.default_rng(seed)
    xs = [rng.standard_normal((cin, b * b)).astype(np.float32) for b in bsz]
    w = (rng.standard_normal((cout, cin, 3, 3)) / np.sqrt(9 * cin)).astype(np.float32)
    bias = (rng.standard_normal(cout) * 0.1).astype(np.float32)
    res = [rng.standard_normal((cout, b * b)).astype(np.float32) for b in bsz] if with_res else None
    return xs, w, bias, res


@pytest.mark.parametrize("case", LAYER_SHAPES, ids=[f"{c[1]}x{c[2]}n{len(c[0])}b{min(c[0])}" for c in LAYER_SHAPES])
def test_split_convolution_has_the_board_kernels_bits(case):
    """Every forced split (1, 2, 4 strips, one strip per row, the engine's choice) of every epilogue variant gives the fp16
    outputs of the one-workgroup-per-board kernel, and those are within test_gpu_layers.py's bound of the float64 convolution."""
    bsz, cin, cout = case
    for k, (act, with_res) in enumerate(VARIANTS):
        xs, w, bias, res = _layer_tensors(bsz, cin, cout, with_res, seed=cin + cout + 7 * k)
        board = _taps.ok(_taps.conv(True, bsz, cin, cout, 3, act, xs, w, bias, res))
        assert board.kind == KIND_BOARD, "the yardstick is the board kernel"
        for strips in (1, 2, 4, max(bsz), 0):
            t = _taps.ok(_taps.conv_split(bsz, cin, cout, act, xs, w, bias, res, strips))
            assert t.kind == KIND_SPLIT
            for y, yb in zip(t.outs, board.outs):
                assert np.array_equal(y, yb), (case, act, with_res, strips, float(np.nanmax(np.abs(y - yb))))
        # ... and the float64 direct convolution on the fp16-rounded operands, with test_gpu_layers.py's fp16 tolerance
        ref = conv_ref([x.astype(np.float16).astype(np.float64) for x in xs], bsz, w.astype(np.float16).astype(np.float64),
                       bias.astype(np.float64), [r.astype(np.float16).astype(np.float64) for r in res] if res else None, 3, False, act, False)
        scale = max(float(np.abs(r).max()) for r in ref)
        for got, exp in zip(board.outs, ref):
            assert float(np.abs(got - exp).max()) <= 4e-3 * scale


def test_split_convolution_every_activation_and_post_residual_layer():
    """All eight activations with the residual added in front of them (the tower's post-residual layers), one strip per two rows."""
    bsz = [19, 13]
    for act in range(8):
        xs, w, bias, res = _layer_tensors(bsz, 64, 128, True, seed=300 + act)
        board = _taps.ok(_taps.conv(True, bsz, 64, 128, 3, act, xs, w, bias, res))
        assert board.kind == KIND_BOARD
        t = _taps.ok(_taps.conv_split(bsz, 64, 128, act, xs, w, bias, res, strips=10, channel_tiles=2))
        for y, yb in zip(t.outs, board.outs):
            assert np.array_equal(y, yb), act


def test_split_tap_refuses_what_the_kernel_does_not_cover():
    x, w = [np.zeros((96, 361), np.float32)], np.zeros(96 * 96 * 9, np.float32)
    assert _taps.conv_split([19], 96, 96, 0, x, w, None).rc == -1 and "64-channel" in _taps.last_error()   # 96 weight rows: the layer keeps the default route
    x, w = [np.zeros((64, 361), np.float32)], np.zeros(128 * 64 * 9, np.float32)
    assert _taps.conv_split([19], 64, 128, 0, x, w, None, channel_tiles=3).rc == -1 and "channel tiles" in _taps.last_error()


# ---------------------------------------------------------------------------------------------------------------- 2. whole net
BATCHES = [[9], [13], [19], [19, 9, 13, 9, 19, 13, 9, 9, 19, 13, 7, 19, 9, 13, 16]]


@pytest.mark.parametrize("name", ["net_20b256", "net_40b384", "net_6b96"])
def test_latency_context_has_the_bits_of_the_separate_se_default_context(name, tmp_weights_dir):
    """Lone boards of 9, 13, 19 and a mixed batch of 15.  net_6b96 (96 channels: no whole 64-channel tiles) checks the layers
    that keep their route."""
    g = Golden(name, tmp_weights_dir)
    lib = _lib.hip()
    ref = make_pipe(g.weights_path, SEPARATE)
    lat = make_pipe(g.weights_path, latency=True)
    try:
        assert lib.sayuri_hip_latency_state(lat.ctx(0)) == 1 and lib.sayuri_hip_latency_state(ref.ctx(0)) == 0
        assert lib.sayuri_hip_tower_state(lat.ctx(0)) == 0 and lib.sayuri_hip_tower_state(ref.ctx(0)) == 0
        for k, sizes in enumerate(BATCHES):
            gr = grid_of(W.synthetic_planes(len(sizes), sizes, seed=5100 + k), sizes)
            a = hip_forward_raw(ref.ctx(0), gr, sizes, B)
            b = hip_forward_raw(lat.ctx(0), gr, sizes, B)
            assert np.abs(a[0]).max() > 0
            for x, y, what in zip(a, b, ("prob", "pass", "misc", "own")):
                assert np.array_equal(x, y), (name, sizes, what, float(np.abs(x - y).max()))
    finally:
        ref.Destroy()
        lat.Destroy()


# ---------------------------------------------------------------------------------------------------------------- 3. goldens
@pytest.mark.parametrize("name", [fx["name"] for fx in FIXTURES if fx["name"].startswith("tiny")] +
                         ["net_20b256", "net_40b384"])
def test_latency_context_golden_parity(name, tmp_weights_dir):
    g = Golden(name, tmp_weights_dir)
    cases = [(g.planes(c), c["board_size"], c["offset"], g.expected(c)) for c in g.cases if c.get("winograd", 1) == 1]
    pipe = make_pipe(g.weights_path, latency=True, batch=16)
    try:
        check(pipe, cases, fp16_tol, name + "-latency")
    finally:
        pipe.Destroy()


# ---------------------------------------------------------------------------------------------------------------- 4. batch mates
@pytest.mark.parametrize("name", ["net_20b256", "net_40b384"])
def test_a_position_does_not_depend_on_its_batch_mates_in_latency_mode(name, tmp_weights_dir):
    """The construction of test_gpu_net.py's test of that name, in a latency context -- whose split changes with the batch size
    -- and across forced splits: SAYURI_LATENCY_SPLIT = 1, 2, 4 give the bits of the engine's choice."""
    g = Golden(name, tmp_weights_dir)
    probes = {bs: W.synthetic_planes(1, bs, seed=4200 + bs)[0] for bs in (9, 13, 19)}
    rng = np.random.default_rng(77)
    alone = {}
    pipe = make_pipe(g.weights_path, latency=True)
    try:
        ctx = pipe.ctx(0)
        for bs, probe in probes.items():
            alone[bs] = [np.array(t[0]) for t in hip_forward_raw(ctx, grid_of([probe], [bs]), [bs], B)]
            assert np.abs(alone[bs][0]).max() > 0
            mates = [[19] * 5 + [9] * 7 + [13] * 3, [9] * 40, [19] * 30 + [13] * 3 + [9] * 2, [13] * 9 + [7] * 6 + [19] * 2 + [9] * 21 + [16] * 3]
            for k, sizes in enumerate(mates):
                sizes = list(sizes)
                rng.shuffle(sizes)
                at = int(rng.integers(0, len(sizes) + 1))
                sizes.insert(at, bs)
                planes = W.synthetic_planes(len(sizes), sizes, seed=900 + 10 * bs + k)
                planes[at] = probe
                got = [np.array(t[at]) for t in hip_forward_raw(ctx, grid_of(planes, sizes), sizes, B)]
                for a, b, what in zip(alone[bs], got, ("prob", "pass", "misc", "own")):
                    assert np.array_equal(a, b), (name, bs, k, what, float(np.abs(a - b).max()))
    finally:
        pipe.Destroy()
    for split in (1, 2, 4):
        pipe = make_pipe(g.weights_path, {"SAYURI_LATENCY_SPLIT": str(split)}, latency=True)
        try:
            for bs, probe in probes.items():
                got = [np.array(t[0]) for t in hip_forward_raw(pipe.ctx(0), grid_of([probe], [bs]), [bs], B)]
                for a, b, what in zip(alone[bs], got, ("prob", "pass", "misc", "own")):
                    assert np.array_equal(a, b), (name, "split", split, bs, what)
        finally:
            pipe.Destroy()


# ---------------------------------------------------------------------------------------------------------------- 5. packed, tickets
def test_packed_planes_and_two_tickets_in_latency_mode(tmp_weights_dir):
    """submit_packed gives the submit bits, and two tickets in flight (different batches, six rounds) give the solo bits."""
    g = Golden("net_20b256", tmp_weights_dir)
    pool = Pool()
    rng = np.random.default_rng(11)
    pipe = make_pipe(g.weights_path, latency=True, batch=MAXB)
    pinned = Pinned()
    try:
        ctx = pipe.ctx(0)
        idxs = [pool.draw(rng, 3, "mixed"), pool.draw(rng, 11, "wild")]
        solo = [hip_forward_raw(ctx, pool.grid[i], pool.bsz[i], B) for i in idxs]
        for i, s in zip(idxs, solo):
            for a, b in zip(s, hip_forward_packed_raw(ctx, pool.rec[i], 37, pool.bsz[i], B)):
                assert np.array_equal(a, b)
        for packed in (False, True):
            tick = [pinned.submit(ctx, 0, pool, idxs[0], packed), pinned.submit(ctx, 1, pool, idxs[1], packed)]
            for r in range(6):
                i = r & 1
                got = pinned.wait(ctx, i, tick[i], len(idxs[i]))
                for a, b in zip(solo[i], got):
                    assert np.array_equal(a, b), (packed, r)
                if r < 4:
                    tick[i] = pinned.submit(ctx, i, pool, idxs[i], packed)
    finally:
        pinned.close()
        pipe.Destroy()


# ---------------------------------------------------------------------------------------------------------------- 6. default untouched
def test_default_context_is_untouched_and_flags_are_checked(tmp_weights_dir, monkeypatch):
    g = Golden("net_20b256", tmp_weights_dir)
    lib = _lib.hip()
    plain = make_pipe(g.weights_path)
    try:
        assert lib.sayuri_hip_latency_state(plain.ctx(0)) == 0 and lib.sayuri_hip_tower_state(plain.ctx(0)) == 1
    finally:
        plain.Destroy()
    lat = make_pipe(g.weights_path, latency=True)
    try:
        assert lib.sayuri_hip_latency_state(lat.ctx(0)) == 1 and lib.sayuri_hip_tower_state(lat.ctx(0)) == 0
    finally:
        lat.Destroy()
    env = make_pipe(g.weights_path, {"SAYURI_LATENCY": "1"})   # the switch for callers that cannot pass a flag
    try:
        assert lib.sayuri_hip_latency_state(env.ctx(0)) == 1
    finally:
        env.Destroy()
    with pytest.raises(RuntimeError, match="fp16 engine"):
        make_pipe(g.weights_path, latency=True, fp16=False)
    # ... and at the C-ABI itself: NULL and a message
    blk = (_lib.BlockDesc * 1)(_lib.BlockDesc(1, 0, 0, 0, 0, 0))
    d = _lib.NetDesc(5, 43, 64, 1, 16, 16, 5, 5, 1, 15, 5, 0, 0, blk)
    assert lib.sayuri_hip_create_ex(0, ctypes.byref(d), 4, 19, 0, 1) is None
    assert b"fp16" in lib.sayuri_hip_last_error()


# ---------------------------------------------------------------------------------------------------------------- 7. faster
def test_latency_context_needs_at_most_half_the_device_time_of_a_lone_board(tmp_weights_dir, capsys):
    """net_20b256, one 19x19 position, inputs resident: device time per forward (sayuri_hip_time_runs) of a latency context
    against a default context in the same process, interleaved, 3 rounds of 200 forwards, medians.  The floor of one half is
    reasoned, not measured: the split puts at least 8x the CUs on every layer's MFMA work, which leaves room for the launch
    overhead of about a hundred small kernels and for box noise, while a broken or mis-routed kernel (ratio near 1) fails.
    Measured on an MI355X (profiles/r07_latency_small_batch.json; DESIGN.md Kernel 1e): default 1.795 ms, latency 0.639 ms,
    ratio 0.356; this test's own run printed 1.792 / 0.636 / 0.355."""
    g = Golden("net_20b256", tmp_weights_dir)
    lib = _lib.hip()
    gr = grid_of(W.synthetic_planes(1, [19], seed=1), [19])
    pipes = {"default": make_pipe(g.weights_path), "latency": make_pipe(g.weights_path, latency=True)}
    try:
        times = {k: [] for k in pipes}
        bs = np.asarray([19], np.int32)
        for k, p in pipes.items():
            assert lib.sayuri_hip_upload(p.ctx(0), 1, _lib.fp(gr), bs.ctypes.data_as(_lib.c_int_p)) == 0
            ms = ctypes.c_float(0)
            assert lib.sayuri_hip_time_runs(p.ctx(0), 50, ctypes.byref(ms)) == 0   # warm-up
        for _ in range(3):
            for k, p in pipes.items():
                ms = ctypes.c_float(0)
                assert lib.sayuri_hip_time_runs(p.ctx(0), 200, ctypes.byref(ms)) == 0, lib.sayuri_hip_last_error()
                times[k].append(ms.value / 200)
        d, l = float(np.median(times["default"])), float(np.median(times["latency"]))
        with capsys.disabled():
            print(f"\n[latency] net_20b256, one 19x19 board, device ms per forward: default {d:.4f}, latency {l:.4f}, ratio {l / d:.3f}")
        assert l <= 0.5 * d, (d, l)
    finally:
        for p in pipes.values():
            p.Destroy()


# ---------------------------------------------------------------------------------------------------------------- 8. fuzz arm
def test_latency_bit_identity_fuzz(tmp_weights_dir, capsys):
    """20 scenarios drawn the way test_gpu_fuzz.py draws them -- network, 1..64 positions, uniform / mixed / wild sizes, one or two
    tickets in flight, packed or fp32 planes -- in a latency context, every sample against the bits of its position in the
    separate-SE default context."""
    pool = Pool()
    rng = np.random.default_rng(20261016)
    nets = ["net_20b256", "net_40b384", "net_6b96"]
    paths = {n: Golden(n, tmp_weights_dir).weights_path for n in nets}
    refs, pipes = {}, {}
    pinned = Pinned()
    failures, ran = [], []
    try:
        for k in range(20):
            name = str(rng.choice(nets, p=[0.45, 0.35, 0.2]))
            sc = dict(k=k, net=name, n=int(rng.integers(1, 65)), mix=str(rng.choice(["uniform19", "mixed", "mixed", "wild"])),
                      tickets=int(rng.integers(1, 3)), packed=bool(rng.integers(0, 2)))
            if name not in refs:
                ref = make_pipe(paths[name], SEPARATE, batch=MAXB)
                try:
                    outs = [hip_forward_raw(ref.ctx(0), pool.grid[lo:lo + 96], pool.bsz[lo:lo + 96], B) for lo in range(0, len(pool.bsz), 96)]
                finally:
                    ref.Destroy()
                refs[name] = tuple(np.concatenate([o[j] for o in outs]) for j in range(4))
                pipes[name] = make_pipe(paths[name], latency=True, batch=MAXB)
            ctx = pipes[name].ctx(0)
            batches = []
            if sc["tickets"] == 1:
                for _ in range(2):
                    idx = pool.draw(rng, sc["n"], sc["mix"])
                    got = (hip_forward_packed_raw(ctx, pool.rec[idx], 37, pool.bsz[idx], B) if sc["packed"] else
                           hip_forward_raw(ctx, pool.grid[idx], pool.bsz[idx], B))
                    batches.append((idx, got))
            else:
                n2, mix2 = int(rng.integers(1, 65)), str(rng.choice(["uniform19", "mixed", "wild"]))
                idxs = [pool.draw(rng, sc["n"], sc["mix"]), pool.draw(rng, n2, mix2)]
                tick = [pinned.submit(ctx, 0, pool, idxs[0], sc["packed"]), pinned.submit(ctx, 1, pool, idxs[1], sc["packed"])]
                for r in range(6):
                    i = r & 1
                    batches.append((idxs[i], pinned.wait(ctx, i, tick[i], len(idxs[i]))))
                    if r < 4:
                        idxs[i] = pool.draw(rng, len(idxs[i]), sc["mix"] if i == 0 else mix2)
                        tick[i] = pinned.submit(ctx, i, pool, idxs[i], sc["packed"])
            ran.append(sc)
            for idx, got in batches:
                bad = wrong_samples(refs[name], got, idx)
                if len(bad):
                    failures.append((dict(sc), bad.tolist()[:16], len(idx), len(bad)))
    finally:
        pinned.close()
        for p in pipes.values():
            p.Destroy()
    with capsys.disabled():
        print(f"\n[latency fuzz] {len(ran)} scenarios, two tickets in {sum(1 for s in ran if s['tickets'] == 2)}, "
              f"packed {sum(1 for s in ran if s['packed'])}; wrong batches: {len(failures)}")
    assert not failures, failures[:5]
    assert any(s["tickets"] == 2 for s in ran) and any(s["packed"] for s in ran) and len({s["net"] for s in ran}) == 3
