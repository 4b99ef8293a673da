"""The latency context (include/sayuri_hip.h: sayuri_hip_create_ex with SAYURI_HIP_LATENCY; csrc/hip/conv_split.h): every fp16 3x3
tower convolution cut into many small workgroups, for the batches of 1 to 16 positions of a playing engine.

The split kernel accumulates in the board kernel's K order (32-channel chunk, kernel row, tap; bias first) and shares its
epilogue arithmetic, so the checks are on BITS, against code that existed before the feature:
  layer level  sayuri_hip_test_conv_split == sayuri_hip_test_conv (board kernel, kind 2), for every forced split
  whole net    a latency context == a default context created under SAYURI_SE_FUSED=0 SAYURI_SE_SPLIT=0 SAYURI_TOWER=0
The tolerance checks (float64 direct convolution, the goldens) reuse the helpers and bounds of test_gpu_layers.py / test_gpu_net.py.
"""
import ctypes
import os

import numpy as np
import pytest

import test_gpu_fuzz as FZ
from _golden import Golden
from golden_specs import FIXTURES
from sayuri_amd import _lib
from sayuri_amd import weights as W
from sayuri_amd.pipe import HipForwardPipe, hip_forward_packed_raw, hip_forward_raw
from test_gpu_layers import KIND_BOARD, conv_ref
from test_gpu_net import check, fp16_tol

pytestmark = pytest.mark.gpu

B = 19
KIND_SPLIT = 4
SEPARATE = {"SAYURI_SE_FUSED": "0", "SAYURI_SE_SPLIT": "0", "SAYURI_TOWER": "0"}
SWITCHES = tuple(SEPARATE) + ("SAYURI_LATENCY", "SAYURI_LATENCY_SPLIT", "SAYURI_CHAINS", "SAYURI_CONV")


def make_pipe(path, env=None, latency=False, batch=64, fp16=True):
    """A pipe created under exactly `env` of the engine's switches (they are read once, at creation)."""
    keep = {k: os.environ.get(k) for k in SWITCHES}
    for k in SWITCHES:
        os.environ.pop(k, None)
    os.environ.update(env or {})
    try:
        return HipForwardPipe(path, board_size=B, batch_size=batch, fp16=fp16, latency=latency)
    finally:
        for k, v in keep.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v



def grid_of(planes, bsz):
    gr = np.zeros((len(bsz), 43, B * B), np.float32)
    for i, (p, bs) in enumerate(zip(planes, bsz)):
        gr[i].reshape(43, B, B)[:, :bs, :bs] = p.reshape(43, bs, bs)
    return gr


# ---------------------------------------------------------------------------------------------------------------- 1. layer level
LAYER_SHAPES = [
    # bsz, cin, cout
    ([19], 256, 256),
    ([19, 19, 19], 128, 128),
    ([19, 13], 384, 384),
    ([9], 256, 256),
    ([13], 128, 384),
    ([19, 19, 13, 13, 9, 9, 9, 9, 19, 13], 256, 256),   # mixed sizes: boards that share a board tile are cut per sample
    ([13, 9, 9, 19, 13, 9], 43, 128),                   # an input convolution (cin padded to 64: two chunks)
    ([9] * 9, 128, 256),
]
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
    lib = _lib.hip()
    n = len(bsz)
    bs_arr = np.asarray(bsz, np.int32)
    for k, (act, with_res) in enumerate(VARIANTS):
        xs, w, bias, res = _layer_tensors(bsz, cin, cout, with_res, seed=cin + cout + 7 * k)
        xcat = np.concatenate([x.ravel() for x in xs])
        rcat = np.concatenate([r.ravel() for r in res]) if res else None
        board = np.zeros(sum(cout * b * b for b in bsz), np.float32)
        rc = lib.sayuri_hip_test_conv(0, 1, n, bs_arr.ctypes.data_as(_lib.c_int_p), B, cin, cout, 3, 0, act, 0, _lib.fp(xcat), _lib.fp(w.ravel()),
                                      _lib.fp(bias), _lib.fp(rcat) if res else None, _lib.fp(board))
        assert rc == 0, lib.sayuri_hip_last_error().decode()
        assert lib.sayuri_hip_test_last_conv_kind() == KIND_BOARD, "the yardstick is the board kernel"
        for strips in (1, 2, 4, max(bsz), 0):
            y = np.full_like(board, np.nan)
            rc = lib.sayuri_hip_test_conv_split(0, n, bs_arr.ctypes.data_as(_lib.c_int_p), B, cin, cout, act, _lib.fp(xcat), _lib.fp(w.ravel()),
                                                _lib.fp(bias), _lib.fp(rcat) if res else None, _lib.fp(y), 0, strips)
            assert rc == 0, lib.sayuri_hip_last_error().decode()
            assert lib.sayuri_hip_test_last_conv_kind() == KIND_SPLIT
            assert np.array_equal(y, board), (case, act, with_res, strips, float(np.nanmax(np.abs(y - board))))
        # ... and the float64 direct convolution on the fp16-rounded operands, with test_gpu_layers.py's fp16 tolerance
        ref = conv_ref([x.astype(np.float16).astype(np.float64) for x in xs], bsz, w.astype(np.float16).astype(np.float64),
                       bias.astype(np.float64), [r.astype(np.float16).astype(np.float64) for r in res] if res else None, 3, False, act, False)
        scale = max(float(np.abs(r).max()) for r in ref)
        off = 0
        for i, b in enumerate(bsz):
            got = board[off:off + cout * b * b].reshape(cout, b * b)
            off += cout * b * b
            assert float(np.abs(got - ref[i]).max()) <= 4e-3 * scale


def test_split_convolution_every_activation_and_post_residual_layer():
    """All eight activations with the residual added in front of them (the tower's post-residual layers), one strip per two rows."""
    lib = _lib.hip()
    bsz = [19, 13]
    bs_arr = np.asarray(bsz, np.int32)
    for act in range(8):
        xs, w, bias, res = _layer_tensors(bsz, 64, 128, True, seed=300 + act)
        xcat, rcat = np.concatenate([x.ravel() for x in xs]), np.concatenate([r.ravel() for r in res])
        out = []
        for split in (None, 10):
            y = np.zeros(sum(128 * b * b for b in bsz), np.float32)
            if split is None:
                rc = lib.sayuri_hip_test_conv(0, 1, 2, bs_arr.ctypes.data_as(_lib.c_int_p), B, 64, 128, 3, 0, act, 0, _lib.fp(xcat), _lib.fp(w.ravel()),
                                              _lib.fp(bias), _lib.fp(rcat), _lib.fp(y))
                assert rc == 0 and lib.sayuri_hip_test_last_conv_kind() == KIND_BOARD
            else:
                rc = lib.sayuri_hip_test_conv_split(0, 2, bs_arr.ctypes.data_as(_lib.c_int_p), B, 64, 128, act, _lib.fp(xcat), _lib.fp(w.ravel()),
                                                    _lib.fp(bias), _lib.fp(rcat), _lib.fp(y), 2, split)
                assert rc == 0, lib.sayuri_hip_last_error().decode()
            out.append(y)
        assert np.array_equal(out[0], out[1]), act


def test_split_tap_refuses_what_the_kernel_does_not_cover():
    lib = _lib.hip()
    bs_arr = np.asarray([19], np.int32)
    x, w, y = np.zeros(96 * 361, np.float32), np.zeros(96 * 96 * 9, np.float32), np.zeros(96 * 361, np.float32)
    rc = lib.sayuri_hip_test_conv_split(0, 1, bs_arr.ctypes.data_as(_lib.c_int_p), B, 96, 96, 0, _lib.fp(x), _lib.fp(w), None, None, _lib.fp(y), 0, 0)
    assert rc == -1 and b"64-channel" in lib.sayuri_hip_last_error()   # 96 weight rows: the layer keeps the default route
    x, w, y = np.zeros(64 * 361, np.float32), np.zeros(128 * 64 * 9, np.float32), np.zeros(128 * 361, np.float32)
    rc = lib.sayuri_hip_test_conv_split(0, 1, bs_arr.ctypes.data_as(_lib.c_int_p), B, 64, 128, 0, _lib.fp(x), _lib.fp(w), None, None, _lib.fp(y), 3, 0)
    assert rc == -1 and b"channel tiles" in lib.sayuri_hip_last_error()


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
    pool = FZ.Pool()
    rng = np.random.default_rng(11)
    pipe = make_pipe(g.weights_path, latency=True, batch=FZ.MAXB)
    pinned = FZ.Pinned()
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
    pool = FZ.Pool()
    rng = np.random.default_rng(20261016)
    nets = ["net_20b256", "net_40b384", "net_6b96"]
    paths = {n: Golden(n, tmp_weights_dir).weights_path for n in nets}
    refs, pipes = {}, {}
    pinned = FZ.Pinned()
    failures, ran = [], []
    try:
        for k in range(20):
            name = str(rng.choice(nets, p=[0.45, 0.35, 0.2]))
            sc = dict(k=k, net=name, n=int(rng.integers(1, 65)), mix=str(rng.choice(["uniform19", "mixed", "mixed", "wild"])),
                      tickets=int(rng.integers(1, 3)), packed=bool(rng.integers(0, 2)))
            if name not in refs:
                ref = make_pipe(paths[name], SEPARATE, batch=FZ.MAXB)
                try:
                    outs = [hip_forward_raw(ref.ctx(0), pool.grid[lo:lo + 96], pool.bsz[lo:lo + 96], B) for lo in range(0, len(pool.bsz), 96)]
                finally:
                    ref.Destroy()
                refs[name] = tuple(np.concatenate([o[j] for o in outs]) for j in range(4))
                pipes[name] = make_pipe(paths[name], latency=True, batch=FZ.MAXB)
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
                bad = FZ.wrong_samples(refs[name], got, idx)
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
