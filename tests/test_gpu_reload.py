"""Live weight reload on the GPU (include/sayuri_hip.h: sayuri_hip_reload_*; HipForwardPipe::Reload): a new network of the same
architecture goes into a context that keeps serving forwards, between two forwards, and the old one's memory is given back.

Networks "A" and "B" are one spec under two seeds.  "Solo bits" are the outputs of a fresh pipe created on that file: a reloaded
context must give the new network's solo bits, bit for bit, in every kernel family whose weight images differ, and a forward that
was in flight across the commit the bits of the network it was sent to."""
import ctypes
import os
import threading

import numpy as np
import pytest

from _pipes import B, grid_of, make_pipe
from sayuri_amd import _lib, hipraw
from sayuri_amd import weights as W
from sayuri_amd.pipe import Weights

pytestmark = pytest.mark.gpu

BSZ = (19, 9, 13, 19, 2)
RES3 = lambda: W.NetSpec.residual(3, 128, 32)   # an SE unit in block 3


def blocks_of(kind, **kw):
    return [W.BlockSpec(kind, se=False, **kw), W.BlockSpec(kind, se=True, **kw)]


FAMILIES = {
    # name: (spec, pipe arguments, the persistent tower launch is what runs)
    "res3x128": (RES3, {}, True),
    "res3x128-latency": (RES3, {"latency": True}, False),
    "res2x256": (lambda: W.NetSpec.residual(2, 256, 32), {}, True),
    "nested2x128_64": (lambda: W.NetSpec(128, blocks_of("NestedBottleneckBlock", bottleneck_channels=64), 32, 32), {}, None),
    "mixer2x128-replk": (lambda: W.NetSpec(128, blocks_of("MixerBlock", ffn_channels=192), 32, 32, policy_head="RepLK"), {}, None),
    "res2x16-fp32": (lambda: W.NetSpec.residual(2, 16, 8), {"fp16": False}, False),
}


def same_bits(a, b):
    return len(a) == len(b) and all(x.shape == y.shape and np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(a, b))


def write_pair(tmp, spec, name="net"):
    a, b = str(tmp / f"{name}_a.bin"), str(tmp / f"{name}_b.bin")
    W.write_weights(a, spec, seed=11)
    W.write_weights(b, spec, seed=12)
    return a, b


def solo(path, planes, bsz, **kw):
    p = make_pipe(path, batch=64, **kw)
    try:
        return p.Forward(planes, list(bsz))
    finally:
        p.Destroy()


# ---------------------------------------------------------------- 1. a reloaded context is the new network, bit for bit
@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_reloaded_context_gives_the_new_networks_solo_bits(tmp_path, family):
    spec, kw, tower = FAMILIES[family]
    a, b = write_pair(tmp_path, spec())
    planes = W.synthetic_planes(len(BSZ), list(BSZ), seed=5)
    sa, sb = solo(a, planes, BSZ, **kw), solo(b, planes, BSZ, **kw)
    assert not same_bits(sa, sb), "two seeds, one answer: the test could not tell the networks apart"
    lib = _lib.hip()
    pipe = make_pipe(a, batch=64, **kw)
    try:
        assert pipe.AcceptsReload() and pipe.weights_generation() == 0
        if tower is not None:
            assert lib.sayuri_hip_tower_state(pipe.ctx(0)) == (1 if tower else 0)
        assert same_bits(pipe.Forward(planes, list(BSZ)), sa)
        pipe.Reload(b)
        assert pipe.weights_generation() == 1
        assert same_bits(pipe.Forward(planes, list(BSZ)), sb), "after the reload the context is not network B"
        assert same_bits(pipe.BatchForward(planes, list(BSZ)), solo_batch(b, planes, kw)), "blocking forward after the reload"
        pipe.Reload(a)
        assert pipe.weights_generation() == 2
        assert same_bits(pipe.Forward(planes, list(BSZ)), sa), "reloading A again does not give A"
    finally:
        pipe.Destroy()


def solo_batch(path, planes, kw):
    p = make_pipe(path, batch=64, **kw)
    try:
        return p.BatchForward(planes, list(BSZ))
    finally:
        p.Destroy()


# ---------------------------------------------------------------- raw C-ABI helpers (residual networks)
L_INPUT, L_P_HD, L_P_INTER, L_PROB, L_PASS, L_V_HD, L_V_INTER, L_V_OWN, L_V_MISC, L_BLOCK0 = 0, 1, 4, 5, 6, 7, 8, 9, 10, 16
S_CONV1, S_CONV2, S_SQUEEZE, S_EXCITE = 0, 1, 7, 8


def residual_layers(w):
    """(layer id, tensor name) of every layer of a residual network, as HipForwardPipe loads them"""
    out = [(L_INPUT, "input_conv")]
    for i in range(w.info[2]):
        out += [(L_BLOCK0 + 16 * i + S_CONV1, f"tower.{i}.conv1"), (L_BLOCK0 + 16 * i + S_CONV2, f"tower.{i}.conv2")]
        if w.block_info(i)[1]:
            out += [(L_BLOCK0 + 16 * i + S_SQUEEZE, f"tower.{i}.squeeze"), (L_BLOCK0 + 16 * i + S_EXCITE, f"tower.{i}.excite")]
    return out + [(L_P_HD, "p_hd_conv"), (L_P_INTER, "p_inter_fc"), (L_PROB, "prob_conv"), (L_PASS, "pass_fc"), (L_V_HD, "v_hd_conv"),
                  (L_V_INTER, "v_inter_fc"), (L_V_OWN, "v_ownership"), (L_V_MISC, "v_misc")]


def netdesc(w, **change):
    """the sayuri_hip_netdesc of a loaded residual network; change: netdesc fields, or blocks = {index: {field: value}}"""
    n = w.info[2]
    blocks = (_lib.BlockDesc * (n + 1))()
    for i in range(n):
        t, se, se_size, btl, ffn = w.block_info(i)
        blocks[i] = _lib.BlockDesc(t, se, se_size, btl, ffn, 0)
    for i, fields in change.pop("blocks", {}).items():
        for k, v in fields.items():
            setattr(blocks[i], k, v)
    d = _lib.NetDesc(w.info[0], w.info[1], w.info[3], n, w.info[4], w.info[5], w.info[6], w.info[7], w.info[8], w.info[9], w.info[10],
                     w.info[11], 0, ctypes.cast(blocks, ctypes.POINTER(_lib.BlockDesc)))
    for k, v in change.items():
        setattr(d, k, v)
    return d, blocks


def load_tensors(ctx, w, skip=None):
    lib = _lib.hip()
    for lid, name in residual_layers(w):
        for kind, suffix in ((0, ".w"), (1, ".b")):
            if (lid, kind) == skip:
                continue
            t = w.tensor(name + suffix)
            assert t is not None and t.size, name + suffix
            assert lib.sayuri_hip_load_tensor(ctx, lid, kind, _lib.fp(t), t.size) == 0, lib.sayuri_hip_last_error()


def stage(ctx, path):
    """begin + every tensor + prepare of the network in `path`, through the C-ABI"""
    lib, w = _lib.hip(), Weights(path)
    d, keep = netdesc(w)
    assert lib.sayuri_hip_reload_begin(ctx, ctypes.byref(d)) == 0, lib.sayuri_hip_last_error()
    load_tensors(ctx, w)
    assert lib.sayuri_hip_reload_prepare(ctx) == 0, lib.sayuri_hip_last_error()
    w.close()


# ---------------------------------------------------------------- 2. a forward in flight across the commit keeps its network
N_FLIGHT = 64


@pytest.fixture(scope="module")
def res3(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("reload_res3")
    a, b = write_pair(tmp, RES3())
    planes = W.synthetic_planes(N_FLIGHT, [B] * N_FLIGHT, seed=8)
    gr = grid_of(planes, [B] * N_FLIGHT)
    raw = {}
    for key, path in (("a", a), ("b", b)):
        p = make_pipe(path, batch=N_FLIGHT)
        try:
            raw[key] = hipraw.hip_forward_raw(p.ctx(0), gr, [B] * N_FLIGHT, B)
        finally:
            p.Destroy()
    assert not same_bits(raw["a"], raw["b"])
    return {"a": a, "b": b, "grid": gr, "raw": raw}


@pytest.mark.parametrize("order", ["reload_between", "prepared_first"])
def test_forward_in_flight_across_the_commit_keeps_its_network(res3, order):
    lib = _lib.hip()
    pipe = make_pipe(res3["a"], batch=N_FLIGHT)
    sets = [hipraw.PinnedSet(N_FLIGHT, B, 43 * B * B) for _ in range(2)]
    try:
        ctx = pipe.ctx(0)
        for s in sets:
            s.planes[:] = res3["grid"].ravel()
            s.bsz[:] = B
        if order == "prepared_first":
            stage(ctx, res3["b"])
        t0 = hipraw.submit(ctx, sets[0], N_FLIGHT)
        if order == "prepared_first":
            assert lib.sayuri_hip_reload_commit(ctx) == 1, lib.sayuri_hip_last_error()
        else:
            pipe.Reload(res3["b"])
        t1 = hipraw.submit(ctx, sets[1], N_FLIGHT)
        hipraw.wait(ctx, t0)
        hipraw.wait(ctx, t1)
        assert same_bits(sets[0].outputs(N_FLIGHT), res3["raw"]["a"]), "the forward enqueued before the commit is not network A"
        assert same_bits(sets[1].outputs(N_FLIGHT), res3["raw"]["b"]), "the forward enqueued after the commit is not network B"
        assert lib.sayuri_hip_weights_generation(ctx) == 1
    finally:
        pipe.Destroy()
        for s in sets:
            s.close()


# ---------------------------------------------------------------- 3. under load through the pipe
def test_reload_under_load_through_the_pipe(tmp_path):
    a, b = write_pair(tmp_path, RES3())
    threads, rounds = 4, 200
    bsz = [19, 9, 13, 19]
    planes = W.synthetic_planes(threads, bsz, seed=9)
    sa, sb = solo(a, planes, bsz), solo(b, planes, bsz)
    pipe = make_pipe(a, batch=64)
    seen = [[] for _ in range(threads)]
    errs, begun_after = [], [None] * threads
    reloaded = threading.Event()

    def worker(k):
        try:
            for _ in range(rounds):
                after = reloaded.is_set()
                got = pipe.Forward([planes[k]], [bsz[k]])[0]
                kind = "A" if same_bits([got], [sa[k]]) else "B" if same_bits([got], [sb[k]]) else "?"
                seen[k].append(kind)
                if after and begun_after[k] is None:
                    begun_after[k] = kind
        except Exception as e:  # noqa: BLE001
            errs.append(repr(e))

    try:
        ths = [threading.Thread(target=worker, args=(k,)) for k in range(threads)]
        [t.start() for t in ths]
        while min(len(s) for s in seen) < rounds // 2 and not errs and any(t.is_alive() for t in ths):
            threading.Event().wait(0.001)
        pipe.Reload(b)
        reloaded.set()
        [t.join() for t in ths]
        assert not errs, errs
        for k, s in enumerate(seen):
            assert len(s) == rounds and "?" not in s, (k, "".join(s))
            assert "".join(s) == "A" * s.count("A") + "B" * s.count("B"), (k, "".join(s))
            assert s[-1] == "B" and begun_after[k] in (None, "B"), (k, begun_after[k])
        assert same_bits(pipe.Forward(planes, bsz), sb)
    finally:
        pipe.Destroy()


# ---------------------------------------------------------------- 4. refusals leave the context as it was
def test_refusals_leave_the_context_as_it_was(res3, tmp_path):
    lib = _lib.hip()
    gr, n = res3["grid"][:5], 5
    pipe = make_pipe(res3["a"], batch=N_FLIGHT)
    wb = Weights(res3["b"])
    err = lambda: lib.sayuri_hip_last_error().decode()

    def still_a(what):
        got = hipraw.hip_forward_raw(ctx, gr, [B] * n, B)
        assert same_bits(got, [x[:n] for x in res3["raw"]["a"]]), what
        assert lib.sayuri_hip_weights_generation(ctx) == 0, what

    try:
        ctx = pipe.ctx(0)
        still_a("before anything")
        # load_tensor after the first forward, outside a reload: refused as before
        t = wb.tensor("input_conv.b")
        assert lib.sayuri_hip_load_tensor(ctx, L_INPUT, 1, _lib.fp(t), t.size) == -1 and "after the first forward" in err()
        still_a("load_tensor outside a reload")
        for change, word in ((dict(residual_blocks=4), "residual_blocks"), (dict(residual_channels=96), "residual_channels"),
                             (dict(blocks={1: dict(apply_se=1, se_size=32), 2: dict(apply_se=0)}), "block 1"),
                             (dict(policy_head_type=1, policy_dw_filter=7), "policy_head_type")):
            if "residual_blocks" in change:   # one block more: the description needs the block itself
                w4 = str(tmp_path / "four.bin")
                W.write_weights(w4, W.NetSpec.residual(4, 128, 32), seed=3)
                wx = Weights(w4)
                d, keep = netdesc(wx)
                wx.close()
            else:
                d, keep = netdesc(wb, **change)
            assert lib.sayuri_hip_reload_begin(ctx, ctypes.byref(d)) == -1, change
            assert word in err(), (change, err())
            assert lib.sayuri_hip_reload_commit(ctx) == -1 and lib.sayuri_hip_reload_abort(ctx) == -1   # nothing was opened
            still_a(change)
        # commit without prepare; a second begin while one is open
        d, keep = netdesc(wb)
        assert lib.sayuri_hip_reload_begin(ctx, ctypes.byref(d)) == 0, err()
        assert lib.sayuri_hip_reload_commit(ctx) == -1 and "not prepared" in err()
        assert lib.sayuri_hip_reload_begin(ctx, ctypes.byref(d)) == -1 and "already open" in err()
        still_a("an open, unprepared reload")
        assert lib.sayuri_hip_reload_abort(ctx) == 0
        # prepare with one tensor missing
        bytes_before = lib.sayuri_hip_device_bytes(ctx)
        assert lib.sayuri_hip_reload_begin(ctx, ctypes.byref(d)) == 0, err()
        load_tensors(ctx, wb, skip=(L_BLOCK0 + 16 + S_CONV2, 0))
        assert lib.sayuri_hip_reload_prepare(ctx) == -1 and "missing tensors" in err()
        assert lib.sayuri_hip_reload_commit(ctx) == -1           # the failed prepare closed the reload
        assert lib.sayuri_hip_device_bytes(ctx) == bytes_before  # ... and freed what it had built
        still_a("a prepare with a tensor missing")
        # and the context still takes a good reload
        stage(ctx, res3["b"])
        assert lib.sayuri_hip_reload_commit(ctx) == 1
        assert same_bits(hipraw.hip_forward_raw(ctx, gr, [B] * n, B), [x[:n] for x in res3["raw"]["b"]])
    finally:
        wb.close()
        pipe.Destroy()


# ---------------------------------------------------------------- 5. nothing leaks
def test_device_bytes_return_after_every_reload(res3):
    lib = _lib.hip()
    pipe = make_pipe(res3["a"], batch=N_FLIGHT)
    s = hipraw.PinnedSet(N_FLIGHT, B, 43 * B * B)
    try:
        ctx = pipe.ctx(0)
        s.planes[:] = res3["grid"].ravel()
        s.bsz[:] = B

        def forward():
            hipraw.wait(ctx, hipraw.submit(ctx, s, N_FLIGHT))

        forward()
        forward()   # (both tickets have their tables)
        before = lib.sayuri_hip_device_bytes(ctx)
        sizes = []
        for k in range(3):
            pipe.Reload(res3["b" if k % 2 == 0 else "a"])
            forward()
            forward()
            sizes.append(lib.sayuri_hip_device_bytes(ctx))
        assert sizes[2] == sizes[0], sizes
        assert sizes[0] == before, (before, sizes)
        assert same_bits(s.outputs(N_FLIGHT), res3["raw"]["b"])
    finally:
        s.close()
        pipe.Destroy()


# ---------------------------------------------------------------- 6. self-play rolls over
def selfplay_rollover(tmp_path, live, num_games):
    from sayuri_amd import search as S
    from sayuri_amd.pipe import HipForwardPipe
    wdir, out = tmp_path / "weights", tmp_path / "out"
    wdir.mkdir()
    out.mkdir()
    spec = W.NetSpec.residual(2, 32, 8)
    a = str(wdir / "net-0001.bin")
    W.write_weights(a, spec, seed=11)
    pipe = HipForwardPipe(a, board_size=9, batch_size=8)
    dropped, halts = [], []

    def on_stats(st, halt):
        halts.append(halt)
        if st["games_done"] >= 8 and not dropped:
            W.write_weights(str(tmp_path / "b.tmp"), spec, seed=12)
            os.rename(str(tmp_path / "b.tmp"), str(wdir / "net-0002.bin"))
            dropped.append(st["games_done"])
        return halt

    try:
        st = S.selfplay(pipe, dict(playouts=4, parallel_games=8, num_games=num_games, seed=5, selfplay_query=["bkp:9:7:1"],
                                   live_weights=int(live), weights_dir=str(wdir), weights_file=a, target_directory=str(out)),
                        on_stats=on_stats, stats_interval=0.05, move_cap=60)
        gen = pipe.weights_generation()
        planes = W.synthetic_planes(2, [9, 9], seed=4)
        now = pipe.Forward(planes, [9, 9])
    finally:
        pipe.Destroy()
    log_dir = out / "weights_log"
    logs = [p.read_text().splitlines() for p in log_dir.iterdir()] if log_dir.is_dir() else []
    return st, gen, logs, halts, now, planes, str(wdir / "net-0002.bin"), a


def test_selfplay_rolls_over_to_the_new_network(tmp_path):
    st, gen, logs, halts, now, planes, b, a = selfplay_rollover(tmp_path, live=True, num_games=40)
    assert st["games_done"] == 40 == st["max_games"], st       # exactly the games asked for: no cap from WindDown
    assert st["weight_swaps"] == 1 and gen == 1, (st, gen)
    assert len(logs) == 1 and len(logs[0]) == 2, logs
    assert logs[0][0].split()[0] == "0" and logs[0][0].split()[2] == "net-0001.bin" and logs[0][1].split()[2] == "net-0002.bin", logs
    assert int(logs[0][1].split()[0]) >= 8, logs
    assert not any(halts), "a halt wish was raised although the network went in live"
    p = make_pipe(b, batch=8)
    try:
        assert same_bits(now, p.Forward(planes, [9, 9])), "after the run the pipe is not the new network"
    finally:
        p.Destroy()


def test_selfplay_without_live_weights_winds_down_as_before(tmp_path):
    """live_weights=0 on the same script.  WindDown caps max_games at (games begun + 25) rounded up to 25: at least 50 with 8 games
    in flight, so the cap shows on a long run and leaves a run of 40 games at 40 -- either way nothing is swapped or logged."""
    st, gen, logs, halts, *_ = selfplay_rollover(tmp_path, live=False, num_games=100000)
    assert st["games_done"] == st["max_games"] < 100000 and st["max_games"] % 25 == 0, st
    assert st["weight_swaps"] == 0 and gen == 0 and not logs and halts[-1], (st, gen, logs)
