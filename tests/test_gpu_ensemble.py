"""Ensemble requests on the device: sayuri_hip_forward_packed_symm / sayuri_hip_submit_packed_symm (pack_bits_symm_kernel,
csrc/hip/small_ops.h) expand one packed record under a board symmetry per device sample, the pipe sends the eight symmetries
of a position as one request (HipForwardPipe::ForwardEnsemble) and Network's kAverage uses it.

A position's bits do not depend on its batch and the packed route gives the bits of the fp32 route, so every check here is
on BITS against code that existed before the feature: sayuri_hip_forward_packed on records permuted on the host (the rule
itself is checked against the engine's encoder in tests/test_ensemble_cpu.py), and kAverage as eight evaluations in a row."""
import ctypes
import threading
import time

import numpy as np
import pytest

import test_gpu_fuzz as FZ
from _ensemble import GAME_OF_SIZE, GOLDEN_GAMES, golden_game_at, permute_record
from _golden import Golden
from sayuri_amd import _lib
from sayuri_amd import search as S
from sayuri_amd.engine import pack_planes
from sayuri_amd.pipe import HipForwardPipe, hip_forward_packed_raw, hip_forward_packed_symm_raw
from test_gpu_latency import make_pipe

pytestmark = pytest.mark.gpu

B, WORDS = 19, 37 * 12 + 8
SIZES = (2, 3, 5, 9, 13, 19)   # 2 and 3: the bs-1-t edges; 19: the twelfth record word
FP, IP = FZ.FP, FZ.IP
K_AVERAGE = 2
# sayuri_engine_net_output's layout behind the two maps of n cells
FIELDS = ("pass_probability", "wdl0", "wdl1", "wdl2", "wdl_winrate", "stm_winrate", "final_score", "q_error", "score_error")


@pytest.fixture(scope="module")
def case():
    """One random record per size with distinct random scalars, its eight host permutations (pairwise different), and the 48
    device samples (record, symmetry) in shuffled order."""
    rng = np.random.default_rng(808)
    recs, turned = [], {}
    for k, bs in enumerate(SIZES):
        p = np.zeros((43, bs * bs), np.float32)
        p[:37] = rng.integers(0, 2, size=(37, bs * bs))
        p[37:] = rng.normal(size=(6, 1)).astype(np.float32)
        recs.append(pack_planes(p, 37))
        for s in range(8):
            turned[k, s] = permute_record(recs[k], 37, bs, s)
        assert len({turned[k, s].tobytes() for s in range(8)}) == 8, f"{bs}x{bs}: two symmetries of the record coincide"
    order = [(k, s) for k in range(len(SIZES)) for s in range(8)]
    rng.shuffle(order)
    src = np.asarray([k for k, _ in order], np.int32)
    symm = np.asarray([s for _, s in order], np.int32)
    bsz = np.asarray([SIZES[k] for k in src], np.int32)
    host = np.stack([turned[k, s] for k, s in order]).astype(np.uint32)
    return dict(recs=np.stack(recs).astype(np.uint32), src=src, symm=symm, bsz=bsz, host=host)


def assert_bits(got, want, what):
    for a, b, name in zip(got, want, ("prob", "pass", "misc", "own")):
        assert np.array_equal(a, b), (what, name, int((a != b).sum()))


def assert_symmetries_differ(outs, src, symm):
    """The outputs of symmetries 1..7 are not symmetry 0's (a kernel that ignored `symm` would still be self-consistent)."""
    for k in set(src.tolist()):
        i0 = int(np.flatnonzero((src == k) & (symm == 0))[0])
        for i in np.flatnonzero((src == k) & (symm != 0)):
            assert not np.array_equal(outs[0][i], outs[0][i0]), (k, int(symm[i]))


class SymmPinned:
    """Two sets of page-locked buffers for sayuri_hip_submit_packed_symm / wait: records, the four outputs."""

    def __init__(self, lib, nmax):
        self.lib, self.nmax = lib, nmax
        lib.sayuri_hip_host_alloc.restype = ctypes.c_void_p
        lib.sayuri_hip_host_alloc.argtypes = [ctypes.c_size_t]
        lib.sayuri_hip_host_free.argtypes = [ctypes.c_void_p]
        lib.sayuri_hip_wait.argtypes = [ctypes.c_void_p, ctypes.c_int]
        lib.sayuri_hip_submit_packed_symm.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, IP, IP, IP,
                                                      FP, FP, FP, FP, IP]
        self.sizes = (nmax * WORDS, nmax * 5 * B * B, nmax * 5, nmax * 15, nmax * B * B)
        self.sets = [[lib.sayuri_hip_host_alloc(k * 4) for k in self.sizes] for _ in range(2)]
        assert all(q for ptrs in self.sets for q in ptrs)

    def close(self):
        for ptrs in self.sets:
            for q in ptrs:
                self.lib.sayuri_hip_host_free(ctypes.c_void_p(q))

    def submit(self, ctx, i, recs, bsz, src, symm):
        rc_, pr, pa, mi, ow = self.sets[i]
        np.ctypeslib.as_array(ctypes.cast(rc_, ctypes.POINTER(ctypes.c_uint32)), (recs.size,))[:] = recs.ravel()
        tick = ctypes.c_int(-1)
        bsz, symm = np.ascontiguousarray(bsz, np.int32), np.ascontiguousarray(symm, np.int32)
        src = None if src is None else np.ascontiguousarray(src, np.int32)
        rc = self.lib.sayuri_hip_submit_packed_symm(ctx, len(symm), ctypes.c_void_p(rc_), len(recs), 37, bsz.ctypes.data_as(IP),
                                                    None if src is None else src.ctypes.data_as(IP), symm.ctypes.data_as(IP),
                                                    ctypes.cast(pr, FP), ctypes.cast(pa, FP), ctypes.cast(mi, FP), ctypes.cast(ow, FP),
                                                    ctypes.byref(tick))
        assert rc == 0, self.lib.sayuri_hip_last_error()
        return tick.value   # (the small tables are copied by the call: the temporaries above may go)

    def wait(self, ctx, i, tick, n):
        assert self.lib.sayuri_hip_wait(ctx, tick) == 0, self.lib.sayuri_hip_last_error()
        _, pr, pa, mi, ow = self.sets[i]
        return (np.ctypeslib.as_array(ctypes.cast(pr, FP), (n, 5, B * B)).copy(), np.ctypeslib.as_array(ctypes.cast(pa, FP), (n, 5)).copy(),
                np.ctypeslib.as_array(ctypes.cast(mi, FP), (n, 15)).copy(), np.ctypeslib.as_array(ctypes.cast(ow, FP), (n, B * B)).copy())


# ---------------------------------------------------------------------------------------------------------------- 1. expansion
@pytest.mark.parametrize("name,fp16,latency", [("tiny_all", True, False), ("tiny_all", False, False), ("net_6b96", True, False),
                                               ("net_20b256", True, True)],
                         ids=["tiny_all-fp16", "tiny_all-fp32", "net_6b96-default", "net_20b256-latency"])
def test_device_expansion_is_exact(tmp_weights_dir, case, name, fp16, latency):
    """The eight symmetries of six records (2x2 ... 19x19) as 48 device samples of one mixed batch, shuffled: the four outputs
    are those of sayuri_hip_forward_packed on the 48 host-permuted records, bit for bit -- with the records in pageable
    memory (copied) and in sayuri_hip_host_alloc memory (submit: read in place by the kernel)."""
    g = Golden(name, tmp_weights_dir)
    lib = _lib.hip()
    pipe = make_pipe(g.weights_path, latency=latency, batch=64, fp16=fp16)
    pinned = SymmPinned(lib, 64)
    try:
        ctx = pipe.ctx(0)
        want = hip_forward_packed_raw(ctx, case["host"], 37, case["bsz"], B)
        got = hip_forward_packed_symm_raw(ctx, case["recs"], 37, case["bsz"], case["src"], case["symm"], B)
        assert_bits(got, want, "pageable records")
        assert_symmetries_differ(got, case["src"], case["symm"])
        tick = pinned.submit(ctx, 0, case["recs"], case["bsz"], case["src"], case["symm"])
        assert_bits(pinned.wait(ctx, 0, tick, len(case["symm"])), want, "records in page-locked memory, in place")
        # the blocking form on page-locked records
        got = hip_forward_packed_symm_raw(ctx, pinned.sets[0][0], 37, case["bsz"], case["src"], case["symm"], B, n_records=len(SIZES))
        assert_bits(got, want, "records in page-locked memory, blocking call")
    finally:
        pinned.close()
        pipe.Destroy()


# ---------------------------------------------------------------------------------------------------------------- 3. identity, arguments
def test_identity_map_and_argument_checks(tmp_weights_dir, case):
    g = Golden("net_6b96", tmp_weights_dir)
    lib = _lib.hip()
    pipe = make_pipe(g.weights_path, batch=16)
    try:
        ctx = pipe.ctx(0)
        recs, bsz = case["host"][:12], case["bsz"][:12]
        zero = np.zeros(12, np.int32)
        want = hip_forward_packed_raw(ctx, recs, 37, bsz, B)
        assert_bits(hip_forward_packed_symm_raw(ctx, recs, 37, bsz, None, zero, B), want, "symm = 0, src = NULL")
        bad_symm, bad_src = zero.copy(), np.arange(12, dtype=np.int32)
        bad_symm[7] = 8
        bad_src[3] = 12
        for what, kw in (("symm", dict(src=None, symm=bad_symm)), ("src", dict(src=bad_src, symm=zero)),
                         ("n_records", dict(src=None, symm=zero, n_records=0))):
            with pytest.raises(RuntimeError, match=what):
                hip_forward_packed_symm_raw(ctx, recs, 37, bsz, board=B, **kw)
            assert_bits(hip_forward_packed_symm_raw(ctx, recs, 37, bsz, None, zero, B), want, "a good call after a refused one")
        with pytest.raises(RuntimeError, match="batch size"):   # n > max_batch: 17 samples of one record
            hip_forward_packed_symm_raw(ctx, recs, 37, np.full(17, bsz[0], np.int32), np.zeros(17, np.int32), np.zeros(17, np.int32), B)
        assert_bits(hip_forward_packed_symm_raw(ctx, recs, 37, bsz, None, zero, B), want, "a good call after n > max_batch")
    finally:
        pipe.Destroy()


# ---------------------------------------------------------------------------------------------------------------- 4. two tickets
@pytest.mark.parametrize("latency", [True, False], ids=["latency", "default"])
def test_two_tickets_in_flight(tmp_weights_dir, case, latency):
    """submit_packed_symm on tickets 0 and 1 with different batches, six rounds: every result has the solo bits.  Default
    context: a uniform 19x19 batch of 64 (the persistent tower launch) beside the mixed batch of 48."""
    g = Golden("net_20b256", tmp_weights_dir)
    lib = _lib.hip()
    pipe = make_pipe(g.weights_path, latency=latency, batch=96)
    pinned = SymmPinned(lib, 96)
    try:
        ctx = pipe.ctx(0)
        if not latency:
            assert lib.sayuri_hip_tower_state(ctx) == 1
        k19 = SIZES.index(19)
        n_big = 24 if latency else 64
        big_symm = (np.arange(n_big) % 8).astype(np.int32)
        big_host = np.stack([permute_record(case["recs"][k19], 37, 19, int(s)) for s in range(8)])[big_symm].astype(np.uint32)
        batches = [dict(recs=case["recs"], bsz=case["bsz"], src=case["src"], symm=case["symm"], host=case["host"]),
                   dict(recs=case["recs"][k19:k19 + 1], bsz=np.full(n_big, 19, np.int32), src=np.zeros(n_big, np.int32), symm=big_symm,
                        host=big_host)]
        solo = [hip_forward_packed_raw(ctx, b["host"], 37, b["bsz"], B) for b in batches]
        sub = lambda i: pinned.submit(ctx, i, batches[i]["recs"], batches[i]["bsz"], batches[i]["src"], batches[i]["symm"])  # noqa: E731
        tick = [sub(0), sub(1)]
        for r in range(6):
            i = r & 1
            assert_bits(pinned.wait(ctx, i, tick[i], len(batches[i]["symm"])), solo[i], ("round", r))
            if r < 4:
                tick[i] = sub(i)
    finally:
        pinned.close()
        pipe.Destroy()


# ---------------------------------------------------------------------------------------------------------------- 5. the facade
def golden_positions():
    golden = np.load(GOLDEN_GAMES)
    for bs, gi in GAME_OF_SIZE.items():
        n = len(golden[f"g{gi}_moves"])
        for step in (3, n // 3, (2 * n) // 3):
            yield bs, step, golden_game_at(golden, gi, step)


def assert_same_output(on, off, n, what):
    for name, a, b in [("probabilities", on[:n], off[:n]), ("ownership", on[n:2 * n], off[n:2 * n])] + \
                      [(f, on[2 * n + k:2 * n + k + 1], off[2 * n + k:2 * n + k + 1]) for k, f in enumerate(FIELDS)]:
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), (what, name)


@pytest.mark.parametrize("name,latency", [("net_6b96", False), ("net_20b256", True)], ids=["net_6b96-default", "net_20b256-latency"])
def test_average_through_the_facade_has_the_same_bits(tmp_weights_dir, name, latency):
    """kAverage with device_ensemble on == off, field by field, on three positions of the golden games per board size;
    one batch per call with it on, eight evaluations either way."""
    g = Golden(name, tmp_weights_dir)
    pipe = HipForwardPipe(g.weights_path, board_size=B, batch_size=16, fp16=True, waittime_ms=0, latency=latency, ensemble=2)
    try:
        assert pipe.AcceptsEnsemble()
        nets = {on: S.Network(pipe=pipe, options=dict(device_ensemble=on, no_cache=True)) for on in (True, False)}
        for bs, step, game in golden_positions():
            t0 = pipe.pump_times()
            on = nets[True].output(game, ensemble=K_AVERAGE)
            t1 = pipe.pump_times()
            off = nets[False].output(game, ensemble=K_AVERAGE)
            t2 = pipe.pump_times()
            assert_same_output(on, off, game.n, (bs, step))
            assert t1["batches"] - t0["batches"] == 1 and t1["evals"] - t0["evals"] == 8, (t0, t1)
            assert t2["evals"] - t1["evals"] == 8
        assert nets[True].queries() == nets[False].queries() == 8 * 9
        assert pipe.ensemble_fallbacks() == 0
        for n in nets.values():
            n.close()
    finally:
        pipe.Destroy()


# ---------------------------------------------------------------------------------------------------------------- 6. capacity
def test_capacity_fallback_keeps_the_bits(tmp_weights_dir):
    """ensemble=1, two threads calling kAverage at once: a batch expands one of them, the other is served the identity in
    its slot and evaluates the rest the old way -- every result is the off-path result, and it did happen."""
    g = Golden("net_6b96", tmp_weights_dir)
    golden = np.load(GOLDEN_GAMES)
    pipe = HipForwardPipe(g.weights_path, board_size=B, batch_size=16, fp16=True, waittime_ms=2, ensemble=1)
    try:
        games = [golden_game_at(golden, GAME_OF_SIZE[9], 20), golden_game_at(golden, GAME_OF_SIZE[13], 31)]
        off_net = S.Network(pipe=pipe, options=dict(device_ensemble=False, no_cache=True))
        want = [off_net.output(gm, ensemble=K_AVERAGE) for gm in games]
        nets = [S.Network(pipe=pipe, options=dict(no_cache=True)) for _ in games]
        errs = []
        start = threading.Barrier(2)

        def worker(i):
            try:
                for r in range(40):
                    start.wait()
                    assert_same_output(nets[i].output(games[i], ensemble=K_AVERAGE), want[i], games[i].n, (i, r))
            except Exception as e:  # noqa: BLE001
                errs.append(repr(e))
                start.abort()

        ths = [threading.Thread(target=worker, args=(i,)) for i in range(2)]
        [t.start() for t in ths]
        [t.join() for t in ths]
        assert not errs, errs
        assert pipe.ensemble_fallbacks() > 0, "two callers at once and one expansion per batch: none fell back"
        for n in nets + [off_net]:
            n.close()
    finally:
        pipe.Destroy()


# ---------------------------------------------------------------------------------------------------------------- 7. faster
def test_device_ensemble_halves_the_average(tmp_weights_dir, capsys):
    """net_20b256, latency pipe, one 19x19 golden position, kAverage through the facade: device_ensemble on against off,
    interleaved, medians of 3 rounds x 100 calls (wall time per call), as tools/ensemble_bench.py measures it.  The floor
    of one half is reasoned, not measured: by profiles/r07_latency_small_batch.json the device work is one trip of 0.766 ms
    (eight boards) against eight of 0.657 ms, and the host encodes once instead of eight times; a factor of three is left for
    the collector's close timing and box noise, while a path that silently falls back has ratio ~1 and fails.
    Measured on an MI355X (this test's own run; DESIGN.md Kernel 1f): off 5.783 ms, on 0.894 ms, ratio 0.155."""
    g = Golden("net_20b256", tmp_weights_dir)
    golden = np.load(GOLDEN_GAMES)
    game = golden_game_at(golden, GAME_OF_SIZE[19], 120)
    pipe = HipForwardPipe(g.weights_path, board_size=B, batch_size=16, fp16=True, waittime_ms=0, latency=True, ensemble=2)
    try:
        nets = {k: S.Network(pipe=pipe, options=dict(device_ensemble=(k == "on"), no_cache=True)) for k in ("off", "on")}
        times = {k: [] for k in nets}
        for net in nets.values():
            for _ in range(10):
                net.output(game, ensemble=K_AVERAGE)
        for _ in range(3):
            for k, net in nets.items():
                t0 = time.perf_counter()
                for _ in range(100):
                    net.output(game, ensemble=K_AVERAGE)
                times[k].append((time.perf_counter() - t0) / 100 * 1e3)
        off, on = float(np.median(times["off"])), float(np.median(times["on"]))
        with capsys.disabled():
            print(f"\n[ensemble] net_20b256 latency pipe, one 19x19 position, kAverage ms per call: off {off:.4f}, on {on:.4f}, ratio {on / off:.3f}")
        assert pipe.ensemble_fallbacks() == 0
        assert on <= 0.5 * off, (off, on)
        for n in nets.values():
            n.close()
    finally:
        pipe.Destroy()


# ---------------------------------------------------------------------------------------------------------------- default untouched
class _Block(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int32) for n in ("type", "apply_se", "se_size", "btl", "ffn", "dw")]


class _Desc(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int32) for n in ("version", "input_channels", "residual_channels", "residual_blocks", "policy_head_channels",
                                              "value_head_channels", "probabilities_channels", "pass_probability_outputs",
                                              "ownership_channels", "value_misc_outputs", "default_act", "policy_head_type",
                                              "policy_dw_filter")] + [("blocks", ctypes.POINTER(_Block))]


def direct_context(path, max_batch):
    """A context made at the C-ABI itself -- sayuri_hip_create(max_batch) and every tensor of a residual-block network loaded,
    the calls HipForwardPipe's BuildCtx makes -- so that what a pipe adds to its context can be told from outside."""
    from sayuri_amd.pipe import Weights
    lib = _lib.hip()
    lib.sayuri_hip_create.restype = ctypes.c_void_p
    lib.sayuri_hip_create.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int]
    lib.sayuri_hip_load_tensor.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, FP, ctypes.c_size_t]
    lib.sayuri_hip_destroy.argtypes = [ctypes.c_void_p]
    w = Weights(path)
    ver, cin, nblocks, C, cp, cv, pc, po, oc, mo, act, ptype = w.info
    assert ptype == 0
    blocks = (_Block * nblocks)()
    for b in range(nblocks):
        bi = w.block_info(b)
        assert bi[0] == 1, "residual blocks only"
        blocks[b] = _Block(1, bi[1], bi[2], 0, 0, 0)
    desc = _Desc(ver, cin, C, nblocks, cp, cv, pc, po, oc, mo, act, 0, 0, blocks)
    ctx = lib.sayuri_hip_create(0, ctypes.byref(desc), max_batch, B, 1)
    assert ctx, lib.sayuri_hip_last_error()
    layers = [(0, "input_conv"), (1, "p_hd_conv"), (4, "p_inter_fc"), (5, "prob_conv"), (6, "pass_fc"), (7, "v_hd_conv"),
              (8, "v_inter_fc"), (9, "v_ownership"), (10, "v_misc")]
    for b in range(nblocks):
        layers += [(16 + 16 * b + 0, f"tower.{b}.conv1"), (16 + 16 * b + 1, f"tower.{b}.conv2")]
        if blocks[b].apply_se:
            layers += [(16 + 16 * b + 7, f"tower.{b}.squeeze"), (16 + 16 * b + 8, f"tower.{b}.excite")]
    for lid, name in layers:
        for kind, suffix in ((0, ".w"), (1, ".b")):
            t = w.tensor(name + suffix)
            assert t is not None, name + suffix
            assert lib.sayuri_hip_load_tensor(ctx, lid, kind, t.ctypes.data_as(FP), t.size) == 0, lib.sayuri_hip_last_error()
    w.close()
    return ctx


def test_a_pipe_without_ensembles_is_the_pipe_it_was(tmp_weights_dir):
    """ensemble = 0: no entry point is offered, kAverage is eight evaluations, and the pipe's context holds exactly the device
    memory of a context of batch_size samples made directly at the C-ABI (sayuri_hip_create, no pipe involved) that has done
    the same work: single 9x9 packed records through submit / wait on both tickets.  A default-constructed pipe likewise
    against a directly made context of 256 samples.  With E slots the context is one of batch_size + 7 E samples plus the two
    small tables of every ticket that has carried a symmetry batch."""
    g = Golden("net_6b96", tmp_weights_dir)
    lib = _lib.hip()
    bytes_of_ctx = lambda c: int(lib.sayuri_hip_device_bytes(ctypes.c_void_p(c)))  # noqa: E731
    bytes_of = lambda p: bytes_of_ctx(p.ctx(0))  # noqa: E731
    plain = HipForwardPipe(g.weights_path, board_size=B, batch_size=16, fp16=True, waittime_ms=0)
    default = HipForwardPipe(g.weights_path)
    ens = HipForwardPipe(g.weights_path, board_size=B, batch_size=16, fp16=True, waittime_ms=0, ensemble=2)
    big = HipForwardPipe(g.weights_path, board_size=B, batch_size=30, fp16=True, waittime_ms=0)
    direct = {n: direct_context(g.weights_path, n) for n in (16, 256)}
    pinned = SymmPinned(lib, 1)
    try:
        assert not plain.AcceptsEnsemble() and ens.AcceptsEnsemble()
        for n, pipe in ((16, plain), (256, default)):
            assert bytes_of(pipe) == bytes_of_ctx(direct[n]), ("untouched", n)
        game = golden_game_at(np.load(GOLDEN_GAMES), GAME_OF_SIZE[9], 12)
        outs = {}
        for key, pipe in (("plain", plain), ("default", default), ("big", big), ("ens", ens)):
            net = S.Network(pipe=pipe, options=dict(no_cache=True))
            before = pipe.pump_times()
            outs[key] = net.output(game, ensemble=K_AVERAGE)
            after = pipe.pump_times()
            assert after["evals"] - before["evals"] == 8 and net.queries() == 8
            assert after["batches"] - before["batches"] == (1 if key == "ens" else 8)
            net.close()
        assert_same_output(outs["ens"], outs["plain"], game.n, "E = 0 against E = 2")
        # the same work on the directly made contexts: one 9x9 record, plain submit_packed, tickets 0 and 1 four times each
        lib.sayuri_hip_submit_packed.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int, IP, FP, FP, FP, FP, IP]
        rec, _ = game.planes_packed(0)
        rc_, pr, pa, mi, ow = pinned.sets[0]
        np.ctypeslib.as_array(ctypes.cast(rc_, ctypes.POINTER(ctypes.c_uint32)), (WORDS,))[:] = rec
        nine = np.asarray([9], np.int32)
        for ctx in direct.values():
            for _ in range(8):
                tick = ctypes.c_int(-1)
                assert lib.sayuri_hip_submit_packed(ctypes.c_void_p(ctx), 1, ctypes.c_void_p(rc_), 37, nine.ctypes.data_as(IP), ctypes.cast(pr, FP),
                                                    ctypes.cast(pa, FP), ctypes.cast(mi, FP), ctypes.cast(ow, FP), ctypes.byref(tick)) == 0
                assert lib.sayuri_hip_wait(ctypes.c_void_p(ctx), tick.value) == 0
        for n, pipe in ((16, plain), (256, default)):
            assert bytes_of(pipe) == bytes_of_ctx(direct[n]), ("after eight evaluations", n)
        # E = 2: a pipe of 16 + 14 samples plus the two small tables (256 bytes each) of every ticket that carried such a batch
        assert bytes_of(big) < bytes_of(ens) <= bytes_of(big) + 4 * 256
        with pytest.raises(RuntimeError, match="ensemble"):
            plain.ForwardEnsemble(np.zeros((43, 81), np.float32), 9)
    finally:
        pinned.close()
        for c in direct.values():
            lib.sayuri_hip_destroy(ctypes.c_void_p(c))
        for p in (plain, default, ens, big):
            p.Destroy()
