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

from _ensemble import GAME_OF_SIZE, GOLDEN_GAMES, golden_game_at, permute_record
from _golden import Golden
from _pipes import make_pipe
from sayuri_amd import _lib, hipraw
from sayuri_amd import search as S
from sayuri_amd.engine import pack_planes
from sayuri_amd.pipe import HipForwardPipe, hip_forward_packed_raw, hip_forward_packed_symm_raw

pytestmark = pytest.mark.gpu

B, WORDS = 19, 37 * 12 + 8
SIZES = (2, 3, 5, 9, 13, 19)   # 2 and 3: the bs-1-t edges; 19: the twelfth record word
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


def submit_symm(ctx, s, recs, bsz, src, symm):
    """The records and board sizes into the set, then sayuri_hip_submit_packed_symm -> ticket."""
    s.records[:recs.size] = recs.ravel()
    s.bsz[:len(symm)] = bsz
    return hipraw.submit_packed_symm(ctx, s, len(recs), 37, src, symm)


def wait_copy(ctx, s, tick, n):
    hipraw.wait(ctx, tick)
    return tuple(a.copy() for a in s.outputs(n))


# ---------------------------------------------------------------------------------------------------------------- 1. expansion
@pytest.mark.parametrize("name,fp16,latency", [("tiny_all", True, False), ("tiny_all", False, False), ("net_6b96", True, False),
                                               ("net_20b256", True, True)],
                         ids=["tiny_all-fp16", "tiny_all-fp32", "net_6b96-default", "net_20b256-latency"])
def test_device_expansion_is_exact(tmp_weights_dir, case, name, fp16, latency):
    """The eight symmetries of six records (2x2 ... 19x19) as 48 device samples of one mixed batch, shuffled: the four outputs
    are those of sayuri_hip_forward_packed on the 48 host-permuted records, bit for bit -- with the records in pageable
    memory (copied) and in sayuri_hip_host_alloc memory (submit: read in place by the kernel)."""
    g = Golden(name, tmp_weights_dir)
    pipe = make_pipe(g.weights_path, latency=latency, batch=64, fp16=fp16)
    pinned = hipraw.PinnedSet(64, B, WORDS)
    try:
        ctx = pipe.ctx(0)
        want = hip_forward_packed_raw(ctx, case["host"], 37, case["bsz"], B)
        got = hip_forward_packed_symm_raw(ctx, case["recs"], 37, case["bsz"], case["src"], case["symm"], B)
        assert_bits(got, want, "pageable records")
        assert_symmetries_differ(got, case["src"], case["symm"])
        tick = submit_symm(ctx, pinned, case["recs"], case["bsz"], case["src"], case["symm"])
        assert_bits(wait_copy(ctx, pinned, tick, len(case["symm"])), want, "records in page-locked memory, in place")
        # the blocking form on page-locked records
        got = hip_forward_packed_symm_raw(ctx, pinned.records.ctypes.data, 37, case["bsz"], case["src"], case["symm"], B, n_records=len(SIZES))
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
    pinned = [hipraw.PinnedSet(96, B, WORDS) for _ in range(2)]
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
        sub = lambda i: submit_symm(ctx, pinned[i], batches[i]["recs"], batches[i]["bsz"], batches[i]["src"], batches[i]["symm"])  # noqa: E731
        tick = [sub(0), sub(1)]
        for r in range(6):
            i = r & 1
            assert_bits(wait_copy(ctx, pinned[i], tick[i], len(batches[i]["symm"])), solo[i], ("round", r))
            if r < 4:
                tick[i] = sub(i)
    finally:
        for s in pinned:
            s.close()
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
def direct_context(path, max_batch):
    """A context made at the C-ABI itself -- sayuri_hip_create(max_batch) and every tensor of a residual-block network loaded,
    the calls HipForwardPipe's BuildCtx makes -- so that what a pipe adds to its context can be told from outside."""
    from sayuri_amd.pipe import Weights
    lib = _lib.hip()
    w = Weights(path)
    ver, cin, nblocks, C, cp, cv, pc, po, oc, mo, act, ptype = w.info
    assert ptype == 0
    blocks = (_lib.BlockDesc * nblocks)()
    for b in range(nblocks):
        bi = w.block_info(b)
        assert bi[0] == 1, "residual blocks only"
        blocks[b] = _lib.BlockDesc(1, bi[1], bi[2], 0, 0, 0)
    desc = _lib.NetDesc(ver, cin, C, nblocks, cp, cv, pc, po, oc, mo, act, 0, 0, blocks)
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
            assert lib.sayuri_hip_load_tensor(ctx, lid, kind, _lib.fp(t), t.size) == 0, lib.sayuri_hip_last_error()
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
    bytes_of_ctx = lambda c: int(lib.sayuri_hip_device_bytes(c))  # noqa: E731
    bytes_of = lambda p: bytes_of_ctx(p.ctx(0))  # noqa: E731
    plain = HipForwardPipe(g.weights_path, board_size=B, batch_size=16, fp16=True, waittime_ms=0)
    default = HipForwardPipe(g.weights_path)
    ens = HipForwardPipe(g.weights_path, board_size=B, batch_size=16, fp16=True, waittime_ms=0, ensemble=2)
    big = HipForwardPipe(g.weights_path, board_size=B, batch_size=30, fp16=True, waittime_ms=0)
    direct = {n: direct_context(g.weights_path, n) for n in (16, 256)}
    pinned = hipraw.PinnedSet(1, B, WORDS)
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
        rec, _ = game.planes_packed(0)
        pinned.records[:] = rec
        pinned.bsz[0] = 9
        for ctx in direct.values():
            for _ in range(8):
                hipraw.wait(ctx, hipraw.submit_packed(ctx, pinned, 1, 37))
        for n, pipe in ((16, plain), (256, default)):
            assert bytes_of(pipe) == bytes_of_ctx(direct[n]), ("after eight evaluations", n)
        # E = 2: a pipe of 16 + 14 samples plus the two small tables (256 bytes each) of every ticket that carried such a batch
        assert bytes_of(big) < bytes_of(ens) <= bytes_of(big) + 4 * 256
        with pytest.raises(RuntimeError, match="ensemble"):
            plain.ForwardEnsemble(np.zeros((43, 81), np.float32), 9)
    finally:
        pinned.close()
        for c in direct.values():
            lib.sayuri_hip_destroy(c)
        for p in (plain, default, ens, big):
            p.Destroy()
