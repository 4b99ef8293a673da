"""The SE unit as ONE launch (se_unit_kernel, csrc/hip/small_ops.h; SAYURI_SE_ONE, csrc/hip/engine_plan.h): workgroups of 1024
threads whose three phases are the bodies of se_pool / se_fc / se_scale -- several per sample on large boards, each pooling the
whole sample and scaling its share into the skip's buffer.  SAYURI_SE_ONE=1 / 0 force a form; with the switch unset a latency
context takes the one launch whenever every workgroup's scale phase is a single pass (Engine::se_unit; DESIGN.md Kernel 1g).

The phases keep the summation order of the kernels they replace, so the checks are on BITS, against the three launches:
  routing      the profile rows of a forward name the form that ran                                  (tests 1 and 3)
  whole net    a latency context, and one under SAYURI_SE_ONE=1, == one under =0                     (test 2)
               a separate-SE default context under SAYURI_SE_ONE=1 == the same without it            (test 3, fp16 and fp32)
  layer level  the se_unit tap under SAYURI_SE_ONE=1 == the tap without it                           (test 4)
  speed        a lone board on 20b x 256, one launch per unit against three: 19x19 and 9x9           (test 5)
The tolerance checks reuse se_unit_f64 of _kref.py with test_gpu_smallops.py's bounds, and check / fp16_tol of _pipes.py.
"""
import ctypes
import os

import numpy as np
import pytest

import _pipes
import _taps
from _cases import SE_LAYERS, SE_SEED, SE_UNIT_BATCHES, se_inputs, se_unit_x
from _golden import Golden
from _kref import se_apply_f64, se_gate_f64, se_pool_f64, se_unit_f64
from _pipes import check, fp16_tol, grid_of
from sayuri_amd import _lib
from sayuri_amd import weights as W
from sayuri_amd.pipe import Weights, hip_forward_raw

pytestmark = pytest.mark.gpu

B = 19
SEPARATE = {"SAYURI_SE_FUSED": "0", "SAYURI_SE_SPLIT": "0", "SAYURI_TOWER": "0"}
THREE = ("se_pool", "se_fc", "se_scale")
MIXED15 = [19, 9, 13, 9, 19, 13, 9, 9, 19, 13, 7, 19, 9, 13, 16]  # test_gpu_latency.py's mixed batch


def make_pipe(monkeypatch, path, se_one=None, env=None, **kw):
    """_pipes.make_pipe under SAYURI_SE_ONE = se_one (None: unset); the switch is read when the context is created."""
    if se_one is None:
        monkeypatch.delenv("SAYURI_SE_ONE", raising=False)
    else:
        monkeypatch.setenv("SAYURI_SE_ONE", str(se_one))
    try:
        return _pipes.make_pipe(path, env, **{"batch": 64, **kw})
    finally:
        monkeypatch.delenv("SAYURI_SE_ONE", raising=False)


def forward(pipe, sizes, seed):
    return hip_forward_raw(pipe.ctx(0), grid_of(W.synthetic_planes(len(sizes), sizes, seed=seed), sizes), sizes, B)


def launches(pipe):
    """kernel class -> launches of one run of the context's last batch"""
    rows = (_lib.KernelStat * 64)()
    k = _lib.hip().sayuri_hip_profile_run(pipe.ctx(0), rows, 64)
    assert k >= 0, _lib.hip().sayuri_hip_last_error()
    return {rows[i].name.decode(): rows[i].launches for i in range(k)}


def se_blocks(path):
    """the network's blocks with an SE unit, counted from its weights"""
    w = Weights(path)
    try:
        return sum(1 for b in range(w.info[2]) if w.block_info(b)[1])
    finally:
        w.close()


def assert_form(names, units, one):
    got_one, got_three = names.get("se_unit", 0), [names.get(k, 0) for k in THREE]
    assert (got_one, got_three) == ((units, [0, 0, 0]) if one else (0, [units] * 3)), names


# ---------------------------------------------------------------------------------------------------------------- 1. routing
SMALL = [9, 7, 5, 9, 2, 9]


@pytest.mark.parametrize("name", ["net_20b256", "net_40b384"])
def test_latency_forward_runs_every_se_unit_as_one_launch(name, tmp_weights_dir, monkeypatch):
    """A latency context's forward -- a lone 19x19 board, the mixed batch of 15, small boards -- has one se_unit launch per SE
    block of the network and no se_pool / se_fc / se_scale, with nothing set and under SAYURI_SE_ONE=1; under SAYURI_SE_ONE=0 the
    reverse; a default context with nothing set has no se_unit row.  The boundary of the engine's rule (Engine::se_unit: every
    workgroup's share of a board at most 4096 pieces, 256 / boards workgroups per board at the most) is pinned at 64 full boards:
    256 channels take the one launch there (4 x 2888 pieces), 384 channels keep the three (4 x 4332), and SAYURI_SE_ONE=1
    overrides that."""
    g = Golden(name, tmp_weights_dir)
    units = se_blocks(g.weights_path)
    assert units > 0
    for se_one, one in ((None, True), (1, True), (0, False)):
        pipe = make_pipe(monkeypatch, g.weights_path, se_one, latency=True)
        try:
            for k, sizes in enumerate(([19], MIXED15, SMALL)):
                assert np.abs(forward(pipe, sizes, 7100 + k)[0]).max() > 0
                assert_form(launches(pipe), units, one)
            assert np.abs(forward(pipe, [19] * 64, 7110)[0]).max() > 0
            assert_form(launches(pipe), units, one and (se_one == 1 or name == "net_20b256"))
        finally:
            pipe.Destroy()
    pipe = make_pipe(monkeypatch, g.weights_path)
    try:
        forward(pipe, MIXED15, 7101)
        assert launches(pipe).get("se_unit", 0) == 0
    finally:
        pipe.Destroy()


# ---------------------------------------------------------------------------------------------------------------- 2. whole net, latency
def _spec(blocks, C, head, act, se_ratio=4):
    s = W.NetSpec.residual(blocks, C, head, se_every=1, activation=act)
    s.se_ratio = se_ratio
    return s


SYNTHETIC = {
    # the smallest shapes at which the kernel can go wrong
    "2b32-mish": lambda: _spec(2, 32, 16, "mish"),      # cs = 32: 64 pixel rows per pass of a pooling slice
    "2b48-relu": lambda: _spec(2, 48, 16, "relu"),      # cs = 64 > C: pad channels
    "2b320-mish": lambda: _spec(2, 320, 32, "mish"),    # 40 pieces per row: 16 idle threads per slice
    "2b320-relu": lambda: _spec(2, 320, 32, "relu"),
    "2b48-se3": lambda: _spec(2, 48, 16, "mish", 16),   # se = 3, no multiple of 4: the squeeze FC's block_fc branch
}
NET_BATCHES = [[19], [13], [9], [2], [3, 5], MIXED15, [19] * 16]


def _net_path(name, tmp_weights_dir):
    if name in SYNTHETIC:
        path = os.path.join(tmp_weights_dir, f"se_one_{name}.bin")
        if not os.path.exists(path):
            W.write_weights(path, SYNTHETIC[name](), seed=31)
        return path
    return Golden(name, tmp_weights_dir).weights_path


@pytest.mark.parametrize("name", ["net_20b256", "net_40b384", "net_6b96"] + list(SYNTHETIC))
def test_latency_context_has_the_bits_of_three_launches(name, tmp_weights_dir, monkeypatch):
    """All four outputs of a latency context with the switch unset (one launch per unit, several workgroups per large board) and
    of one under SAYURI_SE_ONE=1 equal those of a latency context created under SAYURI_SE_ONE=0, on lone boards of 19, 13, 9 and
    2, on [3, 5], a mixed batch of 15 and 16 full boards."""
    path = _net_path(name, tmp_weights_dir)
    units = se_blocks(path)
    one = make_pipe(monkeypatch, path, 1, latency=True)
    rule = make_pipe(monkeypatch, path, None, latency=True)
    three = make_pipe(monkeypatch, path, 0, latency=True)
    try:
        for k, sizes in enumerate(NET_BATCHES):
            a = forward(three, sizes, 7200 + k)
            assert np.abs(a[0]).max() > 0
            for arm, pipe in (("one", one), ("rule", rule)):
                for x, y, what in zip(a, forward(pipe, sizes, 7200 + k), ("prob", "pass", "misc", "own")):
                    assert np.array_equal(x, y), (name, arm, sizes, what, float(np.abs(x - y).max()))
        assert_form(launches(one), units, True)
        assert_form(launches(rule), units, True)
        assert_form(launches(three), units, False)
    finally:
        one.Destroy()
        rule.Destroy()
        three.Destroy()


# ---------------------------------------------------------------------------------------------------------------- 3. default context, fp32
@pytest.mark.parametrize("fp16", [True, False], ids=["fp16", "fp32"])
@pytest.mark.parametrize("name", ["net_6b96", "tiny_all"])
def test_default_context_under_the_switch_has_the_bits_of_three_launches(name, fp16, tmp_weights_dir, monkeypatch):
    """A default context whose SE units run as kernels of their own (SAYURI_TOWER=0 SAYURI_SE_FUSED=0 SAYURI_SE_SPLIT=0), fp16 and
    the fp32 engine: SAYURI_SE_ONE=1 gives the bits of the context without it, the profile rows say which form ran, and tiny_all's
    goldens hold under the switch at their usual tolerance."""
    g = Golden(name, tmp_weights_dir)
    units = se_blocks(g.weights_path)
    assert units > 0
    outs = {}
    for se_one in (1, None):
        pipe = make_pipe(monkeypatch, g.weights_path, se_one, SEPARATE, fp16=fp16)
        try:
            outs[se_one] = [forward(pipe, sizes, 7300 + k) for k, sizes in enumerate(NET_BATCHES)]
            assert_form(launches(pipe), units, se_one == 1)
            if se_one == 1 and name == "tiny_all":
                cases = [(g.planes(c), c["board_size"], c["offset"], g.expected(c)) for c in g.cases if c.get("winograd", 1) == 1]
                check(pipe, cases, fp16_tol if fp16 else 1e-4, name + "-se-one")
        finally:
            pipe.Destroy()
    for sizes, a, b in zip(NET_BATCHES, outs[None], outs[1]):
        assert np.abs(a[0]).max() > 0
        for x, y, what in zip(a, b, ("prob", "pass", "misc", "own")):
            assert np.array_equal(x, y), (name, fp16, sizes, what, float(np.abs(x - y).max()))


# ---------------------------------------------------------------------------------------------------------------- 4. layer level
UNIT_BATCHES = SE_UNIT_BATCHES + ((2,), (3,), (19,))


def _tap(monkeypatch, se_one, *args):
    if se_one:
        monkeypatch.setenv("SAYURI_SE_ONE", "1")
    else:
        monkeypatch.delenv("SAYURI_SE_ONE", raising=False)
    try:
        return _taps.ok(_taps.se_unit(*args))
    finally:
        monkeypatch.delenv("SAYURI_SE_ONE", raising=False)


@pytest.mark.parametrize("fp16", [False, True], ids=["fp32", "fp16"])
@pytest.mark.parametrize("draw", ["spread", "probe"])
@pytest.mark.parametrize("act", [5, 1, 0])
def test_se_unit_tap_under_the_switch_has_the_bits_of_three_launches(act, draw, fp16, monkeypatch):
    """The se_unit tap (_taps.se_unit) under SAYURI_SE_ONE=1 against the tap without it, on test_gpu_smallops.py's two draws: y and the
    gate equal bit for bit, with and without a residual, and the =1 result within that file's bounds of se_unit_f64 (2e-3 / 2e-5
    of the output scale, the gate at 1e-4).  This test cannot tell which form the tap ran -- the tap has no reader for it; the
    profile rows of tests 1 and 3 prove the routing of the same launch function."""
    for C, se in SE_LAYERS:
        for bsz in UNIT_BATCHES:
            T, fc = se_inputs(draw, SE_SEED, tuple(bsz), C, se)
            xs = [se_unit_x(T, i, fp16) for i in range(len(bsz))]
            for rs in (T.rs, None):
                one = _tap(monkeypatch, True, fp16, bsz, C, se, act, xs, rs, fc)
                three = _tap(monkeypatch, False, fp16, bsz, C, se, act, xs, rs, fc)
                assert np.array_equal(one.gate, three.gate), (draw, bsz, C, se, act, fp16, rs is not None, "gate")
                for i, bs in enumerate(bsz):
                    assert np.array_equal(one.outs[i], three.outs[i]), (draw, bsz, C, se, act, fp16, rs is not None, i)
                    gamma, beta = se_gate_f64(se_pool_f64(xs[i], bs), *fc, act)
                    exp_gate = np.concatenate([gamma, beta])
                    gerr = float(np.abs(one.gate[i] - exp_gate).max()) / (1e-4 * max(1.0, float(np.abs(exp_gate).max())))
                    ref = se_apply_f64(xs[i], rs[i] if rs else None, gamma, beta, act)
                    tol = (2e-3 if fp16 else 2e-5) * max(1.0, float(np.abs(ref).max()))
                    assert np.isfinite(one.outs[i]).all()
                    assert gerr <= 1.0, (draw, bsz, C, i, "gate", gerr)
                    err = float(np.abs(one.outs[i] - ref).max())
                    assert err <= tol, (draw, bsz, C, se, act, fp16, rs is not None, i, err, tol)


@pytest.mark.parametrize("fp16", [False, True], ids=["fp32", "fp16"])
def test_se_unit_tap_under_the_switch_test_can_fail(fp16, monkeypatch):
    """as test_gpu_smallops.py's test_se_unit_kernels_test_can_fail, under SAYURI_SE_ONE=1"""
    C, se, act, bsz = 128, 32, 5, (19, 16, 14)
    T, fc = se_inputs("spread", SE_SEED, bsz, C, se)
    xs = [se_unit_x(T, i, fp16) for i in range(len(bsz))]
    w1 = fc[0].copy()
    w1[:, C:2 * C] = 0.0  # zero_scaled_mean: a valid but different weight set
    outs = _tap(monkeypatch, True, fp16, bsz, C, se, act, xs, T.rs, (w1,) + fc[1:]).outs
    for i, bs in enumerate(bsz):
        ref = se_unit_f64(xs[i], T.rs[i], *fc, bs, act)
        ratio = float(np.abs(outs[i] - ref).max()) / ((2e-3 if fp16 else 2e-5) * max(1.0, float(np.abs(ref).max())))
        print(f"SE unit, one launch, {'fp16' if fp16 else 'fp32'} without the scaled-mean columns, {bs}x{bs}: {ratio:.1f} x tol")
        assert ratio <= 1.0 if bs == 14 else ratio >= 4.0, (fp16, bs, ratio)


# ---------------------------------------------------------------------------------------------------------------- 5. not slower
def _one_against_three(board, se_one, tmp_weights_dir, monkeypatch, capsys):
    """net_20b256, one position, inputs resident: device time per forward (sayuri_hip_time_runs) of two latency contexts in one
    process -- SAYURI_SE_ONE = se_one, and SAYURI_SE_ONE=0 (the three launches: the code path before the kernel existed) --
    interleaved, a warm-up of 50, then 3 rounds of 200 forwards.  -> the medians and the spread (max - min) of the
    three-launch arm's rounds."""
    g = Golden("net_20b256", tmp_weights_dir)
    lib = _lib.hip()
    gr = grid_of(W.synthetic_planes(1, [board], seed=1), [board])
    pipes = {"one": make_pipe(monkeypatch, g.weights_path, se_one, latency=True),
             "three": make_pipe(monkeypatch, g.weights_path, 0, latency=True)}
    try:
        times = {k: [] for k in pipes}
        bs = np.asarray([board], np.int32)
        for k, p in pipes.items():
            assert lib.sayuri_hip_upload(p.ctx(0), 1, _lib.fp(gr), bs.ctypes.data_as(_lib.c_int_p)) == 0
            ms = ctypes.c_float(0)
            assert lib.sayuri_hip_time_runs(p.ctx(0), 50, ctypes.byref(ms)) == 0   # warm-up
        for _ in range(3):
            for k, p in pipes.items():
                ms = ctypes.c_float(0)
                assert lib.sayuri_hip_time_runs(p.ctx(0), 200, ctypes.byref(ms)) == 0, lib.sayuri_hip_last_error()
                times[k].append(ms.value / 200)
        assert launches(pipes["one"]).get("se_unit", 0) == se_blocks(g.weights_path) and launches(pipes["three"]).get("se_unit", 0) == 0
        one, three = float(np.median(times["one"])), float(np.median(times["three"]))
        spread = max(times["three"]) - min(times["three"])
        with capsys.disabled():
            print(f"\n[se one] net_20b256, one {board}x{board} board, device ms per forward: one launch {one:.4f}, three launches {three:.4f}, "
                  f"ratio {one / three:.3f}, spread of the three-launch rounds {spread:.4f}")
        return one, three, spread, times
    finally:
        for p in pipes.values():
            p.Destroy()


def test_one_launch_per_se_unit_is_not_slower_on_a_lone_board(tmp_weights_dir, monkeypatch, capsys):
    """One 19x19 board, the default latency context against SAYURI_SE_ONE=0: `one` must be below `three` by more than the spread
    of the three-launch arm's rounds.  The arms differ by 12 launches of a few microseconds each; the rounds of such a run differ
    by a few tenths of a microsecond.  Measured on an MI355X (profiles/r10_latency_se_one.json; DESIGN.md Kernel 1g): one launch
    0.6138 ms, three launches 0.6395, ratio 0.960; this test's own run printed 0.6138 / 0.6384 / 0.961, spread below 0.0001."""
    one, three, spread, times = _one_against_three(19, None, tmp_weights_dir, monkeypatch, capsys)
    assert three - one > spread, (one, three, spread, times)


def test_one_launch_per_se_unit_is_not_slower_on_a_small_board(tmp_weights_dir, monkeypatch, capsys):
    """The same on one 9x9 board (three workgroups per sample instead of twelve).  Measured on an MI355X: 0.5791 against
    0.6052 ms, ratio 0.957, spread 0.0001 (profiles/r10_latency_se_one.json: 0.580 / 0.609)."""
    one, three, spread, times = _one_against_three(9, None, tmp_weights_dir, monkeypatch, capsys)
    assert three - one > spread, (one, three, spread, times)
