"""The latency context's weight ring (csrc/hip/conv_split.h: conv_split_kernel<NJ, ST>; SAYURI_LATENCY_RING and split_ring,
csrc/hip/engine_plan.h): the thin strips of a small batch (NJ = 1, 2, 3 column tiles per wave) have a kernel with a ring of four
weight groups instead of three whose K loop waits for nothing but its DMA counts, and the engine's rule runs it at NJ = 1.  The
K order is the three-stage kernel's, so the checks are on BITS:
  layer level  the conv_split tap under SAYURI_LATENCY_RING = 3, the deep value and unset == the board kernel (conv tap, kind 2),
               on the smallest shapes that reach each hazard of the deeper ring                                        (test 1)
  exact        the SPLIT_EXACT cases of _cases.py against their one correct output, under the forced deep ring         (test 2)
  whole net    latency contexts under the switch = 3, the deep value and unset give the same four outputs, and
               sayuri_hip_last_split_ring says which ring ran                                                          (test 3)
  batch mates  with the switch unset a position's bits do not depend on a batch that crosses the rule's boundary       (test 4)
tests/_pipes.make_pipe does not know the switch: it is set and cleared here, around pipe creation and around every tap call.
"""
import numpy as np
import pytest

import _pipes
import _taps
from _cases import SPLIT_EXACT, case_id, layer_reference, split_strips
from _golden import Golden
from _kref import assert_exact
from _pipes import Pinned, Pool
from _taps import KIND_BOARD, KIND_SPLIT
from sayuri_amd import _lib
from sayuri_amd import weights as W
from sayuri_amd.pipe import hip_forward_raw
from test_gpu_latency import BATCHES, VARIANTS, _layer_tensors, grid_of

pytestmark = pytest.mark.gpu

B = 19
DEEP = 4          # conv_split.h: kSplitDeepStages
SWITCH = "SAYURI_LATENCY_RING"
EPILOGUES = VARIANTS[:2] + [(0, False)]   # Mish with and without the residual, and no residual + identity


def last_ring(ctx=None):
    return int(_lib.hip().sayuri_hip_last_split_ring(ctx))


def ring_plan(bsz, cout, strips, ring):
    return int(_lib.hip().sayuri_hip_split_ring_plan(len(bsz), _lib.ip(np.asarray(bsz, np.int32)), B, cout, strips, ring))


def under(monkeypatch, ring):
    if ring is None:
        monkeypatch.delenv(SWITCH, raising=False)
    else:
        monkeypatch.setenv(SWITCH, str(ring))


def tap_split(monkeypatch, ring, *args):
    """the conv_split tap under SAYURI_LATENCY_RING = ring (None: unset); the tap reads the switch per call"""
    under(monkeypatch, ring)
    try:
        return _taps.ok(_taps.conv_split(*args), ring, args[0], args[-1])
    finally:
        monkeypatch.delenv(SWITCH, raising=False)


def make_pipe(monkeypatch, path, ring=None, env=None, **kw):
    """_pipes.make_pipe under SAYURI_LATENCY_RING = ring (None: unset); the switch is read when the context is created."""
    under(monkeypatch, ring)
    try:
        return _pipes.make_pipe(path, env, **{"batch": 64, **kw})
    finally:
        monkeypatch.delenv(SWITCH, raising=False)


# ---------------------------------------------------------------------------------------------------------------- 1. layer level
HAZARDS = [
    # bsz, cin, cout, strips (19 strips of a 19x19 board: NJ = 1; 7: NJ = 2; 4: NJ = 3 and 192 halo positions)
    ([19], 32, 128, (19, 4)),                      # one chunk, three groups: fewer than the ring, no halo ahead
    ([13, 9, 9, 19, 13, 9], 43, 128, (19, 4)),     # two chunks, six groups; mixed boards leave strips of the grid idle
    ([19], 96, 128, (19, 7)),                      # 9 groups: no multiple of the ring
    ([19, 13], 384, 384, (19, 4)),                 # 36 groups, the halo prefetch across twelve chunks
    ([19], 256, 256, (19, 7, 4)),                  # 24 groups, every thin NJ and its halo size
    ([9], 256, 256, (3,)),                         # NJ = 1 with three rows per strip
]


@pytest.mark.parametrize("case", HAZARDS, ids=[f"{c[1]}x{c[2]}n{len(c[0])}b{min(c[0])}" for c in HAZARDS])
def test_deep_ring_has_the_board_kernels_bits(case, monkeypatch):
    """Every forced split of every epilogue under the three-stage ring, the deep ring and the engine's rule gives the fp16 outputs
    of the one-workgroup-per-board kernel, and sayuri_hip_last_split_ring(NULL) names the forced ring after each forced call."""
    bsz, cin, cout, strip_counts = case
    for k, (act, with_res) in enumerate(EPILOGUES):
        xs, w, bias, res = _layer_tensors(bsz, cin, cout, with_res, seed=cin + cout + 11 * k)
        board = _taps.ok(_taps.conv(True, bsz, cin, cout, 3, act, xs, w, bias, res))
        assert board.kind == KIND_BOARD, "the yardstick is the board kernel"
        for strips in strip_counts:
            for ring in (3, DEEP, None):
                t = tap_split(monkeypatch, ring, bsz, cin, cout, act, xs, w, bias, res, strips)
                assert t.kind == KIND_SPLIT
                if ring is not None:
                    assert last_ring() == ring, (case, strips, ring)
                else:
                    assert last_ring() == ring_plan(bsz, cout, strips, 0), (case, strips)
                for y, yb in zip(t.outs, board.outs):
                    assert np.array_equal(y, yb), (case, act, with_res, strips, ring, float(np.nanmax(np.abs(y - yb))))


def test_a_ring_no_variant_has_is_refused(monkeypatch):
    """The deep ring forced on a strip of twelve column tiles per wave, and a depth no variant has (8): -1 and a message."""
    x, w = [np.zeros((64, 361), np.float32)], np.zeros(128 * 64 * 9, np.float32)
    for ring, strips in ((DEEP, 1), (8, 19)):
        under(monkeypatch, ring)
        try:
            assert _taps.conv_split([19], 64, 128, 0, x, w, None, strips=strips).rc == -1
            assert "ring" in _taps.last_error() and str(ring) in _taps.last_error()
        finally:
            monkeypatch.delenv(SWITCH, raising=False)


# ---------------------------------------------------------------------------------------------------------------- 2. exact arithmetic
@pytest.mark.parametrize("c", SPLIT_EXACT, ids=case_id)
def test_deep_ring_exact(c, monkeypatch):
    """test_gpu_exact.py's test_split_kernel_exact under the forced deep ring, at the strip counts where the plan function says the
    deep ring exists and fits -- at least half of every case's (tests/test_latency_ring_cpu.py checks the same without a GPU)."""
    (xs, w, bias, res), exp = layer_reference(c)
    ran = 0
    for strips in split_strips(c.bsz):
        if ring_plan(list(c.bsz), c.cout, strips, DEEP) != DEEP:
            continue
        t = tap_split(monkeypatch, DEEP, c.bsz, c.cin, c.cout, c.act, xs, w, bias, res, strips)
        assert t.kind == KIND_SPLIT and last_ring() == DEEP, (c, strips, t.kind)
        assert_exact(t.outs, exp, (c, "strips", strips, "ring", DEEP))
        ran += 1
    assert 2 * ran >= len(split_strips(c.bsz)), (c, ran)


# ---------------------------------------------------------------------------------------------------------------- 3. whole net
NET_BATCHES = BATCHES + [[19] * 16]   # [9], [13], [19], the mixed batch of 15, sixteen full boards


@pytest.mark.parametrize("name", ["net_20b256", "net_40b384"])
def test_latency_contexts_agree_across_rings(name, tmp_weights_dir, monkeypatch):
    """Latency contexts under SAYURI_LATENCY_RING=3, under the deep value and with the switch unset: the same four outputs, bit for
    bit.  The forced deep context runs 4 strips per board (SAYURI_LATENCY_SPLIT=4: NJ = 3, 2, 1 for boards of 19, 13 and 9, so
    every launch has a deep variant whatever the batch).  sayuri_hip_last_split_ring: the deep ring after a lone 19x19 board
    under the rule, three stages after 64 full boards and everywhere under =3, nothing (0) in a default context."""
    g = Golden(name, tmp_weights_dir)
    three = make_pipe(monkeypatch, g.weights_path, 3, latency=True)
    deep = make_pipe(monkeypatch, g.weights_path, DEEP, {"SAYURI_LATENCY_SPLIT": "4"}, latency=True)
    rule = make_pipe(monkeypatch, g.weights_path, None, latency=True)
    plain = make_pipe(monkeypatch, g.weights_path, None)
    try:
        assert last_ring(rule.ctx(0)) == 0      # nothing ran yet
        for k, sizes in enumerate(NET_BATCHES):
            gr = grid_of(W.synthetic_planes(len(sizes), sizes, seed=8100 + k), sizes)
            a = hip_forward_raw(three.ctx(0), gr, sizes, B)
            assert np.abs(a[0]).max() > 0
            assert last_ring(three.ctx(0)) == 3, sizes
            for arm, pipe in (("deep", deep), ("rule", rule)):
                for x, y, what in zip(a, hip_forward_raw(pipe.ctx(0), gr, sizes, B), ("prob", "pass", "misc", "own")):
                    assert np.array_equal(x, y), (name, arm, sizes, what, float(np.abs(x - y).max()))
            assert last_ring(deep.ctx(0)) == DEEP, sizes
            if sizes == [19]:
                assert last_ring(rule.ctx(0)) == DEEP
        sizes = [19] * 64
        gr = grid_of(W.synthetic_planes(64, sizes, seed=8110), sizes)
        a, b = hip_forward_raw(three.ctx(0), gr, sizes, B), hip_forward_raw(rule.ctx(0), gr, sizes, B)
        assert last_ring(rule.ctx(0)) == 3 and last_ring(three.ctx(0)) == 3
        for x, y in zip(a, b):
            assert np.array_equal(x, y)
        hip_forward_raw(plain.ctx(0), gr[:1], [19], B)
        assert last_ring(plain.ctx(0)) == 0
    finally:
        for p in (three, deep, rule, plain):
            p.Destroy()


# ---------------------------------------------------------------------------------------------------------------- 4. batch mates
@pytest.mark.parametrize("name", ["net_20b256", "net_40b384"])
def test_a_position_does_not_depend_on_batches_that_cross_the_ring_rule(name, tmp_weights_dir, monkeypatch):
    """Switch unset.  A 19x19 probe alone runs the deep ring; inside [19] * 30 + [13] * 3 + [9] * 2 and inside 40 boards of 9x9 its
    launches are one strip per board, NJ = 12, three stages: the same bits.  The second of these batches is submitted on one
    ticket while another batch is in flight on the other."""
    g = Golden(name, tmp_weights_dir)
    pool = Pool()
    probe = int(pool.by_size[19][3])
    nines, full, mid = pool.by_size[9], pool.by_size[19], pool.by_size[13]
    mates = [np.concatenate([full[4:20], full[21:35], [probe], mid[:3], nines[:2]]),   # the probe at sample 30 of 36
             np.concatenate([nines[:17], [probe], np.resize(nines, 23)])]              # ... and at 17 of 41
    other = np.concatenate([mid[5:12], full[:3]])
    pipe = make_pipe(monkeypatch, g.weights_path, None, latency=True)
    pinned = Pinned()
    try:
        ctx = pipe.ctx(0)
        alone = [np.array(t[0]) for t in hip_forward_raw(ctx, pool.grid[[probe]], pool.bsz[[probe]], B)]
        assert np.abs(alone[0]).max() > 0 and last_ring(ctx) == DEEP
        idx = mates[0]
        got = hip_forward_raw(ctx, pool.grid[idx], pool.bsz[idx], B)
        assert last_ring(ctx) == 3
        at = int(np.flatnonzero(idx == probe)[0])
        for a, b, what in zip(alone, got, ("prob", "pass", "misc", "own")):
            assert np.array_equal(a, np.array(b[at])), (name, 0, what)
        idx = mates[1]
        tick = [pinned.submit(ctx, 0, pool, other, False), pinned.submit(ctx, 1, pool, idx, False)]
        got_other = pinned.wait(ctx, 0, tick[0], len(other))
        got = pinned.wait(ctx, 1, tick[1], len(idx))
        at = int(np.flatnonzero(idx == probe)[0])
        for a, b, what in zip(alone, got, ("prob", "pass", "misc", "own")):
            assert np.array_equal(a, np.array(b[at])), (name, 1, what)
        solo_other = hip_forward_raw(ctx, pool.grid[other], pool.bsz[other], B)
        for a, b in zip(solo_other, got_other):
            assert np.array_equal(a, b)
    finally:
        pinned.close()
        pipe.Destroy()
