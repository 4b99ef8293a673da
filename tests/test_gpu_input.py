"""The input stage at the image: what pack_input_kernel, pack_input_flat_kernel, pack_bits_kernel and pack_bits_symm_kernel
(csrc/hip/small_ops.h) leave in the input convolution's NHWC buffer, through the pack_input tap of _taps.py -- the kernel, its
chunk, LDS and workgroups per sample chosen by the engine's own pack_plan (engine_plan.h) -- against pack_image_ref (_kref.py),
bit for bit: no tolerance anywhere in this module.

The whole image and a guard region behind it start as a sentinel and come back raw: every row of every slot, every pad channel.
So a case sees a lost or misplaced cell, a value rounded otherwise than to nearest even, a pad channel that is not +0, a row
>= bs*bs or a slot outside [n0, n0 + ns) that was written, and a store past the last slot.  Two draws per case (_cases.py):
"placement", where a sample's values differ from one another and from sample to sample, and "rounding", fp32 values that are
no fp16 values (ties of both parities, the ends of the normal range).  tests/test_input_reference_cpu.py pins the reference to
the engine's own unpacking and shows that each defect it names changes the expected image of these very cases.

Every case asserts what the tap reports: the kernel that ran, the channel stride, the workgroups per sample, and whether there
was more than one pass -- the count is read from the report, not assumed."""
import numpy as np
import pytest

import _taps
from _cases import (F16_OFF_BOARD, F32_OFF_BOARD, PACK_BOTH_ROUTES, PACK_CASES, PACK_GUARD_ROWS, PACK_IDS, PACK_MAX_BINARY, PACK_SENTINEL,
                    PACK_STAGE_BATCH, PACK_SYMM_CASES, pack_draw, pack_order, pack_reference, planes_of_records)
from _golden import Golden
from sayuri_amd import hipraw
from sayuri_amd.engine import pack_planes
from sayuri_amd.pipe import HipForwardPipe

pytestmark = pytest.mark.gpu


def run_case(c, draw, **inputs):
    """the tap on the case (inputs: planes= / records= in place of the draw's) -> its result, the report asserted"""
    D = pack_draw(c, draw)
    perm, bsz = pack_order(c)
    args = dict(planes=D.planes, records=D.records)
    args.update(inputs)
    r = _taps.ok(_taps.pack_input(c.fp16, bsz, c.cin, PACK_SENTINEL, binary=0 if args["planes"] is not None else c.binary, src=c.src, symm=c.symm,
                                  n_records=0 if args["planes"] is not None else c.nrec, perm=None if c.perm is None else perm, n0=c.n0, ns=c.ns,
                                  stage_batch=PACK_STAGE_BATCH if c.stage else 0, in_place=bool(c.in_place), guard_rows=PACK_GUARD_ROWS,
                                  max_board=c.board, **args), c.name, draw)
    return r


def assert_same_image(r, exp, what):
    got = np.concatenate([r.image.reshape(-1, r.cs), r.guard])
    assert got.shape == exp.shape, (what, got.shape, exp.shape)
    bad = np.argwhere(got.view(np.uint32) != exp.view(np.uint32))
    assert bad.size == 0, (what, len(bad), "elements differ; the first (row of the buffer, channel, got, expected):",
                           [(int(p), int(ch), float(got[p, ch]), float(exp[p, ch])) for p, ch in bad[:8]])
    return got.size


@pytest.mark.parametrize("draw", ["placement", "rounding"])
@pytest.mark.parametrize("c", PACK_CASES, ids=PACK_IDS)
def test_input_image_is_the_reference_bit_for_bit(c, draw):
    r = run_case(c, draw)
    passes = r.passes
    print(f"{c.name} [{draw}]: kernel {r.kernel}, cs {r.cs}, {r.split} workgroup(s) per sample, {passes} pass(es)")
    assert (r.kernel, r.cs, r.split) == (c.kernel, (c.cin + 31) // 32 * 32, c.split), (c.name, r.kernel, r.cs, r.split)
    assert (passes > 1) == c.multi and passes >= 1, (c.name, "passes per workgroup (chunked) or base passes (flat):", passes)
    compared = assert_same_image(r, pack_reference(c, draw, PACK_SENTINEL), (c.name, draw))
    print(f"{c.name} [{draw}]: {compared} elements equal")
    if c.form == "planes" and draw == "placement":   # the off-board cells of the NN grid hold a value of their own: it went nowhere
        off = F16_OFF_BOARD.view(np.float16).astype(np.float32) if c.fp16 else F32_OFF_BOARD
        assert not (r.image == off).any() and not (r.guard == off).any(), (c.name, "an off-board cell of the NN grid reached the image")


@pytest.mark.parametrize("c", PACK_SYMM_CASES[:9], ids=[c.name for c in PACK_SYMM_CASES[:9]])
def test_every_symmetry_shows_another_image(c):
    """A kernel that ignored symm would agree with itself: the seven other symmetries of a record differ from its symmetry 0, in
    what the kernel wrote as in the reference."""
    r = run_case(c, "placement")
    perm, bsz = pack_order(c)
    exp = pack_reference(c, "placement", PACK_SENTINEL)[:len(bsz) * c.board ** 2].reshape(r.image.shape)
    at = {(c.src[j], c.symm[j]): i for i, j in enumerate(perm)}   # (record, symmetry) -> device sample
    for rec in range(c.nrec):
        for s in range(1, 8):
            for img in (r.image, exp):
                assert not np.array_equal(img[at[rec, s]], img[at[rec, 0]]), (c.name, "record", rec, "symmetry", s, "shows what symmetry 0 shows")


@pytest.mark.parametrize("c,binary", PACK_BOTH_ROUTES, ids=[c.name for c, _ in PACK_BOTH_ROUTES])
def test_planes_and_records_leave_one_image(c, binary):
    """Packable planes through the plane kernel of the case and as records through pack_bits_kernel: one image, element for
    element (the net tests compare the two routes at the outputs)."""
    rng = np.random.default_rng([77, binary] + list(c.cbsz))
    scal = rng.standard_normal((len(c.cbsz), 8)).astype(np.float32)
    records = np.stack([pack_planes(np.concatenate([rng.integers(0, 2, (binary, b * b)).astype(np.float32),
                                                    np.repeat(scal[j, :c.cin - binary, None], b * b, axis=1)]), binary) for j, b in enumerate(c.cbsz)])
    planes = planes_of_records(records, binary, c.cbsz, c.cin, c.board)
    a = run_case(c, "placement", planes=planes, records=None)
    perm, bsz = pack_order(c)
    b = _taps.ok(_taps.pack_input(c.fp16, bsz, c.cin, PACK_SENTINEL, records=records, binary=binary, perm=None if c.perm is None else perm, n0=c.n0, ns=c.ns,
                                  guard_rows=PACK_GUARD_ROWS, max_board=c.board), c.name)
    assert a.kernel == c.kernel and b.kernel == "bits"
    assert np.array_equal(a.image.view(np.uint32), b.image.view(np.uint32)) and np.array_equal(a.guard.view(np.uint32), b.guard.view(np.uint32)), c.name
    assert_same_image(a, pack_reference(c, "placement", PACK_SENTINEL, planes=planes), c.name)


def test_the_tap_refuses_what_the_engine_refuses():
    """More bit planes than a record holds (the bit kernels' LDS copy has kPackedMaxBinary planes), a board off the grid, a slot, a
    record or a symmetry that does not exist: refused with a message before anything is launched."""
    rec = np.zeros((2, 41 * 12 + 8), np.uint32)
    for fp16 in (True, False):
        r = _taps.pack_input(fp16, [19, 9], 43, PACK_SENTINEL, records=rec, binary=41)
        assert r.rc == -1 and f"at most {PACK_MAX_BINARY}" in _taps.last_error() and r.kernel is None, (r.rc, _taps.last_error())
    rec = np.zeros((2, 37 * 12 + 8), np.uint32)
    for kw, what in ((dict(binary=0), "bad binary plane count"), (dict(binary=30), "bad binary plane count"),
                     (dict(binary=37, perm=[0, 2]), "perm"), (dict(binary=37, symm=[0, 8]), "is no board symmetry"),
                     (dict(binary=37, symm=[0, 1], src=[0, 2]), "is outside the 2 records"), (dict(binary=37, n0=1, ns=2), "sample range")):
        r = _taps.pack_input(True, [19, 9], 43, PACK_SENTINEL, records=rec, **kw)
        assert r.rc == -1 and what in _taps.last_error() and r.kernel is None, (kw, r.rc, _taps.last_error())
    r = _taps.pack_input(True, [19, 20], 43, PACK_SENTINEL, records=rec, binary=37)
    assert r.rc == -1 and "board size" in _taps.last_error()


def test_forward_packed_refuses_more_bit_planes_than_a_record_holds(tmp_weights_dir):
    """On a 43-plane net binary_planes = 41, 42, 43 passed the engine's check and overran the bit kernels' record copy and the
    record buffer.  Now refused, with the limit in the message, and the context goes on: the next good call gives the bits it gave."""
    g = Golden("tiny_res", tmp_weights_dir)
    bsz = [19, 9, 13]
    rng = np.random.default_rng(5)
    planes = [np.concatenate([rng.integers(0, 2, (37, b * b)).astype(np.float32), np.repeat(rng.standard_normal((6, 1)).astype(np.float32), b * b, axis=1)])
              for b in bsz]
    records = np.stack([pack_planes(p, 37) for p in planes])
    pipe = HipForwardPipe(g.weights_path, board_size=19, batch_size=8, fp16=True)
    try:
        ctx = pipe.ctx(0)
        before = hipraw.hip_forward_packed_raw(ctx, records, 37, bsz, 19)
        for binary in (41, 42, 43):
            with pytest.raises(RuntimeError, match=f"at most {PACK_MAX_BINARY}"):
                hipraw.hip_forward_packed_raw(ctx, np.zeros((3, binary * 12 + 8), np.uint32), binary, bsz, 19)
        after = hipraw.hip_forward_packed_raw(ctx, records, 37, bsz, 19)
        for a, b in zip(before, after):
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
        assert np.abs(before[0]).max() > 0
    finally:
        pipe.Destroy()
