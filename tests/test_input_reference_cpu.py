"""CPU side of tests/test_gpu_input.py: pack_image_ref (_kref.py) is held to the engine's own unpacking and packing of records
(sayuri_amd.engine, _ensemble.permute_record), the case table (_cases.py) to the rule it claims to exercise, the flat
kernel's reciprocal division is checked for every value it can meet, and every defect the reference can be given changes the
expected image of the committed cases -- so the GPU module, which compares bit for bit with that image, would see it.

The cap of the can-fail part: a defect must move at least one element in EVERY case it applies to, and apply to at least one."""
import os
import re

import numpy as np
import pytest

import _taps
from _cases import (PACK_BIT_CASES, PACK_BOTH_ROUTES, PACK_CASES, PACK_FLAT_PASS, PACK_IDS, PACK_MAX_BINARY, PACK_PLANE_CASES, PACK_SENTINEL,
                    PACK_STAGE_BATCH, PACK_SYMM_CASES, chunked_passes, pack_draw, pack_order, pack_reference, pack_rule, planes_of_records)
from _ensemble import permute_record
from _kref import PACK_DEFECTS, pack_image_ref
from sayuri_amd import _lib
from sayuri_amd.engine import expand_packed, pack_planes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def r16(a, fp16):
    return a.astype(np.float16).astype(np.float32) if fp16 else a


def launched(c):
    """[(device sample, slot, board)] of the case's launch"""
    perm, bsz = pack_order(c)
    return [(i, perm[i], bsz[i]) for i in range(c.n0, c.n0 + c.ns)]


def same(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


# ---------------------------------------------------------------------------------------------- the reference against the engine
@pytest.mark.parametrize("c", PACK_BIT_CASES + PACK_SYMM_CASES, ids=[c.name for c in PACK_BIT_CASES + PACK_SYMM_CASES])
@pytest.mark.parametrize("draw", ["placement", "rounding"])
def test_reference_shows_what_the_engine_unpacks(c, draw):
    """Every written row of the reference image is the engine's expand_packed of the sample's record -- for a symmetry case of
    the record _ensemble.permute_record builds for that symmetry -- rounded to the engine's type; everything else is the sentinel
    or the +0 of a pad channel."""
    D, B2, cs = pack_draw(c, draw), c.board ** 2, (c.cin + 31) // 32 * 32
    img = pack_reference(c, draw, PACK_SENTINEL)
    rest = np.ones(len(img), bool)
    for i, j, bs in launched(c):
        rec = D.records[j] if c.form == "bits" else permute_record(D.records[c.src[j]], c.binary, bs, c.symm[j])
        if c.beyond:   # the engine's unpacking never looks past the board either
            assert np.array_equal(pack_planes(expand_packed(rec, c.binary, bs, c.cin), c.binary)[:c.binary * 12] | rec[:c.binary * 12], rec[:c.binary * 12])
        want = np.zeros((bs * bs, cs), np.float32)
        want[:, :c.cin] = r16(expand_packed(rec, c.binary, bs, c.cin), c.fp16).T
        assert same(img[i * B2:i * B2 + bs * bs], want), (c.name, i)
        rest[i * B2:i * B2 + bs * bs] = False
    assert rest.any() and (img[rest] == np.float32(PACK_SENTINEL)).all()


@pytest.mark.parametrize("c,binary", PACK_BOTH_ROUTES, ids=[c.name for c, _ in PACK_BOTH_ROUTES])
def test_reference_gives_both_routes_one_image(c, binary):
    """pack_planes of packable planes, read back as records, is the image of the planes themselves"""
    rng = np.random.default_rng([78, binary] + list(c.cbsz))
    planes = [np.concatenate([rng.integers(0, 2, (binary, b * b)).astype(np.float32), np.repeat(rng.standard_normal((c.cin - binary, 1)).astype(np.float32), b * b, axis=1)])
              for b in c.cbsz]
    records = np.stack([pack_planes(p, binary) for p in planes])
    grid = planes_of_records(records, binary, c.cbsz, c.cin, c.board)
    for j, b in enumerate(c.cbsz):
        assert np.array_equal(grid[j].reshape(c.cin, c.board, c.board)[:, :b, :b].reshape(c.cin, b * b), planes[j])
    a = pack_reference(c, "placement", PACK_SENTINEL, planes=grid)
    b = pack_reference(c, "placement", PACK_SENTINEL, planes=None, records=records, binary=binary)
    assert same(a, b)


# ---------------------------------------------------------------------------------------------- the flat kernel's division
def test_reciprocal_division_is_exact_for_every_element_the_flat_kernel_meets():
    """pack_input_flat_kernel splits e = (c*B + y)*B + x with (int)((e + 0.5f) * (1.0f / d)) in float32.  For every grid 2..19 and
    every e < 65536 that gives e // B^2, (e % B^2) // B and e % B; small_ops.h says (e + 0.5) / d is never within 1e-3 of an
    integer there, which is why the rounding of the reciprocal and of the product cannot cross one."""
    e = np.arange(65536, dtype=np.int64)
    half = np.float32(0.5)
    for B in range(2, 20):
        B2 = B * B
        r_b2, r_b = np.float32(1.0) / np.float32(B2), np.float32(1.0) / np.float32(B)
        c = ((e.astype(np.float32) + half) * r_b2).astype(np.int64)   # the cast truncates, as (int) does
        r = e - c * B2
        y = ((r.astype(np.float32) + half) * r_b).astype(np.int64)
        x = r - y * B
        assert np.array_equal(c, e // B2) and np.array_equal(y, (e % B2) // B) and np.array_equal(x, e % B), B
        for d in (B2, B):
            frac = (e + 0.5) / d
            assert np.abs(frac - np.rint(frac)).min() > 1e-3, (B, d)


def test_the_flat_condition_keeps_every_index_below_65536():
    """The flat kernel visits e < total rounded up to whole passes of 16 384; the engine takes it only for total < 65536 (and a
    sample that fits 64 KiB), so no e reaches 65536 -- at any grid or channel count, in both types.  The condition is read out of
    engine_plan.h as well: the restatement in _cases.pack_rule is not its only witness."""
    text = open(os.path.join(ROOT, "sayuri_amd", "csrc", "hip", "engine_plan.h")).read()
    assert re.search(r"flat_lds <= 64 \* 1024 && \(size_t\)cin \* board \* board < 65536", text)
    seen = 0
    for fp16 in (True, False):
        for board in range(2, 26):
            for cin in range(1, 513):
                kernel, _, passes = pack_rule(fp16, cin, board)
                if kernel == "flat":
                    seen += 1
                    assert passes * PACK_FLAT_PASS - 1 < 65536 and cin * board * board < 65536
    assert seen > 1000


# ---------------------------------------------------------------------------------------------- the case table
def test_the_cases_reach_the_branches_they_name():
    """By the restated rule: the kernel each plane case names, one pass or more; and between them the table holds what the suite's
    nets never reach -- the chunked kernel in fp16, its second pass in both types, the flat kernel in fp32 and its second base pass --
    every board 2..19, the grids 9, 13 and 19, cin 43, 38, 64 and 6, both bit kernels split, in place, staged and resident."""
    reached = set()
    for c in PACK_PLANE_CASES:
        kernel, chunk, base = pack_rule(c.fp16, c.cin, c.board)
        passes = base if kernel == "flat" else max(chunked_passes(chunk, bs) for _, _, bs in launched(c))
        assert (kernel, passes > 1) == (c.kernel, c.multi), (c.name, kernel, chunk, passes)
        reached.add((kernel, c.fp16, passes > 1))
    assert reached == {(k, t, m) for k in ("flat", "chunked") for t in (True, False) for m in (False, True)} - {("flat", False, True)}
    assert pack_rule(False, 192, 19)[1] == 83 and pack_rule(True, 384, 19)[1] == 83 and pack_rule(True, 352, 19)[1] == 91   # cs >= 353 is the first with two passes
    assert pack_rule(True, 64, 19) == ("flat", 0, 2) and pack_rule(True, 65, 19)[0] == "chunked" and pack_rule(False, 43, 15)[0] == "flat" and pack_rule(False, 43, 16)[0] == "chunked"
    for form, cases in (("planes", PACK_PLANE_CASES), ("records", PACK_BIT_CASES + PACK_SYMM_CASES)):
        assert {bs for c in cases for _, _, bs in launched(c)} == set(range(2, 20)), form
        assert {c.board for c in cases} == {9, 13, 19}, form
    assert {c.cin for c in PACK_PLANE_CASES} >= {43, 38, 64, 6, 96, 192, 384}
    assert {(c.cin, c.binary) for c in PACK_BIT_CASES} >= {(43, 37), (38, 34), (6, 2), (48, PACK_MAX_BINARY)}
    for cases in (PACK_BIT_CASES, PACK_SYMM_CASES):
        assert {(c.stage, c.in_place) for c in cases} == {(0, 0), (0, 1), (1, 0), (1, 1)} and any(c.beyond for c in cases)
        assert {c.fp16 for c in cases} == {True, False}
    for c in PACK_CASES:
        n = len(c.cbsz)
        assert n <= 16 and n < PACK_STAGE_BATCH and 0 <= c.n0 and c.n0 + c.ns <= n and c.split == (1 if c.kernel == "flat" or c.in_place else 4)
    assert any(c.n0 > 0 and c.n0 + c.ns < len(c.cbsz) for c in PACK_CASES) and any(c.perm is None for c in PACK_CASES)
    for c in PACK_SYMM_CASES[:9]:   # all eight symmetries of each record, the two records of two board sizes
        assert sorted(zip(c.src, c.symm)) == [(r, s) for r in (0, 1) for s in range(8)] and len({b for b in c.cbsz}) == 2


# ---------------------------------------------------------------------------------------------- the tests can fail
def applies(defect, c, draw):
    rows = launched(c)
    records = c.form != "planes"
    if defect == "round_toward_zero":
        return draw == "rounding" and c.fp16 and (not records or c.cin > c.binary)
    if draw != "placement":
        return False
    if defect in ("swap_xy", "lost_last_cell"):
        return True
    if defect == "sample_stride_on_grid":
        return not records and any(bs < c.board for _, _, bs in rows)
    if defect == "grid_stride_on_sample":
        return records and any(bs < c.board for _, _, bs in rows)
    if defect == "perm_backwards":
        perm, _ = pack_order(c)
        return c.perm is not None and any(int(np.argsort(perm)[i]) != j for i, j, _ in rows)
    if defect == "map_ignored":
        return c.form == "symm" and any(c.src[j] != j % c.nrec for _, j, _ in rows)
    if defect.startswith("symm_bit_"):
        return c.form == "symm" and any(c.symm[j] & int(defect[-1]) for _, j, _ in rows)
    if defect == "pad_nonzero":
        return c.cin % 32 != 0
    if defect == "scalar_neighbour":
        return records and c.cin > c.binary
    raise AssertionError(defect)


@pytest.mark.parametrize("defect", PACK_DEFECTS)
def test_every_defect_changes_the_expected_image(defect):
    """x and y swapped, one grid's stride where the other's belongs, the last cell of a workgroup's pixel range lost, perm applied
    backwards, the record map or one symmetry bit ignored, a pad channel that is not 0, a scalar from the neighbouring plane, and
    -- on the rounding draw -- rounding toward zero: each moves at least one element of the expected image in every case it
    applies to, and each applies to at least one."""
    hit = 0
    for c in PACK_CASES:
        for draw in ("placement", "rounding"):
            if not applies(defect, c, draw):
                continue
            good, bad = pack_reference(c, draw, PACK_SENTINEL), pack_reference(c, draw, PACK_SENTINEL, defect=defect)
            moved = int(np.count_nonzero(good.view(np.uint32) != bad.view(np.uint32)))
            assert moved >= 1, (defect, c.name, draw, "the defect leaves the expected image as it is")
            hit += 1
    assert hit >= 1, (defect, "applies to no case")


def test_pad_channels_are_plus_zero_and_compared_by_their_bits():
    """a -0 in a pad channel is a difference to the comparison the GPU module makes"""
    c = PACK_PLANE_CASES[0]
    good = pack_reference(c, "placement", PACK_SENTINEL)
    i, _, bs = launched(c)[0]
    row = i * c.board ** 2
    assert not np.signbit(good[row, c.cin:]).any() and not good[row, c.cin:].any()
    bad = good.copy()
    bad[row, c.cin] = -0.0
    assert np.array_equal(good, bad) and not same(good, bad)


# ---------------------------------------------------------------------------------------------- the binding
def test_the_new_tap_is_in_the_header_and_in_the_table():
    header = open(os.path.join(ROOT, "include", "sayuri_hip.h")).read()
    for name in _taps.PACK_TAPS:
        assert name in _lib.HIP_ABI and re.search(r"\bint " + name + r"\(", header)
    assert len(_lib.HIP_ABI[_taps.PACK_TAPS[0]][1]) == 20
    assert "at most 40 bit planes" in header and f"kPackedMaxBinary = {PACK_MAX_BINARY};" in open(os.path.join(ROOT, "sayuri_amd", "csrc", "hip", "small_ops.h")).read()
    host = open(os.path.join(ROOT, "sayuri_amd", "csrc", "host", "packed_planes.h")).read()
    assert f"kMaxBinary = {PACK_MAX_BINARY};" in host   # the host's limit and the device's are one number
