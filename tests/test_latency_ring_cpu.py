"""CPU-only checks of the latency context's weight ring (csrc/hip/conv_split.h: conv_split_kernel<NJ, ST>; csrc/hip/engine_plan.h:
split_ring, SAYURI_LATENCY_RING; include/sayuri_hip.h: sayuri_hip_split_ring_plan).

  * The plan.  sayuri_hip_split_ring_plan is host arithmetic of the real device library, which loads without a device: the
    ring split_plan gives a batch and a layer width, under the engine's rule and forced.
  * The code object.  The cross-compiled library holds the deep instantiations for the thin variants and the three-stage
    kernel for all five; the template arguments are read from the symbol names.
"""
import os
import re
import subprocess

import numpy as np
import pytest

from _cases import SPLIT_EXACT, split_strips
from sayuri_amd import _build, _lib
from test_kernel_hygiene import OBJDUMP, device_code_object

DEEP = 4                      # the deep ring's stages (conv_split.h: kSplitDeepStages)
THIN = (1, 2, 3)              # the column tiles per wave that have a deep instantiation
ALL_NJ = (1, 2, 3, 6, 12)
MIXED15 = [19, 9, 13, 9, 19, 13, 9, 9, 19, 13, 7, 19, 9, 13, 16]


def lib():
    if not os.path.exists(_build.HIP_SO):
        _build.build_hip()
    return _lib.hip()


def plan(bsz, cout, strips=0, ring=0):
    return lib().sayuri_hip_split_ring_plan(len(bsz), _lib.ip(np.asarray(bsz, np.int32)), 19, cout, strips, ring)


def last_error():
    return lib().sayuri_hip_last_error().decode()


def test_split_ring_plan():
    """The engine's rule: a lone 19x19 board (19 strips of one row, NJ = 1) runs the deep ring at 256 and at 384 channels, 64 full
    boards (one strip each, NJ = 12) three stages; SAYURI_LATENCY_RING=3's value gives three stages everywhere; a deep ring
    forced on NJ = 12 and a layer of 96 weight rows are refused with a message; the order of a mixed batch's boards does not
    matter."""
    for cout in (256, 384):
        assert plan([19], cout) == DEEP, (cout, last_error())
        assert plan([19] * 64, cout) == 3
        assert plan([9], cout) == DEEP and plan([13], cout) == DEEP
    for bsz in ([19], [9], [19] * 8, [19] * 64, MIXED15):
        for cout in (64, 128, 256, 384):
            for strips in (0, 1, 2, 4, 19):
                assert plan(bsz, cout, strips, 3) == 3, (bsz, cout, strips, last_error())
    # forced: the deep ring exists for NJ = 1, 2, 3 (19, 7 and 4 strips of a 19x19 board) and for nothing wider
    for strips, want in ((19, DEEP), (7, DEEP), (4, DEEP), (2, -1), (1, -1)):
        assert plan([19], 256, strips, DEEP) == want, strips
    assert plan([19] * 64, 256, 0, DEEP) == -1
    msg = last_error()
    assert "ring" in msg and str(DEEP) in msg, msg
    assert plan([19], 256, 19, 8) == -1 and "ring" in last_error()      # a depth that no instantiation has
    assert plan([19], 256, 0, -1) == -1 and "ring" in last_error()
    assert plan([19], 96, 0, 0) == -1
    assert "64-channel" in last_error(), last_error()
    assert plan([], 256) == -1 and plan([19, 23], 256) == -1
    # a mixed batch: the same plan whatever the order of its boards
    rng = np.random.default_rng(5)
    for cout in (256, 384):
        for strips in (0, 4, 19):
            for ring in (0, 3, DEEP):
                want = plan(MIXED15, cout, strips, ring)
                for _ in range(6):
                    assert plan(list(rng.permutation(MIXED15)), cout, strips, ring) == want, (cout, strips, ring)
    # the rule looks at NJ only: deep at NJ = 1, three stages from NJ = 2 on (4 and 16 full boards: 16 and 4 strips each)
    for cout in (256, 384):
        assert plan([19] * 2, cout) == DEEP and plan([9] * 2, cout) == DEEP
        assert plan([19], cout, 19) == DEEP and plan([19], cout, 7) == 3 and plan([19], cout, 4) == 3 and plan([19], cout, 2) == 3
    assert plan([19] * 4, 256) == 3 and plan([19] * 16, 256) == 3 and plan([9] * 16, 256) == DEEP


def test_exact_cases_reach_the_deep_ring():
    """tests/test_gpu_latency_ring.py runs the SPLIT_EXACT cases under the forced deep ring at the strip counts where the plan
    function says it exists and fits: that is at least half of every case's strip counts."""
    for c in SPLIT_EXACT:
        ran = [s for s in split_strips(c.bsz) if plan(list(c.bsz), c.cout, s, DEEP) == DEEP]
        assert 2 * len(ran) >= len(split_strips(c.bsz)), (c, ran)


@pytest.mark.skipif(not os.path.exists(OBJDUMP), reason="needs the ROCm llvm tools")
def test_split_kernel_instantiations(tmp_path):
    """conv_split_kernel<NJ, ST> in the gfx950 code object: ST = 3 for every NJ, a deeper ring for NJ = 1, 2, 3 and for no other."""
    so = _build.HIP_SO
    if not os.path.exists(so):
        _build.build_hip()
    co = device_code_object(so, tmp_path)
    syms = subprocess.run([OBJDUMP, "-t", co], capture_output=True, text=True, check=True).stdout
    have = set()
    for m in re.finditer(r"conv_split_kernelILi(\d+)ELi(\d+)EE\w*", syms):
        if not m.group(0).endswith(".kd"):
            have.add((int(m.group(1)), int(m.group(2))))
    assert {(nj, 3) for nj in ALL_NJ} <= have, sorted(have)
    deep = {(nj, st) for nj, st in have if st > 3}
    assert {nj for nj, _ in deep} == set(THIN), sorted(have)
    assert {st for _, st in deep} == {DEEP}, sorted(have)
