"""conv_dw.h without a GPU: the plan (sayuri_hip_dw_plan is host arithmetic) and the code object inside libsayuri_hip.so."""
import os
import re
import subprocess

import numpy as np
import pytest

from sayuri_amd import _build, _lib
from test_kernel_hygiene import OBJDUMP, READELF, device_code_object

KIB = 1024
DW_MAX_LDS = 64 * KIB  # kDwMaxLds
DW_K = (3, 5, 7)


def plan(bsz, channels, k, strips=0, max_board=19):
    """-> (rc, {slice, strips, grid, lds})"""
    out = np.zeros(4, np.int32)
    rc = _lib.hip().sayuri_hip_dw_plan(len(bsz), _lib.ip(np.asarray(bsz, np.int32)), max_board, channels, k, strips, _lib.ip(out))
    return rc, dict(zip(("slice", "strips", "grid", "lds"), (int(v) for v in out)))


def cut(bs, strips, k):
    """the items of one slice of a bs x bs board (dw_rows, conv_dw.h): [(first row, end row, first staged row, end staged row)]"""
    rp = -(-bs // max(1, min(strips, bs)))
    return [(r0, min(bs, r0 + rp), max(0, r0 - k // 2), min(bs, min(bs, r0 + rp) + k // 2)) for r0 in range(0, bs, rp)]


def lds_of(items, bs, k, slice_channels):
    """dw_lds_bytes: the weights and the widest item's image, each in whole DMA blocks of 64 16-byte slots"""
    sp = slice_channels // 8
    pix = max((h1 - h0) * bs for _, _, h0, h1 in items)
    return (-(-k * k * 2 * sp // 64) + -(-pix * sp // 64)) * 1024


def check_plan(bsz, channels, k, asked):
    rc, p = plan(bsz, channels, k, asked)
    assert rc == 0, (bsz, channels, k, asked, _lib.hip().sayuri_hip_last_error())
    cs = -(-channels // 32) * 32
    assert p["slice"] == (64 if cs % 64 == 0 else 32) and cs % p["slice"] == 0
    if asked:
        assert p["strips"] == asked
    cuts = [cut(bs, p["strips"], k) for bs in bsz]
    for bs, items in zip(bsz, cuts):
        rows = [r for r0, r1, _, _ in items for r in range(r0, r1)]
        assert rows == list(range(bs)), (bs, items)  # whole rows, every row of the sample exactly once, no empty strip
        assert all(r0 < r1 for r0, r1, _, _ in items)
        for r0, r1, h0, h1 in items:
            assert 0 <= h0 <= r0 and r1 <= h1 <= bs  # the halo rows stay inside the board ...
            assert h0 == max(0, r0 - k // 2) and h1 == min(bs, r1 + k // 2)  # ... and are all a strip's taps can reach
    assert p["grid"] == len(bsz) * max(len(items) for items in cuts) * (cs // p["slice"]), (bsz, asked, p)
    assert p["lds"] == max(lds_of(items, bs, k, p["slice"]) for bs, items in zip(bsz, cuts)), (bsz, asked, p)
    assert 0 < p["lds"] <= DW_MAX_LDS
    return p


def test_a_lone_board_is_cut_finely_and_a_full_batch_not_at_all():
    for k in DW_K:
        p = check_plan([19], 256, k, 0)
        assert p["strips"] > 1 and p["grid"] > 256 // p["slice"], p  # more than one item per slice
        p = check_plan([19] * 256, 256, k, 0)
        assert p["strips"] == 1 and p["grid"] == 256 * (256 // p["slice"]), p


@pytest.mark.parametrize("channels", [16, 32, 40, 48, 64, 96, 256, 384])
def test_strips_are_whole_rows_cover_a_sample_once_and_keep_their_halo_inside_the_board(channels):
    rng = np.random.default_rng(channels)
    mixed = [19, 9, 13, 9, 19, 13, 7, 16]
    batches = [[19], [9], [2], [3] * 7, [5, 2, 3], [19] * 64, [13] * 5 + [19]] + [list(rng.permutation(mixed)) for _ in range(3)]
    for bsz in batches:
        for k in DW_K:
            for asked in (0, 1, 2, 5, max(bsz)):
                if asked <= max(bsz):
                    check_plan(bsz, channels, k, asked)


def test_a_mixed_batch_has_the_same_plan_in_any_order():
    mixed = [19, 9, 13, 9, 19, 13, 7, 16, 2]
    want = check_plan(mixed, 256, 7, 0)
    rng = np.random.default_rng(5)
    for _ in range(6):
        assert check_plan(list(rng.permutation(mixed)), 256, 7, 0) == want


def test_what_the_plan_does_not_cover_is_refused_with_a_message():
    lib = _lib.hip()
    for k in (1, 2, 4, 6, 9):
        assert plan([19], 256, k)[0] == -1 and b"k = %d" % k in lib.sayuri_hip_last_error()
    assert plan([19], 256, 7, strips=20)[0] == -1 and b"more than the 19 rows" in lib.sayuri_hip_last_error()
    assert plan([5, 2, 3], 64, 3, strips=6)[0] == -1 and b"more than the 5 rows" in lib.sayuri_hip_last_error()
    assert plan([5, 2, 3], 64, 3, strips=5)[0] == 0
    # an uncut 25x25 board on a 64-channel slice is 79 KiB of pixels: forced, it is refused; left to the plan, it is cut until it fits
    assert plan([25], 64, 7, strips=1, max_board=25)[0] == -1 and b"bytes of LDS" in lib.sayuri_hip_last_error()
    rc, p = plan([25], 64, 7, strips=0, max_board=25)
    assert rc == 0 and p["lds"] <= DW_MAX_LDS, p
    assert plan([20], 64, 7)[0] == -1 and b"board size" in lib.sayuri_hip_last_error()


def test_every_plan_query_refuses_a_bad_geometry_under_its_own_name():
    """The three plan queries build their geometry with one function (engine_plan.h, host_geom): no samples, a board larger than
    max_board and a board of 1 are refused by each, and the message starts with the query's own prefix."""
    lib, out = _lib.hip(), np.zeros(4, np.int32)
    queries = {
        b"split_ring_plan: ": lambda n, bsz: lib.sayuri_hip_split_ring_plan(n, _lib.ip(bsz), 19, 256, 0, 0),
        b"pw_plan: ": lambda n, bsz: lib.sayuri_hip_pw_plan(n, _lib.ip(bsz), 19, 256, 128, 0, _lib.ip(out)),
        b"dw_plan: ": lambda n, bsz: lib.sayuri_hip_dw_plan(n, _lib.ip(bsz), 19, 256, 7, 0, _lib.ip(out)),
    }
    for prefix, query in queries.items():
        assert query(1, np.asarray([19], np.int32)) >= 0, prefix
        for n, bsz, why in ((0, [19], b"bad argument"), (2, [19, 20], b"bad board size"), (2, [1, 19], b"bad board size")):
            assert query(n, np.asarray(bsz, np.int32)) == -1, (prefix, n, bsz)
            assert lib.sayuri_hip_last_error() == prefix + why, (prefix, n, bsz, lib.sayuri_hip_last_error())


@pytest.mark.skipif(not (os.path.exists(OBJDUMP) and os.path.exists(READELF)), reason="needs the ROCm llvm tools")
def test_depthwise_kernels_code_object(tmp_path):
    so = _build.HIP_SO
    if not os.path.exists(so):
        _build.build_hip()
    co = device_code_object(so, tmp_path)
    asm = subprocess.run([OBJDUMP, "-d", "--no-show-raw-insn", co], capture_output=True, text=True, check=True).stdout
    kernels, name = {}, None
    for line in asm.splitlines():
        m = re.match(r"^[0-9a-f]+ <(.+)>:$", line)
        if m:
            name = m.group(1)
            kernels[name] = []
        elif name and line.strip():
            kernels[name].append(line.split("//")[0].strip())
    dw = {k: v for k, v in kernels.items() if "conv_dw_kernel" in k}
    # one variant per k the plan accepts, and no other
    assert sorted(int(re.search(r"conv_dw_kernelILi(\d+)E", k).group(1)) for k in dw) == sorted(DW_K), sorted(dw)
    notes = subprocess.run([READELF, "--notes", co], capture_output=True, text=True, check=True).stdout
    blocks = notes.split(".agpr_count")
    for name, body in dw.items():
        assert any(i.startswith("global_load_lds_dwordx4") for i in body), name  # staged by LDS-DMA
        assert any(i.startswith("ds_read_b128") for i in body), name
        assert any(i.startswith(("v_fma_f32", "v_fmac_f32", "v_pk_fma_f32", "v_fma_mix_f32")) for i in body), name
        assert not [i for i in body if i.startswith("scratch_")], name
        assert not [i for i in body if "atomic" in i or i.startswith("s_sleep")], name  # no workgroup waits for another
        meta = [b for b in blocks if name in b]
        assert meta, name
        assert re.search(r"\.private_segment_fixed_size:\s+0\b", meta[0]), name + ": scratch"
        assert re.search(r"\.vgpr_spill_count:\s+0\b", meta[0]) and re.search(r"\.sgpr_spill_count:\s+0\b", meta[0]), name + ": spills"
        # the LDS is all dynamic: the code object declares none of its own, so what a launch gets is what the plan says
        # (<= kDwMaxLds, checked above for every plan)
        assert re.search(r"\.group_segment_fixed_size:\s+0\b", meta[0]), name + ": static LDS"
