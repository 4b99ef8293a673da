"""conv_pw.h without a GPU: the plan (sayuri_hip_pw_plan is host arithmetic), the code object inside libsayuri_hip.so, and -- where
the live reference is built -- the CPU oracle the GPU tests lean on, at a real width for the block kinds with tower 1x1 layers."""
import os
import re
import subprocess

import numpy as np
import pytest

from _oracle import PortNet, RefNet, ref_available
from sayuri_amd import _build, _lib
from sayuri_amd import weights as W
from test_kernel_hygiene import OBJDUMP, READELF, device_code_object

KIB = 1024
PW_NJ = (1, 2, 3, 6, 12)  # column tiles per wave of the variants the plan can pick


def plan(bsz, cin, cout, pieces=0, max_board=19):
    """-> (rc, {pieces, grid, nj, lds})"""
    out = np.zeros(4, np.int32)
    rc = _lib.hip().sayuri_hip_pw_plan(len(bsz), _lib.ip(np.asarray(bsz, np.int32)), max_board, cin, cout, pieces, _lib.ip(out))
    return rc, dict(zip(("pieces", "grid", "nj", "lds"), (int(v) for v in out)))


def cols(bs):
    return (bs * bs + 15) // 16


def pieces_of(bs, asked):
    """pieces a bs x bs board is really cut into (pw_cols, conv_pw.h): whole column tiles, no more pieces than tiles, at most 24 tiles a piece"""
    cp = min(-(-cols(bs) // max(1, min(asked, cols(bs)))), 24)
    return -(-cols(bs) // cp), cp


def test_a_lone_board_is_cut_finely_and_a_full_batch_not_at_all():
    rc, p = plan([19], 256, 128)
    assert rc == 0 and p["pieces"] > 1, p
    n, cp = pieces_of(19, p["pieces"])
    assert n > 1 and p["grid"] == 1 * n * 2 and 2 * p["nj"] >= cp, p
    rc, p = plan([19] * 256, 256, 128)
    assert rc == 0 and p["pieces"] == 1 and p["grid"] == 256 * 1 * 2 and p["nj"] == 12, p


@pytest.mark.parametrize("cin,cout", [(256, 128), (128, 256), (384, 192), (192, 384), (32, 64)])
def test_the_grid_is_samples_x_pieces_x_channel_tiles_and_a_piece_stays_inside_its_sample(cin, cout):
    """A workgroup's piece is (sample, piece index): column tiles [i cp, (i + 1) cp) of that sample's own pixels.  The grid has the
    same number of pieces for every sample -- the most any board of the batch has -- so a piece never reaches into a neighbour."""
    for bsz in ([19], [9], [2], [19, 9, 13, 9, 19, 13, 7, 16], [3] * 7, [19] * 64, [13] * 5 + [19]):
        for asked in (0, 1, 2, 5, 23):
            rc, p = plan(bsz, cin, cout, asked)
            assert rc == 0, (bsz, asked, _lib.hip().sayuri_hip_last_error())
            cut = [pieces_of(bs, p["pieces"]) for bs in bsz]
            assert p["grid"] == len(bsz) * max(n for n, _ in cut) * (cout // 64), (bsz, asked, p)
            assert all(n * cp >= cols(bs) and (n - 1) * cp < cols(bs) for (n, cp), bs in zip(cut, bsz))  # the pieces tile the sample, none is empty
            assert p["nj"] in PW_NJ and 2 * p["nj"] >= max(cp for _, cp in cut)
            assert min(cp for _, cp in cut) >= 1  # never smaller than one column tile
            assert p["lds"] <= 160 * KIB
            if asked:
                assert p["pieces"] == asked


def test_lds_stays_within_the_cu_for_every_width():
    for cin in (32, 96, 256, 384):
        for n in (1, 4, 16, 64, 256):
            rc, p = plan([19] * n, cin, 128)
            assert rc == 0 and 0 < p["lds"] <= 160 * KIB, (cin, n, p)


def test_a_layer_outside_the_route_is_refused_with_a_message():
    lib = _lib.hip()
    assert plan([19], 256, 96)[0] == -1 and b"64-channel" in lib.sayuri_hip_last_error()
    assert plan([19], 48, 128)[0] == -1 and b"32-channel" in lib.sayuri_hip_last_error()
    assert plan([25], 64, 64, pieces=1, max_board=25)[0] == -1 and b"column tiles" in lib.sayuri_hip_last_error()
    assert plan([25], 64, 64, pieces=0, max_board=25)[0] == 0
    assert plan([20], 64, 64)[0] == -1 and b"board size" in lib.sayuri_hip_last_error()


@pytest.mark.skipif(not (os.path.exists(OBJDUMP) and os.path.exists(READELF)), reason="needs the ROCm llvm tools")
def test_pointwise_kernels_code_object(tmp_path):
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
    pw = {k: v for k, v in kernels.items() if "conv_pw_kernel" in k}
    # every variant the plan can pick, and no other
    assert sorted(int(re.search(r"conv_pw_kernelILi(\d+)E", k).group(1)) for k in pw) == sorted(PW_NJ), sorted(pw)
    picked = {plan([bs] * n, 256, 128, asked)[1]["nj"] for bs in (2, 9, 19) for n in (1, 64) for asked in (0, 1, 2, 4, 8, 23)}
    assert picked == set(PW_NJ), picked
    notes = subprocess.run([READELF, "--notes", co], capture_output=True, text=True, check=True).stdout
    blocks = notes.split(".agpr_count")
    for name, body in pw.items():
        assert any(i.startswith("v_mfma_f32_16x16x32_f16") for i in body), name
        assert any(i.startswith("global_load_lds_dwordx4") for i in body), name
        assert not [i for i in body if i.startswith("scratch_")], name
        assert not [i for i in body if "atomic" in i or i.startswith("s_sleep")], name  # no workgroup waits for another
        meta = [b for b in blocks if name in b]
        assert meta, name
        assert re.search(r"\.private_segment_fixed_size:\s+0\b", meta[0]), name + ": scratch"
        assert re.search(r"\.vgpr_spill_count:\s+0\b", meta[0]) and re.search(r"\.sgpr_spill_count:\s+0\b", meta[0]), name + ": spills"
        # The K loop holds no full wait but the one of a layer's last chunks, which sits in a branch of its own next to the counted
        # wait.  hipcc lays the loop out either way round (MFMAs first or the waits first), so the loop is taken as everything from
        # a few instructions in front of its first counted wait or first MFMA to its last MFMA or barrier.
        mf = [i for i, ins in enumerate(body) if ins.startswith("v_mfma")]
        bar = [i for i, ins in enumerate(body) if ins.startswith("s_barrier")]
        counted = [i for i, ins in enumerate(body) if ins.startswith("s_waitcnt") and re.search(r"vmcnt\([1-9]", ins)]
        assert counted and bar, name
        loop = body[max(0, min(counted[0], mf[0]) - 8):max(mf[-1], bar[-1]) + 1]
        waits = [ins for ins in loop if ins.startswith("s_waitcnt") and "vmcnt" in ins]
        assert sum("vmcnt(0)" in w for w in waits) <= 1, (name, waits)


@pytest.mark.skipif(not ref_available(), reason="oracle/_ref not built")
@pytest.mark.parametrize("kind,channels,inner,ffn", [("NestedBottleneckBlock", 128, 64, None), ("MixerBlock", 128, None, 192)])
def test_port_agrees_with_the_live_reference_at_a_real_width(kind, channels, inner, ffn, tmp_weights_dir):
    """the bound of test_oracle.py (ATOL = 2e-5)"""
    blocks = [W.BlockSpec(kind, se=bool(i), bottleneck_channels=inner, ffn_channels=ffn) for i in range(2)]
    path = os.path.join(tmp_weights_dir, f"pw_cpu_{kind}.bin")
    W.write_weights(path, W.NetSpec(channels, blocks, 32, 32, activation="mish"), seed=33)
    port, ref = PortNet(path, True), RefNet(path, True)
    assert port.info == ref.info
    for bs in (9, 19):
        planes = W.synthetic_planes(1, bs, seed=70 + bs)[0]
        got, exp = port.forward(planes, bs), ref.forward(planes, bs)
        assert np.isfinite(got).all() and np.abs(got - exp).max() <= 2e-5, (kind, bs, float(np.abs(got - exp).max()))
