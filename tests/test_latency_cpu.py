"""CPU-only checks of the latency mode (include/sayuri_hip.h: sayuri_hip_create_ex; csrc/hip/conv_split.h).

  * The serial stand-in of the device side (tests/fake_hip/fake_hip.c) knows the ABI it was written against and nothing newer.
    The host library must go on serving a default pipe on it, and must answer a pipe that asks for latency=True with an error
    that names the missing entry point -- not call into whatever else exports it, not crash.
  * The cross-compiled split kernels: matrix-core and LDS-DMA instructions present, no scratch, no wait of a workgroup for
    another one (the launch boundary is the kernel's only synchronisation).
"""
import os
import re
import subprocess
import sys
import textwrap

import pytest

from _golden import Golden
from sayuri_amd import _build
from test_kernel_hygiene import OBJDUMP, READELF, device_code_object

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE_SRC = os.path.join(ROOT, "tests", "fake_hip", "fake_hip.c")

DRIVER = textwrap.dedent(r"""
    import sys
    import numpy as np
    from sayuri_amd import _lib
    from sayuri_amd.pipe import HipForwardPipe
    lib = _lib.hip()
    assert not hasattr(lib, "sayuri_hip_create_ex"), "the stand-in is expected NOT to know the new entry point"
    rng = np.random.default_rng(3)
    pipe = HipForwardPipe(sys.argv[1], board_size=9, batch_size=8, fp16=True, waittime_ms=0)
    outs = pipe.Forward([rng.integers(0, 4, size=(43, 81)).astype(np.float32) for _ in range(5)], [9] * 5)
    assert len(outs) == 5 and all(np.isfinite(o).all() for o in outs)
    pipe.Destroy()
    print("default pipe ok")
    try:
        HipForwardPipe(sys.argv[1], board_size=9, batch_size=8, fp16=True, waittime_ms=0, latency=True)
    except RuntimeError as e:
        print("latency refused:", e)
    else:
        raise SystemExit("a latency pipe was created on a device library without sayuri_hip_create_ex")
    pipe = HipForwardPipe(sys.argv[1], board_size=9, batch_size=8, fp16=True, waittime_ms=0)   # and the library still works
    pipe.Destroy()
    print("still ok")
""")


def test_host_library_on_a_device_library_without_create_ex(tmp_path, tmp_weights_dir):
    _build.build_host()
    fake = str(tmp_path / "libfake_hip.so")
    subprocess.check_call(["gcc", "-O2", "-fPIC", "-shared", "-Wall", FAKE_SRC, "-o", fake, "-lpthread"])
    weights = Golden("tiny_res", tmp_weights_dir).weights_path
    env = dict(os.environ, SAYURI_FAKE_HIP_LIB=fake, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    env.pop("SAYURI_LATENCY", None)
    r = subprocess.run([sys.executable, "-c", DRIVER, weights], env=env, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "default pipe ok" in r.stdout and "still ok" in r.stdout
    refused = [l for l in r.stdout.splitlines() if l.startswith("latency refused:")]
    assert refused and "sayuri_hip_create_ex" in refused[0], r.stdout


@pytest.mark.skipif(not (os.path.exists(OBJDUMP) and os.path.exists(READELF)), reason="needs the ROCm llvm tools")
def test_split_kernels_code_object(tmp_path):
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
    split = {k: v for k, v in kernels.items() if "conv_split_kernel" in k}
    assert len(split) >= 4, sorted(split)
    notes = subprocess.run([READELF, "--notes", co], capture_output=True, text=True, check=True).stdout
    blocks = notes.split(".agpr_count")
    for name, body in split.items():
        assert any(i.startswith("v_mfma_f32_16x16x32_f16") for i in body), name
        assert any(i.startswith("global_load_lds_dwordx4") for i in body), name
        assert not [i for i in body if i.startswith("scratch_")], name
        meta = [b for b in blocks if name in b]
        assert meta, name
        assert re.search(r"\.private_segment_fixed_size:\s+0\b", meta[0]), name + ": scratch"
        assert re.search(r"\.vgpr_spill_count:\s+0\b", meta[0]), name + ": vector spills"
        # No workgroup waits for another one.  A wait on global memory is a backward branch whose loop body reads global memory
        # and does no matrix work (the K loop, the one legitimate loop, is full of MFMAs); atomics and s_sleep are the other
        # marks of an exchange, and the kernel has no business with either.
        assert not [i for i in body if "atomic" in i or i.startswith("s_sleep") or i.startswith("buffer_wbl2") or i.startswith("s_memrealtime")], name
        # instruction addresses of this kernel, in order (objdump prints them behind "//")
        raw = []
        grab = False
        for line in asm.splitlines():
            m = re.match(r"^[0-9a-f]+ <(.+)>:$", line)
            if m:
                grab = m.group(1) == name
                continue
            if grab and line.strip():
                m2 = re.match(r"^\s*(\S.*?)\s*//\s*([0-9A-Fa-f]+):", line)
                if m2:
                    raw.append((int(m2.group(2), 16), m2.group(1).strip()))
        at = {a: i for i, (a, _) in enumerate(raw)}
        for i, (a, ins) in enumerate(raw):
            m = re.match(r"s_cbranch_\w+\s+(-?\d+)", ins) or re.match(r"s_branch\s+(-?\d+)", ins)
            if not m:
                continue
            off = int(m.group(1))
            off = off - 65536 if off >= 32768 else off
            target = a + 4 + 4 * off
            if target <= a and target in at:  # a loop
                loop = [x for _, x in raw[at[target]:i + 1]]
                reads_global = any(x.startswith(("global_load", "buffer_load", "flat_load", "s_load", "s_buffer_load")) for x in loop)
                works = any(x.startswith("v_mfma") for x in loop)
                assert works or not reads_global, f"{name}: a loop that reads global memory without matrix work (a spin wait?): {loop[:6]}"
