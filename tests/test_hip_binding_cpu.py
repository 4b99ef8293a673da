"""The Python binding of the device C-ABI (include/sayuri_hip.h) has one owner, sayuri_amd/_lib.py, and the ticket helpers
of sayuri_amd/hipraw.py do what the hand-written copies did.  No GPU: the real library is loaded for its symbols only, the
helpers run on the stand-in (tests/fake_hip/fake_hip.c)."""
import ctypes
import glob
import os
import re
import subprocess
import sys
import textwrap

from _golden import Golden
from sayuri_amd import _build, _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE_SRC = os.path.join(ROOT, "tests", "fake_hip", "fake_hip.c")

RESTYPES = {"sayuri_hip_create": ctypes.c_void_p, "sayuri_hip_create_ex": ctypes.c_void_p, "sayuri_hip_host_alloc": ctypes.c_void_p,
            "sayuri_hip_last_error": ctypes.c_char_p, "sayuri_hip_device_bytes": ctypes.c_size_t, "sayuri_hip_host_free": None,
            "sayuri_hip_destroy": None}   # everything else: c_int


def prototypes():
    """-> {name: (return type, [parameter text, ...])} of every function the header declares."""
    header = open(os.path.join(ROOT, "include", "sayuri_hip.h")).read()
    header = re.sub(r"/\*.*?\*/", " ", header, flags=re.S)
    protos = {}
    for ret, name, params in re.findall(r"([A-Za-z_][\w \t]*?[\w*])\s*\b(sayuri_hip_[a-z_0-9]+)\s*\(([^)]*)\)\s*;", header):
        params = " ".join(params.split())
        protos[name] = (" ".join(ret.split()), [] if params == "void" else [p.strip() for p in params.split(",")])
    return protos


def is_pointer_type(t):
    return t in (ctypes.c_void_p, ctypes.c_char_p) or issubclass(t, ctypes._Pointer)


def test_every_function_of_the_header_has_its_signature():
    protos = prototypes()
    assert set(protos) == set(_lib.HIP_SYMBOLS), set(protos) ^ set(_lib.HIP_SYMBOLS)
    lib = _lib.hip()   # the real library: it loads without a device
    assert "SAYURI_FAKE_HIP_LIB" not in os.environ and lib._name == _build.HIP_SO
    for name, (ret, params) in protos.items():
        fn = getattr(lib, name)
        assert fn.argtypes is not None and len(fn.argtypes) == len(params), (name, fn.argtypes, params)
        want = RESTYPES.get(name, ctypes.c_int)
        assert fn.restype is want, (name, fn.restype)
        assert ("*" in ret) == (want in (ctypes.c_void_p, ctypes.c_char_p)), (name, ret)
        for text, t in zip(params, fn.argtypes):
            if "*" in text or "[" in text:
                assert is_pointer_type(t), (name, text, t)
            else:
                assert not is_pointer_type(t), (name, text, t)


def test_signatures_are_assigned_in_one_place():
    pat = re.compile(r"\b(sayuri_hip_[a-z_0-9]+)\.(argtypes|restype)\s*=[^=]")
    found = []
    for folder in ("sayuri_amd", "tests", "tools"):
        for path in glob.glob(os.path.join(ROOT, folder, "**", "*.py"), recursive=True):
            if os.path.relpath(path, ROOT) == os.path.join("sayuri_amd", "_lib.py"):
                continue
            for k, line in enumerate(open(path), 1):
                found += [(os.path.relpath(path, ROOT), k, m.group(1)) for m in pat.finditer(line) if m.group(1) in _lib.HIP_SYMBOLS]
    assert not found, found


def test_every_layer_tap_has_its_one_caller_in_taps():
    """tests/_taps.py names every layer tap of HIP_ABI, and no other file under tests/ names one."""
    taps = {name for name in _lib.HIP_ABI if "_test_" in name}
    pat = re.compile(os.path.commonprefix(sorted(taps)).encode() + rb"\w+")
    named = {}
    for path in glob.glob(os.path.join(ROOT, "tests", "**", "*"), recursive=True):
        if os.path.isfile(path) and "__pycache__" not in path:
            named[os.path.relpath(path, ROOT)] = {m.decode() for m in pat.findall(open(path, "rb").read())}
    assert taps and named.pop(os.path.join("tests", "_taps.py")) == taps
    assert not any(named.values()), {k: v for k, v in named.items() if v}


DRIVER = textwrap.dedent(r"""
    import os, sys
    import numpy as np
    from sayuri_amd import hipraw
    from sayuri_amd.engine import pack_planes
    from sayuri_amd.pipe import HipForwardPipe

    B, N, WORDS = 9, 8, 37 * 12 + 8
    rng = np.random.default_rng(17)

    def position(bs):
        p = np.zeros((43, bs * bs), np.float32)
        p[:37] = rng.integers(0, 2, size=(37, bs * bs))
        p[37:] = rng.normal(size=(6, 1)).astype(np.float32)
        return p

    def grid_of(planes, bsz):
        g = np.zeros((len(bsz), 43, B * B), np.float32)
        for i, (p, bs) in enumerate(zip(planes, bsz)):
            g[i].reshape(43, B, B)[:, :bs, :bs] = p.reshape(43, bs, bs)
        return g

    def same(got, want, what):
        for a, b in zip(got, want):
            assert a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32)), what

    def make_pipe(**env):
        os.environ.update(env)       # the stand-in reads its switches when a context is created
        try:
            return HipForwardPipe(sys.argv[1], board_size=B, batch_size=N, fp16=True, waittime_ms=0)
        finally:
            for k in env:
                del os.environ[k]

    batches = []                     # two batches of mixed 7x7 / 9x9 positions: 5 and 3
    for n in (5, 3):
        bsz = [int(b) for b in rng.choice([7, 9], size=n)]
        bsz[0], bsz[-1] = 7, 9
        planes = [position(bs) for bs in bsz]
        batches.append(dict(n=n, bsz=bsz, grid=grid_of(planes, bsz), rec=np.stack([pack_planes(p, 37) for p in planes]).astype(np.uint32)))

    pipe = make_pipe()
    ctx = pipe.ctx(0)
    for packed in (False, True):
        want = [hipraw.hip_forward_packed_raw(ctx, b["rec"], 37, b["bsz"], B) if packed else hipraw.hip_forward_raw(ctx, b["grid"], b["bsz"], B)
                for b in batches]
        assert not np.array_equal(want[0][0][:3], want[1][0])
        with hipraw.PinnedSet(N, B, WORDS if packed else 43 * B * B) as s0, hipraw.PinnedSet(N, B, WORDS if packed else 43 * B * B) as s1:
            sets = (s0, s1)

            def submit(i):
                b, s = batches[i], sets[i]
                s.bsz[:b["n"]] = b["bsz"]
                if packed:
                    s.records[:b["rec"].size] = b["rec"].ravel()
                    return hipraw.submit_packed(ctx, s, b["n"], 37)
                s.planes[:b["grid"].size] = b["grid"].ravel()
                return hipraw.submit(ctx, s, b["n"])

            tick = [submit(0), submit(1)]
            assert sorted(tick) == [0, 1]
            for r in range(6):
                i = r & 1
                hipraw.wait(ctx, tick[i])
                same(sets[i].outputs(batches[i]["n"]), want[i], (packed, r))
                for a in sets[i].outputs(N):
                    a[:] = np.nan        # the next round must write its results itself
                if r < 4:
                    tick[i] = submit(i)
            if packed:                   # a caller's pageable records, kept referenced until the wait
                hold = batches[1]["rec"].copy()
                s0.records[:] = 0
                s0.bsz[:3] = batches[1]["bsz"]
                hipraw.wait(ctx, hipraw.submit_packed(ctx, s0, 3, 37, hold))
                same(s0.outputs(3), want[1], "pageable records")
            # a third batch in flight is refused
            tick = [submit(0), submit(1)]
            try:
                submit(0)
            except RuntimeError:
                pass
            else:
                raise SystemExit("a third submit without a wait went through")
            for t in tick:
                hipraw.wait(ctx, t)
        for name in hipraw.PinnedSet.VIEWS:   # closed: no view of freed memory is handed out
            try:
                getattr(s0, name)
            except RuntimeError:
                continue
            raise SystemExit(f"a closed PinnedSet still hands out {name}")
        for use in (lambda: s0.outputs(1), lambda: hipraw.submit(ctx, s0, 1), lambda: hipraw.submit_packed(ctx, s0, 1, 37)):
            try:
                use()
            except RuntimeError:
                continue
            raise SystemExit("a closed PinnedSet was used")
        s0.close()                            # and closing twice frees nothing twice
    pipe.Destroy()
    print("two tickets ok")

    # query: the stand-in's worker finishes batches in order, DELAY_US after their submit, and forgets a ticket that has been
    # waited for.  So: ticket a is still running right after its submit, and finished once the LATER ticket b has been waited for.
    pipe = make_pipe(FAKE_HIP_DELAY_US="20000")
    ctx = pipe.ctx(0)
    with hipraw.PinnedSet(N, B, 43 * B * B) as s0, hipraw.PinnedSet(N, B, 43 * B * B) as s1:
        for s in (s0, s1):
            s.bsz[:3] = batches[1]["bsz"]
            s.planes[:batches[1]["grid"].size] = batches[1]["grid"].ravel()
        a, b = hipraw.submit(ctx, s0, 3), hipraw.submit(ctx, s1, 3)
        assert hipraw.query(ctx, a) == 0
        hipraw.wait(ctx, b)
        assert hipraw.query(ctx, a) == 1
        hipraw.wait(ctx, a)
    pipe.Destroy()
    print("query ok")

    pipe = make_pipe(FAKE_HIP_FAIL_SUBMIT="2")
    ctx = pipe.ctx(0)
    with hipraw.PinnedSet(N, B, 43 * B * B) as s:
        s.bsz[:3] = batches[1]["bsz"]
        s.planes[:batches[1]["grid"].size] = batches[1]["grid"].ravel()
        hipraw.wait(ctx, hipraw.submit(ctx, s, 3))
        try:
            hipraw.submit(ctx, s, 3)
        except RuntimeError as e:
            print("second submit:", e)
        else:
            raise SystemExit("FAKE_HIP_FAIL_SUBMIT=2 and the second submit went through")
        hipraw.wait(ctx, hipraw.submit(ctx, s, 3))   # the context goes on
        same(s.outputs(3), hipraw.hip_forward_raw(ctx, batches[1]["grid"], batches[1]["bsz"], B), "after a refused submit")
    pipe.Destroy()
""")


def test_ticket_helpers_on_the_stand_in(tmp_path, tmp_weights_dir):
    """hipraw's PinnedSet / submit / submit_packed / wait / query on the CPU stand-in of the device library, tiny_res, board 9,
    batch 8: two sets, two tickets in flight, six rounds, fp32 planes and packed records of 5 and 3 mixed 7x7 / 9x9 positions,
    every batch bit for bit what hip_forward_raw / hip_forward_packed_raw give on the same context (the stand-in's network is
    a deterministic function of each sample's planes); a third submit without a wait and FAKE_HIP_FAIL_SUBMIT=2 raise; a
    closed set refuses use.  query: the stand-in answers -1 for a ticket that has been waited for, so "0 before, 1 after a
    wait" is shown on the earlier of two tickets across the wait for the later one."""
    _build.build_host()
    fake = str(tmp_path / "libfake_hip.so")
    subprocess.check_call(["gcc", "-O2", "-fPIC", "-shared", "-Wall", FAKE_SRC, "-o", fake, "-lpthread"])
    weights = Golden("tiny_res", tmp_weights_dir).weights_path
    env = dict(os.environ, SAYURI_FAKE_HIP_LIB=fake, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    for k in [k for k in env if k.startswith("FAKE_HIP_")] + ["SAYURI_LATENCY"]:
        env.pop(k, None)
    r = subprocess.run([sys.executable, "-c", DRIVER, weights], env=env, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "two tickets ok" in r.stdout and "query ok" in r.stdout
    refused = [l for l in r.stdout.splitlines() if l.startswith("second submit:")]
    assert refused and "fake_hip: submit 2 failed on request (3 positions)" in refused[0], r.stdout
