"""Python face of the host library: the weights loader and HipForwardPipe, with the method
names of the reference's plugin interface (src/neural/network_basic.h:132-161)."""
from __future__ import annotations

import ctypes
from typing import List, Optional, Sequence

import numpy as np

from . import _lib
from .hipraw import hip_forward_packed_raw, hip_forward_packed_symm_raw, hip_forward_raw  # noqa: F401  (their importers' address)

PLANES_LEN = 43 * 361  # InputData::planes
OUT_LEN = 2 * 361 + 9
MAX_BOARD = 19
HIP_LATENCY = 1  # include/sayuri_hip.h: SAYURI_HIP_LATENCY


class Weights:
    """DNNWeights as parsed + BN-folded by the product loader (csrc/host/weights_loader.cc)."""

    def __init__(self, path: str):
        lib = _lib.host()
        self._h = lib.sayuri_weights_load(path.encode())
        if not self._h:
            raise RuntimeError(f"Fail to load the network file! Cause: {lib.sayuri_host_last_error().decode()}")
        info = (ctypes.c_int * 12)()
        lib.sayuri_weights_info(self._h, info)
        self.info = list(info)

    def block_info(self, i: int) -> List[int]:
        b = (ctypes.c_int * 5)()
        if _lib.host().sayuri_weights_block_info(self._h, i, b):
            raise IndexError(i)
        return list(b)

    def tensor(self, name: str) -> Optional[np.ndarray]:
        lib = _lib.host()
        n = lib.sayuri_weights_tensor(self._h, name.encode(), None, 0)
        if n < 0:
            return None
        out = np.zeros(n, np.float32)
        if n:
            lib.sayuri_weights_tensor(self._h, name.encode(), _lib.fp(out), n)
        return out

    def close(self):
        if self._h:
            _lib.host().sayuri_weights_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class HipForwardPipe:
    """One process, one pipe; `device` = -1 uses every visible GPU (one pump thread each)."""

    def __init__(self, weights_path: str, board_size: int = MAX_BOARD, batch_size: int = 256, fp16: bool = True,
                 device: int = 0, waittime_ms: int = 2, latency: bool = False, ensemble: int = 0):
        """latency: a latency context per GPU (include/sayuri_hip.h, SAYURI_HIP_LATENCY) -- every 3x3 tower convolution cut
        into many small workgroups, for the batches of 1 to 16 positions of a playing or analysing engine.  fp16 only.
        ensemble: E > 0 lets every batch expand up to E ensemble requests (ForwardEnsemble; Network kAverage) on the device:
        the contexts take batch_size + 7 * E samples.  0 = off, the pipe as without the argument."""
        lib = _lib.host()
        if ensemble:
            self._h = lib.sayuri_pipe_create_ens(weights_path.encode(), board_size, batch_size, int(fp16), device,
                                                 waittime_ms, HIP_LATENCY if latency else 0, int(ensemble))
        elif latency:
            self._h = lib.sayuri_pipe_create_ex(weights_path.encode(), board_size, batch_size, int(fp16), device,
                                                waittime_ms, HIP_LATENCY)
        else:
            self._h = lib.sayuri_pipe_create(weights_path.encode(), board_size, batch_size, int(fp16), device,
                                             waittime_ms)
        if not self._h:
            raise RuntimeError(f"HipForwardPipe: {lib.sayuri_host_last_error().decode()}")
        self.board_size = board_size
        self.batch_size = batch_size
        self.fp16 = fp16
        self.latency = latency
        self.ensemble = int(ensemble)

    # -- NetworkForwardPipe surface
    def Valid(self) -> bool:
        return self._h is not None

    def GetNumWorkers(self) -> int:
        return _lib.host().sayuri_pipe_num_workers(self._h)

    def Construct(self, board_size: int, batch_size: int):
        if _lib.host().sayuri_pipe_reconstruct(self._h, board_size, batch_size):
            raise RuntimeError(_lib.host().sayuri_host_last_error().decode())
        self.board_size, self.batch_size = board_size, batch_size

    def Destroy(self):
        if self._h:
            _lib.host().sayuri_pipe_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.Destroy()
        except Exception:
            pass

    def netbench(self, threads: int, seconds: float = 5.0, board: int = MAX_BOARD):
        """The reference's `netbench` measure (gtp.cc:1468-1568): threads blocked in Forward()
        for `seconds`; returns (evals_per_sec, total_evals).  Includes queue + PCIe both ways."""
        eps, tot = ctypes.c_double(0), ctypes.c_long(0)
        if _lib.host().sayuri_pipe_netbench(self._h, threads, seconds, board, ctypes.byref(eps), ctypes.byref(tot)):
            raise RuntimeError(_lib.host().sayuri_host_last_error().decode())
        return eps.value, tot.value

    def pump_times(self):
        """-> dict of pump-thread time (us) since construction + batch / eval counters (PumpCounter, hip_forward_pipe.h):
        forward_us            in the submit call (expanding a mixed batch, sayuri_hip_submit / sayuri_hip_submit_packed)
        fill_us               handing finished batches out (snapshot, flags, root of the wake tree) and re-opening their sets
        wait_batch_us         asleep: nothing to send, nothing to retire
        wait_copies_us        inside sayuri_hip_wait, i.e. waiting for the GPU (NOT for plane copies: wait_plane_copies_us)
        wake_parked_us        waking callers parked for a free staging set when the fill set rotates
        partial_batches       a count: batches sent with fewer than batch_size requests
        gpu_queue_empty_us    nothing was enqueued on the GPU between two batches
        wait_plane_copies_us  waiting for a closed set's callers to finish their plane copies, and for the consumers of the
                              set's previous batch
        batches, evals        batches and positions evaluated (BatchForward included)"""
        t = (ctypes.c_double * 8)()
        b, e = ctypes.c_long(0), ctypes.c_long(0)
        _lib.host().sayuri_pipe_pump_times(self._h, t, ctypes.byref(b), ctypes.byref(e))
        return {"forward_us": t[0], "fill_us": t[1], "wait_batch_us": t[2], "wait_copies_us": t[3],
                "wake_parked_us": t[4], "partial_batches": int(round(t[5])), "gpu_queue_empty_us": t[6],
                "wait_plane_copies_us": t[7], "batches": b.value, "evals": e.value}

    def ctx(self, gpu: int = 0) -> int:
        c = _lib.host().sayuri_pipe_ctx(self._h, gpu)
        if not c:
            raise RuntimeError("no such gpu in this pipe")
        return c

    def _eval(self, mode: int, planes: Sequence[np.ndarray], board_sizes: Sequence[int], komi=None, offsets=None,
              gpu: int = 0) -> List[np.ndarray]:
        n = len(planes)
        buf = np.zeros((n, PLANES_LEN), np.float32)
        for i, p in enumerate(planes):
            flat = np.ascontiguousarray(p, np.float32).ravel()
            buf[i, :flat.size] = flat
        bsz = np.asarray(board_sizes, np.int32)
        km = np.asarray(komi if komi is not None else [7.5] * n, np.float32)
        off = np.asarray(offsets if offsets is not None else [0] * n, np.int32)
        out = np.zeros((n, OUT_LEN), np.float32)
        if _lib.host().sayuri_pipe_eval(self._h, mode, gpu, n, _lib.fp(buf), _lib.ip(bsz), _lib.fp(km), _lib.ip(off), _lib.fp(out)):
            raise RuntimeError(_lib.host().sayuri_host_last_error().decode())
        res = []
        for i in range(n):
            s = int(bsz[i]) ** 2
            res.append(np.concatenate([out[i, :s], out[i, 361:361 + s], out[i, 722:]]))
        return res

    def BatchForward(self, planes, board_sizes, komi=None, offsets=None, gpu: int = 0):
        """-> per sample: prob[bs*bs], own[bs*bs], pass, wdl[3], stm, score, q_err, score_err, offset
        (the packing of oracle so_forward / ref_forward)."""
        return self._eval(0, planes, board_sizes, komi, offsets, gpu)

    def Forward(self, planes, board_sizes, komi=None, offsets=None):
        """n concurrent blocking Forward() calls through the batching queue."""
        return self._eval(1, planes, board_sizes, komi, offsets)

    def AcceptsGroup(self) -> bool:
        return bool(_lib.host().sayuri_pipe_accepts_group(self._h))

    def ForwardGroup(self, cases):
        """cases: (planes, board_size[, komi[, offset]]) per position, packable as for ForwardPacked -> their results in
        Forward()'s packing, from ONE HipForwardPipe::ForwardGroup call of this thread: the requests go out together, without
        waiting for other callers or the pipe's timers."""
        cases = [tuple(c) + (7.5, 0)[len(c) - 2:] for c in cases]
        n = len(cases)
        buf = np.zeros((n, PLANES_LEN), np.float32)
        for i, c in enumerate(cases):
            flat = np.ascontiguousarray(c[0], np.float32).ravel()
            buf[i, :flat.size] = flat
        bsz = np.asarray([c[1] for c in cases], np.int32)
        km = np.asarray([c[2] for c in cases], np.float32)
        off = np.asarray([c[3] for c in cases], np.int32)
        out = np.zeros((n, OUT_LEN), np.float32)
        if _lib.host().sayuri_pipe_group_eval(self._h, n, _lib.fp(buf), _lib.ip(bsz), _lib.fp(km), _lib.ip(off), _lib.fp(out)):
            raise RuntimeError(_lib.host().sayuri_host_last_error().decode())
        return [np.concatenate([out[i, :int(bsz[i]) ** 2], out[i, 361:361 + int(bsz[i]) ** 2], out[i, 722:]]) for i in range(n)]

    def AcceptsReload(self) -> bool:
        """False on a device library without the live-reload entry points (sayuri_hip_reload_*)."""
        return bool(_lib.host().sayuri_pipe_accepts_reload(self._h))

    def Reload(self, weights_path: str):
        """A new network of the SAME architecture into the running pipe (HipForwardPipe::Reload): parsed, staged and built on
        this thread while other threads' requests keep being served, then swapped in between two batches.  Returns when every
        GPU's context has it: a request that begins afterwards gets the new network.  Raises with the loader's or the device's
        message when the file or the architecture is refused; the pipe then serves the network it had."""
        if _lib.host().sayuri_pipe_reload(self._h, weights_path.encode()):
            raise RuntimeError(f"HipForwardPipe.Reload: {_lib.host().sayuri_host_last_error().decode()}")

    def weights_generation(self) -> int:
        """0 for a pipe that was never reloaded, +1 per reload."""
        return int(_lib.host().sayuri_pipe_weights_generation(self._h))

    def AcceptsEnsemble(self) -> bool:
        return bool(_lib.host().sayuri_pipe_accepts_ensemble(self._h))

    def ensemble_fallbacks(self) -> int:
        """Ensemble requests that found their batch's capacity used up and were served as a plain identity request."""
        return int(_lib.host().sayuri_pipe_ensemble_fallbacks(self._h))

    def ForwardEnsemble(self, planes, board_size: int, komi: float = 7.5, offset: int = 0):
        """One position's identity planes (packable, as for ForwardPacked) -> (all, results): results[s] is the raw result of
        the planes under board symmetry s in Forward()'s packing; all is False when only results[0] was evaluated."""
        flat = np.zeros(PLANES_LEN, np.float32)
        p = np.ascontiguousarray(planes, np.float32).ravel()
        flat[:p.size] = p
        out = np.zeros((8, OUT_LEN), np.float32)
        rc = _lib.host().sayuri_pipe_forward_ensemble(self._h, _lib.fp(flat), board_size, komi, offset, _lib.fp(out))
        if rc < 0:
            raise RuntimeError(_lib.host().sayuri_host_last_error().decode())
        s = board_size * board_size
        return rc == 8, [np.concatenate([out[i, :s], out[i, 361:361 + s], out[i, 722:]]) for i in range(8 if rc == 8 else 1)]

    def ensemble_mix(self, planes, board_sizes, kinds, komi=None, offsets=None, fiber_threads: int = 2):
        """Test tap (sayuri_pipe_ensemble_mix): the requests at once, request i as kinds[i] -- 0 / 1 ForwardEnsemble from a
        fiber / an OS thread, 2 / 3 ForwardPacked from a fiber / a thread, 4 Forward from a thread.  -> per request the list
        of its results (eight, or one) in Forward()'s packing."""
        n = len(planes)
        buf = np.zeros((n, PLANES_LEN), np.float32)
        for i, p in enumerate(planes):
            flat = np.ascontiguousarray(p, np.float32).ravel()
            buf[i, :flat.size] = flat
        bsz = np.asarray(board_sizes, np.int32)
        km = np.asarray(komi if komi is not None else [7.5] * n, np.float32)
        off = np.asarray(offsets if offsets is not None else [0] * n, np.int32)
        kd = np.asarray(kinds, np.int32)
        out = np.zeros((n, 8, OUT_LEN), np.float32)
        got = np.zeros(n, np.int32)
        if _lib.host().sayuri_pipe_ensemble_mix(self._h, n, _lib.fp(buf), _lib.ip(bsz), _lib.fp(km), _lib.ip(off), _lib.ip(kd), fiber_threads, _lib.fp(out), _lib.ip(got)):
            raise RuntimeError(_lib.host().sayuri_host_last_error().decode())
        res = []
        for i in range(n):
            s = int(bsz[i]) ** 2
            res.append([np.concatenate([out[i, k, :s], out[i, k, 361:361 + s], out[i, k, 722:]]) for k in range(int(got[i]))])
        return res

    def ForwardPacked(self, planes, board_sizes, komi=None, offsets=None, mixed: bool = False):
        """The same through ForwardPacked() (csrc/host/packed_planes.h): the planes are packed into bit planes + scalars on
        the way in (they must be packable: 0/1 binary planes, constant scalar planes).  mixed: odd requests packed, even
        ones fp32, so that batches hold both kinds."""
        return self._eval(3 if mixed else 2, planes, board_sizes, komi, offsets)


def packed_symmetry(record: np.ndarray, binary: int, board_size: int, symmetry: int) -> np.ndarray:
    """PackedPlanes::Symmetry (csrc/host/packed_planes.h): the record the encoder builds for `symmetry` from the identity's."""
    record = np.ascontiguousarray(record, np.uint32)
    out = np.zeros_like(record)
    if _lib.host().sayuri_packed_symmetry(record.ctypes.data, binary, board_size, symmetry, out.ctypes.data):
        raise ValueError("packed_symmetry: bad arguments")
    return out
