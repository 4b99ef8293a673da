"""Work on a raw context (sayuri_hip_ctx*, e.g. HipForwardPipe.ctx()) at the C-ABI of include/sayuri_hip.h: the blocking forwards
on numpy arrays, and the pump's path -- submit / wait on tickets over sets of page-locked buffers -- for tests and tools."""
from __future__ import annotations

import ctypes
from typing import Optional

import numpy as np

from . import _lib
from ._lib import fp, ip


def _ok(rc: int) -> None:
    if rc:
        raise RuntimeError(_lib.hip().sayuri_hip_last_error().decode())


class PinnedSet:
    """One set of page-locked buffers (sayuri_hip_host_alloc) as the pump owns two of: the input of up to nmax samples of
    in_words 32-bit words each -- `planes` (float32) and `records` (uint32) are flat views of the same memory -- `bsz`
    (int32 [nmax]) and the outputs `prob` [nmax][prob_ch][B*B], `pass_`, `misc`, `own`.  The views die with close()."""
    VIEWS = ("planes", "records", "bsz", "prob", "pass_", "misc", "own", "io")

    def __init__(self, nmax: int, board: int, in_words: int, prob_ch: int = 5, pass_outs: int = 5, misc_outs: int = 15):
        lib = _lib.hip()
        self.nmax, self.board = nmax, board
        self._ptrs, v = [], {}
        try:
            for name, dtype, shape in (("planes", np.float32, (nmax * in_words,)), ("bsz", np.int32, (nmax,)),
                                       ("prob", np.float32, (nmax, prob_ch, board * board)), ("pass_", np.float32, (nmax, pass_outs)),
                                       ("misc", np.float32, (nmax, misc_outs)), ("own", np.float32, (nmax, board * board))):
                nbytes = 4 * int(np.prod(shape))
                p = lib.sayuri_hip_host_alloc(nbytes)
                if not p:
                    raise RuntimeError(f"sayuri_hip_host_alloc({nbytes}) failed")
                self._ptrs.append(p)
                v[name] = np.frombuffer((ctypes.c_ubyte * nbytes).from_address(p), dtype).reshape(shape)
        except Exception:
            self.close()
            raise
        v["records"] = v["planes"].view(np.uint32)
        v["io"] = (ip(v["bsz"]), fp(v["prob"]), fp(v["pass_"]), fp(v["misc"]), fp(v["own"]))  # the tail of every submit
        self._views = v

    def __getattr__(self, name):  # reached for the views only
        if name in PinnedSet.VIEWS:
            views = self.__dict__.get("_views")
            if views is None:
                raise RuntimeError("PinnedSet is closed")
            return views[name]
        raise AttributeError(name)

    def outputs(self, n: int):
        """prob, pass, misc, own of the first n samples: views, good until the set's next submit."""
        return self.prob[:n], self.pass_[:n], self.misc[:n], self.own[:n]

    def close(self):
        self._views = None
        while self._ptrs:
            _lib.hip().sayuri_hip_host_free(self._ptrs.pop())

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def _ticket(call, *args) -> int:
    tick = ctypes.c_int(-1)
    _ok(call(*args, ctypes.byref(tick)))
    return tick.value


def submit(ctx: int, s: PinnedSet, n: int) -> int:
    """sayuri_hip_submit of the set's first n samples (planes, bsz) -> ticket."""
    return _ticket(_lib.hip().sayuri_hip_submit, ctx, n, fp(s.planes), *s.io)


def submit_packed(ctx: int, s: PinnedSet, n: int, binary: int, records: Optional[np.ndarray] = None) -> int:
    """sayuri_hip_submit_packed of n records -- the set's own, or a caller's (pageable) uint32 array, which the caller keeps
    referenced until the wait -- with the set's bsz -> ticket."""
    if records is None:
        records = s.records
    assert records.dtype == np.uint32 and records.flags.c_contiguous and records.size >= n * (binary * 12 + 8)
    return _ticket(_lib.hip().sayuri_hip_submit_packed, ctx, n, records.ctypes.data, binary, *s.io)


def submit_packed_symm(ctx: int, s: PinnedSet, n_records: int, binary: int, src, symm) -> int:
    """sayuri_hip_submit_packed_symm: the set's first n_records records, sample i = record src[i] (None: the identity map)
    under symmetry symm[i], bsz[i] its board size -> ticket.  The call copies the two tables."""
    symm = np.ascontiguousarray(symm, np.int32)
    src = None if src is None else ip(np.ascontiguousarray(src, np.int32))
    bsz, *outs = s.io
    return _ticket(_lib.hip().sayuri_hip_submit_packed_symm, ctx, len(symm), s.records.ctypes.data, n_records, binary, bsz, src, ip(symm), *outs)


def wait(ctx: int, ticket: int) -> None:
    _ok(_lib.hip().sayuri_hip_wait(ctx, ticket))


def query(ctx: int, ticket: int) -> int:
    """1 = finished, 0 = still running."""
    done = _lib.hip().sayuri_hip_query(ctx, ticket)
    _ok(done < 0)
    return done


def _outputs(n: int, board: int, prob_ch: int, pass_outs: int, misc_outs: int):
    return (np.zeros((n, prob_ch, board * board), np.float32), np.zeros((n, pass_outs), np.float32),
            np.zeros((n, misc_outs), np.float32), np.zeros((n, board * board), np.float32))


def hip_forward_raw(ctx: int, planes_grid: np.ndarray, board_sizes, board: int, prob_ch: int = 5, pass_outs: int = 5,
                    misc_outs: int = 15):
    """sayuri_hip_forward on NN-grid planes [n][43][board*board] -> prob, pass, misc, own."""
    planes_grid = np.ascontiguousarray(planes_grid, np.float32)
    bsz = np.asarray(board_sizes, np.int32)
    out = _outputs(planes_grid.shape[0], board, prob_ch, pass_outs, misc_outs)
    _ok(_lib.hip().sayuri_hip_forward(ctx, planes_grid.shape[0], fp(planes_grid), ip(bsz), *map(fp, out)))
    return out


def hip_forward_packed_raw(ctx: int, records: np.ndarray, binary: int, board_sizes, board: int, prob_ch: int = 5, pass_outs: int = 5,
                           misc_outs: int = 15):
    """sayuri_hip_forward_packed on packed records [n][binary*12 + 8] (uint32) -> prob, pass, misc, own."""
    records = np.ascontiguousarray(records, np.uint32)
    assert records.shape[1] == binary * 12 + 8
    bsz = np.asarray(board_sizes, np.int32)
    out = _outputs(records.shape[0], board, prob_ch, pass_outs, misc_outs)
    _ok(_lib.hip().sayuri_hip_forward_packed(ctx, records.shape[0], records.ctypes.data, binary, ip(bsz), *map(fp, out)))
    return out


def hip_forward_packed_symm_raw(ctx: int, records, binary: int, board_sizes, src, symm, board: int, prob_ch: int = 5,
                                pass_outs: int = 5, misc_outs: int = 15, n_records: Optional[int] = None):
    """sayuri_hip_forward_packed_symm: device sample i = record src[i] (None: the identity map) under board symmetry symm[i]
    -> prob, pass, misc, own per device sample.  records: uint32 [n_records][binary*12 + 8], or the address of such an array
    (memory from sayuri_hip_host_alloc) with n_records given."""
    if isinstance(records, np.ndarray):
        records = np.ascontiguousarray(records, np.uint32)
        assert records.shape[1] == binary * 12 + 8
        n_records = records.shape[0] if n_records is None else n_records
        addr = records.ctypes.data
    else:
        addr = int(records)
    sym = np.ascontiguousarray(symm, np.int32)
    bsz = np.ascontiguousarray(board_sizes, np.int32)
    sr = None if src is None else np.ascontiguousarray(src, np.int32)
    out = _outputs(sym.shape[0], board, prob_ch, pass_outs, misc_outs)
    _ok(_lib.hip().sayuri_hip_forward_packed_symm(ctx, sym.shape[0], addr, n_records, binary, ip(bsz), None if sr is None else ip(sr),
                                                  ip(sym), *map(fp, out)))
    return out


def conv_pw_layer(board_sizes, cin: int, cout: int, act: int, xs, w, bias=None, res=None, pieces: int = 0, max_board: int = 19):
    """The layer tap of the tower's pointwise kernel (sayuri_hip_test_conv_pw, csrc/hip/conv_pw.h): one fp16 1x1 layer on host
    tensors, no context.  xs / res: per-sample [C][b*b] arrays (res None: no residual), w [cout][cin], pieces per sample (0: the
    engine's choice).  -> (rc, per-sample [cout][b*b] outputs that start as NaN, sayuri_hip_test_last_conv_kind); rc -1 is a
    refusal whose message sayuri_hip_last_error holds."""
    lib = _lib.hip()
    bsz = np.asarray(board_sizes, np.int32)
    cat = lambda arrs: None if arrs is None else fp(np.concatenate([np.ascontiguousarray(a, np.float32).ravel() for a in arrs]))
    one = lambda a: None if a is None else fp(np.ascontiguousarray(a, np.float32))
    y = np.full(cout * int((bsz.astype(np.int64) ** 2).sum()), np.nan, np.float32)
    rc = lib.sayuri_hip_test_conv_pw(0, len(bsz), ip(bsz), max_board, cin, cout, act, cat(xs), one(w), one(bias), cat(res), fp(y), pieces)
    outs, off = [], 0
    for b in bsz:
        outs.append(y[off:off + cout * b * b].reshape(cout, b * b))
        off += cout * b * b
    return rc, outs, lib.sayuri_hip_test_last_conv_kind()


def conv_dw_layer(board_sizes, channels: int, k: int, act: int, xs, w, bias=None, res=None, strips: int = 0, max_board: int = 19,
                  use_fp16: bool = True):
    """The layer tap of the depthwise kernel on LDS (sayuri_hip_test_conv_dw, csrc/hip/conv_dw.h): one fp16 depthwise k x k layer
    on host tensors, no context.  xs / res: per-sample [channels][b*b] arrays (res None: no residual; given, it is added behind
    the activation), w [channels][k*k], strips per sample (0: the engine's choice).  -> (rc, per-sample [channels][b*b] outputs
    that start as NaN, sayuri_hip_test_last_conv_kind); rc -1 is a refusal whose message sayuri_hip_last_error holds."""
    lib = _lib.hip()
    bsz = np.asarray(board_sizes, np.int32)
    cat = lambda arrs: None if arrs is None else fp(np.concatenate([np.ascontiguousarray(a, np.float32).ravel() for a in arrs]))
    one = lambda a: None if a is None else fp(np.ascontiguousarray(a, np.float32))
    y = np.full(channels * int((bsz.astype(np.int64) ** 2).sum()), np.nan, np.float32)
    rc = lib.sayuri_hip_test_conv_dw(0, int(use_fp16), len(bsz), ip(bsz), max_board, channels, k, act, cat(xs), one(w), one(bias),
                                     cat(res), strips, fp(y))
    outs, off = [], 0
    for b in bsz:
        outs.append(y[off:off + channels * b * b].reshape(channels, b * b))
        off += channels * b * b
    return rc, outs, lib.sayuri_hip_test_last_conv_kind()


def conv_dw_pad_bits(which: int = 0):
    """The pad channels [channels, stride) of every board pixel after this thread's last conv_dw_layer, raw fp16 bits
    (sayuri_hip_test_last_dw_pad): which = 0 the kernel on LDS, 1 depthwise_kernel on the same operands."""
    lib = _lib.hip()
    n = lib.sayuri_hip_test_last_dw_pad(which, None, 0)
    bits = np.zeros(max(n, 1), np.uint16)
    if n < 0 or lib.sayuri_hip_test_last_dw_pad(which, bits.ctypes.data_as(ctypes.POINTER(ctypes.c_uint16)), n) != n:
        raise RuntimeError(lib.sayuri_hip_last_error().decode())
    return bits[:n]
