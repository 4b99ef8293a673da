"""One Python caller per layer tap of the device library (include/sayuri_hip.h: sayuri_hip_test_*; the signatures are
sayuri_amd/_lib.py's), and the only place in tests/ that names one.

One convention: activations are a list of per-sample [C][b*b] arrays (anything that iterates so), weights any contiguous shape,
res=None is no residual, the SE unit's FCs one tuple fc = (w1, b1, w2, b2), the twelve head tensors one sequence.  Every output
starts as NaN on the host -- what comes back finite was written -- and comes back cut per sample.  A call returns a small named
result with the tap's return code and what the tap's last_* readers say about the launch; it does not assert rc == 0 (1 is "the
form does not apply", -1 a refusal with a message): ok(r) does."""
import collections

import numpy as np

from sayuri_amd import _lib

# sayuri_hip_test_last_conv_kind: the kernel family that ran
KIND_GENERIC, KIND_GLDS, KIND_BOARD, KIND_DEPTHWISE, KIND_SPLIT, KIND_BOARD_SX = range(6)
# sayuri_hip_test_last_se_form: both FC images staged into LDS / the FCs read fp32 weights from L2 (0: nothing was launched)
SE_STAGED, SE_FROM_L2 = 1, 2
MAX_BOARD = 19

Conv = collections.namedtuple("Conv", "rc outs kind")            # conv, conv_split
ConvSe = collections.namedtuple("ConvSe", "rc outs form")
ConvSx = collections.namedtuple("ConvSx", "rc outs kind kts")
SeUnit = collections.namedtuple("SeUnit", "rc outs gate")         # gate [n][2C] = sigmoid(gamma) | beta
Heads = collections.namedtuple("Heads", "rc prob pas misc own")  # on the NN grid: prob [n][prob_ch][B2], own [n][B2]
TowerRun = collections.namedtuple("TowerRun", "rc outs form report")  # outs[layer][sample]; report = (layers, row-order layers, links)


def last_error():
    return _lib.hip().sayuri_hip_last_error().decode()


def ok(r, *what):
    """the tap ran: -> r"""
    assert r.rc == 0, what + (r.rc, last_error())
    return r


def split(flat, bsz, C):
    outs, off = [], 0
    for b in bsz:
        outs.append(flat[off:off + C * b * b].reshape(C, b * b))
        off += C * b * b
    return outs


def _f(a):
    return None if a is None else _lib.fp(np.ascontiguousarray(a, np.float32))


def _cat(arrs):
    return None if arrs is None else _lib.fp(np.concatenate([np.ascontiguousarray(a, np.float32).ravel() for a in arrs]))


def _i(a):
    return _lib.ip(np.asarray(a, np.int32))


def _nan(*shape):
    return np.full(shape, np.nan, np.float32)


def _npix(bsz):
    return sum(b * b for b in bsz)


def conv(fp16, bsz, cin, cout, k, act, xs, w, bias, res=None, depthwise=False, post=False, max_board=MAX_BOARD):
    """one layer on the kernel the engine would pick; post: act(conv + bias) + res"""
    lib, y = _lib.hip(), _nan(cout * _npix(bsz))
    rc = lib.sayuri_hip_test_conv(0, int(fp16), len(bsz), _i(bsz), max_board, cin, cout, k, int(depthwise), act, int(post), _cat(xs), _f(w), _f(bias),
                                  _cat(res), _lib.fp(y))
    return Conv(rc, split(y, bsz, cout), lib.sayuri_hip_test_last_conv_kind())


def conv_split(bsz, cin, cout, act, xs, w, bias, res=None, strips=0, channel_tiles=0, max_board=MAX_BOARD):
    """the fp16 3x3 layer on the latency context's kernel; strips per board (0: the engine's choice)"""
    lib, y = _lib.hip(), _nan(cout * _npix(bsz))
    rc = lib.sayuri_hip_test_conv_split(0, len(bsz), _i(bsz), max_board, cin, cout, act, _cat(xs), _f(w), _f(bias), _cat(res), _lib.fp(y), channel_tiles,
                                        strips)
    return Conv(rc, split(y, bsz, cout), lib.sayuri_hip_test_last_conv_kind())


def se_unit(fp16, bsz, C, se, act, xs, res, fc, max_board=MAX_BOARD):
    """se_pool / se_fc / se_scale"""
    y, gate = _nan(C * _npix(bsz)), _nan(len(bsz), 2 * C)
    rc = _lib.hip().sayuri_hip_test_se_unit(0, int(fp16), len(bsz), _i(bsz), max_board, C, se, act, _cat(xs), _cat(res), *map(_f, fc), _lib.fp(y),
                                            _lib.fp(gate))
    return SeUnit(rc, split(y, bsz, C), gate)


def conv_se(bsz, C, se, act, xs, w, bias, res, fc, via_tower=0, max_board=MAX_BOARD):
    """the C -> C 3x3 layer with the SE unit inside: conv_board_se_kernel, or the SE stage of a one-layer tower run"""
    lib, y = _lib.hip(), _nan(C * _npix(bsz))
    rc = lib.sayuri_hip_test_conv_se(0, len(bsz), _i(bsz), max_board, C, se, act, int(via_tower), _cat(xs), _f(w), _f(bias), _cat(res), *map(_f, fc),
                                     _lib.fp(y))
    return ConvSe(rc, split(y, bsz, C), lib.sayuri_hip_test_last_se_form())


def conv_sx(bsz, C, se, act, xs, w, bias, res, fc, max_board=MAX_BOARD):
    """the same layer split over 2..4 channel tiles per board tile (conv_board_sx_kernel); kts: the tiles it ran on"""
    lib, y = _lib.hip(), _nan(C * _npix(bsz))
    rc = lib.sayuri_hip_test_conv_sx(0, len(bsz), _i(bsz), max_board, C, se, act, _cat(xs), _f(w), _f(bias), _cat(res), *map(_f, fc), _lib.fp(y))
    return ConvSx(rc, split(y, bsz, C), lib.sayuri_hip_test_last_conv_kind(), lib.sayuri_hip_test_last_sx_kts())


def _heads(tap, lead, bsz, chans, dims, act, tensors, ws, max_board):
    n, B2 = len(bsz), max_board * max_board
    ws = [np.ascontiguousarray(w, np.float32) for w in ws]
    w12 = (_lib.c_float_p * 12)(*map(_lib.fp, ws))
    prob_ch, pass_outs, misc_outs = dims
    out = _nan(n, prob_ch, B2), _nan(n, pass_outs), _nan(n, misc_outs), _nan(n, B2)
    rc = tap(*lead, n, _i(bsz), max_board, *chans, *dims, act, *tensors, w12, *map(_lib.fp, out))
    return Heads(rc, *out)


def head_tail(fp16, bsz, Cp, Cv, act, pcs, vcs, ws, dims=(5, 5, 15), max_board=MAX_BOARD):
    """head_tail_kernel on the activated head planes pcs [Cp][b*b], vcs [Cv][b*b]; dims = (prob_ch, pass_outs, misc_outs)"""
    return _heads(_lib.hip().sayuri_hip_test_head_tail, (0, int(fp16)), bsz, (Cp, Cv), dims, act, (_cat(pcs), _cat(vcs)), ws, max_board)


def head_board(bsz, C, Cp, Cv, act, ts, p_w, p_b, v_w, v_b, ws, dims=(5, 5, 15), max_board=MAX_BOARD):
    """head_board_kernel on the trunk ts [C][b*b] and the two 1x1 head convolutions"""
    return _heads(_lib.hip().sayuri_hip_test_head_board, (0,), bsz, (C, Cp, Cv), dims, act, (_cat(ts), _f(p_w), _f(p_b), _f(v_w), _f(v_b)), ws, max_board)


def head_boards(r, bsz, max_board=MAX_BOARD):
    """a head tap's outputs cut to each sample's board -> [(prob [prob_ch][b*b], pass, own [b*b], misc)]; the off-board cells of the
    NN grid must have stayed 0"""
    outs = []
    for i, b in enumerate(bsz):
        prob, own = r.prob[i].reshape(-1, max_board, max_board), r.own[i].reshape(max_board, max_board)
        mask = np.ones((max_board, max_board), bool)
        mask[:b, :b] = False
        assert not prob[:, mask].any() and not own[mask].any(), (i, b, "an off-board cell was written")
        outs.append((prob[:, :b, :b].reshape(-1, b * b), r.pas[i], own[:b, :b].ravel(), r.misc[i]))
    return outs


def tower_run(spec, D, chain=1, max_board=MAX_BOARD):
    """A run of spec.L board convolutions as one launch of the persistent tower kernel.  spec: bsz, C, cin0, L, acts, res_from, se =
    (layer, SE width) or None; D: xs, ws and bias of every layer, fc."""
    lib, per = _lib.hip(), spec.C * _npix(spec.bsz)
    y, report = _nan(spec.L * per), np.zeros(3, np.int32)
    layer, width = spec.se or (-1, 0)
    rc = lib.sayuri_hip_test_tower_run(0, len(spec.bsz), _i(spec.bsz), max_board, spec.C, spec.cin0, spec.L, _i(spec.acts), _i(spec.res_from), _cat(D.ws),
                                       _f(D.bias), layer, width, *map(_f, D.fc if spec.se else [None] * 4), chain, _cat(D.xs), _lib.fp(y))
    assert lib.sayuri_hip_test_last_tower_run(_lib.ip(report)) == 0
    return TowerRun(rc, [split(y[l * per:(l + 1) * per], spec.bsz, spec.C) for l in range(spec.L)], lib.sayuri_hip_test_last_se_form(),
                    tuple(int(v) for v in report))


# sayuri_hip_test_last_pack: the input-stage kernel that ran
PACK_KERNELS = ("chunked", "flat", "bits", "symm")
PACK_TAPS = ("sayuri_hip_test_pack_input", "sayuri_hip_test_last_pack")
Pack = collections.namedtuple("Pack", "rc image guard kernel cs split passes")  # image [n][max_board^2][cs], guard [guard_rows][cs], as stored


def pack_input(fp16, bsz, cin, sentinel, planes=None, records=None, binary=0, src=None, symm=None, n_records=0, perm=None, n0=0, ns=None, stage_batch=0,
               in_place=False, guard_rows=0, max_board=MAX_BOARD):
    """One input-stage kernel on host data, chosen and launched by the engine's own code.  bsz: the board of every DEVICE sample;
    perm: the caller's slot of each (None: no table).  planes [n][cin][max_board^2], or records (uint32 [.][binary*12 + 8]) read
    by slot, or -- symm given -- by the record map src (None: the identity) under symm.  stage_batch > 0: the geometry (and the
    map) go through the staging kernels from a ring laid out for that batch size; in_place: the records stay in pinned host
    memory.  The whole image and guard_rows rows behind it start as `sentinel` and come back raw."""
    lib, n = _lib.hip(), len(bsz)
    cs = (cin + 31) // 32 * 32
    out = np.full((n * max_board * max_board + guard_rows, cs), np.nan, np.float32)
    rec = None if records is None else np.ascontiguousarray(records, np.uint32)
    rc = lib.sayuri_hip_test_pack_input(0, int(fp16), n, _i(bsz), max_board, cin, _f(planes), None if rec is None else rec.ctypes.data,
                                        n_records or (0 if rec is None else len(rec)), binary, None if src is None else _i(src),
                                        None if symm is None else _i(symm), None if perm is None else _i(perm), n0, n - n0 if ns is None else ns,
                                        stage_batch, int(in_place), float(sentinel), guard_rows, _lib.fp(out))
    report = np.zeros(4, np.int32)
    assert lib.sayuri_hip_test_last_pack(_lib.ip(report)) == 0
    k = int(report[0])
    return Pack(rc, out[:n * max_board * max_board].reshape(n, max_board * max_board, cs), out[n * max_board * max_board:],
                PACK_KERNELS[k] if 0 <= k < 4 else None, int(report[1]), int(report[2]), int(report[3]))
