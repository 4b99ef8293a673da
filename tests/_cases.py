"""What more than one kernel test module uses: the case tables, the seeded draws (cached: a draw and its float64 convolution
are computed once per process) and the shared bounds.  The GPU modules run the kernels on these; the test_*_reference_cpu.py
modules prove on the very same draws that the cases are sensitive and inside their regimes.  The references are in _kref.py."""
import collections
import functools

import numpy as np

from _kref import act_np, conv3x3_f64, exact_conv, exact_layer, head_tail_f64, r16, se_unit_f64


# ---- layer shapes
CASES = [
    # bsz, cin, cout, k
    ([19], 32, 32, 3),
    ([19, 19, 19], 64, 64, 3),
    ([9, 13, 19, 7, 19], 32, 64, 3),       # mixed boards in one batch, tiles crossing samples
    ([19] * 4, 43, 96, 3),                   # input conv shape of the 6b96 net (cin padded to 64)
    ([19] * 3, 96, 96, 3),
    ([19] * 2, 256, 256, 3),                 # the tower conv of the 20b256 net
    ([13] * 5, 128, 192, 3),
    ([19] * 2, 256, 32, 1),                  # head conv
    ([9, 19], 48, 72, 1),                    # mixer ffn-like 1x1 with odd channel counts
    ([19] * 2, 384, 384, 3),                 # 40b384 tower conv (two ko tiles)
    ([2, 3, 5, 19], 32, 32, 3),              # tiny boards
]


BOARD_CASES = [
    # bsz, cin, cout: fp16 3x3 layers the one-workgroup-per-board kernel (conv_board.h) takes
    ([19] * 3, 256, 256),                         # the tower conv of the 20b256 net, one board per tile (12 + 11 column tiles)
    ([19] * 4, 43, 256),                          # its input conv (cin padded to 64: two chunks)
    ([19] * 2, 384, 384),                         # 40b384: two 192-channel tiles per board (odd row-tile count per wave)
    ([13] * 5, 128, 192),                         # two boards per tile + a half-empty last tile
    ([9] * 9, 64, 128),                           # four boards per tile, 128-channel tile (two row tiles per wave)
    ([19, 19, 13, 13, 9, 9, 9, 9, 19, 13], 256, 256),   # mixed sizes: one size per tile
    ([7] * 13, 32, 128),                          # seven boards per tile
    ([19], 256, 256),                             # a batch of one
]


# the latency context's split kernel (test_gpu_latency.py)
LAYER_SHAPES = [
    # bsz, cin, cout
    ([19], 256, 256),
    ([19, 19, 19], 128, 128),
    ([19, 13], 384, 384),
    ([9], 256, 256),
    ([13], 128, 384),
    ([19, 19, 13, 13, 9, 9, 9, 9, 19, 13], 256, 256),   # mixed sizes: boards that share a board tile are cut per sample
    ([13, 9, 9, 19, 13, 9], 43, 128),                   # an input convolution (cin padded to 64: two chunks)
    ([9] * 9, 128, 256),
]


# ---- inputs of the split-channel SE convolution tests.  With x ~ N(0, 1) per pixel a channel's mean is ~ 1 / sqrt(npix) and
# the unit's gates sit near 0.5: a wrong mean row of the squeeze image would move nothing.  So the convolution gets a bias
# of O(1) per channel (pooled means of O(1) that differ by channel), and the two FCs are scaled to pre-activations of O(1)
# (gates spread over ~0.1 .. 0.9).  tests/test_sx_reference_cpu.py proves on these very draws that the unit's terms matter.
SX_TOL = 3e-3


class SxTrunk:
    """x, w, bias, res of one C -> C 3x3 layer over the boards `bsz` (x, w, res rounded to fp16 as the kernel sees them), and
    the float64 convolution of each sample, computed once on demand."""

    def __init__(self, seed, bsz, C):
        rng = np.random.default_rng([seed, C] + list(bsz))
        self.bsz, self.C = list(bsz), C
        self.xs = [r16(rng.standard_normal((C, b * b)).astype(np.float32), True) for b in bsz]
        self.rs = [r16(rng.standard_normal((C, b * b)).astype(np.float32), True) for b in bsz]
        self.w = r16((rng.standard_normal((C, C, 3, 3)) / np.sqrt(9 * C)).astype(np.float32), True)
        self.bias = rng.standard_normal(C).astype(np.float32)
        self._conv = {}

    def conv(self, i):
        if i not in self._conv:
            self._conv[i] = conv3x3_f64(self.xs[i], self.w, self.bias, self.bsz[i])
            self._conv[i].setflags(write=False)
        return self._conv[i]


@functools.lru_cache(maxsize=None)
def sx_trunk(seed, bsz, C):
    return SxTrunk(seed, bsz, C)


@functools.lru_cache(maxsize=None)
def sx_fc(seed, C, se):
    """w1 [se][3C], b1 [se], w2 [2C][se], b2 [2C] of the unit"""
    rng = np.random.default_rng([seed, C, se, 77])
    w1 = (rng.standard_normal((se, 3 * C)) / np.sqrt(3 * C)).astype(np.float32)
    b1 = (rng.standard_normal(se) * 0.5).astype(np.float32)
    w2 = (rng.standard_normal((2 * C, se)) / np.sqrt(se)).astype(np.float32)
    b2 = (rng.standard_normal(2 * C) * 0.5).astype(np.float32)
    return w1, b1, w2, b2


def sx_reference(T, fc, i, act, with_res):
    return se_unit_f64(T.conv(i), T.rs[i] if with_res else None, *fc, T.bsz[i], act)


# ====================================================================================================================
# Pooled statistics of the one-workgroup SE kernels and of the heads.
#
# With x ~ N(0, 1) a test cannot see a wrong pooled statistic: a channel mean is ~ 1 / sqrt(npix), a single pixel moves it by
# 1 / npix, the maximum is never negative.  The draws below are inputs on which each statistic carries weight; test_gpu_smallops.py
# compares the kernels on them with float64 references (conv3x3_f64 + se_unit_f64, head_tail_f64).  tests/test_se_head_reference_cpu.py pins
# head_tail_f64 to the oracle's tap and proves, on these very draws, that every listed defect of the pooling moves the
# reference by >= 4x the GPU tests' tolerance, and that the staged kernel's fp16 images cost <= half of it.
#
#   spread draws  the sx_trunk / sx_fc recipe: pooled means of O(1) that differ by channel, gates over ~0.1 .. 0.9.
#   probe draws   what random data cannot show -- one pixel too few or too many, a maximum that sees an empty cell.  The input
#                 is small noise with one spike per channel at a boundary pixel of the kernels' pixel partitions (by channel
#                 group, probe_pixels), the convolution passes it on (identity centre tap + a small remainder), one channel
#                 group sits at a negative level so that its true maximum is negative, and the FCs are probes: a hidden unit
#                 reads the mean or the maximum of ONE channel group and the next FC carries it to that group with a known gain.
PROBE_NOISE = 0.05
PROBE_GROUPS = 8  # channel c belongs to group c % 8: 0..5 spike at probe_pixels(bs)[g], 6 the negative level, 7 noise alone (the unit: a level of 1)
PROBE_NEG = 6
PROBE_B1 = 2.0    # the hidden probes sit at 2 + gain * statistic: every activation has slope ~1 there


def probe_pixels(bs):
    """pixel 0, the last pixel, the first pixel of the last 16-pixel column tile, the end of the first row, the start of the
    last row, the first pixel of the second wave column (conv_board.h: column tiles (ncols + 1) / 2 .. of the tile)"""
    npix = bs * bs
    ncols = (npix + 15) // 16
    return (0, npix - 1, 16 * ((npix - 1) // 16), bs - 1, npix - bs, min(npix - 1, 16 * ((ncols + 1) // 2)))


def probe_amp(bs):
    """height of the spike: 8 on 9x9 and larger; lower on the smallest boards, where one pixel is a large share of the mean
    (a spike of 8 over 4 pixels would carry the output scale, which the tolerance is relative to, to ~40)"""
    return 8.0 if bs >= 9 else max(1.0, 8.0 * bs * bs / 81.0)


def probe_planes(rng, C, bs, level=None):
    """[C][bs*bs] float64: noise, the spike of each channel's group, `level` added to the channels of the negative group"""
    x = PROBE_NOISE * rng.standard_normal((C, bs * bs))
    g = np.arange(C) % PROBE_GROUPS
    for k, p in enumerate(probe_pixels(bs)):
        x[g == k, p] += probe_amp(bs)
    if level is not None:
        x[g == PROBE_NEG] += level
    return x


def probe_fc(C, outs, rows):
    """[outs][3C] float32 probe rows over a (mean, scaled mean, max) vector, and their bias: row k reads one statistic of one
    channel group, rows[k] = (group, "mean" | "scaled" | "max", gain); the gain is divided over the group's channels; the other
    rows are 0"""
    w, b = np.zeros((outs, 3 * C), np.float32), np.zeros(outs, np.float32)
    g = np.arange(C) % PROBE_GROUPS
    for k, (group, kind, gain) in enumerate(rows):
        sel = np.flatnonzero(g == group)
        w[k, ("mean", "scaled", "max").index(kind) * C + sel] = gain / len(sel)
        b[k] = PROBE_B1
    return w, b


class SeProbe:
    """SxTrunk's counterpart of the probe draws (same attributes)."""

    def __init__(self, seed, bsz, C):
        rng = np.random.default_rng([seed, C, 11] + list(bsz))
        self.bsz, self.C = list(bsz), C
        self.xs = [r16(probe_planes(rng, C, b).astype(np.float32), True) for b in bsz]
        self.rs = [r16((0.25 * rng.standard_normal((C, b * b))).astype(np.float32), True) for b in bsz]
        w = 0.02 * rng.standard_normal((C, C, 3, 3)) / np.sqrt(9 * C)
        w[np.arange(C), np.arange(C), 1, 1] += 1.0
        self.w = r16(w.astype(np.float32), True)
        self.bias = np.choose(np.arange(C) % PROBE_GROUPS, [0.0] * 6 + [-2.0, 1.0]).astype(np.float32)
        self._conv = {}

    conv = SxTrunk.conv


# The unit's probes: (channel group, statistic, squeeze gain, group whose beta shows it, excite gain) -- all powers of two, exact
# in the fp16 images.  Spike groups: mean -> beta 4 * 4 (a pixel of 8 in 361 moves beta by 0.35), maximum -> beta 1/4 * 1/2 (a lost
# spike of 8 moves it by 1).  The negative group's maximum (-1.9) shows in the level group's beta, 1/2 * 1 (a 0 in its place: 0.95):
# its own channels sit at -2, where ReLU and HardSwish would hide any beta.  The level group (conv bias 1: a mean of 1): mean
# 2 * 2 (divided by 384 on 19x19: 0.24), scaled mean 1 * 2 (a neighbour size's factor, or none on 13x13 / 15x15: 0.2).  Separate
# gains: with one gain for all, either "pixel 0 twice" drowns or the output scale, which the tolerance follows, blows up.
PROBE_LEVEL = 7
SE_PROBES = ([(g, "mean", 4.0, g, 4.0) for g in range(6)] + [(g, "max", 0.25, g, 0.5) for g in range(6)] +
             [(PROBE_NEG, "max", 0.5, PROBE_LEVEL, 1.0), (PROBE_LEVEL, "mean", 2.0, PROBE_LEVEL, 2.0), (PROBE_LEVEL, "scaled", 1.0, PROBE_LEVEL, 2.0)])


@functools.lru_cache(maxsize=None)
def se_probe_fc(seed, C, se):
    """w1, b1, w2, b2 of the probe unit (SE_PROBES); gamma from its bias alone"""
    rng = np.random.default_rng([seed, C, se, 78])
    w1, b1 = probe_fc(C, se, [p[:3] for p in SE_PROBES])
    w2, b2 = np.zeros((2 * C, se), np.float32), np.zeros(2 * C, np.float32)
    b2[:C] = (rng.standard_normal(C) * 0.5).astype(np.float32)
    g = np.arange(C) % PROBE_GROUPS
    for k, p in enumerate(SE_PROBES):
        w2[C + np.flatnonzero(g == p[3]), k] = p[4]
    b2[C:] = -PROBE_B1 * w2[C:].sum(axis=1)  # the probes' resting level taken out again
    b2[C + np.flatnonzero(g == PROBE_LEVEL)] += 4.0  # keeps the level group's output above 0 on every board size (ReLU)
    return w1, b1, w2, b2


@functools.lru_cache(maxsize=None)
def se_inputs(draw, seed, bsz, C, se):
    """(trunk, (w1, b1, w2, b2)) of one layer of the pooled-statistics cases; draw = "spread" | "probe" """
    if draw == "spread":
        return sx_trunk(seed, tuple(bsz), C), sx_fc(seed, C, se)
    assert draw == "probe"
    return SeProbe(seed, tuple(bsz), C), se_probe_fc(seed, C, se)


# The cases: (C, se) whose images make_se_images stages, and two it refuses (the FCs then read fp32 weights from L2: C = 256, se = 128
# is what the engine meets; at C = 128 the images fit far beyond the usual widths, and the L2 form's thread layout needs 512 % (se / 4) == 0).
SE_SEED = 41
SE_LAYERS = ((256, 64), (128, 32))
SE_L2_LAYERS = ((256, 128), (128, 256))
SE_BATCHES = ((19, 19), (19, 18, 17, 16, 15, 14), (2,), (3,), (5,), (9,), (13,))  # one sample per tile
SE_ACT_BATCH = (19, 15)
SE_L2_BATCHES = ((19, 17, 14), (9,))
SE_UNIT_BATCHES = ((19, 16, 14), (9, 9, 9, 13, 13, 2))  # se_pool / se_fc / se_scale: any batch


def se_case_batches(C, se, act):
    """the batches of test_conv_se_pooled_statistics at this layer and activation (none: no such case)"""
    if (C, se) in SE_L2_LAYERS:
        return SE_L2_BATCHES if act == 5 else ()
    return (SE_BATCHES if act in (5, 0) else ()) + ((SE_ACT_BATCH,) if (C, se) == (128, 32) else ())


SE_CASES = [(C, se, act) for C, se in SE_LAYERS + SE_L2_LAYERS for act in (5, 0, 1, 2, 3, 4, 6, 7) if se_case_batches(C, se, act)]
SE_CASE_IDS = [f"C{c}se{s}act{a}" for c, s, a in SE_CASES]


def se_unit_x(T, i, fp16):
    """the unit's input of the separate kernels' cases: the trunk's convolution as the engine would have stored it"""
    return r16(T.conv(i).astype(np.float32), fp16)


HEAD_SEED = 43
HEAD_BOARDS = (19, 14, 13, 9, 2)
HEAD_PAIRS = ((32, 32), (24, 48))
HEAD_DIMS = dict(prob_ch=5, pass_outs=5, misc_outs=15)
# probe gains of the heads: p_inter / v_inter rows as probe_fc; the statistic reaches pass / misc through the random second FC
HEAD_PROBES = [(g, "mean", 32.0) for g in range(6)] + [(g, "max", 0.25) for g in range(6)] + [(PROBE_NEG, "max", 2.0)]


def head_weights(draw, rng, Cp, Cv):
    """weights12.  spread: the recipe of test_head_tail_kernel with biases of 0.5 N(0, 1); probe: p_inter / v_inter are probe rows."""
    d = HEAD_DIMS
    shapes = [(Cp, 3 * Cp), (Cp,), (d["pass_outs"], Cp), (d["pass_outs"],), (3 * Cv, 3 * Cv), (3 * Cv,), (d["misc_outs"], 3 * Cv), (d["misc_outs"],),
              (d["prob_ch"], Cp), (d["prob_ch"],), (Cv,), (1,)]
    ws = [(rng.standard_normal(s) / np.sqrt(s[-1]) if len(s) > 1 else 0.5 * rng.standard_normal(s)).astype(np.float32) for s in shapes]
    if draw == "probe":
        ws[0], ws[1] = probe_fc(Cp, Cp, HEAD_PROBES)
        ws[4], ws[5] = probe_fc(Cv, 3 * Cv, HEAD_PROBES[:6])
    ws[8], ws[10] = r16(ws[8], True), r16(ws[10], True)  # head_board_kernel holds the per-pixel weights as an fp16 image
    return ws


class HeadDraw:
    """Inputs of the head kernels over the boards `bsz`.  C = 0: the activated head planes themselves (head_tail_kernel), rounded
    to fp16 where the kernel stores them so; C > 0: a trunk and the two 1x1 head convolutions in front (head_board_kernel), the
    planes are their float64 result.  planes(i, act) -> (pc, vc) of sample i, computed once."""

    def __init__(self, draw, seed, bsz, Cp, Cv, C=0, fp16=True):
        rng = np.random.default_rng([seed, Cp, Cv, C, int(draw == "probe")] + list(bsz))
        self.bsz, self.Cp, self.Cv, self.C = list(bsz), Cp, Cv, C
        self.ws = head_weights(draw, rng, Cp, Cv)
        self._planes = {}
        if C == 0:
            if draw == "spread":
                mk = lambda ch, b: rng.standard_normal((ch, b * b)) + rng.standard_normal((ch, 1))
                self.pcs, self.vcs = [mk(Cp, b) for b in bsz], [mk(Cv, b) for b in bsz]
            else:
                self.pcs = [probe_planes(rng, Cp, b, level=-2.0) for b in bsz]
                self.vcs = [probe_planes(rng, Cv, b) for b in bsz]
            self.pcs = [r16(p.astype(np.float32), fp16) for p in self.pcs]
            self.vcs = [r16(v.astype(np.float32), fp16) for v in self.vcs]
            return
        if draw == "spread":
            self.ts = [rng.standard_normal((C, b * b)) for b in bsz]
            p_w, v_w = rng.standard_normal((Cp, C)) / np.sqrt(C), rng.standard_normal((Cv, C)) / np.sqrt(C)
            self.p_b, self.v_b = rng.standard_normal(Cp).astype(np.float32), rng.standard_normal(Cv).astype(np.float32)
        else:
            # trunk channel j carries the spike of policy channel j, channel Cp + j that of value channel j; dominant rows pass them on
            self.ts = [PROBE_NOISE * rng.standard_normal((C, b * b)) for b in bsz]
            for t, b in zip(self.ts, bsz):
                t[:Cp] = probe_planes(rng, Cp, b)
                t[Cp:Cp + Cv] = probe_planes(rng, Cv, b)
            p_w, v_w = 0.02 * rng.standard_normal((Cp, C)) / np.sqrt(C), 0.02 * rng.standard_normal((Cv, C)) / np.sqrt(C)
            p_w[np.arange(Cp), np.arange(Cp)] += 1.0
            v_w[np.arange(Cv), Cp + np.arange(Cv)] += 1.0
            # the negative group rests where Mish is lowest (-0.31 at -1.2); the identity keeps -1.2
            self.p_b = np.where(np.arange(Cp) % PROBE_GROUPS == PROBE_NEG, -1.2, 0.0).astype(np.float32)
            self.v_b = np.zeros(Cv, np.float32)
        self.ts = [r16(t.astype(np.float32), True) for t in self.ts]
        self.p_w, self.v_w = r16(p_w.astype(np.float32), True), r16(v_w.astype(np.float32), True)

    def planes(self, i, act):
        if self.C == 0:
            return self.pcs[i], self.vcs[i]
        if (i, act) not in self._planes:
            t = self.ts[i].astype(np.float64)
            self._planes[i, act] = (act_np(self.p_w.astype(np.float64) @ t + self.p_b[:, None], act),
                                    act_np(self.v_w.astype(np.float64) @ t + self.v_b[:, None], act))
        return self._planes[i, act]

    def reference(self, i, act, **kw):
        return head_tail_f64(*self.planes(i, act), self.ws, self.bsz[i], act, **kw)


@functools.lru_cache(maxsize=None)
def head_inputs(draw, seed, bsz, Cp, Cv, C=0, fp16=True):
    return HeadDraw(draw, seed, tuple(bsz), Cp, Cv, C, fp16)


# ---- runs of the persistent tower (test_gpu_tower_run.py)
PLAIN_TOL = 4e-3  # times max|ref|: test_gpu_layers.py, fp16


class RunSpec:
    """One run: boards, width, the first layer's input channels, per layer activation and residual source (-1 none, 0 the run's
    input, k the output of layer k-1), the SE layer (index, SE width) or None."""

    def __init__(self, bsz, C, acts, res_from, cin0=None, se=None, seed=0):
        self.bsz, self.C, self.acts, self.res_from = tuple(bsz), C, tuple(acts), tuple(res_from)
        self.cin0 = C if cin0 is None else cin0
        self.se, self.seed = se, seed
        self.L = len(self.acts)
        assert len(self.res_from) == self.L

    def __repr__(self):
        return f"run(C={self.C} cin0={self.cin0} boards={list(self.bsz)} acts={self.acts} res={self.res_from} se={self.se})"


class RunDraw:
    """x of every sample, w and bias of every layer (x, w fp16-exact), the SE unit's FCs"""

    def __init__(self, bsz, C, cin0, L, se, seed):
        rng = np.random.default_rng([seed, C, cin0, L] + list(bsz))
        self.xs = [r16(rng.standard_normal((cin0, b * b)).astype(np.float32), True) for b in bsz]
        self.ws = []
        for l in range(L):
            cin = cin0 if l == 0 else C
            self.ws.append(r16((rng.standard_normal((C, cin, 3, 3)) / np.sqrt(9 * cin)).astype(np.float32), True))
        self.bias = (rng.standard_normal((L, C)) * 0.1).astype(np.float32)
        self.fc = sx_fc(seed, C, se[1]) if se else None
        self._w64 = {}

    def w64(self, l):
        if l not in self._w64:
            self._w64[l] = self.ws[l].astype(np.float64)
        return self._w64[l]


@functools.lru_cache(maxsize=8)
def _draw(bsz, C, cin0, L, se, seed):
    return RunDraw(bsz, C, cin0, L, se, seed)


def run_draw(spec):
    return _draw(spec.bsz, spec.C, spec.cin0, spec.L, spec.se, spec.seed)


def layer_io(spec, D, outs, l):
    """what layer l of the run read: (input of every sample, residual of every sample or None)"""
    xin = D.xs if l == 0 else outs[l - 1]
    r = spec.res_from[l]
    return xin, None if r < 0 else (D.xs if r == 0 else outs[r - 1])


def layer_f64(spec, D, l, i, x, res, w64=None):
    """(float64 reference of layer l on sample i given its input x and residual, its tolerance)"""
    b = spec.bsz[i]
    conv = conv3x3_f64(x, D.w64(l) if w64 is None else w64, D.bias[l], b)
    if spec.se and spec.se[0] == l:
        ref = se_unit_f64(conv, res, *D.fc, b, spec.acts[l])
        return ref, SX_TOL * max(1.0, float(np.abs(ref).max()))
    ref = act_np(conv + (np.asarray(res, np.float64) if res is not None else 0.0), spec.acts[l])
    return ref, PLAIN_TOL * float(np.abs(ref).max())


BLOCK3 = (-1, 0, 1)  # layer 1 adds the run's input, layer 2 the output of layer 0: one hand-over (0 -> 1), one refused (1 has a residual)
RES_BLOCKS8 = (-1, 0, -1, 2, -1, 4, -1, 6)  # four residual blocks: conv, conv + the block's input


def blocks_spec(C):
    return RunSpec((19, 19), C, (5,) * 8, RES_BLOCKS8, seed=700)


SWAP = {2: 3, 3: 2}
CAN_FAIL_BAR = 4.0  # times the tolerance: the bar of the project's can-fail cases


# ---- exact arithmetic (test_gpu_exact.py)
TIERS = {"unit": (2, 1), "wide": (16, 8)}  # |x|, |w| at most
BIAS_MAX, RES_MAX = 8, 16


def exact_draw(tier, bsz, cin, cout, k, depthwise, seed):
    """-> (xs [sample] = [cin][b*b], w [cout][cin | 1][k][k], bias [cout], res [sample] = [cout][b*b]), float32 integers of `tier`"""
    xa, wa = TIERS[tier]
    rng = np.random.default_rng([seed, xa, cin, cout, k, int(depthwise)] + list(bsz))
    xc = cout if depthwise else cin
    xs = [rng.integers(-xa, xa + 1, (xc, b * b)).astype(np.float32) for b in bsz]
    w = rng.integers(-wa, wa + 1, (cout, 1 if depthwise else cin, k, k)).astype(np.float32)
    bias = rng.integers(-BIAS_MAX, BIAS_MAX + 1, cout).astype(np.float32)
    res = [rng.integers(-RES_MAX, RES_MAX + 1, (cout, b * b)).astype(np.float32) for b in bsz]
    return xs, w, bias, res


# ------------------------------------------------------------------------------------------------ the cases
Case = collections.namedtuple("Case", "tier fp16 bsz cin cout k depthwise act with_res post seed")
SeCase = collections.namedtuple("SeCase", "tier bsz C se act with_res seed")
EPILOGUES = ((0, False), (1, True), (1, False), (0, True))  # activation, with residual


def case_id(c):
    if isinstance(c, SeCase):
        return f"{c.tier}-C{c.C}se{c.se}n{len(c.bsz)}b{min(c.bsz)}act{c.act}res{int(c.with_res)}"
    return (f"{c.tier}-{'fp16' if c.fp16 else 'fp32'}-{c.cin}x{c.cout}k{c.k}{'dw' if c.depthwise else ''}n{len(c.bsz)}b{min(c.bsz)}"
            f"act{c.act}res{int(c.with_res)}{'post' if c.post else ''}")


# the generic kernel's own shapes (kind 0 in fp32 and in fp16: no board or LDS-DMA kernel has these channel tiles, or k = 1)
GENERIC_SHAPES = [CASES[2], CASES[3], CASES[8], CASES[7], CASES[10]]
assert [s[1:] for s in GENERIC_SHAPES] == [(32, 64, 3), (43, 96, 3), (48, 72, 1), (256, 32, 1), (32, 32, 3)]
GENERIC_EXACT = [Case("unit", fp16, tuple(bsz), cin, cout, k, False, act, with_res, False, 10 + j)
                 for j, (bsz, cin, cout, k) in enumerate(GENERIC_SHAPES) for fp16 in (False, True) for act, with_res in EPILOGUES]

WIDE_CHANNELS = (256, 384, 512)  # where the wide draw rounds enough (tests/test_exact_reference_cpu.py)
BOARD_EXACT = [Case(tier, True, tuple(bsz), cin, cout, 3, False, act, with_res, False, 30 + j)
               for j, (bsz, cin, cout) in enumerate(BOARD_CASES) for tier in ("unit", "wide") if tier == "unit" or (cin in WIDE_CHANNELS and cin == cout)
               for act, with_res in EPILOGUES[:2]]

SPLIT_SHAPES = [LAYER_SHAPES[5], LAYER_SHAPES[6]]
assert [s[1:] for s in SPLIT_SHAPES] == [(256, 256), (43, 128)]
SPLIT_EXACT = ([Case("unit", True, tuple(bsz), cin, cout, 3, False, act, with_res, False, 50 + j)
                for j, (bsz, cin, cout) in enumerate(SPLIT_SHAPES) for act, with_res in EPILOGUES[:2]] +
               [Case("wide", True, (19,), 256, 256, 3, False, act, with_res, False, 52) for act, with_res in EPILOGUES[:2]])


def split_strips(bsz):
    return (1, 2, max(bsz), 0)


DEPTHWISE_BOARDS = (19, 9, 2, 3, 5)  # the last three are smaller than the 5 x 5 and 7 x 7 kernels
# post_residual = 1: act(conv + bias) + res.  The kernel has no residual in front of the activation (the tap passes none on when
# post_residual = 0), so those cases have no residual.
DEPTHWISE_EXACT = [Case("unit", fp16, DEPTHWISE_BOARDS, 1, C, k, True, act, bool(post), bool(post), 60 + k)
                   for k in (3, 5, 7) for fp16 in (False, True) for C in (48, 40) for post in (0, 1) for act in (0, 1)]

SE_BOARDS = ((19, 19), (14,), (9,))
SE_EXACT = [SeCase(tier, bsz, C, se, act, with_res, 70 + j)
            for j, (C, se) in enumerate(((256, 64), (128, 32), (256, 128))) for bsz in SE_BOARDS
            for tier in ("unit", "wide") if tier == "unit" or C in WIDE_CHANNELS for act, with_res in EPILOGUES[:2]]
SX_BOARDS = SE_BOARDS + ((10,) * 4 + (11,) * 3 + (12,) * 3,)
SX_EXACT = [SeCase(tier, bsz, C, se, act, with_res, 80 + j)
            for j, (C, se) in enumerate(((384, 96), (512, 64))) for bsz in SX_BOARDS for tier in ("unit", "wide") for act, with_res in EPILOGUES[:2]]


@functools.lru_cache(maxsize=2)
def draw_conv(tier, bsz, cin, cout, k, depthwise, seed):
    """(exact_draw, [exact_conv of every sample]): the cases of one shape share the draw and its convolution"""
    draw = exact_draw(tier, bsz, cin, cout, k, depthwise, seed)
    return draw, [exact_conv(draw[0][i], draw[1], b, k, depthwise) for i, b in enumerate(bsz)]


def layer_reference(c, store=np.float16):
    """((xs, w, bias, res | None), [the exact output of every sample]) of a Case"""
    (xs, w, bias, res), conv = draw_conv(c.tier, c.bsz, c.cin, c.cout, c.k, c.depthwise, c.seed)
    res = res if c.with_res else None
    exp = [exact_layer(xs[i], w, bias, res[i] if res else None, b, c.k, c.depthwise, c.act, post=c.post, conv=conv[i],
                       store=store if c.fp16 or store is None else np.float32) for i, b in enumerate(c.bsz)]
    return (xs, w, bias, res), exp


def se_identity_fc(C, se, seed):
    """The SE unit whose gate is the identity: w1 [se][3C] = 0, b1 = 0, w2 [2C][se] = 0, b2 = (+32 for gamma, small integers for beta)"""
    beta = np.random.default_rng([seed, C, se, 99]).integers(-4, 5, C).astype(np.float32)
    fc = (np.zeros((se, 3 * C), np.float32), np.zeros(se, np.float32), np.zeros((2 * C, se), np.float32),
          np.concatenate([np.full(C, 32.0, np.float32), beta]))
    return fc, beta


def se_reference(c, store=np.float16):
    """((xs, w, bias, res | None), fc, [the exact output of every sample]) of an SeCase"""
    (xs, w, bias, res), conv = draw_conv(c.tier, c.bsz, c.C, c.C, 3, False, c.seed)
    res = res if c.with_res else None
    fc, beta = se_identity_fc(c.C, c.se, c.seed)
    exp = [exact_layer(xs[i], w, bias, res[i] if res else None, b, 3, False, c.act, beta=beta, conv=conv[i], store=store) for i, b in enumerate(c.bsz)]
    return (xs, w, bias, res), fc, exp


# ---- tower runs: layer 0 dense unit weights on the unit draw's x, later layers unit weights at a density that keeps three
# layers inside the regime (about 144 non-zero weights per output: |y| grows by ~12 per layer, so layer 2 runs to ~4e4 and
# rounds on its own).  The run around a compiled-epilogue layer is sparse from the start (about 4 weights per output in layers 0
# and 1), so that what HardSwish writes -- multiples of 2^-12 -- stays below 2^12 in sum.
HSWISH = 7
TOWER_BOARDS = ((19, 19, 19), (13,) * 5, (2, 3, 5, 19))
TowerCase = collections.namedtuple("TowerCase", "name bsz acts res_from first43 sparse skip gen")
TOWER_CASES = ([TowerCase(f"{name}-{'x'.join(map(str, sorted(set(bsz))))}", bsz, acts, BLOCK3, False, False, (), 3 if bsz == TOWER_BOARDS[0] else 0)
                for bsz in TOWER_BOARDS for name, acts in (("relu", (1, 1, 1)), ("identity", (0, 0, 0)))] +
               [TowerCase(f"input43-{'x'.join(map(str, sorted(set(bsz))))}", bsz, (1, 0, 1), (-1, -1, 1), True, False, (), 3 if bsz == TOWER_BOARDS[0] else 0)
                for bsz in (TOWER_BOARDS[0], TOWER_BOARDS[2])] +
               [TowerCase(f"hardswish-middle-{'x'.join(map(str, sorted(set(bsz))))}", bsz, (1, HSWISH, 0), BLOCK3, False, True, (1,), 2 if bsz == TOWER_BOARDS[0] else 0)
                for bsz in TOWER_BOARDS[:2]])
TOWER_WIDTHS = (256, 128)


def tower_spec(tc, C):
    return RunSpec(tc.bsz, C, tc.acts, tc.res_from, cin0=43 if tc.first43 else None, seed=90)


class ExactRunDraw:
    """x of every sample, w and bias of every layer, as tower_run takes them"""

    def __init__(self, spec, sparse):
        rng = np.random.default_rng([spec.seed, spec.C, spec.cin0, spec.L, int(sparse)] + list(spec.bsz))
        self.xs = [rng.integers(-2, 3, (spec.cin0, b * b)).astype(np.float32) for b in spec.bsz]
        self.ws = []
        for l in range(spec.L):
            cin = spec.cin0 if l == 0 else spec.C
            density = 1.0 if l == 0 and not sparse else (4.0 if sparse and l < 2 else 144.0) / (9 * cin)
            w = rng.integers(0, 2, (spec.C, cin, 3, 3)) * 2 - 1
            self.ws.append((w * (rng.random(w.shape) < density)).astype(np.float32))
        self.bias = rng.integers(-BIAS_MAX, BIAS_MAX + 1, (spec.L, spec.C)).astype(np.float32)
        self.fc = None


@functools.lru_cache(maxsize=4)
def tower_draw(tc, C):
    return ExactRunDraw(tower_spec(tc, C), tc.sparse)


def exact_run_layer(spec, D, outs, l, store=np.float16):
    """layer l's exact outputs from what layer l - 1 wrote (`outs`) -> [sample]"""
    xin, res = layer_io(spec, D, outs, l)
    return [exact_layer(xin[i], D.ws[l], D.bias[l], res[i] if res is not None else None, b, 3, False, spec.acts[l], store=store)
            for i, b in enumerate(spec.bsz)]


# ---- can-fail: (name, shape ..., the changed weight (k, c), in the last 32-channel chunk -- c = 42 is the last real channel of a
# 43-channel input convolution in front of its padding).  Unit tier, identity, no residual.
CAN_FAIL = [("board", Case("unit", True, (19, 19), 384, 384, 3, False, 0, False, False, 101), (383, 383)),
            ("board-input43", Case("unit", True, (19,) * 4, 43, 256, 3, False, 0, False, False, 102), (255, 42)),
            ("split", Case("unit", True, (13, 9, 9, 19, 13, 9), 43, 128, 3, False, 0, False, False, 103), (64, 42)),
            ("generic", Case("unit", True, (9, 13, 19, 7, 19), 32, 64, 3, False, 0, False, False, 104), (63, 31)),
            ("generic-input43", Case("unit", True, (19,) * 4, 43, 96, 3, False, 0, False, False, 105), (95, 42))]
CAN_FAIL_TAPS = ((1, 1), (0, 2))  # an interior tap and a corner tap
CAN_FAIL_TOWER = TowerCase("one-layer", (19, 19, 19), (0,), (-1,), False, False, (), 1)


# ====================================================================================================================
# The input stage (test_gpu_input.py, test_input_reference_cpu.py): planes or packed records -> the input convolution's image.
#
# A case names the CALLER's slots (cbsz: the board of slot j; for a symmetry case slot j shows record src[j] under symm[j]) and
# the device order perm (device sample i shows slot perm[i]): "sorted" is the engine's own (largest board first, stable), a
# tuple any permutation.  kernel / split / multi are what the tap's report must say: the kernel that ran, the workgroups per
# sample, and whether a workgroup made more than one pass (chunked) or the sample took more than one `base` pass (flat).
PackCase = collections.namedtuple("PackCase", "name fp16 form board cbsz cin binary perm n0 ns kernel split multi stage in_place beyond src symm nrec")
PACK_SPLIT = 4           # kPackSplit
PACK_FLAT_PASS = 16384   # kPackFlatThreads * kPackFlatLoads
PACK_MAX_BINARY = 40     # kPackedMaxBinary
PACK_STAGE_BATCH = 24    # the max_batch the staging ring of a staged case is laid out for (> every case's n)
PACK_GUARD_ROWS = 64
PACK_SENTINEL = -65504.0   # exact in fp16 and in fp32, and no value of a draw


def pack_rule(fp16, cin, board):
    """Engine::pack_input's rule for fp32 planes restated (engine_plan.h pack_plan): -> ("flat", 0, base passes) when a sample's
    image fits 64 KiB of LDS and its planes are below 2^16 floats, else ("chunked", pixels per pass, None)"""
    elem, cs, B2 = (2 if fp16 else 4), (cin + 31) // 32 * 32, board * board
    stride = cs * elem + 16
    if B2 * stride <= 64 * 1024 and cin * B2 < 65536:
        return "flat", 0, -(-cin * B2 // PACK_FLAT_PASS)
    return "chunked", min((B2 + PACK_SPLIT - 1) // PACK_SPLIT, 64 * 1024 // stride), None


def chunked_passes(chunk, bs):
    return -(-((bs * bs + PACK_SPLIT - 1) // PACK_SPLIT) // chunk)


def _pack_case(name, fp16, form, board, cbsz, cin, binary=0, perm="sorted", n0=0, ns=None, kernel=None, multi=False, stage=0, in_place=0, beyond=0,
               src=None, symm=None, nrec=0):
    n = len(cbsz)
    if kernel is None:
        kernel = {"bits": "bits", "symm": "symm"}[form]
    split = 1 if kernel == "flat" or in_place else PACK_SPLIT
    return PackCase(name, fp16, form, board, tuple(cbsz), cin, binary, perm, n0, n - n0 if ns is None else ns, kernel, split, multi, stage, in_place, beyond,
                    src, symm, nrec or n)


def pack_order(c):
    """-> (perm, bsz in device order)"""
    n = len(c.cbsz)
    perm = sorted(range(n), key=lambda j: -c.cbsz[j]) if c.perm == "sorted" else list(range(n) if c.perm is None else c.perm)
    return perm, [c.cbsz[j] for j in perm]


_SHUFFLE12 = (7, 2, 11, 0, 5, 9, 3, 10, 1, 8, 6, 4)   # no involution: used backwards it is another permutation
_SHUFFLE8 = (5, 0, 3, 7, 1, 6, 4, 2)
_SHUFFLE5 = (3, 0, 4, 1, 2)
PACK_PLANE_CASES = [
    # ---- the flat kernel (one workgroup per sample)
    _pack_case("f16-flat-g19-c43-sorted", True, "planes", 19, (9, 19, 2, 13, 3, 19, 7, 5, 16, 11, 18, 4), 43, kernel="flat"),
    _pack_case("f16-flat-g19-c38-shuffled-mid", True, "planes", 19, (6, 8, 10, 12, 14, 15, 17, 19, 2, 3, 19, 13), 38, perm=_SHUFFLE12, n0=3, ns=7, kernel="flat"),
    _pack_case("f16-flat-g19-c64-two-base-passes", True, "planes", 19, (19, 3, 17, 2, 12), 64, perm=_SHUFFLE5, kernel="flat", multi=True),
    _pack_case("f16-flat-g9-c384-two-base-passes", True, "planes", 9, (9, 2, 5, 8, 3), 384, kernel="flat", multi=True),
    _pack_case("f16-flat-g19-c6", True, "planes", 19, (19, 2, 3, 11), 6, perm=None, kernel="flat"),
    _pack_case("f16-flat-g13-c43-mid", True, "planes", 13, (13, 4, 9, 2, 13, 3, 10, 6), 43, perm=_SHUFFLE8, n0=2, ns=5, kernel="flat"),
    _pack_case("f32-flat-g13-c43-sorted", False, "planes", 13, (5, 13, 2, 3, 9, 11, 12, 13), 43, kernel="flat"),
    _pack_case("f32-flat-g9-c38-shuffled", False, "planes", 9, (9, 2, 3, 7, 9, 4, 6, 8), 38, perm=_SHUFFLE8, kernel="flat"),
    _pack_case("f32-flat-g13-c64", False, "planes", 13, (13, 2, 7, 3, 12), 64, perm=_SHUFFLE5, n0=1, ns=3, kernel="flat"),
    # ---- the chunked kernel, one pass per workgroup
    _pack_case("f32-chunked-g19-c43-sorted", False, "planes", 19, (9, 19, 2, 13, 3, 19, 7, 5, 16, 11, 18, 4), 43, kernel="chunked"),
    _pack_case("f32-chunked-g19-c38-shuffled-mid", False, "planes", 19, (6, 8, 10, 12, 14, 15, 17, 19, 2, 3, 19, 13), 38, perm=_SHUFFLE12, n0=4, ns=6, kernel="chunked"),
    _pack_case("f32-chunked-g19-c64", False, "planes", 19, (19, 2, 3, 14, 5), 64, perm=_SHUFFLE5, kernel="chunked"),
    _pack_case("f16-chunked-g19-c96", True, "planes", 19, (19, 3, 17, 2, 12, 19, 6, 9), 96, perm=_SHUFFLE8, kernel="chunked"),
    # ---- the chunked kernel, more than one pass (the first 19x19 workgroups whose pixel range does not fit the LDS at once)
    _pack_case("f32-chunked-g19-c192-passes", False, "planes", 19, (19, 2, 18, 3, 19), 192, perm=_SHUFFLE5, kernel="chunked", multi=True),
    _pack_case("f16-chunked-g19-c384-passes", True, "planes", 19, (3, 19, 2, 19), 384, n0=1, ns=3, kernel="chunked", multi=True),
]

# both bit kernels five ways: split, in place, staged, resident, and with every record bit at or beyond bs*bs set
_WAYS = (dict(), dict(in_place=1), dict(stage=1), dict(stage=1, in_place=1), dict(beyond=1))
_WAY_IDS = ("split-resident", "inplace-resident", "split-staged", "inplace-staged", "split-beyond")
_BIT_SHAPES = (
    # fp16, grid, caller's boards, cin, binary, perm, n0, ns
    (True, 19, (9, 19, 2, 13, 3, 19, 7, 5, 16, 11, 18, 4), 43, 37, "sorted", 0, None),
    (False, 19, (6, 8, 10, 12, 14, 15, 17, 19, 2, 3, 19, 13), 38, 34, _SHUFFLE12, 3, 7),
    (True, 13, (13, 4, 9, 2, 13, 3, 10, 6), 43, 37, _SHUFFLE8, 0, None),
    (False, 9, (9, 2, 3, 7, 9, 4, 6, 8), 43, 37, "sorted", 2, 5),
    (True, 19, (19, 2, 3, 17, 12), 48, 40, _SHUFFLE5, 0, None),    # the record limit itself: 40 bit planes, 8 scalars
)
PACK_BIT_CASES = [_pack_case(f"bits-{'f16' if s[0] else 'f32'}-g{s[1]}-c{s[3]}-{wid}", s[0], "bits", s[1], s[2], s[3], s[4], perm=s[5], n0=s[6], ns=s[7], **way)
                  for s, way, wid in zip(_BIT_SHAPES, _WAYS, _WAY_IDS)]
PACK_BIT_CASES.append(_pack_case("bits-f16-g19-c6", True, "bits", 19, (19, 2, 5, 3), 6, 2, perm=None))


def _symm_case(k, big, small):
    """all eight symmetries of one record of each of two board sizes, as sixteen shuffled device samples"""
    fp16, cin, binary = ((True, 43, 37), (False, 38, 34), (False, 43, 37))[k % 3]
    rng = np.random.default_rng([911, big, small])
    slots = [(r, s) for r in (0, 1) for s in range(8)]
    slots = [slots[j] for j in rng.permutation(16)]
    src, symm = tuple(r for r, _ in slots), tuple(s for _, s in slots)
    cbsz = tuple((big, small)[r] for r in src)
    perm = "sorted" if k % 2 == 0 else tuple(int(v) for v in rng.permutation(16))
    way = _WAYS[k % 5]
    return _pack_case(f"symm-{'f16' if fp16 else 'f32'}-b{big}+{small}-{_WAY_IDS[k % 5]}", fp16, "symm", 19, cbsz, cin, binary, perm=perm, src=src, symm=symm,
                      nrec=2, **way)


PACK_SYMM_CASES = [_symm_case(k, 19 - k, 2 + k) for k in range(9)]   # (19, 2), (18, 3) ... (11, 10): every size once
# the map and a window: three records, device samples that skip one of them, a launch over the middle samples only
PACK_SYMM_CASES.append(_pack_case("symm-f16-g13-three-records-mid", True, "symm", 13, (13, 7, 13, 7, 7, 13, 13, 7), 43, 37, perm=_SHUFFLE8, n0=2, ns=5,
                                  src=(2, 0, 2, 0, 0, 2, 2, 0), symm=(5, 3, 0, 6, 1, 7, 2, 4), nrec=3, stage=1))
PACK_CASES = PACK_PLANE_CASES + PACK_BIT_CASES + PACK_SYMM_CASES
PACK_IDS = [c.name for c in PACK_CASES]
# the plane cases whose planes can also travel as records (cin - binary scalars): both routes must leave one image
PACK_BOTH_ROUTES = [(c, b) for c, b in ((PACK_PLANE_CASES[0], 37), (PACK_PLANE_CASES[1], 34), (PACK_PLANE_CASES[6], 37), (PACK_PLANE_CASES[9], 37),
                                        (PACK_PLANE_CASES[10], 34))]

F16_OFF_BOARD = np.uint16(0x7BFF)   # 65504: the fp16 normal the off-board cells of a placement draw hold, and nothing else
F32_OFF_BOARD = np.float32(-3.0e7)
# a tie between two fp16 neighbours, just above and below one, a quarter and three quarters of the way, one fp32 ulp above the
# lower neighbour and one below the upper: the low 13 bits of the fp32 mantissa
ROUNDING_TAILS = np.array([0x1000, 0x1001, 0x0FFF, 0x0800, 0x1800, 0x0001, 0x1FFF], np.uint32)


def _f16_normals(rng, count):
    """`count` fp16 normals (0x0400..0x7BFE and their negatives: all but the off-board value) as float32, each as rarely as possible"""
    pool = np.concatenate([np.arange(0x0400, 0x7BFF, dtype=np.uint16), np.arange(0x8400, 0xFBFF, dtype=np.uint16)])
    picks = np.concatenate([rng.permutation(pool) for _ in range(-(-count // len(pool)))])[:count]
    return picks.view(np.float16).astype(np.float32)


def _rounding_values(rng, count):
    """fp32 values that are no fp16 values, inside the fp16 normal range: a random fp16 normal below 65504 as the lower neighbour
    (either parity) plus one of ROUNDING_TAILS; the first entries sit at the two ends of the range"""
    h = rng.integers(0x0400, 0x7BFF, count).astype(np.uint16)
    tails = ROUNDING_TAILS[rng.integers(0, len(ROUNDING_TAILS), count)]
    ends = [(0x0400, 0x1000), (0x0401, 0x1000), (0x0400, 0x0001), (0x7BFE, 0x1000), (0x7BFD, 0x1000), (0x7BFE, 0x1FFF), (0x7BFF, 0x0FFF)]
    for k, (hh, tt) in enumerate(ends[:count]):
        h[k], tails[k] = hh, tt
    bits = h.view(np.float16).astype(np.float32).view(np.uint32) | tails
    sign = rng.integers(0, 2, count).astype(np.uint32)
    sign[:len(ends)] = 0   # (-65504 is the image's sentinel)
    bits |= sign << np.uint32(31)
    return bits.view(np.float32)


def _record(rng, binary, bs, scalars, beyond):
    rec = np.zeros(binary * 12 + 8, np.uint32)
    on = rng.integers(0, 2, (binary, bs * bs))
    bits = rec[:binary * 12].reshape(binary, 12)
    for c in range(binary):
        cells = np.flatnonzero(on[c])
        np.bitwise_or.at(bits[c], cells >> 5, np.uint32(1) << (cells & 31).astype(np.uint32))
    if beyond:   # every bit at or beyond the board's last cell, up to the end of the twelfth word
        cells = np.arange(bs * bs, 12 * 32)
        for c in range(binary):
            np.bitwise_or.at(bits[c], cells >> 5, np.uint32(1) << (cells & 31).astype(np.uint32))
    rec[binary * 12:] = np.asarray(scalars, np.float32).view(np.uint32)
    return rec


class PackDraw:
    """The inputs of one case on one draw ("placement" | "rounding"): planes [n][cin][board^2] on the NN grid, or records
    [nrec][binary*12 + 8] (record r of a symmetry case has the board of the slots that name it)."""

    def __init__(self, c, draw):
        rng = np.random.default_rng([5150, PACK_CASES.index(c), int(draw == "rounding")])
        n, B = len(c.cbsz), c.board
        self.planes = self.records = None
        if c.form == "planes":
            self.planes = np.empty((n, c.cin, B, B), np.float32)
            self.planes[:] = F16_OFF_BOARD.view(np.float16).astype(np.float32) if c.fp16 or draw == "rounding" else F32_OFF_BOARD
            for j, bs in enumerate(c.cbsz):
                count = c.cin * bs * bs
                if draw == "rounding":
                    v = _rounding_values(rng, count)
                elif c.fp16:
                    v = _f16_normals(rng, count)
                else:   # distinct fp32 values that are mostly no fp16 values: k / 256, k = 1 .. count in a shuffled order, signs mixed
                    v = ((rng.permutation(count) + 1) / 256.0 * rng.choice((-1.0, 1.0), count)).astype(np.float32)
                self.planes[j, :, :bs, :bs] = v.reshape(c.cin, bs, bs)
            self.planes = self.planes.reshape(n, c.cin, B * B)
            return
        sizes = list(c.cbsz) if c.form == "bits" else [c.cbsz[c.src.index(r)] if r in c.src else 2 for r in range(c.nrec)]
        recs = []
        for bs in sizes:   # eight distinct scalars per record, the slots past cin - binary included
            scal = _rounding_values(rng, 8) if draw == "rounding" else (_f16_normals(rng, 8) if c.fp16 else ((rng.permutation(8) + 1) / 256.0 * (1 + rng.integers(0, 999))).astype(np.float32))
            recs.append(_record(rng, c.binary, bs, scal, c.beyond))
        self.records = np.stack(recs)


@functools.lru_cache(maxsize=None)
def pack_draw(c, draw):
    return PackDraw(c, draw)


def pack_reference(c, draw, sentinel, **kw):
    """pack_image_ref of the case on the draw (kw: a defect, or other inputs in place of the draw's)"""
    from _kref import pack_image_ref
    D = pack_draw(c, draw)
    perm, bsz = pack_order(c)
    args = dict(planes=D.planes, records=D.records, binary=c.binary, src=c.src, symm=c.symm, perm=None if c.perm is None else perm, n0=c.n0, ns=c.ns,
                guard_rows=PACK_GUARD_ROWS, split=c.split)
    args.update(kw)
    return pack_image_ref(c.fp16, bsz, c.board, c.cin, sentinel, **args)


def planes_of_records(records, binary, cbsz, cin, board):
    """the NN-grid planes [n][cin][board^2] that record j of board cbsz[j] stands for (off-board cells 0)"""
    from _kref import record_bits
    out = np.zeros((len(cbsz), cin, board, board), np.float32)
    for j, bs in enumerate(cbsz):
        out[j, :binary, :bs, :bs] = record_bits(records[j], binary, np.arange(bs * bs)).reshape(binary, bs, bs)
        out[j, binary:, :bs, :bs] = records[j][binary * 12:binary * 12 + cin - binary].view(np.float32)[:, None, None]
    return out.reshape(len(cbsz), cin, board * board)


# ====================================================================================================================
# The activation sweep (test_gpu_act_sweep.py, test_act_sweep_reference_cpu.py): an identity convolution -- a channel permutation in
# the centre tap, bias 0 -- delivers any chosen value exactly to an epilogue, so one layer puts every finite fp16 value through it.
SWEEP_SEED = 1905
F16_FINITE = np.concatenate([np.arange(0x0000, 0x7C00, dtype=np.uint16), np.arange(0x8000, 0xFC00, dtype=np.uint16)])   # 63 488 patterns
# every activation's edges: 0, HardSwish's +-3, Mish's guard at 20, +-11.09 where fp16 exp overflows, the ends of the range
SWEEP_EDGES = (0.0, -0.0, 3.0, -3.0, 20.0, 11.09, -11.09, 65504.0, -65504.0)
# fp32 engine: points next to the edges that are no fp16 values, and +-87.3 / +-88.8 / +-104 where fp32 exp under- and overflows
F32_POINTS = np.array([np.nextafter(np.float32(v), np.float32(d)) for v in (0.0, 3.0, -3.0, 20.0) for d in (-np.inf, np.inf)] +
                      [87.3, -87.3, 88.8, -88.8, 104.0, -104.0], np.float32)
SWEEP_MODES = ("none", "sweep", "small")   # no residual; another permutation of the same sweep; a small residual (|z| < 32 off the grid)


def sweep_edge_bits():
    """the fp16 patterns of SWEEP_EDGES and of their fp16 neighbours on both sides (where finite)"""
    b = np.array(SWEEP_EDGES, np.float16).view(np.uint16).astype(np.int64)
    bits = np.concatenate([b, b + 1, b - 1])
    bits = bits[((bits & 0x7FFF) < 0x7C00) & (bits >= 0)]
    return np.unique(bits.astype(np.uint16))


@functools.lru_cache(maxsize=None)
def sweep_values(n, seed, normals_only=False, f32_points=False):
    """n >= 63 488 (+ the fp32 points) pre-activations as float32: every finite fp16 value once (normals_only: the 61 442 zeros
    and normals), the fp32 points once where asked, the remaining slots repeats of the edges and their neighbours, shuffled with
    a fixed seed.  Read-only."""
    pool = F16_FINITE
    if normals_only:
        pool = pool[((pool & 0x7FFF) >= 0x0400) | ((pool & 0x7FFF) == 0)]
    vals = pool.view(np.float16).astype(np.float32)
    if f32_points:
        vals = np.concatenate([vals, F32_POINTS])
    assert n >= len(vals), (n, len(vals))
    edges = sweep_edge_bits()
    if normals_only:
        edges = edges[((edges & 0x7FFF) >= 0x0400) | ((edges & 0x7FFF) == 0)]
    edges = edges.view(np.float16).astype(np.float32)
    fill = np.resize(np.concatenate([edges, F32_POINTS]) if f32_points else edges, n - len(vals))
    out = np.concatenate([vals, fill])
    out = out[np.random.default_rng([SWEEP_SEED, seed, n]).permutation(n)]
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def sweep_small(n, seed):
    """n fp16 values spread over (-16, 16), as float32: the small residual"""
    out = np.random.default_rng([SWEEP_SEED, seed, n, 3]).uniform(-16.0, 16.0, n).astype(np.float16).astype(np.float32)
    out.setflags(write=False)
    return out


def sweep_planes(v, bsz, C):
    """a flat draw cut into per-sample [C][b*b] planes (views)"""
    outs, off = [], 0
    for b in bsz:
        outs.append(v[off:off + C * b * b].reshape(C, b * b))
        off += C * b * b
    assert off == len(v)
    return outs


def sweep_inputs(bsz, C, mode, seed=0, normals_only=False, f32_points=False):
    """(xs, res | None) of one sweep case over the boards bsz with C channels; mode one of SWEEP_MODES"""
    n = C * sum(b * b for b in bsz)
    xs = sweep_planes(sweep_values(n, seed, normals_only, f32_points), bsz, C)
    if mode == "none":
        return xs, None
    return xs, sweep_planes(sweep_values(n, seed + 1000, normals_only, f32_points) if mode == "sweep" else sweep_small(n, seed), bsz, C)


@functools.lru_cache(maxsize=None)
def sweep_perm(C, seed, identity=False):
    """the channel permutation pi of a case (identity: a depthwise tap has no other)"""
    return np.arange(C) if identity else np.random.default_rng([SWEEP_SEED, seed, C, 7]).permutation(C)


def perm_weights(pi, k, depthwise=False):
    """w[c][pi(c)][centre] = 1, everything else 0 (depthwise: w[c][0][centre] = 1) -> [C][C | 1][k][k] float32"""
    C = len(pi)
    w = np.zeros((C, 1 if depthwise else C, k, k), np.float32)
    w[np.arange(C), 0 if depthwise else pi, k // 2, k // 2] = 1.0
    return w
