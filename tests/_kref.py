"""The numpy references of the kernel parity tests, each once: float64 restatements of what the CPU oracle computes (the
activations, the direct convolution, the SE unit, the head tail), the exact-arithmetic reference of test_gpu_exact.py and the
reference, bound and predicate of the activation sweep (test_gpu_act_sweep.py).  No
GPU, no device library: the test_*_reference_cpu.py modules pin these functions to the oracle and to each other.

conv_ref is the general layer (any k, depthwise, residual in front of or behind the activation) written as the oracle writes
it; conv3x3_f64 is the cheap 3x3 convolution of one sample as nine matrix products, pinned to conv_ref by
test_tower_run_reference_cpu.py.  The two stay independent implementations."""
import numpy as np


def r16(a, fp16):
    return a.astype(np.float16).astype(np.float32) if fp16 else a


def act_np(x, act):
    """The eight activations of the reference (src/neural/activation.h:36-81), float64."""
    if act == 0:
        return x
    if act == 1:
        return np.maximum(x, 0)
    if act == 2:  # ELU
        return np.where(x > 0, x, np.expm1(np.minimum(x, 0)))
    if act == 3:  # SELU
        return np.where(x > 0, 1.05070098 * x, 1.05070098 * 1.67326324 * np.expm1(np.minimum(x, 0)))
    if act == 4:  # GELU, tanh form
        return 0.5 * x * (1 + np.tanh(0.7978845608028654 * (x + 0.044715 * x ** 3)))
    if act == 5:
        return x * np.tanh(np.log1p(np.exp(x)))
    if act == 6:
        return x / (1 + np.exp(-x))
    if act == 7:  # HardSwish
        return np.where(x >= 3, x, np.where(x <= -3, 0.0, x * (x + 3) / 6))
    raise ValueError(act)


def conv_ref(xs, bsz, w, bias, res, k, depthwise, act, post):
    """xs: list of [C][bs*bs] arrays; returns list of [K][bs*bs] float64."""
    outs = []
    pad = k // 2
    for i, (x, bs) in enumerate(zip(xs, bsz)):
        C = x.shape[0]
        img = np.zeros((C, bs + 2 * pad, bs + 2 * pad))
        img[:, pad:pad + bs, pad:pad + bs] = x.reshape(C, bs, bs)
        K = w.shape[0]
        y = np.zeros((K, bs, bs))
        for kr in range(k):
            for kc in range(k):
                patch = img[:, kr:kr + bs, kc:kc + bs]
                if depthwise:
                    y += patch * w[:, 0, kr, kc][:, None, None]
                else:
                    y += np.einsum("kc,cyx->kyx", w[:, :, kr, kc].astype(np.float64), patch)
        y = y.reshape(K, bs * bs)
        if bias is not None:
            y = y + bias[:, None]
        if post:
            y = act_np(y, act)
            if res is not None:
                y = y + res[i]
        else:
            if res is not None:
                y = y + res[i]
            y = act_np(y, act)
        outs.append(y)
    return outs


def conv3x3_f64(x, w, bias, b):
    """float64 direct 3x3 convolution of one sample as nine matrix products: x [C][b*b], w [K][C][3][3] -> [K][b*b]"""
    w64 = np.asarray(w, np.float64)
    C, K = x.shape[0], w64.shape[0]
    xp = np.zeros((C, b + 2, b + 2), np.float64)
    xp[:, 1:-1, 1:-1] = np.asarray(x, np.float64).reshape(C, b, b)
    y = np.zeros((K, b * b), np.float64)
    for dy in range(3):
        for dx in range(3):
            y += np.matmul(np.ascontiguousarray(w64[:, :, dy, dx]), np.ascontiguousarray(xp[:, dy:dy + b, dx:dx + b]).reshape(C, b * b))
    return y + np.asarray(bias, np.float64)[:, None]


def se_pool_f64(x, bs):
    """GlobalPooling<false> (se_unit.cc:9-40) of x [C][bs*bs] in float64: (mean, mean * (bs - 14) / 10, max) -> [3C]"""
    x = np.asarray(x, np.float64)
    mean = x.sum(axis=1) / float(bs * bs)
    return np.concatenate([mean, mean * ((bs - 14.0) / 10.0), x.max(axis=1)])


def se_gate_f64(pool, w1, b1, w2, b2, act):
    """squeeze FC with `act`, excite FC: pooled [3C] -> (sigmoid(gamma) [C], beta [C]), float64"""
    mid = act_np(np.asarray(w1, np.float64) @ pool + np.asarray(b1, np.float64), act)
    exc = np.asarray(w2, np.float64) @ mid + np.asarray(b2, np.float64)
    C = exc.shape[0] // 2
    return 1.0 / (1.0 + np.exp(-exc[:C])), exc[C:]


def se_apply_f64(x, res, gamma, beta, act):
    v = gamma[:, None] * np.asarray(x, np.float64) + beta[:, None]
    if res is not None:
        v = v + np.asarray(res, np.float64)
    return act_np(v, act)


def se_unit_f64(x, res, w1, b1, w2, b2, bs, act):
    """SEUnit::Forward (se_unit.cc:70-128) on x [C][bs*bs] in float64 throughout: pool = (mean, mean * (bs-14)/10, max),
    squeeze FC with `act`, excite FC, act(sigmoid(gamma) * x + beta + res).  w1 [se][3C], w2 [2C][se]; res or None."""
    gamma, beta = se_gate_f64(se_pool_f64(x, bs), w1, b1, w2, b2, act)
    return se_apply_f64(x, res, gamma, beta, act)


# ---- the heads: float64 restatement of so_tap_head_tail (oracle/sayuri_oracle.c; reference blas_forward_pipe.cc:496-580), in
# pieces a test can replace.  weights12 as the head taps of include/sayuri_hip.h take them.
def head_pool_f64(x, bs, value_head):
    """GlobalPooling<false/true> (se_unit.cc:9-68) of x [C][bs*bs]: (mean, mean * (bs-14)/10, max | mean * ((bs-14)^2/100 - 0.1))"""
    x = np.asarray(x, np.float64)
    mean = x.sum(axis=1) / float(bs * bs)
    d = bs - 14.0
    return np.concatenate([mean, mean * (d / 10.0), mean * (d * d / 100.0 - 0.1) if value_head else x.max(axis=1)])


def head_inter_f64(pool, w, b, act):
    return act_np(np.asarray(w, np.float64) @ pool + np.asarray(b, np.float64), act)


def head_pixel_f64(planes, w, b):
    """a 1x1 convolution with bias over planes [C][S]: w [K][C] -> [K][S]"""
    return np.asarray(w, np.float64) @ planes + np.asarray(b, np.float64)[:, None]


def head_tail_f64(pc, vc, ws, bs, act, ppool=None, vpool=None, spatial_bias=True):
    """-> (prob [prob_ch][S], pass, own [S], misc) from the activated head planes pc [Cp][S], vc [Cv][S].  ppool / vpool: a
    pooled vector to use in place of the sample's own; spatial_bias=False leaves p_inter's output off the policy planes."""
    p_inter_w, p_inter_b, pass_w, pass_b, v_inter_w, v_inter_b, v_misc_w, v_misc_b, prob_w, prob_b, own_w, own_b = ws
    pc, vc = np.asarray(pc, np.float64), np.asarray(vc, np.float64)
    pinter = head_inter_f64(head_pool_f64(pc, bs, False) if ppool is None else ppool, p_inter_w, p_inter_b, act)
    prob = head_pixel_f64(pc + pinter[:, None] if spatial_bias else pc, prob_w, prob_b)
    pas = head_inter_f64(pinter, pass_w, pass_b, 0)
    vinter = head_inter_f64(head_pool_f64(vc, bs, True) if vpool is None else vpool, v_inter_w, v_inter_b, act)
    own = head_pixel_f64(vc, np.asarray(own_w, np.float64).reshape(1, -1), own_b)[0]
    misc = head_inter_f64(vinter, v_misc_w, v_misc_b, 0)
    return prob, pas, own, misc


def head_ratio(a, b, ref, tol):
    """largest |a - b| over the four outputs, each in units of its own tolerance tol * max(1, |ref|max)"""
    return max(float(np.abs(np.asarray(x) - y).max()) / (tol * max(1.0, float(np.abs(r).max()))) for x, y, r in zip(a, b, ref))


# ---- exact arithmetic (test_gpu_exact.py states the principle)
def quantum_bits(*arrays):
    """the smallest q with every value of `arrays` a multiple of 2^-q (0: integers)"""
    for q in range(25):
        if all(a is None or np.array_equal(np.rint(np.asarray(a, np.float64) * 2.0 ** q), np.asarray(a, np.float64) * 2.0 ** q) for a in arrays):
            return q
    raise AssertionError("an operand is no multiple of 2^-24")


def exact_conv(x, w, bs, k, depthwise):
    """The k x k convolution of one sample as k*k matrix products in float64, which holds these sums exactly: x [C][bs*bs], w
    [K][C | 1][k][k] -> (sum w x, sum |w x|), each [K][bs*bs]"""
    x, w64 = np.asarray(x, np.float64), np.asarray(w, np.float64)
    C, K, pad = x.shape[0], w64.shape[0], k // 2
    xp = np.zeros((C, bs + 2 * pad, bs + 2 * pad), np.float64)
    xp[:, pad:pad + bs, pad:pad + bs] = x.reshape(C, bs, bs)
    wa = np.abs(w64)
    S, A = np.zeros((K, bs * bs), np.float64), np.zeros((K, bs * bs), np.float64)
    for dy in range(k):
        for dx in range(k):
            patch = np.ascontiguousarray(xp[:, dy:dy + bs, dx:dx + bs]).reshape(C, bs * bs)
            if depthwise:
                S += w64[:, 0, dy, dx][:, None] * patch
                A += wa[:, 0, dy, dx][:, None] * np.abs(patch)
            else:
                S += np.matmul(np.ascontiguousarray(w64[:, :, dy, dx]), patch)
                A += np.matmul(np.ascontiguousarray(wa[:, :, dy, dx]), np.abs(patch))
    return S, A


def exact_layer(x, w, bias, res, bs, k, depthwise, act, post=False, beta=None, store=np.float16, conv=None):
    """The one correct output of a layer on operands of the exact regime: x [C][bs*bs], w, bias [K] or None, res [K][bs*bs] or None
    -> float16(act(conv + bias + beta + res)) as float32, [K][bs*bs]; post: act(conv + bias) + res (the depthwise kernel's order);
    beta: a second per-channel addend (an SE unit's); store=np.float32: the fp32 kernels' store; store=None: the exact value
    before the store, float64; conv: exact_conv(x, w, bs, k, depthwise) where the caller has it already.  Asserts the regime: act
    is the identity or ReLU, w / bias / beta are integers, A * 2^q < 2^24, |S| < 65504."""
    assert act in (0, 1), "only the identity and ReLU are exact functions"
    assert quantum_bits(w, bias, beta) == 0, "weights and biases are integers"
    q = quantum_bits(x, res)
    S, A = exact_conv(x, w, bs, k, depthwise) if conv is None else conv
    for addend in (bias, beta):
        if addend is not None:
            S = S + np.asarray(addend, np.float64)[:, None]
            A = A + np.abs(np.asarray(addend, np.float64))[:, None]
    r = np.asarray(res, np.float64) if res is not None else 0.0
    A = A + np.abs(r)
    assert float(A.max()) * 2.0 ** q < 2.0 ** 24, ("outside the exact regime: sum |w x| + |bias| + |res| =", float(A.max()), "in units of 2^-%d" % q)
    v = act_np(S, act) + r if post else act_np(S + r, act)
    assert max(float(np.abs(S + r).max()), float(np.abs(v).max())) < 65504.0, "an output leaves the fp16 range"
    return v if store is None else v.astype(store).astype(np.float32)


def exact_diff(got, exp):
    """the predicate of assert_exact: [(sample, channel, pixel, got, exp)] of every value that differs (== on values: -0 equals +0)"""
    bad = []
    for i, (g, e) in enumerate(zip(got, exp)):
        for c, p in zip(*np.nonzero(np.asarray(g) != np.asarray(e))):
            bad.append((i, int(c), int(p), float(g[c, p]), float(e[c, p])))
    return bad


def assert_exact(got, exp, what):
    """every sample's output finite and equal to the reference, value for value"""
    assert len(got) == len(exp), what
    for i, g in enumerate(got):
        assert g.shape == exp[i].shape and np.isfinite(g).all(), (what, "sample", i, "an output nobody wrote, or a non-finite one")
    bad = exact_diff(got, exp)
    assert not bad, (what, len(bad), "values differ; the first (sample, channel, pixel, got, exp):", bad[:8])


def mutated(w, k, c, kr, kc):
    """w with the one entry changed by 1 (still a small integer)"""
    w2 = w.copy()
    w2[k, c, kr, kc] += 1.0
    return w2


def predicted_change(xs, bsz, cout, k, c, kr, kc):
    """what adding 1 to w[k][c][kr][kc] adds to every sample's 3x3 convolution: channel k only, the input channel c shifted by the tap"""
    out = []
    for x, b in zip(xs, bsz):
        xp = np.zeros((b + 2, b + 2), np.float64)
        xp[1:-1, 1:-1] = np.asarray(x[c], np.float64).reshape(b, b)
        d = np.zeros((cout, b * b), np.float64)
        d[k] = xp[kr:kr + b, kc:kc + b].ravel()
        out.append(d)
    return out


def assert_localised(got, exp, delta, what):
    """the real kernel on the changed weight against the UNCHANGED reference: it differs exactly where, and by what, the integer
    arithmetic says"""
    n_pred = sum(int(np.count_nonzero(d)) for d in delta)
    assert n_pred > 0, (what, "the changed weight meets no non-zero input")
    for i, (g, e, d) in enumerate(zip(got, exp, delta)):
        assert np.isfinite(g).all(), (what, "sample", i)
        wrong = np.nonzero((g != e) != (d != 0))
        assert wrong[0].size == 0, (what, "sample", i, wrong[0].size, "outputs differ where none was predicted, or do not where one was; the first (channel, pixel):",
                                    list(zip(*wrong))[:8])
        assert np.array_equal(g.astype(np.float64) - e, d), (what, "sample", i, "an output moved by another amount than the input under the tap")
    return n_pred


# ---- the input stage (test_gpu_input.py): planes or packed records -> the input convolution's NHWC image
PACK_DEFECTS = ("swap_xy", "sample_stride_on_grid", "grid_stride_on_sample", "lost_last_cell", "perm_backwards", "map_ignored", "symm_bit_1",
                "symm_bit_2", "symm_bit_4", "pad_nonzero", "scalar_neighbour", "round_toward_zero")


def f16_toward_zero(a):
    """float32 -> the fp16 value next to it toward zero, as float32 (the defect "round_toward_zero"; normal range only)"""
    a = np.asarray(a, np.float32)
    return (a.view(np.uint32) & np.uint32(0xFFFFE000)).view(np.float32)


def record_bits(rec, binary, cells):
    """bit `cells[...]` of every bit plane of a packed record (uint32 [binary*12 + 8]) -> float32 [binary][len(cells)]; a cell past
    the twelve words reads 0"""
    bits = np.asarray(rec, np.uint32)[:binary * 12].reshape(binary, 12)
    cells = np.asarray(cells)
    inside = cells < 12 * 32
    c = np.where(inside, cells, 0)
    return (((bits[:, c >> 5] >> (c & 31).astype(np.uint32)) & 1) * inside).astype(np.float32)


def pack_image_ref(fp16, bsz, max_board, cin, sentinel, planes=None, records=None, binary=0, src=None, symm=None, perm=None, n0=0, ns=None,
                   guard_rows=0, split=1, defect=None):
    """What an input-stage kernel leaves in a sentinel-filled image: float32 [n * max_board^2 + guard_rows][cs], cs = cin rounded
    up to 32.  bsz [n]: the board of DEVICE sample i, which shows the caller's slot j = perm[i] (None: i).  Row p = y*bs + x of
    slot i, channel c < cin:
        planes [n][cin][max_board^2] (the NN grid)   planes[j][c][y*max_board + x]
        records [.][binary*12 + 8]                   c < binary: bit p of plane c of record j (with symm: record src[j], bit
                                                     symm_index(bs, symm[j])[p]); else the record's scalar c - binary
    rounded to fp16 (nearest even) for the fp16 engine; channels [cin, cs) are +0; rows >= bs*bs, the slots outside [n0, n0 + ns)
    and the guard keep the sentinel.  defect: one of PACK_DEFECTS, the image a kernel with that mistake would leave (split: the
    workgroups per sample, for "lost_last_cell")."""
    assert defect is None or defect in PACK_DEFECTS, defect
    n, B2, cs = len(bsz), max_board * max_board, (cin + 31) // 32 * 32
    ns = n - n0 if ns is None else ns
    img = np.full((n * B2 + guard_rows, cs), sentinel, np.float32)
    perm = np.arange(n) if perm is None else np.asarray(perm)
    if defect == "perm_backwards":
        perm = np.argsort(perm)
    if symm is not None:
        from _ensemble import symm_index
    for i in range(n0, n0 + ns):
        bs, j = int(bsz[i]), int(perm[i])
        y, x = np.divmod(np.arange(bs * bs), bs)
        if defect == "swap_xy":
            y, x = x, y
        rows = np.zeros((bs * bs, cs), np.float32)
        if planes is not None:
            cells = y * (bs if defect == "sample_stride_on_grid" else max_board) + x
            rows[:, :cin] = np.asarray(planes[j], np.float32).reshape(cin, B2)[:, cells].T
        else:
            r, cells = j, y * bs + x
            if symm is not None:
                r = j if src is None or defect == "map_ignored" else int(src[j])
                s = int(symm[j])
                if defect and defect.startswith("symm_bit_"):
                    s &= ~int(defect[-1])
                cells = symm_index(bs, s)[cells]
            if defect == "grid_stride_on_sample":
                ty, tx = np.divmod(cells, bs)
                cells = ty * max_board + tx
            rec = np.asarray(records[r % len(records)], np.uint32)
            rows[:, :binary] = record_bits(rec, binary, cells).T
            scal = rec[binary * 12:binary * 12 + 8].view(np.float32)
            for c in range(binary, cin):
                rows[:, c] = scal[min(7, c - binary + 1) if defect == "scalar_neighbour" else c - binary]
        if fp16:
            rows[:, :cin] = f16_toward_zero(rows[:, :cin]) if defect == "round_toward_zero" else rows[:, :cin].astype(np.float16).astype(np.float32)
        if defect == "pad_nonzero" and cin < cs:
            rows[:, cin] = 1.0
        if defect == "lost_last_cell":
            per = (bs * bs + split - 1) // split
            for part in range(split):
                pend = min(bs * bs, (part + 1) * per)
                if pend > part * per:
                    rows[pend - 1] = sentinel
        img[i * B2:i * B2 + bs * bs] = rows
    return img


# ---- the activation sweep (test_gpu_act_sweep.py states the principle; test_act_sweep_reference_cpu.py pins what follows)
ACT_NAMES = ("identity", "relu", "elu", "selu", "gelu", "mish", "swish", "hardswish")
ACT_K = 8.0          # fp32 evaluation: K * 2^-24 * max(1, |z|, |ref|); derived in the GPU module's docstring, never from a GPU run
F16_OVERFLOW = 65520.0   # the tie between 65504 and the next binade: an fp16 store gives inf from here on
SELU_SCALE, SELU_ALPHA = 1.05070098, 1.67326324


def act_f64(z, act):
    """The eight activations in float64, in forms that stay finite and accurate over |z| <= 1.4e5 (act_np's Mish and Swish
    overflow exp past 709 and lose the tails)."""
    z = np.asarray(z, np.float64)
    neg = np.minimum(z, 0.0)
    if act == 0:
        return z
    if act == 1:
        return np.maximum(z, 0.0)
    if act == 2:
        return np.where(z > 0, z, np.expm1(neg))
    if act == 3:
        return np.where(z > 0, SELU_SCALE * z, SELU_SCALE * SELU_ALPHA * np.expm1(neg))
    if act == 4:   # tanh form; tanh saturates to +-1 without overflow
        return 0.5 * z * (1.0 + np.tanh(0.7978845608028654 * (z + 0.044715 * z * z * z)))
    if act == 5:   # z * tanh(softplus(z)); softplus(z) = z past 30 (log1p(exp(-30)) = 9e-14 of 30), log1p(exp(z)) below
        return z * np.tanh(np.where(z > 30.0, z, np.log1p(np.exp(np.minimum(z, 30.0)))))
    if act == 6:   # two-sided: z / (1 + e^-z) for z >= 0, z e^z / (1 + e^z) below
        e = np.exp(-np.abs(z))
        return np.where(z >= 0, z / (1.0 + e), z * e / (1.0 + e))
    if act == 7:
        return np.where(z >= 3, z, np.where(z <= -3, 0.0, z * (z + 3.0) / 6.0))
    raise ValueError(act)


def ulp16(v):
    """the spacing of fp16 at v: 2^(e - 10) with e the exponent of |v| held to [-14, 15] -- 2^-24 below 2^-14, 32 from 32768 on"""
    a = np.abs(np.asarray(v, np.float64))
    _, ex = np.frexp(a)
    return np.ldexp(1.0, np.clip(np.where(a == 0, -14, ex - 1), -14, 15) - 10)


def act_bound(ref, z, store16=True, K=ACT_K):
    """|got - ref| <= ulp16(ref) / 2 (the one round-to-nearest fp16 store; dropped for an fp32 store) + K 2^-24 max(1, |z|, |ref|)"""
    ref, z = np.asarray(ref, np.float64), np.asarray(z, np.float64)
    b = K * 2.0 ** -24 * np.maximum(1.0, np.maximum(np.abs(z), np.abs(ref)))
    return b + 0.5 * ulp16(ref) if store16 else b


def act_sweep_bad(got, z, act, store16=True, post_res=None, K=ACT_K):
    """The predicate of the activation sweep on flat arrays.  z: the exact float64 argument of the activation (x + res);
    post_res: a residual added BEHIND the activation (the depthwise order), so ref = act(z) + post_res.
    identity / ReLU: got == store(ref) value for value (-0 equals +0, inf equals inf where store(ref) overflows, NaN nothing).
    the other six: no NaN; finite got within act_bound of ref; +-inf (of ref's sign) only if |ref| + bound >= 65520, and
    required if |ref| - bound >= 65520 (fp16 store; an fp32 store never overflows on these data).
    -> (bad mask, |got - ref| / bound where both are finite, else 0)"""
    got, z = np.asarray(got, np.float64).ravel(), np.asarray(z, np.float64).ravel()
    ref = act_f64(z, act)
    if post_res is not None:
        ref = ref + np.asarray(post_res, np.float64).ravel()
    assert got.shape == ref.shape and np.isfinite(ref).all()
    if act in (0, 1):
        with np.errstate(over="ignore"):
            exp = ref.astype(np.float16 if store16 else np.float32).astype(np.float64)
        return got != exp, np.zeros(got.shape)
    bound = act_bound(ref, z, store16, K)
    lim = F16_OVERFLOW if store16 else np.inf
    fin = np.isfinite(got)
    with np.errstate(invalid="ignore"):
        err = np.where(fin, np.abs(got - ref), 0.0)
    bad = np.isnan(got)
    bad |= np.isinf(got) & ((np.abs(ref) + bound < lim) | (np.sign(got) != np.sign(ref)))
    bad |= fin & (np.abs(ref) - bound >= lim)
    bad |= fin & (err > bound)
    return bad, err / bound


def act_units_used(got, z, act, store16=True, post_res=None):
    """how much of K the finite outputs use: the largest (|got - ref| - the store's half ulp) / (2^-24 max(1, |z|, |ref|)); a record, no
    input to the bound"""
    got, z = np.asarray(got, np.float64).ravel(), np.asarray(z, np.float64).ravel()
    ref = act_f64(z, act) + (0.0 if post_res is None else np.asarray(post_res, np.float64).ravel())
    fin = np.isfinite(got)
    with np.errstate(invalid="ignore"):
        over = np.where(fin, np.abs(got - ref), 0.0) - (0.5 * ulp16(ref) if store16 else 0.0)
    return float(np.max(np.where(fin, over, 0.0) / act_bound(ref, z, False, 1.0), initial=0.0))


ACT_DEFECTS = ("hswish_edge_2.5", "hswish_times_0.1667", "selu_alpha_1.67", "selu_scale_1.0507", "gelu_coef_0.0455", "gelu_erf",
               "mish_guard_2", "swish_no_log2e", "elu_no_log2e")


def act_f32_emu(x, act, defect=None):
    """common.h's activate() restated in numpy float32, operation for operation (fast_exp = exp2(x * log2e), __expf = numpy's
    float32 exp -- its error is the larger of the two ways to state it: exp2(x * log2e) gives ELU 1.21 and SELU 2.62 in the K
    table --, rcp = 1 / t, fma through float64); numpy's exp2 and division are correctly rounded where v_exp_f32 / v_rcp_f32 are
    good to 1 ulp.
    defect: one of ACT_DEFECTS, the value a kernel with that mistake would form.  -> float32, before the store"""
    assert defect is None or defect in ACT_DEFECTS, defect
    f = np.float32
    x = np.asarray(x, f)
    with np.errstate(over="ignore", under="ignore", invalid="ignore", divide="ignore"):
        fast_exp = lambda v, log2e=f(1.4426950408889634): np.exp2(v * log2e)
        fma = lambda a, b, c: (a.astype(np.float64) * np.asarray(b, np.float64) + c).astype(f)
        if act == 0:
            return x
        if act == 1:
            return np.where(x > 0, x, f(0))
        if act in (2, 3):
            e = np.exp2(x) if defect == "elu_no_log2e" else np.exp(x)   # __expf
            if act == 2:
                return np.where(x > 0, x, e - f(1))
            scale = f(1.0507) if defect == "selu_scale_1.0507" else f(1.05070098)
            alpha = f(1.67) if defect == "selu_alpha_1.67" else f(1.67326324)
            return np.where(x > 0, scale * x, (scale * alpha) * (e - f(1)))
        if act == 4:
            if defect == "gelu_erf":
                import math
                return (0.5 * x.astype(np.float64) * (1.0 + np.vectorize(math.erf)(x.astype(np.float64) / math.sqrt(2.0)))).astype(f)
            c = f(0.0455) if defect == "gelu_coef_0.0455" else f(0.044715)
            u = f(0.7978845608028654) * (x + c * x * x * x)
            t = f(1) - f(2) / (fast_exp(f(2) * u) + f(1))
            return f(0.5) * x * (f(1) + t)
        if act == 5:
            e = fast_exp(x)
            r = f(1) / fma(e, e + f(2), 2.0)
            return np.where(x > (2 if defect == "mish_guard_2" else 20), x, x * fma(np.full(x.shape, -2, f), r, 1.0))
        if act == 6:
            return x / (f(1) + (np.exp2(-x) if defect == "swish_no_log2e" else fast_exp(-x)))
        if act == 7:
            mid = x * (x + f(3)) * f(0.1667) if defect == "hswish_times_0.1667" else x * (x + f(3)) / f(6)
            return np.where(x >= (2.5 if defect == "hswish_edge_2.5" else 3), x, np.where(x <= -3, f(0), mid))
    raise ValueError(act)


def f16_store_toward_zero(a):
    """float32 -> fp16 by truncation over the whole range (subnormals and overflow to the largest finite value included), as
    float32: the planted store defect of the activation sweep"""
    a = np.asarray(a, np.float32)
    with np.errstate(over="ignore"):
        n = a.astype(np.float16)
    bits = n.view(np.uint16)
    away = np.abs(n.astype(np.float64)) > np.abs(a.astype(np.float64))   # rounded away from zero (inf included): one step back
    return np.where(away, bits - np.uint16(1), bits).astype(np.uint16).view(np.float16).astype(np.float32)
