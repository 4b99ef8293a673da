#!/usr/bin/env python3
"""Close the layer loop of the persistent tower launch in the assembly hipcc emits for tower.hip, and put the SE unit
into it as generated assembly.

    python tower_seam.py tower.s tower_seamed.s [--inv] [--sleep=N] [--align=A --pad=P]

conv_tower.h explains why neither is written in C++.  hipcc compiles, per channel-tile width W, two single-layer kernels
    conv_tower_kernel<W>    K loop | hook | epilogue        (the convolution body)
    tower_se_fc_kernel<W>   pooled partials in LDS -> gate in LDS   (the FCs of the SE unit)
each with ONE argument, a pointer to a TowerLayer, loaded from s[0:1] + 0.  This script turns the pair into one persistent
kernel (entered through the conv_tower_kernel<W> symbol):

  entry stub     s[B:B+1] <- the table pointer (the launch's only argument), s[B+2] <- workgroup id, s[B+3] <- wave id,
                 where B is the first SGPR no compiled body allocates
  dispatch       rebuilds the ABI entry state for the element at s[B:B+1] -- s[0:1] = its address (the element starts
                 with its own address, so it reads as a kernarg segment), s2 = workgroup id, v0 = thread id, exec = -1 --
                 parks the element's has_se in s[B+4] and enters the convolution body
  hook           the `; TOWER_SE_HOOK` asm statement behind the K loop becomes: has_se == 0 ? nothing :
                     pooling over the accumulators IN THE REGISTERS THE K LOOP LEFT THEM IN (read off the `; TOWER_ACC`
                     anchors that precede the hook) -> partial sums / maxima in LDS, the FC images on their way by LDS-DMA
                     far jump into the FC body (its VGPRs renamed into the range the hook statement clobbers), which
                     returns through every one of its s_endpgm
                     the gate, x <- sigmoid(gamma) x + beta, in place
                 and behind it the generated epilogue for the layers the host marks with row_order = 1
  seam           every s_endpgm of the convolution body becomes a branch to:  s_waitcnt vmcnt(0) lgkmcnt(0) (this wave's
                 stores are acknowledged), s_barrier (all eight waves'), then end if the element was the last of the run, else
                 s[B:B+1] += the table's stride and back to dispatch.

The launch kernel's descriptor and metadata get the union of the bodies' resources (SGPRs incl. the five parked ones) and the
whole LDS as its static group segment (the bodies address it from 0).  Scratch: none -- the build fails if any body
wants it.  Fails loudly when the assembly does not look like what it was written against.

How the file is laid out.  main() is the list of stages: parse the options, index the file ONCE (Index: bodies, descriptor
blocks, metadata entries), then per width  check_abi x 2 -> parse_hook -> check_fc_body -> read_anchors -> find_exits ->
choose_parked ->
the edits (FC body, hook text, entry and dispatch, seam, descriptor, metadata), and at the end apply the edits and write.
Stages that check only read and die(); stages that emit only build text.  Every layout number of the C++ side -- field
offsets, the table's stride, the hook's register ranges, column tiles per wave, LDS sizes -- reaches the script as an operand
of the hook statement (parse_hook); the only split of its own is FC_SGPR_CAP.  The hook's text is written through an Emitter
(output lines, label prefix, register allocator); registers are Reg values that print themselves.

What the generated pooling / gate must reproduce bit for bit is board_se_pool / board_se_gate (conv_board.h): the per-layer
kernel conv_board_se_kernel runs those, and SAYURI_TOWER=0/1 give identical outputs (tests/test_gpu_smallops.py).
"""
import argparse
import re
import sys
from types import SimpleNamespace

FC_SGPR_CAP = 40   # the FC body may use s[0:39]; the hook keeps what must survive the call in s[40:frees-1]

CONV_RE = re.compile(r"^(_ZN6sayuri17conv_tower_kernelILi(\d+)EEEvPKNS_10TowerLayerE):")
FC_RE = re.compile(r"^(_ZN6sayuri18tower_se_fc_kernelILi(\d+)EEEvPKNS_10TowerLayerE):")

# the entry state the seam rebuilds for a compiled body, as its descriptor must state it
ABI = (("user_sgpr_count", 2), ("user_sgpr_kernarg_segment_ptr", 1), ("system_sgpr_workgroup_id_x", 1),
       ("system_sgpr_workgroup_id_y", 0), ("system_sgpr_workgroup_id_z", 0), ("system_vgpr_workitem_id", 0),
       ("kernarg_size", 8), ("group_segment_fixed_size", 0), ("user_sgpr_kernarg_preload_length", 0),
       ("uses_dynamic_stack", 0), ("private_segment_fixed_size", 0))

HOOK_KEYS = ("elem", "tid", "wmt", "ui", "cols", "w1h", "w2h", "w1b", "w2b", "psum", "pmax", "gate", "kot", "res", "out", "couts",
             "slotpix", "act", "arith", "mish", "relu", "identity", "roword",
             "stride", "last", "hasse", "freev", "frees", "nj", "epilds", "lds")


def die(msg):
    sys.stderr.write("tower_seam.py: " + msg + "\n")
    sys.exit(1)


class Reg:
    """n consecutive registers of one file.  Prints as the assembler wants it (s7, s[8:9], v[72:75], a12); r[k] is its k-th
    register, r[a:b] the run of those from a to b - 1."""

    def __init__(self, cls, lo, n=1):
        self.cls, self.lo, self.n = cls, lo, n

    def __str__(self):
        return f"{self.cls}{self.lo}" if self.n == 1 else f"{self.cls}[{self.lo}:{self.lo + self.n - 1}]"

    def __getitem__(self, k):
        if isinstance(k, slice):
            return Reg(self.cls, self.lo + k.start, k.stop - k.start)
        return Reg(self.cls, self.lo + k)

    def __iter__(self):
        return (self[k] for k in range(self.n))


def far_jump(sym, t=Reg("s", 4, 2)):
    # the idiom LLVM emits for a far call; the pair t is dead at every place this script uses it
    return [f"\ts_getpc_b64 {t}",
            f"\ts_add_u32 {t[0]}, {t[0]}, {sym}@rel32@lo+4",
            f"\ts_addc_u32 {t[1]}, {t[1]}, {sym}@rel32@hi+12",
            f"\ts_setpc_b64 {t}"]


def is_instruction(ln):
    s = ln.strip()
    return bool(s) and ln.startswith("\t") and not s.startswith(".") and not s.startswith(";")


def rename_vgprs(ln, shift):
    """v<N> -> v<N+shift> in the operands of one line of compiled assembly (mnemonics never match: `v_`)."""
    code, sep, comment = ln.partition(";")
    code = re.sub(r"\bv\[(\d+):(\d+)\]", lambda m: f"v[{int(m.group(1)) + shift}:{int(m.group(2)) + shift}]", code)
    code = re.sub(r"\bv(\d+)\b", lambda m: f"v{int(m.group(1)) + shift}", code)
    return code + sep + comment


def max_reg(body, cls):
    hi = -1
    for ln in body:
        code = ln.split(";")[0]
        for m in re.finditer(r"\b%s\[(\d+):(\d+)\]" % cls, code):
            hi = max(hi, int(m.group(2)))
        for m in re.finditer(r"\b%s(\d+)\b" % cls, code):
            hi = max(hi, int(m.group(1)))
    return hi


def quad_channel(i):
    """conv_board.h board_quad_channel for even tile counts, lane quad 0: first channel (from the wave's first) of the four a lane
    holds of row tile i; quad q adds 8 q"""
    return (i >> 1) * 32 + 4 * (i & 1)


def lds_slot(j, pr, p):
    """which 1 KiB piece of the wave's LDS share holds the residual rows of (column tile j, pair pr): board_epilogue's lds_slot"""
    return (j if j < p.JH else j - p.NRT) * p.npair + pr


# ---------------------------------------------------------------------------------------------------------------- the input

class Index:
    """tower.s, read once: funcs[(width, 'conv' | 'fc')] = name and line range of a compiled body (label line .. the line before
    the `.section .rodata` that follows its last s_endpgm), the lines of every `.amdhsa_kernel` descriptor block by key, the
    line range of every kernel's metadata entry."""

    def __init__(self, lines):
        self.lines, self.funcs, self.desc, self.meta = lines, {}, {}, {}
        body = block = entry = None
        for k, ln in enumerate(lines):
            if body is None:
                m = CONV_RE.match(ln) or FC_RE.match(ln)
                if m:
                    body = dict(name=m.group(1), begin=k)
                    self.funcs[(int(m.group(2)), "conv" if m.re is CONV_RE else "fc")] = body
            elif ln.startswith("\t.section\t.rodata"):
                body["end"] = k
                body = None
            s = ln.strip()
            if s.startswith(".amdhsa_kernel "):
                block = self.desc.setdefault(s[len(".amdhsa_kernel "):], {})
            elif s == ".end_amdhsa_kernel":
                block = None
            elif block is not None and s.startswith(".amdhsa_"):
                block.setdefault(s.split()[0][len(".amdhsa_"):], k)
            if ln.startswith("  - "):
                entry = [k, k]
            elif entry is not None and ln.startswith("    "):
                entry[1] = k
                if s.startswith(".name:"):
                    self.meta.setdefault(ln.split()[-1], entry)
            else:
                entry = None
        if body is not None:
            die("no .rodata section after " + body["name"])
        self.widths = sorted({w for (w, _) in self.funcs})
        if not self.widths:
            die("no conv_tower_kernel in the input")
        for w in self.widths:
            if (w, "conv") not in self.funcs or (w, "fc") not in self.funcs:
                die(f"conv_tower_kernel<{w}> and tower_se_fc_kernel<{w}> must both be present")

    def body(self, f):
        return range(f["begin"] + 1, f["end"])

    def directive(self, name, key):
        """value of `.amdhsa_<key>` inside the descriptor of kernel `name` (and its line index)"""
        idx = self.desc.get(name, {}).get(key)
        if idx is None:
            die(f"descriptor of {name}: no .amdhsa_{key}")
        return int(self.lines[idx].split()[-1]), idx


# ------------------------------------------------------------------------------------------------------------- the checks

def check_abi(ix, f):
    """A compiled body can be entered the way the seam enters it and wants no scratch; notes its register counts in f"""
    for key, want in ABI:
        got, _ = ix.directive(f["name"], key)
        if got != want:
            die(f"{f['name']}: .amdhsa_{key} = {got}, the seam was written for {want}")
    body = [ix.lines[k] for k in ix.body(f)]
    first = next((ln for ln in body if is_instruction(ln)), "")
    if not re.match(r"\ts_load_dwordx2 s\[\d+:\d+\], s\[0:1\], 0x0", first):
        die(f"{f['name']}: the body does not start by loading its argument from s[0:1] ({first.strip()!r})")
    if any(re.match(r"\s*scratch_", ln) for ln in body):
        die(f"{f['name']}: scratch access in a tower body")
    f["sgprs"], _ = ix.directive(f["name"], "next_free_sgpr")
    f["vgprs"], _ = ix.directive(f["name"], "next_free_vgpr")
    f["accum"], _ = ix.directive(f["name"], "accum_offset")


def parse_hook(ix, conv, w):
    """-> (line of the TOWER_SE_HOOK statement, its operands: elem / tid as Reg, everything else as int)"""
    lines, name = ix.lines, conv["name"]
    hooks = [k for k in ix.body(conv) if "; TOWER_SE_HOOK " in lines[k]]
    if len(hooks) != 1:
        die(f"{name}: {len(hooks)} TOWER_SE_HOOK statements")
    named = {}
    for tok in lines[hooks[0]].split("TOWER_SE_HOOK", 1)[1].split():
        key, _, val = tok.partition("=")
        named[key] = val if key in ("elem", "tid") else int(val, 0)
    for key in HOOK_KEYS:
        if key not in named:
            die(f"{name}: the hook statement names no `{key}`")
    hook = SimpleNamespace(**named)
    if hook.wmt != w:
        die(f"{name}: the hook says wmt={hook.wmt}")
    m = re.match(r"^s\[(\d+):(\d+)\]$", hook.elem)
    if not m or int(m.group(1)) < hook.frees or not re.match(r"^v\d+$", hook.tid) or int(hook.tid[1:]) >= hook.freev:
        die(f"{name}: hook operands {hook.elem} / {hook.tid} sit inside the clobbered ranges")
    hook.elem = Reg("s", int(m.group(1)), int(m.group(2)) - int(m.group(1)) + 1)
    hook.tid = Reg("v", int(hook.tid[1:]))
    if w % 2:
        die("the SE hook is written for even row-tile counts (board_row_channel order)")
    if hook.w2b != hook.w1b + 4:
        die("w1_bytes / w2_bytes are not adjacent in BoardSeParams")
    if epi_pieces(hook).nd % (w // 2):
        die("epilogue: register pieces are not whole column tiles")
    return hooks[0], hook


def check_fc_body(ix, fc, hook):
    """The FC body is a subroutine of the hook: no AGPRs, its VGPRs fit behind freev, its SGPRs below FC_SGPR_CAP; -> its last VGPR"""
    name = fc["name"]
    fbody = [ix.lines[k] for k in ix.body(fc)]
    if any(re.search(r"\ba\d+\b|\ba\[\d+:\d+\]|v_accvgpr|v_mfma", ln.split(";")[0]) for ln in fbody):
        die(f"{name}: touches AGPRs (they hold the accumulators)")
    fv, fs = max_reg(fbody, "v"), max_reg(fbody, "s")
    if fv + hook.freev > 127:
        die(f"{name}: v{fv} does not fit behind v{hook.freev} (128 - {hook.freev} VGPRs belong to the hook)")
    if fs >= FC_SGPR_CAP:
        die(f"{name}: s{fs} -- the hook keeps its own values from s{FC_SGPR_CAP} on")
    if any(re.search(r"\bm0\b|ttmp|flat_scratch|s_getpc|s_setpc|s_swappc|s_call", ln.split(";")[0]) for ln in fbody):
        die(f"{name}: uses m0 / calls (not expected in the FC body)")
    return fv


def read_anchors(ix, conv, hk, hook):
    """-> acc[(row tile, column tile)] = the Reg that holds the output tile at the hook, read off the TOWER_ACC anchors"""
    lines, name, w = ix.lines, conv["name"], hook.wmt
    acc, first_anchor = {}, None
    for k in ix.body(conv):
        m = re.search(r"; TOWER_ACC (\d+) (\d+) (\d+) ([av])\[(\d+):(\d+)\]", lines[k])
        if not m:
            continue
        side, ti, tj, kind, lo, hi = int(m.group(1)), int(m.group(2)), int(m.group(3)), m.group(4), int(m.group(5)), int(m.group(6))
        if side != 0 or hi != lo + 3 or (ti, tj) in acc or k > hk:
            die(f"{name}: unexpected anchor {lines[k].strip()!r}")
        if kind == "v" and lo + 3 >= hook.freev:
            die(f"{name}: accumulator tile ({ti}, {tj}) lives in v[{lo}:{hi}], inside the hook's range")
        acc[(ti, tj)] = Reg(kind, lo, 4)
        first_anchor = k if first_anchor is None else first_anchor
    if len(acc) != w * hook.nj:
        die(f"{name}: {len(acc)} anchors for {w * hook.nj} output tiles")
    regs = sorted((t.cls, t.lo) for t in acc.values())
    if any(regs[n][0] == regs[n + 1][0] and regs[n][1] + 4 > regs[n + 1][1] for n in range(len(regs) - 1)):
        die(f"{name}: overlapping accumulator tiles")
    stray = [lines[k].strip() for k in range(first_anchor, hk) if is_instruction(lines[k])]
    if stray:
        die(f"{name}: instructions between the anchors and the hook ({stray[:3]}): the tiles may have moved")
    # the MFMAs' results are read by the pooling: the K loop's s_nop 15 pair must be what precedes the anchors
    before = [lines[k].strip() for k in range(conv["begin"] + 1, first_anchor) if is_instruction(lines[k])][-2:]
    if before != ["s_nop 15", "s_nop 15"]:
        die(f"{name}: {before} in front of the anchors, expected the K loop's two s_nop 15")
    # every accumulator the MFMA stream writes is an anchored tile
    written = set()
    for k in range(conv["begin"] + 1, first_anchor):
        m = re.match(r"\tv_mfma_\w+ ([av])\[(\d+):(\d+)\]", lines[k])
        if m:
            written.add((m.group(1), int(m.group(2))))
    if written != set(regs):
        die(f"{name}: the MFMA stream writes {len(written)} tiles, the anchors name {len(set(regs))} (or others)")
    if any(t.cls == "v" and t.lo % 2 for t in acc.values()):
        die("epilogue: an accumulator tile in VGPRs is not even-aligned")
    return acc


def find_exits(ix, conv):
    """-> the lines of the convolution body's s_endpgm"""
    ends = [k for k in ix.body(conv) if ix.lines[k].strip() == "s_endpgm"]
    if not ends:
        die(f"{conv['name']}: no s_endpgm")
    return ends


def choose_parked(w, conv, fc, fv, hook):
    """-> the five SGPRs above every body's allocation and the hook's range that live across layers"""
    B = (max(conv["sgprs"], fc["sgprs"]) + 1) & ~1
    if B + 5 > 102:
        die(f"width {w}: no five SGPRs left above the compiler's {B}")
    B = max(B, hook.frees + 2)
    if conv["accum"] < hook.freev + fv + 1:
        die(f"width {w}: accum_offset {conv['accum']} below the FC body's renamed VGPRs")
    s = Reg("s", B, 5)
    return SimpleNamespace(all=s, tab=s[0:2], wg=s[2], wave=s[3], has_se=s[4])


# ------------------------------------------------------------------------------------------------------- the hook's text

class Emitter:
    """The text of one hook: its lines, its label prefix and its registers -- v[freev:127] and s[4:frees-1] (s[0:3] are set up
    for the FC call itself), of which the SGPRs asked for with keep=True survive that call."""

    def __init__(self, prefix, hook):
        self.lines, self.prefix, self.freev, self.frees = [], prefix, hook.freev, hook.frees
        self.s_keep = FC_SGPR_CAP
        self.release()

    def release(self):
        """all registers but the kept SGPRs are free again (the FC body has used them)"""
        self.v_next, self.s_low = self.freev, 4

    def __call__(self, text):
        self.lines.append("\t" + text)

    def at(self, name):
        return f"{self.prefix}_{name}"

    def label(self, name):
        self.lines.append(self.at(name) + ":")

    def v(self, n=1, align=1):
        lo = (self.v_next + align - 1) // align * align
        self.v_next = lo + n
        if self.v_next > 128:
            die("the hook ran out of VGPRs")
        return Reg("v", lo, n)

    def s(self, n=1, keep=False):
        lo = ((self.s_keep if keep else self.s_low) + n - 1) // n * n
        if keep:
            self.s_keep = lo + n
            if self.s_keep > self.frees:
                die("the hook ran out of SGPRs")
        else:
            self.s_low = lo + n
            if self.s_low > FC_SGPR_CAP:
                die("the hook ran out of scratch SGPRs")
        return Reg("s", lo, n)


def wave_geometry(e, g, info, wave, t0):
    """board kernels' first lines: which column tiles are this wave's.  info = (board size << 8 | column tiles of the workgroup)"""
    e(f"s_and_b32 {g.ncols}, {info}, 0xff")
    e(f"s_lshr_b32 {g.bs}, {info}, 8")
    e(f"s_add_u32 {g.nj0}, {g.ncols}, 1")
    e(f"s_lshr_b32 {g.nj0}, {g.nj0}, 1")
    e(f"s_lshr_b32 {g.wave_n}, {wave}, 2")
    e(f"s_and_b32 {g.wave_m}, {wave}, 3")
    e(f"s_sub_u32 {t0}, {g.ncols}, {g.nj0}")
    e(f"s_cmp_eq_u32 {g.wave_n}, 0")
    e(f"s_cselect_b32 {g.col0}, 0, {g.nj0}")
    e(f"s_cselect_b32 {g.nj}, {g.nj0}, {t0}")


def read_tile(e, t, tmp):
    """-> where the VALU finds accumulator tile t: itself, or tmp after the four moves out of its AGPRs"""
    if t.cls == "v":
        return t
    for r in range(4):
        e(f"v_accvgpr_read_b32 {tmp[r]}, {t[r]}")
    return tmp


def se_hook(w, hook, acc, park, fc_label):
    """The SE unit between the K loop and the epilogue of width-w's convolution body, as assembly text.
    hook: the operands of the TOWER_SE_HOOK statement; acc[(i, j)] = the registers of output tile (row tile i, column tile j);
    park: the SGPRs that live across layers."""
    e = Emitter(f".Ltower{w}_se", hook)
    r = SimpleNamespace()
    r.m0 = e.s(keep=True)
    r.w1h, r.w2h = e.s(2, keep=True), e.s(2, keep=True)
    r.wb = e.s(2, keep=True)                # w1_bytes, w2_bytes
    r.wbytes = e.s(keep=True)               # bytes of LDS in front of the stage's vectors
    r.wave_m = e.s(keep=True)
    r.info, r.ncols, r.bs, r.nj0, r.wave_n, r.col0, r.nj, r.njm1 = (e.s() for _ in range(8))
    r.t0, r.t1, r.k, r.n = (e.s() for _ in range(4))
    r.p = e.s(2)
    r.valid, r.px0, r.save = e.s(2), e.s(2), e.s(2)
    r.lane, r.lane16, r.px, r.q, r.t, r.addr, r.addr2 = (e.v() for _ in range(7))
    r.ro = e.s(keep=True)                   # BoardParams::row_order of the layer
    r.sets = [(e.v(4, 4), e.v(4, 4)) for _ in range(2)]   # (sums, maxima) of a row tile, alternating
    r.xs = [e.v(4, 4) for _ in range(2)]                  # an AGPR tile on its way through the VALU, alternating

    e(f"; ---- tower_seam.py: the SE unit (width {w}: {hook.wmt} row tiles x {hook.nj} column tiles per wave)")
    e(f"s_cmp_eq_u32 {park.has_se}, 0")
    e(f"s_cbranch_scc1 {e.at('skip')}")
    e(f"s_mov_b32 {r.m0}, m0")
    se_geometry(e, hook, park, r)
    se_stage_images(e, park, r)
    se_pooling(e, hook, acc, r)
    se_call_fc(e, w, hook, park, fc_label)
    se_gate(e, hook, acc, r)
    e(f"s_mov_b32 m0, {r.m0}")
    e.label("skip")
    return e.lines


def se_geometry(e, hook, park, r):
    """the layer's FC images and table entry, this lane's and this wave's place in the tile"""
    E = hook.elem
    e("s_waitcnt lgkmcnt(0)")
    e("s_barrier")                          # every wave is done with the rings
    e(f"s_load_dwordx2 {r.w1h}, {E}, {hex(hook.w1h)}")
    e(f"s_load_dwordx2 {r.w2h}, {E}, {hex(hook.w2h)}")
    e(f"s_load_dwordx2 {r.wb}, {E}, {hex(hook.w1b)}")
    e(f"s_load_dword {r.info}, {E}, {hex(hook.ui)}")
    e(f"v_and_b32_e32 {r.lane}, 63, {hook.tid}")
    e(f"v_lshlrev_b32_e32 {r.lane16}, 4, {r.lane}")
    e(f"v_and_b32_e32 {r.px}, 15, {r.lane}")
    e(f"v_lshrrev_b32_e32 {r.q}, 4, {r.lane}")
    e("s_waitcnt lgkmcnt(0)")
    e(f"s_cmp_gt_i32 {r.info}, -1")
    e(f"s_cbranch_scc1 {e.at('info')}")
    e(f"s_load_dwordx2 {r.p}, {E}, {hex(hook.cols)}")
    e(f"s_lshl_b32 {r.t0}, {park.wg}, 2")
    e("s_waitcnt lgkmcnt(0)")
    e(f"s_load_dword {r.info}, {r.p}, {r.t0}")
    e("s_waitcnt lgkmcnt(0)")
    e.label("info")
    wave_geometry(e, r, r.info, park.wave, r.t0)
    e(f"s_sub_u32 {r.njm1}, {r.nj}, 1")


def se_stage_images(e, park, r):
    """both FC images on their way into LDS: linear 1 KiB pieces, piece k by wave k % 8; the squeeze image of this tile's board
    size first"""
    e(f"s_add_u32 {r.t0}, {r.wb[0]}, {r.wb[1]}")
    e(f"s_cmp_lg_u64 {r.w1h}, 0")
    e(f"s_cselect_b32 {r.wbytes}, {r.t0}, 0")
    e(f"s_cbranch_scc0 {e.at('nostage')}")
    e(f"s_sub_u32 {r.t0}, {r.bs}, 2")
    e(f"s_mul_hi_u32 {r.t1}, {r.t0}, {r.wb[0]}")
    e(f"s_mul_i32 {r.t0}, {r.t0}, {r.wb[0]}")
    e(f"s_add_u32 {r.w1h[0]}, {r.w1h[0]}, {r.t0}")
    e(f"s_addc_u32 {r.w1h[1]}, {r.w1h[1]}, {r.t1}")
    for tag, base, nbytes, lds0 in (("1", r.w1h, r.wb[0], None), ("2", r.w2h, r.wb[1], r.wb[0])):
        e(f"s_lshr_b32 {r.n}, {nbytes}, 10")
        e(f"s_mov_b32 {r.k}, {park.wave}")
        e.label(f"dma{tag}")
        e(f"s_cmp_ge_u32 {r.k}, {r.n}")
        e(f"s_cbranch_scc1 {e.at(f'dma{tag}_done')}")
        e(f"s_lshl_b32 {r.t0}, {r.k}, 10")
        e(f"s_add_u32 {r.p[0]}, {base[0]}, {r.t0}")
        e(f"s_addc_u32 {r.p[1]}, {base[1]}, 0")
        if lds0 is not None:
            e(f"s_add_u32 {r.t0}, {r.t0}, {lds0}")
        e(f"s_mov_b32 m0, {r.t0}")
        e("s_nop 4")
        e(f"global_load_lds_dwordx4 {r.lane16}, {r.p}")
        e(f"s_add_u32 {r.k}, {r.k}, 8")
        e(f"s_branch {e.at(f'dma{tag}')}")
        e.label(f"dma{tag}_done")
    e.label("nostage")


def se_pooling(e, hook, acc, r):
    """per row tile: sums and maxima over the wave's column tiles, reduced over the 16 pixels of a lane row, to LDS"""
    wmt, kot, NJ = hook.wmt, hook.kot, hook.nj
    # last_valid (lane): (col0 + nj - 1) * 16 + px < bs * bs -- a one-sample tile has its unused pixel slots at the end, only
    # the wave's last column tile can hold any
    e(f"s_add_u32 {r.t0}, {r.col0}, {r.njm1}")
    e(f"s_lshl_b32 {r.t0}, {r.t0}, 4")
    e(f"v_add_u32_e32 {r.t}, {r.t0}, {r.px}")
    e(f"s_mul_i32 {r.t1}, {r.bs}, {r.bs}")
    e(f"v_cmp_gt_u32_e64 {r.valid}, {r.t1}, {r.t}")
    e(f"v_cmp_eq_u32_e64 {r.px0}, 0, {r.px}")
    # psum[wave_n * KO_T + wave_m * WMT * 16 + first channel of (row tile i, quad q)] (floats) behind the images
    e(f"s_mul_i32 {r.t0}, {r.wave_n}, {kot * 4}")
    e(f"s_mul_i32 {r.t1}, {r.wave_m}, {wmt * 16 * 4}")
    e(f"s_add_u32 {r.t0}, {r.t0}, {r.t1}")
    e(f"s_add_u32 {r.t0}, {r.t0}, {r.wbytes}")
    e(f"s_add_u32 {r.t0}, {r.t0}, {hook.psum}")
    e(f"v_lshl_add_u32 {r.addr}, {r.q}, 4, {r.t0}")       # natural row order: quad q of row tile i at 16 i + 4 q
    e(f"v_lshl_add_u32 {r.addr2}, {r.q}, 5, {r.t0}")      # board_row_channel order: at quad_channel(i) + 8 q
    e(f"s_load_dword {r.ro}, {hook.elem}, {hex(hook.roword)}")

    def tile_ops(t, S4, M4, X):
        """sum += tile, max = max(max, tile) for output tile t; the caller has set exec"""
        src = read_tile(e, t, X)
        if src.lo % 2 == 0:
            e(f"v_pk_add_f32 {S4[0:2]}, {S4[0:2]}, {src[0:2]}")
            e(f"v_pk_add_f32 {S4[2:4]}, {S4[2:4]}, {src[2:4]}")
        else:
            for k in range(4):
                e(f"v_add_f32_e32 {S4[k]}, {S4[k]}, {src[k]}")
        for k in range(4):
            e(f"v_max_f32_e32 {M4[k]}, {M4[k]}, {src[k]}")

    for i in range(wmt):
        S4, M4 = r.sets[i & 1]
        for k in range(4):
            e(f"v_mov_b32_e32 {S4[k]}, 0")
            e(f"v_mov_b32_e32 {M4[k]}, 0xc59c4000")   # -5000.0f
        e(f"s_cmp_lt_i32 {r.nj}, 1")
        e(f"s_cbranch_scc1 {e.at(f'red{i}')}")
        for j in range(NJ):
            e(f"s_cmp_eq_u32 {r.njm1}, {j}")
            e(f"s_cbranch_scc1 {e.at(f'last{i}_{j}')}")
            tile_ops(acc[(i, j)], S4, M4, r.xs[j & 1])
        e(f"s_branch {e.at(f'red{i}')}")
        for j in range(NJ):
            e.label(f"last{i}_{j}")
            e(f"s_mov_b64 {r.save}, exec")
            e(f"s_and_b64 exec, exec, {r.valid}")
            tile_ops(acc[(i, j)], S4, M4, r.xs[j & 1])
            e(f"s_mov_b64 exec, {r.save}")
            if j + 1 < NJ:
                e(f"s_branch {e.at(f'red{i}')}")
        e.label(f"red{i}")
        e("s_nop 4")   # a VALU result read by a DPP operand: two wait states; exec written by the SALU: five
        for step in (8, 4, 2, 1):
            for op, V4 in (("add", S4), ("max", M4)):
                for k in range(4):
                    e(f"v_{op}_f32_dpp {V4[k]}, {V4[k]}, {V4[k]} row_ror:{step} row_mask:0xf bank_mask:0xf")
        e(f"s_mov_b64 {r.save}, exec")
        e(f"s_and_b64 exec, exec, {r.px0}")
        if i == 0:
            e("s_waitcnt lgkmcnt(0)")      # row_order has arrived
        e(f"s_cmp_eq_u32 {r.ro}, 0")
        e(f"s_cbranch_scc1 {e.at(f'pst{i}')}")
        e(f"ds_write_b128 {r.addr2}, {S4} offset:{quad_channel(i) * 4}")
        e(f"ds_write_b128 {r.addr2}, {M4} offset:{quad_channel(i) * 4 + hook.pmax - hook.psum}")
        e(f"s_branch {e.at(f'pse{i}')}")
        e.label(f"pst{i}")
        e(f"ds_write_b128 {r.addr}, {S4} offset:{i * 64}")
        e(f"ds_write_b128 {r.addr}, {M4} offset:{i * 64 + hook.pmax - hook.psum}")
        e.label(f"pse{i}")
        e(f"s_mov_b64 exec, {r.save}")
    e("s_waitcnt vmcnt(0) lgkmcnt(0)")    # this wave's pieces of the images have landed, its partials are written
    e("s_barrier")


def se_call_fc(e, w, hook, park, fc_label):
    """the FCs: a compiled body of its own, entered with the ABI's entry state; it comes back to tower<w>_se_return"""
    e(f"s_mov_b32 s0, {hook.elem[0]}")
    e(f"s_mov_b32 s1, {hook.elem[1]}")
    e(f"s_mov_b32 s2, {park.wg}")
    e(f"v_mov_b32_e32 v{hook.freev}, {hook.tid}")
    e("s_mov_b64 exec, -1")
    e.lines.extend(far_jump(fc_label))
    e.lines.append(f"tower{w}_se_return:")
    e("s_mov_b64 exec, -1")
    e.release()


def se_gate(e, hook, acc, r):
    """the gate: x <- sigmoid(gamma) x + beta, one fused multiply-add per value, in place"""
    wmt, kot = hook.wmt, hook.kot
    g_lane, g_q, g_addr = e.v(), e.v(), e.v()
    gs = [(e.v(4, 4), e.v(4, 4)) for _ in range(wmt)]     # (sigmoid(gamma), beta) of a row tile's channels
    gx = [e.v(4, 4) for _ in range(2)]
    s_t = e.s()
    e(f"v_and_b32_e32 {g_lane}, 63, {hook.tid}")
    e(f"v_lshrrev_b32_e32 {g_q}, 4, {g_lane}")
    e(f"s_mul_i32 {s_t}, {r.wave_m}, {wmt * 16 * 4}")
    e(f"s_add_u32 {s_t}, {s_t}, {r.wbytes}")
    e(f"s_add_u32 {s_t}, {s_t}, {hook.gate}")
    e(f"s_cmp_eq_u32 {r.ro}, 0")
    e(f"s_cbranch_scc1 {e.at('gnat')}")
    e(f"v_lshl_add_u32 {g_addr}, {g_q}, 5, {s_t}")
    for i in range(wmt):
        e(f"ds_read_b128 {gs[i][0]}, {g_addr} offset:{quad_channel(i) * 4}")
        e(f"ds_read_b128 {gs[i][1]}, {g_addr} offset:{quad_channel(i) * 4 + kot * 4}")
    e(f"s_branch {e.at('gread')}")
    e.label("gnat")
    e(f"v_lshl_add_u32 {g_addr}, {g_q}, 4, {s_t}")
    for i in range(wmt):
        e(f"ds_read_b128 {gs[i][0]}, {g_addr} offset:{i * 64}")
        e(f"ds_read_b128 {gs[i][1]}, {g_addr} offset:{i * 64 + kot * 4}")
    e.label("gread")
    e("s_waitcnt lgkmcnt(0)")
    e("s_barrier")                         # the gate is read: the epilogue's residual rows may land in this LDS

    def fma_tile(i, t):
        G, Bt = gs[i]
        if t.lo % 2 == 0:
            e(f"v_pk_fma_f32 {t[0:2]}, {G[0:2]}, {t[0:2]}, {Bt[0:2]}")
            e(f"v_pk_fma_f32 {t[2:4]}, {G[2:4]}, {t[2:4]}, {Bt[2:4]}")
        else:
            for k in range(4):
                e(f"v_fma_f32 {t[k]}, {G[k]}, {t[k]}, {Bt[k]}")

    tiles = [(i, j) for i in range(wmt) for j in range(hook.nj)]
    agpr = [t for t in tiles if acc[t].cls == "a"]
    for k in range(0, len(agpr), 2):      # AGPR tiles two at a time through the VALU
        pair = list(zip(agpr[k:k + 2], gx))
        for t, x in pair:
            read_tile(e, acc[t], x)
        for t, x in pair:
            fma_tile(t[0], x)
        for t, x in pair:
            for k4 in range(4):
                e(f"v_accvgpr_write_b32 {acc[t][k4]}, {x[k4]}")
    for t in tiles:
        if acc[t].cls == "v":
            fma_tile(t[0], acc[t])


def epi_pieces(hook):
    """how the residual pieces (1 KiB: 8 channels x 64 lanes) of a wave split between its LDS share and registers"""
    npair = hook.wmt // 2
    nd = max(hook.nj * npair - hook.epilds // 1024, 0)      # pieces that go to registers
    return SimpleNamespace(npair=npair, nd=nd, JH=hook.nj // 2, NRT=nd // npair)    # the column tiles [JH, JH + NRT)


def epi_hook(w, hook, acc, park):
    """The epilogue of width-w's convolution body as assembly text, for the layers the host marks with row_order = 1 (Mish, ReLU or
    no activation, one sample per tile with computed table entries, the layer's channels = the channel tile; their weights and bias are in
    board_row_channel order, so a lane's two accumulator quads of a row-tile pair ARE 8 consecutive channels): optional residual, activation, fp16 NHWC store, straight
    from the accumulators where the K loop left them -- the arithmetic of board_epilogue / mish2 (conv_board.h) operation for
    operation, so the outputs equal the compiled epilogue's bit for bit.  What it saves is what hipcc adds: per 16-byte store
    ~14 register moves staging its operands and a conversion + half a packed add per residual value (here one
    v_fma_mix_f32), in front of everything ~200 accumulator moves -- the epilogue is bound by VALU issue (tools/ubench/trans_rate.hip:
    a plain operation 4 cycles of a SIMD, a packed one 5, a transcendental 10.7, v_permlane16_swap 14).  Other layers fall through
    to the compiled epilogue behind this text."""
    p = epi_pieces(hook)
    e = Emitter(f".Ltower{w}_ep", hook)
    r = SimpleNamespace()
    r.res, r.out, r.l2e, r.valid, r.save = e.s(2), e.s(2), e.s(2), e.s(2), e.s(2)
    (r.arith, r.act, r.couts, r.slotpix, r.ui, r.ncols, r.bs, r.nj0, r.wave_n, r.wave_m, r.col0, r.nj, r.npix, r.t0, r.t1, r.late,
     r.step, r.mylds) = (e.s() for _ in range(18))
    r.lane, r.R, r.px, r.cb, r.off, r.pxl, r.t, r.lds, r.a, r.r, r.so = (e.v() for _ in range(11))
    r.rreg = [e.v(4, 4) for _ in range(p.nd)]
    r.X, r.Y, r.RR = e.v(4, 4), e.v(4, 4), e.v(4, 4)
    r.Tm, r.U = e.v(8, 2), e.v(8, 4)

    E = hook.elem
    e(f"; ---- tower_seam.py: the epilogue (width {w}) for Mish layers with computed table entries; others take the compiled one below")
    e(f"s_load_dword {r.arith}, {E}, {hex(hook.roword)}")
    e(f"s_load_dword {r.act}, {E}, {hex(hook.act)}")
    e(f"s_load_dword {r.couts}, {E}, {hex(hook.couts)}")
    e(f"s_load_dword {r.slotpix}, {E}, {hex(hook.slotpix)}")
    e(f"s_load_dword {r.ui}, {E}, {hex(hook.ui)}")
    e(f"s_load_dwordx2 {r.res}, {E}, {hex(hook.res)}")
    e(f"s_load_dwordx2 {r.out}, {E}, {hex(hook.out)}")
    e("s_waitcnt lgkmcnt(0)")
    # row_order = 1: the host gave this layer the board_row_channel image BECAUSE this text will run (Mish, one sample per tile with
    # computed table entries, channels = the channel tile: Engine::board_row_order_ok)
    e(f"s_cmp_eq_u32 {r.arith}, 0")
    e(f"s_cbranch_scc1 {e.at('compiled')}")
    # row_order = 3 (SAYURI_TOWER_NOEPI_AFTER=n, a MEASURING switch of the engine): this layer's epilogue is skipped -- nothing is
    # stored, the activations stay what the last complete forward left (realistic operands for the next layer's MFMAs, unlike a
    # build that never stores: that one multiplies zeros and gains clock).  What a launch costs without its epilogues bounds
    # what hiding them under the MFMA stream could be worth.
    e(f"s_cmp_eq_u32 {r.arith}, 3")
    e(f"s_cbranch_scc1 {e.at('done')}")
    epi_geometry(e, hook, park, r)
    e(f"s_cmp_eq_u64 {r.res}, 0")
    e(f"s_cbranch_scc1 {e.at('tiles_nores')}")
    epi_request_residual(e, hook, p, r)
    epi_wait_ladder(e, hook, p, r)
    # one pair of tile loops (with / without residual) per activation the text covers
    kinds = (("mish", hook.mish), ("relu", hook.relu), ("identity", hook.identity))
    for with_res in (True, False):
        e.label("tiles" if with_res else "tiles_nores")
        tags = {kind: ("r" if with_res else "n") + kind for kind, _ in kinds}
        for kind, code in kinds[1:]:
            e(f"s_cmp_eq_u32 {r.act}, {code}")
            e(f"s_cbranch_scc1 {e.at(tags[kind])}")
        for kind, _ in kinds:
            if kind != "mish":
                e.label(tags[kind])
            epi_tiles(e, hook, p, acc, r, with_res, kind)
    e.label("done")
    e.lines.extend(far_jump(f"tower{w}_seam"))
    e.label("compiled")
    return e.lines


def epi_geometry(e, hook, park, r):
    """geometry of this wave and lane (board_epilogue's first lines), its offsets into the buffers and into LDS"""
    e(f"v_and_b32_e32 {r.lane}, 63, {hook.tid}")
    e(f"v_lshrrev_b32_e32 {r.R}, 4, {r.lane}")
    e(f"v_and_b32_e32 {r.px}, 15, {r.lane}")
    wave_geometry(e, r, r.ui, park.wave, r.t0)
    e(f"s_mul_i32 {r.npix}, {r.bs}, {r.bs}")
    # the weight image's rows are in board_row_channel order: a lane holds channels 32 pr + 8 R .. + 7 of pair pr (the quad of
    # row tile 2 pr, then the quad of 2 pr + 1) -- cb(pr) = wave_m * WMT * 16 + 8 R + 32 pr, no exchange between lanes
    e(f"s_mul_i32 {r.t0}, {r.wave_m}, {hook.wmt * 16}")
    e(f"v_lshl_add_u32 {r.cb}, {r.R}, 3, {r.t0}")
    # byte offset of (this lane's pixel of column tile 0, cb(0)) in the output / residual buffers; column tile j adds j * step
    e(f"s_lshl_b32 {r.t1}, {r.col0}, 4")
    e(f"v_add_u32_e32 {r.pxl}, {r.t1}, {r.px}")
    e(f"s_mul_i32 {r.t0}, {park.wg}, {r.slotpix}")
    e(f"v_add_u32_e32 {r.off}, {r.t0}, {r.pxl}")
    e(f"v_mul_lo_u32 {r.off}, {r.off}, {r.couts}")
    e(f"v_add_u32_e32 {r.off}, {r.off}, {r.cb}")
    e(f"v_lshlrev_b32_e32 {r.off}, 1, {r.off}")
    e(f"s_lshl_b32 {r.step}, {r.couts}, 5")
    e(f"s_mul_i32 {r.mylds}, {park.wave}, {hook.epilds}")
    e(f"v_lshlrev_b32_e32 {r.lds}, 4, {r.lane}")
    e(f"v_add_u32_e32 {r.lds}, {r.mylds}, {r.lds}")
    e(f"s_mov_b32 {r.l2e[0]}, 0x3fb8aa3b")
    e(f"s_mov_b32 {r.l2e[1]}, 0x3fb8aa3b")


def epi_request_residual(e, hook, p, r):
    """residual: ALL rows of the wave requested at once (LDS-DMA into the dead rings, the few that do not fit into registers);
    issue order = first half, second half, register pieces: board_epilogue explains the two-step wait"""
    e("s_waitcnt lgkmcnt(0)")
    e("s_barrier")                     # every wave is done with the rings

    def tile_offset(j):
        """r.a <- byte offset of (this lane's pixel of column tile j, pair 0) in the residual buffer, vcc <- the lanes whose
        pixel exists; a pair's piece is fetched from r.a + 64 pr, from offset 0 by the lanes without a pixel"""
        e(f"v_add_u32_e32 {r.t}, {16 * j}, {r.pxl}")
        e(f"v_cmp_gt_u32_e32 vcc, {r.npix}, {r.t}")
        e(f"s_mul_i32 {r.t0}, {r.step}, {j}")
        e(f"v_add_u32_e32 {r.a}, {r.t0}, {r.off}")

    for j in (j for j in range(hook.nj) if not p.JH <= j < p.JH + p.NRT):
        e(f"s_cmp_le_u32 {r.nj}, {j}")
        e(f"s_cbranch_scc1 {e.at('lds_issued')}")
        tile_offset(j)
        for pr in range(p.npair):
            if pr:
                e(f"v_add_u32_e32 {r.a}, 64, {r.a}")
            e(f"v_cndmask_b32_e32 {r.r}, 0, {r.a}, vcc")
            e(f"s_add_u32 {r.t1}, {r.mylds}, {lds_slot(j, pr, p) * 1024}")
            e(f"s_mov_b32 m0, {r.t1}")
            e("s_nop 1")
            e(f"global_load_lds_dwordx4 {r.r}, {r.res}")
    e.label("lds_issued")
    for k in range(p.nd):
        j, pr = p.JH + k // p.npair, k % p.npair
        if pr == 0:
            e(f"s_cmp_le_u32 {r.nj}, {j}")
            e(f"s_cbranch_scc1 {e.at('reg_issued')}")
            tile_offset(j)
        else:
            e(f"v_add_u32_e32 {r.a}, 64, {r.a}")
        e(f"v_cndmask_b32_e32 {r.r}, 0, {r.a}, vcc")
        e(f"global_load_dwordx4 {r.rreg[k]}, {r.r}, {r.res}")
    e.label("reg_issued")


def epi_wait_ladder(e, hook, p, r):
    """wait for the first half's pieces only: the loads younger than those = the pieces of the column tiles [JH, nj)"""
    e(f"s_sub_i32 {r.late}, {r.nj}, {p.JH}")
    e(f"s_max_i32 {r.late}, {r.late}, 0")
    for t in range(hook.nj - p.JH + 1):
        e(f"s_cmp_eq_u32 {r.late}, {t}")
        e(f"s_cbranch_scc1 {e.at(f'late{t}')}")
    e(f"s_branch {e.at('late0')}")
    for t in range(hook.nj - p.JH, -1, -1):
        e.label(f"late{t}")
        e(f"s_waitcnt vmcnt({t * p.npair})")
        e(f"s_branch {e.at('tiles')}")


def act8(e, r, kind, x_pairs, h):
    """h <- act(the 8 values in the four even-aligned VGPR pairs x_pairs) as 8 fp16 (4 VGPRs); kind = the activation's name in
    common.h"""
    if kind == "mish":
        t = [r.Tm[2 * k:2 * k + 2] for k in range(4)]
        u = [r.U[2 * k:2 * k + 2] for k in range(4)]
        for k in range(4):
            e(f"v_pk_mul_f32 {t[k]}, {x_pairs[k]}, {r.l2e}")
        for k in range(8):
            e(f"v_exp_f32_e32 {r.Tm[k]}, {r.Tm[k]}")
        for k in range(4):
            e(f"v_pk_add_f32 {u[k]}, {t[k]}, 2.0 op_sel_hi:[1,0]")
        for k in range(4):
            e(f"v_pk_fma_f32 {t[k]}, {t[k]}, {u[k]}, 2.0 op_sel_hi:[1,1,0]")
        for k in range(8):
            e(f"v_rcp_f32_e32 {r.Tm[k]}, {r.Tm[k]}")
        for k in range(4):
            e(f"v_pk_fma_f32 {t[k]}, {t[k]}, -2.0, 1.0 op_sel_hi:[1,0,0]")
        for k in range(4):
            e(f"v_pk_mul_f32 {x_pairs[k]}, {x_pairs[k]}, {t[k]}")
    elif kind == "relu":      # x > 0 ? x : 0 as a compare and a select (v_max_f32 might hand back -0)
        for x in (x for pair in x_pairs for x in pair):
            e(f"v_cmp_lt_f32_e32 vcc, 0, {x}")
            e(f"v_cndmask_b32_e32 {x}, 0, {x}, vcc")
    for k in range(4):        # (identity: nothing but the conversion)
        e(f"v_cvt_pk_f16_f32 {h[k]}, {x_pairs[k][0]}, {x_pairs[k][1]}")


def epi_tiles(e, hook, p, acc, r, with_res, kind):
    """the tile loop of one activation: per column tile and row-tile pair  (+ residual) -> activation -> one 16-byte store"""
    # the fp16 result of a pair lives where the pair's temporaries lived (alternating halves: a store's data is rewritten two
    # pairs later at the earliest)
    Hs = [r.U[0:4], r.U[4:8]]
    nstore = 0
    for j in range(hook.nj):
        e(f"s_cmp_le_u32 {r.nj}, {j}")
        e(f"s_cbranch_scc1 {e.at('done')}")
        if j == p.JH and with_res:
            e("s_waitcnt vmcnt(0)")         # the second half's rows (and the first half's stores)
        e(f"v_add_u32_e32 {r.t}, {16 * j}, {r.pxl}")
        e(f"v_cmp_gt_u32_e64 {r.valid}, {r.npix}, {r.t}")
        e(f"s_mul_i32 {r.t0}, {r.step}, {j}")
        e(f"v_add_u32_e32 {r.so}, {r.t0}, {r.off}")
        for pr in range(p.npair):
            in_lds = not (p.JH <= j < p.JH + p.NRT)
            rr = r.RR
            if with_res and in_lds:
                # the piece comes back from LDS (lane-linear: the lane that reads it is the lane that fetched it)
                e(f"ds_read_b128 {r.RR}, {r.lds} offset:{lds_slot(j, pr, p) * 1024}")
            elif with_res:
                rr = r.rreg[(j - p.JH) * p.npair + pr]
            xa, xb = read_tile(e, acc[(2 * pr, j)], r.X), read_tile(e, acc[(2 * pr + 1, j)], r.Y)
            if with_res:
                # + residual: one fused multiply-add per value reads the fp16 half directly (v + (float)rr * 1.0: the same
                # single rounding as conversion + add)
                if in_lds:
                    e("s_waitcnt lgkmcnt(0)")
                for q, x in enumerate([*xa, *xb]):
                    e(f"v_fma_mix_f32 {x}, {rr[q // 2]}, 1.0, {x} op_sel:[{q & 1},0,0] op_sel_hi:[1,0,0]")
            h = Hs[nstore & 1]
            nstore += 1
            act8(e, r, kind, [xa[0:2], xa[2:4], xb[0:2], xb[2:4]], h)
            e(f"s_and_saveexec_b64 {r.save}, {r.valid}")
            e(f"global_store_dwordx4 {r.so}, {h}, {r.out}" + (f" offset:{64 * pr}" if pr else ""))
            e(f"s_mov_b64 exec, {r.save}")
    e(f"s_branch {e.at('done')}")


# ---------------------------------------------------------------------------------------------------------------- the edits
# each returns {line index: the lines that replace it}

def fc_body_edits(ix, fc, w, hook):
    """the FC body as a subroutine: a label to jump to, VGPRs renamed into the hook's range, every s_endpgm a return"""
    lines, edits = ix.lines, {}
    for k in ix.body(fc):
        if lines[k].strip() == "s_endpgm":
            edits[k] = far_jump(f"tower{w}_se_return")
        elif is_instruction(lines[k]):
            edits[k] = [rename_vgprs(lines[k], hook.freev)]
    edits[fc["begin"]] = [lines[fc["begin"]], f"tower{w}_body_fc:", "\t; ---- compiled body (FCs of the SE unit), VGPRs renamed by tower_seam.py"]
    return edits


def entry_edits(ix, conv, w, hook, park, opt):
    """entry stub and dispatch in front of the convolution body"""
    disp, body_conv = f"tower{w}_dispatch", f"tower{w}_body_conv"
    # placement of the convolution body: it starts on a 2^align-byte boundary plus pad bytes (control never falls into a body,
    # so the padding is never executed); the K loop sits at a fixed distance from the body's first instruction
    place = ([f"\t.p2align {opt.align}"] if opt.align else []) + (["\ts_nop 0"] * (opt.pad // 4))
    entry = [f"\t; ---- tower_seam.py: entry stub (table {park.tab}, workgroup {park.wg}, wave {park.wave}, has_se {park.has_se})",
             f"\ts_load_dwordx2 {park.tab}, s[0:1], 0x0",
             f"\ts_mov_b32 {park.wg}, s2",
             f"\tv_readfirstlane_b32 {park.wave}, v0",
             "\ts_nop 0",
             f"\ts_lshr_b32 {park.wave}, {park.wave}, 6",
             "\ts_waitcnt lgkmcnt(0)",
             f"{disp}:",
             f"\ts_load_dword {park.has_se}, {park.tab}, {hex(hook.hasse)}",
             "\ts_mov_b64 exec, -1",
             f"\ts_mov_b32 s0, {park.tab[0]}",
             f"\ts_mov_b32 s1, {park.tab[1]}",
             f"\ts_mov_b32 s2, {park.wg}",
             "\tv_mbcnt_lo_u32_b32 v0, -1, 0",
             "\tv_mbcnt_hi_u32_b32 v0, -1, v0",
             f"\tv_lshl_or_b32 v0, {park.wave}, 6, v0",
             "\ts_waitcnt lgkmcnt(0)",
             f"\ts_branch {body_conv}"] + place + [
             f"{body_conv}:",
             "\t; ---- compiled body (convolution: K loop, hook, epilogue)"]
    return {conv["begin"]: [ix.lines[conv["begin"]]] + entry}


def seam_edits(ends, w, hook, park, opt):
    """every s_endpgm of the convolution body (lines `ends`) branches to the seam, which follows the last of them"""
    seam, done = f".Ltower{w}_seam", f".Ltower{w}_done"
    tail = [f"{seam}:",
            f"tower{w}_seam:",
            "\ts_waitcnt vmcnt(0) lgkmcnt(0)",
            f"\ts_load_dword s4, {park.tab}, {hex(hook.last)}",
            "\ts_waitcnt lgkmcnt(0)",
            "\ts_barrier"]
    if opt.inv:
        tail.append("\tbuffer_inv sc1")
    # measuring builds only: --sleep=N parks every wave for N x 64 cycles here (what does a stall cost a chip that runs at
    # its power limit?)
    tail += ["\ts_sleep 127"] * (opt.sleep // 127) + ([f"\ts_sleep {opt.sleep % 127}"] if opt.sleep % 127 else [])
    tail += ["\ts_cmp_lg_u32 s4, 0",
             f"\ts_cbranch_scc1 {done}",
             f"\ts_add_u32 {park.tab[0]}, {park.tab[0]}, {hook.stride}",
             f"\ts_addc_u32 {park.tab[1]}, {park.tab[1]}, 0"] + far_jump(f"tower{w}_dispatch") + [
             f"{done}:",
             "\ts_endpgm"]
    edits = {k: [f"\ts_branch {seam}"] for k in ends}
    edits[ends[-1]] = edits[ends[-1]] + tail
    return edits


def resource_edits(ix, conv, hook, park):
    """the launch kernel's descriptor and its metadata entry (the runtime sizes LDS from there): all of the LDS, the parked SGPRs"""
    lines, name, edits = ix.lines, conv["name"], {}
    sgprs = park.all.lo + park.all.n
    for key, val in (("next_free_sgpr", sgprs), ("group_segment_fixed_size", hook.lds)):
        _, idx = ix.directive(name, key)
        edits[idx] = [re.sub(r"\d+\s*$", str(val), lines[idx])]
    if name not in ix.meta:
        die("no metadata entry for " + name)
    lo, hi = ix.meta[name]
    seen = set()
    for k in range(lo, hi + 1):
        for key, val in ((".group_segment_fixed_size:", hook.lds), (".sgpr_count:", sgprs + 6)):
            if lines[k].strip().lstrip("- ").startswith(key):
                edits[k] = [re.sub(r"\d+\s*$", str(val), lines[k])]
                seen.add(key)
    if len(seen) != 2:
        die("metadata entry of " + name + " lacks " + str(2 - len(seen)) + " expected keys")
    return edits


# ------------------------------------------------------------------------------------------------------------------- main

def parse_options(argv):
    ap = argparse.ArgumentParser(prog="tower_seam.py", usage="tower_seam.py in.s out.s [--inv] [--sleep=N] [--align=A --pad=P]")
    ap.add_argument("src")
    ap.add_argument("dst")
    ap.add_argument("--inv", action="store_true", help="buffer_inv sc1 in the seam")
    ap.add_argument("--sleep", type=int, default=0, help="measuring builds: park every wave N x 64 cycles in the seam")
    ap.add_argument("--align", type=int, default=0, help="the convolution body starts on a 2^A-byte boundary ...")
    ap.add_argument("--pad", type=int, default=0, help="... plus P bytes")
    return ap.parse_args(argv)


def seam_text(text, opt):
    """tower.s -> tower_seamed.s"""
    ix = Index(text.split("\n"))
    edits = {}      # line index -> replacement list
    for w in ix.widths:
        conv, fc = ix.funcs[(w, "conv")], ix.funcs[(w, "fc")]
        check_abi(ix, conv)
        check_abi(ix, fc)
        hk, hook = parse_hook(ix, conv, w)
        fv = check_fc_body(ix, fc, hook)
        acc = read_anchors(ix, conv, hk, hook)
        ends = find_exits(ix, conv)
        park = choose_parked(w, conv, fc, fv, hook)
        edits.update(fc_body_edits(ix, fc, w, hook))
        edits[hk] = se_hook(w, hook, acc, park, f"tower{w}_body_fc") + epi_hook(w, hook, acc, park)
        edits.update(entry_edits(ix, conv, w, hook, park, opt))
        edits.update(seam_edits(ends, w, hook, park, opt))
        edits.update(resource_edits(ix, conv, hook, park))
    out = []
    for k, ln in enumerate(ix.lines):
        out.extend(edits.get(k, [ln]))
    # one .text section for everything: the seam's far jumps then resolve at assembly time and no comdat group is cut
    return re.sub(r'^\t\.section\t\.text\.[^\n]*,comdat$', "\t.text", "\n".join(out), flags=re.M)


def main(argv=None):
    opt = parse_options(argv)
    with open(opt.src) as f:
        text = f.read()
    text = seam_text(text, opt)
    with open(opt.dst, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
