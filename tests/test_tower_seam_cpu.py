"""tower_seam.py closes the layer loop of the persistent tower in hipcc's assembly and must REJECT assembly that does not look
like what it was written against (the build then goes on without the persistent kernel: test_kernel_hygiene.py).  Each case
here breaks one thing in a copy of lib/obj/tower.s and asserts that the script exits non-zero with the message of the check the
mutation was aimed at.  CPU-only: the script runs in-process on text."""
import importlib.util
import os
import re

import pytest

from sayuri_amd import _build

CONV4 = "_ZN6sayuri17conv_tower_kernelILi4EEEvPKNS_10TowerLayerE"
ANCHOR = re.compile(r"; TOWER_ACC 0 (\d+) (\d+) ([av])\[(\d+):(\d+)\]")


@pytest.fixture(scope="module")
def seam():
    """(the script as a module, the lines of tower.s, their index): read and indexed once, never changed"""
    asm = os.path.join(_build.LIB, "obj", "tower.s")
    if not os.path.exists(asm):
        _build.build_tower_blob(force=True)
    spec = importlib.util.spec_from_file_location("tower_seam", os.path.join(_build.HIP_SRC, "tower_seam.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    lines = open(asm).read().split("\n")
    return mod, lines, mod.Index(lines)


def run(mod, lines, tmp_path):
    src, dst = tmp_path / "tower.s", tmp_path / "tower_seamed.s"
    src.write_text("\n".join(lines))
    mod.main([str(src), str(dst), "--align=8", "--pad=32"])
    return dst


def first_instruction(mod, lines, f):
    return next(k for k in range(f["begin"] + 1, f["end"]) if mod.is_instruction(lines[k]))


def hook_line(lines, ix):
    conv = ix.funcs[(4, "conv")]
    return next(k for k in range(conv["begin"], conv["end"]) if "; TOWER_SE_HOOK " in lines[k])


def anchors(lines, ix):
    conv = ix.funcs[(4, "conv")]
    return [k for k in range(conv["begin"], conv["end"]) if ANCHOR.search(lines[k])]


def kernarg_size_16(mod, lines, ix):
    _, k = ix.directive(CONV4, "kernarg_size")
    lines[k] = re.sub(r"\d+\s*$", "16", lines[k])


def plant_in_fc(instruction):
    def mutate(mod, lines, ix):
        lines.insert(first_instruction(mod, lines, ix.funcs[(4, "fc")]) + 1, "\t" + instruction)
    return mutate


def drop_an_anchor(mod, lines, ix):
    del lines[anchors(lines, ix)[5]]


def overlap_two_anchors(mod, lines, ix):
    """a tile moved two registers up, into the tile that follows it in the register file"""
    at = {}
    for k in anchors(lines, ix):
        m = ANCHOR.search(lines[k])
        at[(m.group(3), int(m.group(4)))] = k
    (cls, lo), k = next((key, k) for key, k in sorted(at.items()) if (key[0], key[1] + 4) in at)
    lines[k] = lines[k].replace(f"{cls}[{lo}:{lo + 3}]", f"{cls}[{lo + 2}:{lo + 5}]")


def duplicate_the_hook(mod, lines, ix):
    k = hook_line(lines, ix)
    lines.insert(k, lines[k])


def other_wmt(mod, lines, ix):
    k = hook_line(lines, ix)
    assert " wmt=4 " in lines[k]
    lines[k] = lines[k].replace(" wmt=4 ", " wmt=6 ")


def no_roword(mod, lines, ix):
    k = hook_line(lines, ix)
    lines[k], n = re.subn(r" roword=\S+", "", lines[k])
    assert n == 1


def nops_of_14(mod, lines, ix):
    last = [k for k in range(ix.funcs[(4, "conv")]["begin"], anchors(lines, ix)[0]) if mod.is_instruction(lines[k])][-2:]
    for k in last:
        assert lines[k].strip() == "s_nop 15"
        lines[k] = lines[k].replace("s_nop 15", "s_nop 14")


def no_sgpr_count(mod, lines, ix):
    lo, hi = ix.meta[CONV4]
    del lines[next(k for k in range(lo, hi + 1) if lines[k].strip().startswith(".sgpr_count:"))]


CASES = [
    ("kernarg_size", kernarg_size_16, ".amdhsa_kernarg_size = 16, the seam was written for 8"),
    ("scratch_in_fc", plant_in_fc("scratch_load_dword v1, off, off offset:4"), "scratch access in a tower body"),
    ("agpr_in_fc", plant_in_fc("v_accvgpr_read_b32 v1, a0"), "touches AGPRs (they hold the accumulators)"),
    ("m0_in_fc", plant_in_fc("s_mov_b32 m0, s5"), "uses m0 / calls (not expected in the FC body)"),
    ("anchor_deleted", drop_an_anchor, "47 anchors for 48 output tiles"),
    ("anchors_overlap", overlap_two_anchors, "overlapping accumulator tiles"),
    ("hook_twice", duplicate_the_hook, "2 TOWER_SE_HOOK statements"),
    ("hook_wmt", other_wmt, "the hook says wmt=6"),
    ("hook_roword", no_roword, "the hook statement names no `roword`"),
    ("s_nop_14", nops_of_14, "['s_nop 14', 's_nop 14'] in front of the anchors, expected the K loop's two s_nop 15"),
    ("metadata_sgpr_count", no_sgpr_count, "lacks 1 expected keys"),
]


@pytest.mark.parametrize("mutate,message", [c[1:] for c in CASES], ids=[c[0] for c in CASES])
def test_seam_rejects(seam, tmp_path, capsys, mutate, message):
    mod, lines, ix = seam
    mutated = list(lines)
    mutate(mod, mutated, ix)
    assert mutated != lines
    with pytest.raises(SystemExit) as exit_:
        run(mod, mutated, tmp_path)
    err = capsys.readouterr().err
    assert exit_.value.code not in (0, None), exit_.value.code
    assert err.startswith("tower_seam.py: ") and message in err.strip().splitlines()[-1], err
    assert not (tmp_path / "tower_seamed.s").exists(), "a rejected input must leave no output"


def test_unmutated_assembly_goes_through(seam, tmp_path):
    mod, lines, _ = seam
    dst = run(mod, list(lines), tmp_path)
    assert dst.stat().st_size > len("\n".join(lines))
