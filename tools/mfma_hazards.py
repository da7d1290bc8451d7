#!/usr/bin/env python
"""Instruction-stream lint around the bf16 MFMAs of the bf16 x 3 layers (cross-compiles without a GPU).

The faults recorded in csrc/rdrf_common.hpp (a stale lo piece, a B operand overwritten two instructions after the MFMA that
read it) were cured by instruction ORDER, which nothing else in the suite looks at.  For every v_mfma_f32_32x32x16_bf16 of a
kernel, inside its basic block:

  RAW distance  instructions between the last VALU instruction that writes a register of its A or B operand and the MFMA
  WAR distance  instructions between the MFMA and the next VALU instruction that overwrites a register of its A or B operand

An s_nop counts as its argument + 1; comments, labels and directives count nothing; a distance is "none" when the block
holds no such VALU instruction (operands that come from LDS / buffer loads only, or a block that ends first).  An MFMA whose
operands cannot be parsed as register ranges is counted as unchecked and printed.

Usage: python tools/mfma_hazards.py [--table] [file.hip | file.s ...]     (default: the five units that hold bf16 MFMAs)
  --table   the machine-readable lines `unit kernel n_mfma unchecked min_raw min_war` only (profiles/*_mfma_hazards.txt)
"""
import collections
import os
import re
import shutil
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "robust-dynrf_amd", "csrc")
UNITS = ("rdrf_fwd.hip", "rdrf_bwd.hip", "rdrf_bwd_fused.hip", "rdrf_render.hip", "rdrf_motion.hip", "rdrf_selftest.hip")
MFMA = "v_mfma_f32_32x32x16_bf16"
NONE = 10 ** 6   # "no such VALU instruction in the block"

_REG = re.compile(r"^([va])(?:(\d+)|\[(\d+):(\d+)\])$")
_LABEL = re.compile(r"^([.\w$@]+):")
_ENDS_BLOCK = re.compile(r"^(s_branch|s_cbranch_|s_endpgm|s_setpc_b64|s_swappc_b64|s_call_b64)")
_TWO_DESTS = ("v_swap_b32", "v_permlane16_swap", "v_permlane32_swap")


def hipcc_flags():
    """CXXFLAGS of csrc/Makefile, read from it so that the lint compiles what the library is built from"""
    for line in open(os.path.join(CSRC, "Makefile")):
        if line.startswith("CXXFLAGS"):
            flags = line.split("=", 1)[1].split()
            return [f.replace("$(ARCH)", "gfx950") for f in flags]
    raise RuntimeError("CXXFLAGS not found in csrc/Makefile")


def assembly(src, extra=()):
    """gfx950 assembly of one translation unit (device side only)"""
    if src.endswith(".s"):
        return open(src).read()
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    cmd = [hipcc] + hipcc_flags() + list(extra) + ["-S", "--cuda-device-only", os.path.basename(src), "-o", "-"]
    r = subprocess.run(cmd, cwd=os.path.dirname(os.path.abspath(src)), capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError(f"{' '.join(cmd)} failed:\n{r.stderr[-2000:]}")
    return r.stdout


def regs(operand):
    """'v[54:57]' -> {('v', 54), ..., ('v', 57)}; None when the operand is not a vector / accumulator register (range)"""
    m = _REG.match(operand.strip())
    if not m:
        return None
    lo = int(m.group(2) if m.group(2) is not None else m.group(3))
    hi = int(m.group(2) if m.group(2) is not None else m.group(4))
    return {(m.group(1), r) for r in range(lo, hi + 1)}


def valu_writes(mnemonic, operands):
    """vector registers a VALU instruction writes (empty for compares, for results in scalar registers and for non-VALU)"""
    if not mnemonic.startswith("v_") or mnemonic.startswith(("v_mfma", "v_smfmac", "v_cmp")) or not operands:
        return set()
    out = set()
    for op in operands[:2 if mnemonic.startswith(_TWO_DESTS) else 1]:
        out |= regs(op) or set()
    return out


def parse(asm):
    """{kernel: [block, ...]}, block = [(mnemonic, [operands], wait states it stands for)]"""
    kernels, cur, block = collections.OrderedDict(), None, None
    for raw in asm.splitlines():
        line = raw.split(";", 1)[0].rstrip()
        if not line.strip():
            continue
        m = _LABEL.match(line)
        if m:
            name = m.group(1)
            if not name.startswith(".L") and not name.startswith("$"):   # a function
                cur = kernels.setdefault(name, [])
            if cur is not None:
                block = []
                cur.append(block)
            continue
        text = line.strip()
        if cur is None or text.startswith("."):
            continue
        parts = text.split(None, 1)
        mnemonic = parts[0]
        operands = [o.strip() for o in parts[1].split(",")] if len(parts) > 1 else []
        cost = int(operands[0], 0) + 1 if mnemonic == "s_nop" and operands else 1
        block.append((mnemonic, operands, cost))
        if _ENDS_BLOCK.match(mnemonic):
            block = []
            cur.append(block)
    return kernels


def analyse(blocks):
    """-> dict(n, unchecked [text], raw [distance per MFMA], war [...]) of one kernel"""
    res = dict(n=0, unchecked=[], raw=[], war=[])
    for block in blocks:
        writes = [valu_writes(m, ops) for m, ops, _ in block]
        for i, (m, ops, _) in enumerate(block):
            if not m.startswith(MFMA):
                continue
            res["n"] += 1
            a, b = (regs(ops[1]), regs(ops[2])) if len(ops) >= 4 else (None, None)
            if a is None or b is None or len(a) != 4 or len(b) != 4:
                res["unchecked"].append(m + " " + ", ".join(ops))
                continue
            ab = a | b
            d, raw = 0, NONE
            for j in range(i - 1, -1, -1):
                if writes[j] & ab:
                    raw = d
                    break
                d += block[j][2]
            d, war = 0, NONE
            for j in range(i + 1, len(block)):
                if writes[j] & ab:
                    war = d
                    break
                d += block[j][2]
            res["raw"].append(raw)
            res["war"].append(war)
    return res


def run(paths=None, extra=()):
    """-> [(unit, kernel, result)] for every kernel with at least one bf16 MFMA, plus (unit, None, None) for a unit without"""
    paths = [os.path.join(CSRC, u) for u in UNITS] if not paths else paths
    from concurrent.futures import ThreadPoolExecutor
    with ThreadPoolExecutor(max_workers=len(paths)) as pool:   # one hipcc per unit, side by side
        texts = list(pool.map(lambda p: assembly(p, extra), paths))
    out = []
    for p, text in zip(paths, texts):
        unit = os.path.splitext(os.path.basename(p))[0]
        kernels = parse(text)
        hit = False
        for name, blocks in kernels.items():
            r = analyse(blocks)
            if r["n"]:
                out.append((unit, name, r))
                hit = True
        if not hit:
            out.append((unit, None, None))
    return out


def fmt(d):
    return "none" if d >= NONE else str(d)


def table_lines(results):
    lines = []
    for unit, name, r in results:
        if name is None:
            lines.append(f"{unit} - 0 0 none none")
        else:
            lines.append(f"{unit} {name} {r['n']} {len(r['unchecked'])} {fmt(min(r['raw'], default=NONE))} {fmt(min(r['war'], default=NONE))}")
    return lines


def read_table(path):
    """{(unit, kernel): (n_mfma, unchecked, min_raw, min_war)} from a committed table (lines starting with # are prose)"""
    t = {}
    for line in open(path):
        f = line.split()
        if not f or f[0].startswith("#"):
            continue
        val = lambda s: NONE if s == "none" else int(s)
        t[(f[0], f[1])] = (int(f[2]), int(f[3]), val(f[4]), val(f[5]))
    return t


def histogram(ds):
    c = collections.Counter(min(d, 32) if d < NONE else NONE for d in ds)
    return " ".join(f"{'none' if k >= NONE else ('32+' if k == 32 else k)}:{v}" for k, v in sorted(c.items()))


def demangle(names):
    if shutil.which("c++filt") is None:
        return dict(zip(names, names))
    txt = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.splitlines()
    return {n: re.sub(r"\(.*", "", t.replace("(anonymous namespace)::", "")) for n, t in zip(names, txt)}


if __name__ == "__main__":
    args = [a for a in sys.argv[1:] if a != "--table"]
    results = run(args)
    if "--table" in sys.argv[1:]:
        print("\n".join(table_lines(results)))
        sys.exit(0)
    nice = demangle([n for _, n, _ in results if n])
    total = unchecked = 0
    for unit, name, r in results:
        if name is None:
            print(f"{unit}: no {MFMA}")
            continue
        total += r["n"]
        unchecked += len(r["unchecked"])
        print(f"{unit}: {nice[name]}\n    {r['n']} bf16 MFMAs, {len(r['unchecked'])} unchecked; min RAW {fmt(min(r['raw'], default=NONE))}, "
              f"min WAR {fmt(min(r['war'], default=NONE))}\n    RAW {histogram(r['raw'])}\n    WAR {histogram(r['war'])}")
        for u in r["unchecked"]:
            print("    unchecked:", u)
    print(f"total: {total} bf16 MFMAs, {unchecked} unchecked ({100.0 * unchecked / max(total, 1):.2f} %)")
