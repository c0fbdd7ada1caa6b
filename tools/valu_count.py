#!/usr/bin/env python3
"""Static instruction counts of the fused ResBlock-step kernel (conv_sx_pair_kernel), per instantiation, from device assembly:
    python tools/valu_count.py [tu_pair.s] [--hist "<1,2,1,4,0,false,1>"] [--kernel conv_sx_pair_kernel]
Without a path the unit is compiled here (hipcc -S --cuda-device-only of csrc/tu_pair.hip, what build()'s ISA checks read; a
file build() left behind under -save-temps=obj, <unit>-hip-amdgcn-amd-amdhsa-gfx950.s, is read the same way when given).
Columns: non-MFMA vector instructions (lines starting with v_), MFMAs, VGPRs, scratch bytes per lane.  --hist prints the
vector-instruction histogram of the instantiations whose name contains the given text."""
import argparse
import collections
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def instantiation(mangled):
    """'_ZN6vitsmi19conv_sx_pair_kernelILi1ELi2E..Lb0ELi1EEEv..' -> '<1,2,..,false,1>' ('' for a non-template)"""
    m = re.search(r"kernelI((?:L[ib]\d+E)+)E", mangled)
    if not m:
        return ""
    parts = []
    for kind, val in re.findall(r"L([ib])(\d+)E", m.group(1)):
        parts.append(val if kind == "i" else ("true" if val == "1" else "false"))
    return "<" + ",".join(parts) + ">"


def kernels(asm_text, want):
    """[(mangled name, instruction mnemonics, {metadata})] of every kernel of `asm_text` whose name contains `want`"""
    out = []
    for m in re.finditer(r"\n(_Z\w+):[^\n]*\n", asm_text):
        name = m.group(1)
        if want not in name:
            continue
        end = asm_text.find(".Lfunc_end", m.end())
        body = asm_text[m.end():end if end > 0 else len(asm_text)]
        ops = []
        for raw in body.split("\n"):
            l = raw.split(";")[0].strip()
            if l and not l.endswith(":") and not l.startswith("."):
                ops.append(l.split()[0])
        # the resource comment block hipcc prints behind the function
        tail = asm_text[end:end + 4000] if end > 0 else ""
        meta = {}
        for key, pat in (("vgprs", r"; NumVgprs: (\d+)"), ("agprs", r"; NumAgprs: (\d+)"), ("scratch", r"; ScratchSize: (\d+)"),
                         ("sgprs", r"; NumSgprs: (\d+)"), ("bytes", r"; codeLenInByte = (\d+)")):
            mm = re.search(pat, tail)
            meta[key] = int(mm.group(1)) if mm else -1
        out.append((name, ops, meta))
    return out


def table(asm_text, want="conv_sx_pair_kernel"):
    rows = []
    for name, ops, meta in kernels(asm_text, want):
        mfma = sum(1 for o in ops if o.startswith("v_mfma"))
        valu = sum(1 for o in ops if o.startswith("v_")) - mfma
        rows.append((instantiation(name), valu, mfma, meta["vgprs"], meta["scratch"], meta["bytes"]))
    return sorted(rows)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("asm", nargs="?", help="device assembly (.s); default: compile csrc/tu_pair.hip")
    ap.add_argument("--kernel", default="conv_sx_pair_kernel")
    ap.add_argument("--unit", default="tu_pair.hip", help="translation unit to compile when no .s is given")
    ap.add_argument("--hist", default=None, help="also print the vector histogram of instantiations containing this text")
    a = ap.parse_args()
    if a.asm:
        with open(a.asm) as f:
            text = f.read()
    else:
        from phoonnx_amd import build
        text = build.isa_of(a.unit)
    print("| instantiation | non-MFMA VALU | MFMA | VGPRs | scratch | code bytes |")
    print("|---|---|---|---|---|---|")
    for inst, valu, mfma, vg, sc, nb in table(text, a.kernel):
        print(f"| `{inst}` | {valu} | {mfma} | {vg} | {sc} | {nb} |")
    if a.hist is not None:
        for name, ops, _ in kernels(text, a.kernel):
            inst = instantiation(name)
            if a.hist not in inst:
                continue
            h = collections.Counter(o for o in ops if o.startswith("v_") and not o.startswith("v_mfma"))
            print(f"\n{inst}:")
            for op, n in h.most_common():
                print(f"  {op:24s} {n}")


if __name__ == "__main__":
    main()
