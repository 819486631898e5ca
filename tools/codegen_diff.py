#!/usr/bin/env python
"""Compare the gfx950 code of two hipcc object files, function by function.

    python tools/codegen_diff.py PARENT.o BRANCH.o [--out FILE.json]

For every function of either code object: the kernel metadata of both sides (verticut_amd.build.kernel_resources; device
functions that are no kernels have none), the instruction count of the disassembly, and whether the disassembly is identical
(instruction text only: addresses, encodings and pc-relative offsets are dropped).  It compares; it does not look for particular instructions.
Exit status 1 if a kernel's vgpr_count, vgpr_spill_count, private_segment_fixed_size or group_segment_fixed_size differs, or its
sgpr_spill_count grew.
"""
import argparse
import json
import os
import re
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from verticut_amd import build as vb  # noqa: E402

EQUAL = ("vgpr_count", "vgpr_spill_count", "private_segment_fixed_size", "group_segment_fixed_size")


def disassembly(obj):
    """{function: [instruction text, ...]} of the gfx950 code object inside obj"""
    objdump = os.path.join(vb.LLVM_BIN, "llvm-objdump")
    with tempfile.TemporaryDirectory() as td:
        co = vb.extract_code_object(obj, os.path.join(td, "gfx950.co"))
        text = subprocess.check_output([objdump, "-d", "--no-show-raw-insn", co]).decode(errors="replace")
    funcs, cur, pcrel = {}, None, 0
    for line in text.splitlines():
        m = re.match(r"^[0-9a-f]+ <(.+)>:$", line)
        if m:
            cur, pcrel = funcs.setdefault(m.group(1), []), 0
        elif cur is not None and line.startswith(("\t", " ")) and line.strip():
            insn = line.split("//")[0].strip()
            if insn:
                if pcrel:   # the two adds behind s_getpc_b64 carry a pc-relative offset: it moves with the layout, not with the code
                    insn, pcrel = re.sub(r"0x[0-9a-f]+$", "<pcrel>", insn), pcrel - 1
                if insn.startswith("s_getpc_b64"):
                    pcrel = 2
                cur.append(insn)
    return funcs


def compare(parent, branch):
    meta = (vb.kernel_resources(parent), vb.kernel_resources(branch))
    code = (disassembly(parent), disassembly(branch))
    out, bad = {}, []
    for name in sorted(set(code[0]) | set(code[1])):
        rec = {"identical": code[0].get(name) == code[1].get(name)}
        for side, i in (("parent", 0), ("branch", 1)):
            if name in code[i]:
                rec[side] = dict(meta[i].get(name, {}), instructions=len(code[i][name]))
        out[name] = rec
        a, b = meta[0].get(name), meta[1].get(name)
        if a and b and (any(a.get(k) != b.get(k) for k in EQUAL) or b.get("sgpr_spill_count", 0) > a.get("sgpr_spill_count", 0)):
            bad.append(name)
    return out, bad


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("parent")
    ap.add_argument("branch")
    ap.add_argument("--out", help="write the JSON here instead of stdout")
    a = ap.parse_args()
    funcs, bad = compare(a.parent, a.branch)
    differ = [n for n, r in funcs.items() if not r["identical"]]
    doc = {"n_functions": len(funcs), "n_identical": len(funcs) - len(differ), "differing": differ,
           "resource_mismatches": bad, "functions": funcs}
    text = json.dumps(doc, indent=1, sort_keys=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
        print("%d functions, %d identical, %d differ, %d resource mismatches -> %s" % (len(funcs), len(funcs) - len(differ), len(differ), len(bad), a.out))
    else:
        print(text)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
