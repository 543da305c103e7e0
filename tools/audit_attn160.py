#!/usr/bin/env python3
"""Build-time audit of csrc/attn160.hip's inline-asm register loads (cdna_hip_programming.md 5.7, item 1): pair_tail160_kernel's parked
self output comes back by `buffer_load_dwordx4 ... sc1` statements hipcc does not track, and is valid only behind the `s_waitcnt vmcnt(6)`
statement that names its registers; matrix_cross160_kernel's lane-major self output comes back the same way, by ten `buffer_load_dwordx4`
statements (without `lds`: not LDS-DMA pieces) valid behind their `s_waitcnt vmcnt(6)`.  Between a load and its wait
hipcc must not read, copy, spill or overwrite the load's registers (it once placed v_mov copies in FRONT of the wait).  Compiles the
file with -save-temps for both 16-bit types and checks every instruction in between; also requires zero spills and no scratch.
Exit code 1 on a violation.   python tools/audit_attn160.py"""
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from diffsim_amd.build import CSRC, FLAGS, HIPCC  # noqa: E402

SRC = os.path.join(CSRC, "attn160.hip")


def regs_of(tok):
    out = set()
    for lo, hi in re.findall(r"v\[(\d+):(\d+)\]", tok):
        out.update(range(int(lo), int(hi) + 1))
    for n in re.findall(r"(?<![\w\[:])v(\d+)\b", tok):
        out.add(int(n))
    return out


def audit(flags):
    with tempfile.TemporaryDirectory() as d:
        cmd = [HIPCC] + FLAGS + ["--cuda-device-only", "-S", SRC, "-o", os.path.join(d, "a.s")] + flags
        subprocess.run(cmd, check=True, capture_output=True)
        lines = open(os.path.join(d, "a.s")).read().split("\n")
    text = "\n".join(lines)
    spills = [int(x) for x in re.findall(r"\.vgpr_spill_count:\s*(\d+)", text)]
    scratch = [int(x) for x in re.findall(r"\.private_segment_fixed_size:\s*(\d+)", text)]
    bad = []
    if any(spills) or any(scratch):
        bad.append(f"spills {spills} scratch {scratch}")
    for kern, groups in (("pair_tail160_kernel", ((r"buffer_load_dwordx4\b.*\bsc1\b", 10, "s_waitcnt vmcnt(6)"),)),
                         ("matrix_cross160_kernel", ((r"buffer_load_dwordx4\b(?!.*\blds\b)", 10, "s_waitcnt vmcnt(6)"),))):
        bad += [f"{kern}: {b}" for b in audit_kernel(function_lines(lines, kern), groups)]
    return bad


def function_lines(lines, name):
    start = next((i for i, l in enumerate(lines) if re.match(r"^_Z\S*%s\S*:" % name, l)), None)
    if start is None:
        return []
    end = next((i for i in range(start, len(lines)) if lines[i].startswith(".Lfunc_end")), len(lines))
    return lines[start:end]


def audit_kernel(lines, groups):
    """groups: (load pattern, count, wait) in program order; each group's loads must be followed by its wait with none of their
    destination registers touched in between"""
    if not lines:
        return ["kernel not found"]
    bad = []
    pos = 0
    for pat, count, wait in groups:
        loads = [i for i in range(pos, len(lines)) if re.search(pat, lines[i])][:count]
        if len(loads) != count:
            return bad + [f"expected {count} loads /{pat}/ , found {len(loads)}"]
        dest = set()
        for i in loads:
            dest |= regs_of(lines[i].split(",")[0])
        end = next((i for i in range(loads[-1], len(lines)) if wait in lines[i]), None)
        if end is None:
            return bad + [f"no {wait} behind the loads"]
        for i in range(loads[0] + 1, end):
            l = lines[i].strip()
            if not l or l.startswith(";") or l.startswith(".") or i in loads:
                continue
            hit = regs_of(l) & dest
            if hit:
                bad.append(f"line {i + 1}: '{l}' touches registers {sorted(hit)[:6]} of loads not yet waited for")
        pos = loads[-1] + 1
    return bad


def main():
    rc = 0
    for name, flags in (("bf16", []), ("fp16", ["-DDSIM_H16_IS_F16"])):
        bad = audit(flags)
        print(f"attn160 asm-load audit [{name}]:", "ok" if not bad else "FAILED")
        for b in bad[:20]:
            print("   ", b)
        rc |= bool(bad)
    return rc


if __name__ == "__main__":
    sys.exit(main())
