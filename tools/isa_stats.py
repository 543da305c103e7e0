"""Development aid: per-kernel register / scratch / instruction-mix summary of a hipcc -save-temps .s file.
    hipcc --offload-arch=gfx950 -O3 -std=c++17 -c x.hip -save-temps ; python tools/isa_stats.py x-hip-amdgcn-amd-amdhsa-gfx950.s [filter]
Comparison mode, for a change that must leave the kernels alone (each side: one .s file or several joined by commas, taken together):
    python tools/isa_stats.py --compare before.s[,before2.s] after.s[,after2.s]
compares, per kernel symbol, the instruction text from its label to the end of the function (.Lfunc_end<N>: -- NOT the first s_endpgm:
hipcc lays early-exit blocks out before a kernel's tail; local labels renumbered, comments dropped) and the register / LDS / scratch
sizes of the metadata.  Every kernel is put in one of three classes: identical; identical up to register names (the same instruction
sequence once register operands are masked, same metadata); differs (printed with instruction counts and metadata, before -> after).
One summary line, exit status 1 unless every kernel is identical."""
import re
import subprocess
import sys


def demangle(names):
    try:
        r = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True)
        return r.stdout.strip().split("\n")
    except FileNotFoundError:
        return names


META = ("vgpr_count", "agpr_count", "sgpr_count", "group_segment_fixed_size", "private_segment_fixed_size")
REG = re.compile(r"\b([vsa])(\d+|\[\d+:\d+\])")


def body(s, name):
    """the text of kernel `name` from its label to the end of the function, whatever s_endpgm it holds on the way"""
    m = re.search(r"^" + re.escape(name) + r":[^\n]*\n(.*?)^\.Lfunc_end\d+:", s, re.S | re.M)
    if not m:
        raise SystemExit(f"isa_stats: kernel {name} is in the metadata but its label .. .Lfunc_end<N>: text was not found")
    return m.group(1)


def entries(s):
    """[(metadata getter, kernel name)] of the amdhsa.kernels list"""
    out = []
    for e in s[s.find("amdhsa.kernels:"):].split("  - .agpr_count:")[1:]:
        e = ".agpr_count:" + e
        g = lambda k, e=e: re.search(r"\." + k + r":\s*(\S+)", e).group(1)
        out.append((g, g("name")))
    return out


def kernels(s):
    """{symbol: (normalised instruction lines, metadata values)} of the text of one .s file"""
    out = {}
    for g, name in entries(s):
        labels = {}
        renum = lambda l: labels.setdefault(l.group(0), ".L%d" % len(labels))
        lines = [re.sub(r"\.LBB\d+_\d+", renum, ln.split(";")[0].strip()) for ln in body(s, name).split("\n")]
        out[name] = ([ln for ln in lines if ln], tuple(g(k) for k in META))
    return out


def masked(lines):
    return [REG.sub(lambda m: m.group(1) + ("#" if m.group(2)[0] != "[" else "[#]"), ln) for ln in lines]


def classify(a, b):
    """'identical', 'identical up to register names' or 'differs' for two (lines, metadata) of one kernel"""
    if a == b:
        return "identical"
    if a[1] == b[1] and masked(a[0]) == masked(b[0]):
        return "identical up to register names"
    return "differs"


def compare_sides(a, b, dup=(), title=""):
    """prints the comparison of two {symbol: (lines, metadata)} maps; 0 when every kernel is identical, else 1"""
    gone, new = sorted(set(a) - set(b)), sorted(set(b) - set(a))
    both = sorted(set(a) & set(b))
    cls = {n: classify(a[n], b[n]) for n in both}
    regs = [n for n in both if cls[n] == "identical up to register names"]
    diff = [n for n in both if cls[n] == "differs"]
    for tag, names in (("only before", gone), ("only after", new), ("identical up to register names", regs), ("differs", diff),
                       ("defined twice on one side", list(dup))):
        for n, d in zip(names, demangle(names)):
            print(f"{tag}: {d}" + (f"  instructions {len(a[n][0])} -> {len(b[n][0])}  {' / '.join(META)} {a[n][1]} -> {b[n][1]}"
                                   if tag == "differs" else ""))
    same = len(both) - len(regs) - len(diff)
    print(f"{title}{len(a)} kernels before, {len(b)} after, {same} identical "
          f"({sum(len(a[n][0]) for n in both if cls[n] == 'identical')} instruction lines), {len(regs)} identical up to register names, "
          f"{len(diff)} differ, {len(gone)} only before, {len(new)} only after, {len(dup)} defined twice on one side")
    return 0 if not (gone or new or regs or diff) else 1


def compare(before, after):
    sides, dup = [], []
    for paths in (before, after):
        side = {}
        for path in paths.split(","):
            for name, k in kernels(open(path).read()).items():
                if name in side:
                    dup.append(name + (" (identical copies)" if side[name] == k else " (DIFFERING copies)"))
                side[name] = k
        sides.append(side)
    return compare_sides(sides[0], sides[1], dup, f"{before} -> {after}: ")


def main():
    if sys.argv[1] == "--compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    s = open(sys.argv[1]).read()
    flt = sys.argv[2] if len(sys.argv) > 2 else None
    rows = [(name, g("agpr_count"), g("vgpr_count"), g("sgpr_count"), g("vgpr_spill_count"), g("private_segment_fixed_size"))
            for g, name in entries(s)]
    dn = demangle([r[0] for r in rows])
    for r, d in zip(rows, dn):
        d = d.replace("dsim::(anonymous namespace)::", "").replace("void ", "").replace("_ZN4dsim12_GLOBAL__N_1", "").replace("EEvNS_8GemmArgsEi", "")
        if flt and flt not in d:
            continue
        # instruction mix of the kernel body
        text = body(s, r[0])
        cnt = lambda pat: len(re.findall(pat, text, re.M))
        mix = dict(mfma=cnt(r"^\s+v_mfma"), valu=cnt(r"^\s+v_(?!mfma)"), ds=cnt(r"^\s+ds_"), vmem=cnt(r"^\s+(buffer|global|scratch)_"),
                   salu=cnt(r"^\s+s_(?!waitcnt|barrier|nop)"), wait=cnt(r"^\s+s_waitcnt"), bar=cnt(r"^\s+s_barrier"))
        print(f"{d[:90]:90s} agpr {r[1]:>3s} vgpr {r[2]:>3s} sgpr {r[3]:>3s} spill {r[4]:>3s} scratch {r[5]:>4s} | "
              + " ".join(f"{k} {v}" for k, v in mix.items()))


if __name__ == "__main__":
    main()
