"""Development aid: per-kernel register / scratch / instruction-mix summary of a hipcc -save-temps .s file.
    hipcc --offload-arch=gfx950 -O3 -std=c++17 -c x.hip -save-temps ; python tools/isa_stats.py x-hip-amdgcn-amd-amdhsa-gfx950.s [filter]
Comparison mode, for a change that must leave the kernels alone (each side: one .s file or several joined by commas, taken together):
    python tools/isa_stats.py --compare before.s[,before2.s] after.s[,after2.s]
compares, per kernel symbol, the instruction text from its label to s_endpgm (local labels renumbered, comments dropped) and the
register / LDS / scratch sizes of the metadata; prints every difference and one summary line, exit status 1 unless identical."""
import re
import subprocess
import sys


def demangle(names):
    try:
        r = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True)
        return r.stdout.strip().split("\n")
    except FileNotFoundError:
        return names


META = ("vgpr_count", "sgpr_count", "group_segment_fixed_size", "private_segment_fixed_size")


def kernels(path):
    """{symbol: (normalised instruction lines, metadata values)} of one .s file"""
    s = open(path).read()
    out = {}
    for e in s[s.find("amdhsa.kernels:"):].split("  - .agpr_count:")[1:]:
        g = lambda k: re.search(r"\." + k + r":\s*(\S+)", e).group(1)
        name = g("name")
        m = re.search(r"^" + re.escape(name) + r":[^\n]*\n(.*?\n\s*s_endpgm)", s, re.S | re.M)
        labels = {}
        renum = lambda l: labels.setdefault(l.group(0), ".L%d" % len(labels))
        lines = [re.sub(r"\.LBB\d+_\d+", renum, ln.split(";")[0].strip()) for ln in (m.group(1) if m else "").split("\n")]
        out[name] = ([ln for ln in lines if ln], tuple(g(k) for k in META))
    return out


def compare(before, after):
    sides, dup = [], []
    for paths in (before, after):
        side = {}
        for path in paths.split(","):
            for name, k in kernels(path).items():
                if name in side:
                    dup.append(name + (" (identical copies)" if side[name] == k else " (DIFFERING copies)"))
                side[name] = k
        sides.append(side)
    a, b = sides
    gone, new = sorted(set(a) - set(b)), sorted(set(b) - set(a))
    diff = [n for n in sorted(set(a) & set(b)) if a[n] != b[n]]
    for tag, names in (("only before", gone), ("only after", new), ("differs", diff), ("defined twice on one side", dup)):
        for n, d in zip(names, demangle(names)):
            print(f"{tag}: {d}" + (f"  text {a[n][0] == b[n][0]} meta {a[n][1]} -> {b[n][1]}" if tag == "differs" else ""))
    same = len(set(a) & set(b)) - len(diff)
    print(f"{before} -> {after}: {len(a)} kernels before, {len(b)} after, {same} identical "
          f"({sum(len(a[n][0]) for n in set(a) & set(b))} instruction lines), {len(diff)} differ, {len(gone)} only before, "
          f"{len(new)} only after, {len(dup)} defined twice on one side")
    return 0 if not (gone or new or diff) else 1


def main():
    if sys.argv[1] == "--compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    s = open(sys.argv[1]).read()
    flt = sys.argv[2] if len(sys.argv) > 2 else None
    md = s[s.find("amdhsa.kernels:"):]
    ents = md.split("  - .agpr_count:")[1:]
    rows = []
    for e in ents:
        g = lambda k: re.search(r"\." + k + r":\s*(\S+)", e).group(1)
        rows.append((g("name"), e.split()[0], g("vgpr_count"), g("sgpr_count"), g("vgpr_spill_count"), g("private_segment_fixed_size")))
    dn = demangle([r[0] for r in rows])
    for r, d in zip(rows, dn):
        d = d.replace("dsim::(anonymous namespace)::", "").replace("void ", "").replace("_ZN4dsim12_GLOBAL__N_1", "").replace("EEvNS_8GemmArgsEi", "")
        if flt and flt not in d:
            continue
        # instruction mix of the kernel body
        m = re.search(r"^" + re.escape(r[0]) + r":[^\n]*\n(.*?)\n\s*s_endpgm", s, re.S | re.M)
        body = m.group(1) if m else ""
        cnt = lambda pat: len(re.findall(pat, body, re.M))
        mix = dict(mfma=cnt(r"^\s+v_mfma"), valu=cnt(r"^\s+v_(?!mfma)"), ds=cnt(r"^\s+ds_"), vmem=cnt(r"^\s+(buffer|global|scratch)_"),
                   salu=cnt(r"^\s+s_(?!waitcnt|barrier|nop)"), wait=cnt(r"^\s+s_waitcnt"), bar=cnt(r"^\s+s_barrier"))
        print(f"{d[:90]:90s} agpr {r[1]:>3s} vgpr {r[2]:>3s} sgpr {r[3]:>3s} spill {r[4]:>3s} scratch {r[5]:>4s} | "
              + " ".join(f"{k} {v}" for k, v in mix.items()))

main()
