#!/usr/bin/env python3
"""Compare the kernels of two device assembly files, function by function.

  hipcc --offload-arch=gfx950 -O3 -std=c++17 ... --cuda-device-only -S a.hip -o a.s   (and b.s)
  tools/asm_compare.py a.s b.s [--rename 'REGEX=REPL' ...] [--resources a.remarks b.remarks]

A function body is normalised before the comparison: `;` comments and blank lines dropped, the
ordinals of .LBB<n>_ block labels dropped (they count functions, so they move when one is added) and
every mangled function name replaced by a placeholder. Functions are paired by demangled name;
--rename rewrites the names of the FIRST file (re.sub, applied in order) where a refactor renamed
them. --resources takes the stderr of the same compiles with -Rpass-analysis=kernel-resource-usage
and prints both resource tables. Exit status 1 when a pair differs or a function has no partner.
"""
import argparse
import re
import subprocess
import sys


def demangle(names):
    for tool in ("llvm-cxxfilt", "/opt/rocm/llvm/bin/llvm-cxxfilt", "c++filt"):
        try:
            out = subprocess.run([tool], input="\n".join(names), capture_output=True, text=True, check=True).stdout
            return dict(zip(names, out.split("\n")))
        except (OSError, subprocess.CalledProcessError):
            continue
    return {n: n for n in names}


def short(name):
    name = re.sub(r"\(anonymous namespace\)::", "", name)
    name = re.sub(r"^void ", "", name)
    return re.sub(r"\(.*\)$", "", name)


def functions(path):
    """{mangled name: normalised body lines} of every function of an assembly file"""
    lines = open(path).read().split("\n")
    names = [m.group(1) for l in lines if (m := re.match(r"\s*\.type\s+([\w.$]+),@function", l))]
    out, cur = {}, None
    name_re = re.compile("|".join(sorted(map(re.escape, names), key=len, reverse=True))) if names else None
    for l in lines:
        m = re.match(r"([\w.$]+):", l)
        if m and m.group(1) in names and cur is None:
            cur = m.group(1)
            out[cur] = []
            continue
        if cur is None:
            continue
        if re.match(r"\.Lfunc_end\d+:", l):
            cur = None
            continue
        l = l.split(";")[0].rstrip()
        if not l.strip():
            continue
        l = re.sub(r"\.LBB\d+_", ".LBB_", l)
        out[cur].append(name_re.sub("<fn>", l))
    return out


def resources(path):
    rows, cur = [], None
    for l in open(path):
        m = re.search(r"remark:\s+(.*?):\s+(\S+) \[-Rpass-analysis", l)
        if not m:
            continue
        if m.group(1) == "Function Name":
            cur = {"name": m.group(2)}
            rows.append(cur)
        elif cur is not None:
            cur[m.group(1)] = m.group(2)
    dm = demangle([r["name"] for r in rows])
    cols = [("VGPR", "VGPRs"), ("AGPR", "AGPRs"), ("SGPR", "TotalSGPRs"), ("occ", "Occupancy [waves/SIMD]"),
            ("vspill", "VGPRs Spill"), ("sspill", "SGPRs Spill"), ("scratch", "ScratchSize [bytes/lane]"),
            ("LDS", "LDS Size [bytes/block]")]
    widths = [6, 6, 6, 5, 8, 8, 9, 9]
    print("%-44s" % "kernel" + "".join("%*s" % (w, c[0]) for w, c in zip(widths, cols)))
    for r in rows:
        print("%-44s" % short(dm[r["name"]]) + "".join("%*s" % (w, r.get(c[1], "?")) for w, c in zip(widths, cols)))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("a")
    ap.add_argument("b")
    ap.add_argument("--rename", action="append", default=[], metavar="REGEX=REPL")
    ap.add_argument("--resources", nargs=2, metavar=("A_REMARKS", "B_REMARKS"))
    args = ap.parse_args()
    if args.resources:
        for title, path in zip((args.a, args.b), args.resources):
            print("== " + title)
            resources(path)
            print()
    fa, fb = functions(args.a), functions(args.b)
    da, db = demangle(list(fa)), demangle(list(fb))
    na = {}
    for mangled in fa:
        n = short(da[mangled])
        for r in args.rename:
            pat, repl = r.split("=", 1)
            n = re.sub(pat, repl, n)
        na[n] = mangled
    nb = {short(db[m]): m for m in fb}
    bad = 0
    for n in sorted(set(na) | set(nb)):
        if n not in na or n not in nb:
            print("%-44s only in %s" % (n, args.b if n in nb else args.a))
            bad += 1
            continue
        x, y = fa[na[n]], fb[nb[n]]
        if x == y:
            print("%-44s identical (%d lines)" % (n, len(x)))
        else:
            ndiff = sum(1 for p, q in zip(x, y) if p != q) + abs(len(x) - len(y))
            print("%-44s DIFFERS (%d / %d lines, %d differ in place)" % (n, len(x), len(y), ndiff))
            bad += 1
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
