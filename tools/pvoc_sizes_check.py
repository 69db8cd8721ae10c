#!/usr/bin/env python3
"""Build tools/pvoc_sizes_check.cpp with the address and undefined-behaviour sanitizers, run it on the
CPU (it compares csrc/pvoc_sizes.h with the definition of the output frame count and a restatement of
the size checks) and compare every line it prints with the Python mirror in fs2amd/_lib.py (pvoc_frames,
pvoc_status). Exit status 0 and "ok" mean: the same numbers everywhere, and nothing reported by either
sanitizer.

    python tools/pvoc_sizes_check.py [--cxx g++]
"""
import argparse
import importlib.util
import os
import subprocess
import sys
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, "expressive-fastspeech2-mandarin_amd")


def mirror():
    """fs2amd/_lib.py alone (it loads no library on import)."""
    spec = importlib.util.spec_from_file_location("_fs2_lib_mirror", os.path.join(PKG, "fs2amd", "_lib.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def check(cxx, sanitize=True):
    """Returns the number of lines compared; raises SystemExit on a mismatch or a sanitizer report.
    sanitize=False builds the same program without the sanitizers (tests/test_pvoc_host.py: the
    comparison alone, with no sanitizer runtime needed where the suite runs)."""
    L = mirror()
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "pvoc_sizes_check")
        san = "-fsanitize=address,undefined"
        flags = [] if not sanitize else ["-Xarch_host", san] if os.path.basename(cxx).startswith("hipcc") else [san]
        if sanitize:
            flags.append("-fno-sanitize-recover=all")
        subprocess.run([cxx, "-O1", "-g", "-std=c++17", *flags,
                        f"-I{os.path.join(REPO, 'include')}", f"-I{os.path.join(PKG, 'csrc')}",
                        os.path.join(REPO, "tools", "pvoc_sizes_check.cpp"), "-o", exe], check=True)
        run = subprocess.run([exe], capture_output=True, text=True)
    if run.returncode != 0 or run.stderr.strip():
        sys.exit(f"the program failed (exit {run.returncode}):\n{run.stderr[-4000:]}")
    n_lines = 0
    for line in run.stdout.splitlines():
        kind, *rest = line.split()
        rest = [v for v in rest if v != "->"]
        if kind == "F":
            want, got = L.pvoc_frames(int(rest[0]), float.fromhex(rest[1])), int(rest[2])
        elif kind == "C":
            *a, rc = [int(v) for v in rest]
            want, got = L.pvoc_status(*a), rc
        else:  # V: rows of 10, 64 and 0 frames at rate 0.5
            J_max, rc = int(rest[0]), int(rest[1])
            fits = max(L.pvoc_frames(T, 0.5) for T in (10, 64, 0)) <= J_max
            want, got = (L.FS2_OK if fits else L.FS2_EINVAL), rc
        if want != got:
            sys.exit(f"mismatch: {line}   Python: {want}")
        n_lines += 1
    return n_lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cxx", default=os.environ.get("CXX", "g++"))
    args = ap.parse_args()
    print(f"ok: {check(args.cxx)} lines agree with the Python mirror; the sanitizers reported nothing")


if __name__ == "__main__":
    main()
