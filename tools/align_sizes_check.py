#!/usr/bin/env python3
"""Build tools/align_sizes_check.cpp with the address and undefined-behaviour sanitizers, run it on
the CPU and compare every line it prints with the Python mirror of csrc/align_sizes.h in
fs2amd/_lib.py (the LDS bytes of fs2_mas with the bitmap in LDS or not, of fs2_forward_sum, the
workspace of the global form, which form a launch takes and what is refused). Exit status 0 and "ok"
mean: the same numbers everywhere, and nothing reported by either sanitizer.

    python tools/align_sizes_check.py [--cxx g++]
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
    sanitize=False builds the same program without the sanitizers (tests/test_align_host.py: the
    comparison alone, with no sanitizer runtime needed where the suite runs)."""
    L = mirror()
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "align_sizes_check")
        san = "-fsanitize=address,undefined"
        flags = [] if not sanitize else ["-Xarch_host", san] if os.path.basename(cxx).startswith("hipcc") else [san]
        if sanitize:
            flags.append("-fno-sanitize-recover=all")
        subprocess.run([cxx, "-O1", "-g", "-std=c++17", *flags,
                        f"-I{os.path.join(REPO, 'include')}", f"-I{os.path.join(PKG, 'csrc')}",
                        os.path.join(REPO, "tools", "align_sizes_check.cpp"), "-o", exe], check=True)
        run = subprocess.run([exe], capture_output=True, text=True)
    if run.returncode != 0 or run.stderr.strip():
        sys.exit(f"the program failed (exit {run.returncode}):\n{run.stderr[-4000:]}")
    n_lines = 0
    for line in run.stdout.splitlines():
        kind, *rest = line.split()
        a = [int(v) for v in rest if v != "->"]
        if kind == "M":
            T, Lx, rows, lds, fs, words = a
            want = (L.mas_lds_bytes(T, Lx, False), L.mas_lds_bytes(T, Lx, True), L.forward_sum_lds_bytes(T, Lx),
                    (Lx + 63) // 64)
            got = (rows, lds, fs, words)
        elif kind == "F":
            T, Lx, bitmap, rc, form = a
            st, fm = L.mas_form(T, Lx, bitmap)
            want, got = (st, -1 if fm is None else fm), (rc, form)
        else:
            B, T, Lx, ws = a
            want, got = (L.mas_ws_bytes(B, T, Lx),), (ws,)
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
