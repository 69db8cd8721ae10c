#!/usr/bin/env python3
"""Build tools/iir_sizes_check.cpp with the address and undefined-behaviour sanitizers, run it on the
CPU (it compares csrc/iir_sizes.h with the definitions of the block counts, a 128-bit restatement of the
workspace size and the status tables of include/fs2hip_iir.h) and compare every line it prints with the
Python mirror in fs2amd/_lib.py (iir_blocks, iir_chunks, loudness_blocks, loudness_workspace_bytes,
iir_status, loudness_status, gain_status). Exit status 0 and "ok" mean: the same numbers everywhere, and
nothing reported by either sanitizer.

    python tools/iir_sizes_check.py [--cxx g++]
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
    sanitize=False builds the same program without the sanitizers (tests/test_loudness_host.py: the
    comparison alone, with no sanitizer runtime needed where the suite runs)."""
    L = mirror()
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "iir_sizes_check")
        san = "-fsanitize=address,undefined"
        flags = [] if not sanitize else ["-Xarch_host", san] if os.path.basename(cxx).startswith("hipcc") else [san]
        if sanitize:
            flags.append("-fno-sanitize-recover=all")
        subprocess.run([cxx, "-O1", "-g", "-std=c++17", *flags,
                        f"-I{os.path.join(REPO, 'include')}", f"-I{os.path.join(PKG, 'csrc')}",
                        os.path.join(REPO, "tools", "iir_sizes_check.cpp"), "-o", exe], check=True)
        run = subprocess.run([exe], capture_output=True, text=True)
    if run.returncode != 0 or run.stderr.strip():
        sys.exit(f"the program failed (exit {run.returncode}):\n{run.stderr[-4000:]}")
    n_lines = 0
    for line in run.stdout.splitlines():
        kind, *rest = line.split()
        a = [int(v) for v in rest if v != "->"]
        if kind == "K":
            want, got = (L.iir_blocks(a[0]), L.iir_chunks(a[0])), (a[1], a[2])
        elif kind == "J":
            want, got = L.loudness_blocks(a[0], a[1]), a[2]
        elif kind == "W":
            want, got = L.loudness_workspace_bytes(a[0], a[1], a[2]), a[3]
        elif kind == "S":
            want, got = L.iir_status(a[0], a[1], a[2], a[3]), a[4]
        elif kind == "L":
            want, got = L.loudness_status(a[0], a[1], a[2]), a[3]
        else:  # G
            want, got = L.gain_status(a[0], a[1], a[2]), a[3]
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
