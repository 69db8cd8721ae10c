#!/usr/bin/env python3
"""Build tools/f0_track_sizes_check.cpp with the address and undefined-behaviour sanitizers, run it on
the CPU (it compares csrc/f0_track_sizes.h with a 128-bit restatement of the same formula over sizes
up to INT32_MAX) and compare every line it prints with the Python mirror in fs2amd/_lib.py (the
workspace bytes and the LDS bytes of fs2_f0_track). Exit status 0 and "ok" mean: the same numbers
everywhere, and nothing reported by either sanitizer.

    python tools/f0_track_sizes_check.py [--cxx g++]
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
    sanitize=False builds the same program without the sanitizers (tests/test_f0_track_host.py: the
    comparison alone, with no sanitizer runtime needed where the suite runs)."""
    L = mirror()
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "f0_track_sizes_check")
        san = "-fsanitize=address,undefined"
        flags = [] if not sanitize else ["-Xarch_host", san] if os.path.basename(cxx).startswith("hipcc") else [san]
        if sanitize:
            flags.append("-fno-sanitize-recover=all")
        subprocess.run([cxx, "-O1", "-g", "-std=c++17", *flags,
                        f"-I{os.path.join(REPO, 'include')}", f"-I{os.path.join(PKG, 'csrc')}",
                        os.path.join(REPO, "tools", "f0_track_sizes_check.cpp"), "-o", exe], check=True)
        run = subprocess.run([exe], capture_output=True, text=True)
    if run.returncode != 0 or run.stderr.strip():
        sys.exit(f"the program failed (exit {run.returncode}):\n{run.stderr[-4000:]}")
    n_lines = 0
    for line in run.stdout.splitlines():
        kind, *rest = line.split()
        a = [int(v) for v in rest if v != "->"]
        if kind == "W":
            B, F, tau_min, tau_max, N, cap, nbytes = a
            want = (L.f0_track_cap(tau_min, tau_max), L.f0_track_workspace_bytes(B, F, tau_min, tau_max, N))
            got = (cap, nbytes)
        else:
            N, K, lds = a
            want, got = (L.f0_track_lds_bytes(N, K),), (lds,)
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
