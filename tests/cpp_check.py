"""Build and run the C++11 adapter checks (tests/cpp/<name>_check.cpp over include/dhtgpu.hpp): one
flag set and one success rule for the CPU modules (build, --host) and the GPU modules (--run)."""
import os
import re
import subprocess

import opendht_amd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAGS = ["-std=c++11", "-O2", "-Wall", "-Wextra", "-Werror"]
NO_ORACLE = ("accept",)    # compares with a brute force of its own


def build(name, dir):
    """tests/cpp/<name>_check.cpp -> dir/<name>_check, linked with libdhtgpu and (but for NO_ORACLE) the oracle"""
    exe = os.path.join(str(dir), name + "_check")
    libdir = os.path.dirname(opendht_amd.LIB_PATH)
    link, rpath = ["-L", libdir, "-ldhtgpu"], ["-Wl,-rpath," + libdir]
    if name not in NO_ORACLE:
        odir = os.path.join(ROOT, "oracle")
        subprocess.check_call(["make", "-s", "-C", odir])
        link += ["-L", odir, "-loracle"]
        rpath.append("-Wl,-rpath," + odir)
    subprocess.check_call(["g++", *FLAGS, "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", name + "_check.cpp"), "-o", exe, *link, *rpath])
    return exe


def run_for_line(exe, args, line, timeout):
    """exit status 0 and one whole output line equal to `line`; returns the output"""
    out = subprocess.run([exe, *args], capture_output=True, text=True, timeout=timeout)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    assert re.search(rf"^{re.escape(line)}$", out.stdout, re.M), out.stdout + out.stderr
    return out.stdout


def run(exe, args, label, timeout):
    return run_for_line(exe, args, f"{label}: 0 mismatches", timeout)
