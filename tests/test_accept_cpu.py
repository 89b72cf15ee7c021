"""CPU-side checks of the accept mask: the register / scratch budget of the view kernels
(opendht_amd/csrc/view.hip, cross-compiled for gfx950) and the C++11 adapter's accept-mask members
(tests/cpp/accept_check.cpp, built against a mock node type; no device is touched)."""
import os
import re
import shutil
import subprocess

import pytest

import opendht_amd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "opendht_amd", "csrc")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


def _usage(path):
    out = subprocess.run([HIPCC, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "--cuda-device-only", "-c",
                          path, "-o", os.devnull, "-Rpass-analysis=kernel-resource-usage"],
                         capture_output=True, text=True, cwd=CSRC, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    kern, res = None, {}
    for line in out.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            kern = m.group(1)
            res[kern] = {}
            continue
        m = re.search(r"(VGPRs|ScratchSize \[bytes/lane\]): (\d+)", line)
        if m and kern:
            res[kern][m.group(1).split()[0]] = int(m.group(2))
    return res


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_view_kernels_no_scratch_and_vgpr_budget():
    """The compaction runs on every mask change: no kernel of view.hip spills, and the compaction
    kernel stays within the 4-waves-per-SIMD step (4 workgroups of 33 KB of LDS per CU)."""
    usage = _usage(os.path.join(CSRC, "view.hip"))
    assert usage, "no kernel resource remarks parsed"
    spills = {k: v["ScratchSize"] for k, v in usage.items() if v.get("ScratchSize", 0)}
    assert not spills, f"kernels spilling to scratch: {spills}"
    compact = [k for k in usage if re.search(r"\dk_view_compactE", k)]
    assert len(compact) == 1, sorted(usage)
    assert usage[compact[0]]["VGPRs"] <= 128, usage[compact[0]]


def build_accept_check(exe):
    src = os.path.join(ROOT, "tests", "cpp", "accept_check.cpp")
    libdir = os.path.dirname(opendht_amd.LIB_PATH)
    subprocess.check_call(["g++", "-std=c++11", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                           src, "-o", exe, "-L", libdir, "-ldhtgpu", "-Wl,-rpath," + libdir])
    return exe


def test_cpp_accept_adapter_compiles(tmp_path):
    """ClosestIndex::set_accept / clear_accept / update_accept / write / set_accept_good compile as
    C++11 with -Wall -Wextra -Werror against a mock node type that has isGood(now)."""
    exe = build_accept_check(str(tmp_path / "accept_check"))
    assert subprocess.check_output([exe], text=True).strip() == "built"


def test_accept_symbols_exported_and_bound():
    """The accept-mask entry points are declared, exported and bound."""
    names = ["dhtgpu_set_accept", "dhtgpu_set_accept_bits_dev", "dhtgpu_update_accept", "dhtgpu_num_accepted",
             "dhtgpu_write_ids"]
    header = open(os.path.join(ROOT, "include", "dhtgpu.h")).read()
    L = opendht_amd.lib()
    for s in names:
        assert re.search(rf"\b{s}\s*\(", header), s
        assert hasattr(L, s) and s in opendht_amd.exported_symbols(), s
    for m in ("set_accept", "update_accept", "write_ids", "set_accept_bits_dev", "num_accepted"):
        assert hasattr(opendht_amd.Context, m), m
