"""CPU-side checks of the resident routing table (dhtgpu_rt_*, opendht_amd/csrc/rtable.hip): the
boundary (header, exports, binding, argument errors), the C++ adapter's host paths against the
oracle, the table snapshots the GPU tests rely on, the kernel's walk rule restated on the CPU, and
the kernels' register and scratch budget.  No GPU needed."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import opendht_amd
import oracle as O
import rtable_cases as RC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "opendht_amd", "csrc")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
RT = ["dhtgpu_rt_set", "dhtgpu_rt_set_good", "dhtgpu_rt_update_good", "dhtgpu_rt_find_closest_dev",
      "dhtgpu_rt_find_closest", "dhtgpu_rt_reply_dev", "dhtgpu_rt_reply", "dhtgpu_rt_closer_dev", "dhtgpu_rt_closer"]
EINVAL = -1


def test_header_library_and_binding_agree():
    src = open(os.path.join(ROOT, "include", "dhtgpu.h")).read()
    declared = set(re.findall(r"^int (dhtgpu_rt_[a-z0-9_]+)\(", src, re.M))
    assert declared == set(RT)
    out = subprocess.check_output(["nm", "-D", "--defined-only", opendht_amd.LIB_PATH], text=True)
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    assert set(RT) <= exported
    assert set(RT) <= set(opendht_amd.exported_symbols())
    L = opendht_amd.lib()
    for s in RT:
        assert getattr(L, s).argtypes is not None, s
    for m in ("rt_set", "rt_set_good", "rt_update_good", "rt_find_closest", "rt_reply", "rt_closer",
              "rt_find_closest_dev", "rt_reply_dev", "rt_closer_dev"):
        assert callable(getattr(opendht_amd.Context, m)), m


def test_null_context_is_einval():
    L = opendht_amd.lib()
    b20 = (ctypes.c_uint8 * 20)()
    u8 = ctypes.cast(b20, ctypes.POINTER(ctypes.c_uint8))
    w = (ctypes.c_uint32 * 16)()
    u32 = ctypes.cast(w, ctypes.POINTER(ctypes.c_uint32))
    assert L.dhtgpu_rt_set(None, u8, 0, None, None, None, None, 0, 0) == EINVAL
    assert L.dhtgpu_rt_set_good(None, u8) == EINVAL
    assert L.dhtgpu_rt_update_good(None, u32, u8, 1) == EINVAL
    assert L.dhtgpu_rt_find_closest(None, u8, 1, 8, u32, u32) == EINVAL
    assert L.dhtgpu_rt_reply(None, u8, 1, u8, u32, None) == EINVAL
    assert L.dhtgpu_rt_closer(None, u8, 1, 8, 1, u8, None) == EINVAL
    assert L.dhtgpu_rt_find_closest_dev(None, None, 0, 0, 8, None, None, None) == EINVAL
    assert L.dhtgpu_rt_reply_dev(None, None, 0, 0, None, None, None, None) == EINVAL
    assert L.dhtgpu_rt_closer_dev(None, None, 0, 0, 8, 1, None, None, None) == EINVAL


@pytest.fixture(scope="module")
def rtable_check(tmp_path_factory):
    """tests/cpp/rtable_check.cpp built as C++11 with -Wall -Wextra -Werror against the mock table shape"""
    exe = str(tmp_path_factory.mktemp("rtable") / "rtable_check")
    libdir = os.path.dirname(opendht_amd.LIB_PATH)
    odir = os.path.join(ROOT, "oracle")
    subprocess.check_call(["make", "-s", "-C", odir])
    subprocess.check_call(["g++", "-std=c++11", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "rtable_check.cpp"), "-o", exe, "-L", libdir, "-ldhtgpu",
                           "-L", odir, "-loracle", "-Wl,-rpath," + libdir, "-Wl,-rpath," + odir])
    return exe


def test_adapter_compiles_as_cxx11(rtable_check):
    assert subprocess.check_output([rtable_check], text=True).strip() == "built"


def test_adapter_host_replies_and_closeness(rtable_check):
    """What ResidentTable runs below its device threshold: replies (findClosestNodes + the packed
    records) and both closeness tests against the oracle on a grown table, af 4 and af 6."""
    out = subprocess.run([rtable_check, "--host"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "(host paths): 0 mismatches" in out.stdout, out.stdout + out.stderr


def test_oracle_and_host_walk_agree_on_the_synthetic_tables(rtable_check, tmp_path):
    """The GPU tests take the oracle's word on tables no onNewNode grows; here the adapter's
    independent host walk (detail::find_closest_host) gives the same nodes on each of them."""
    cases = RC.synthetic() + RC.ties()
    path = str(tmp_path / "cases.bin")
    RC.dump(cases, path)
    out = subprocess.run([rtable_check, "--tables", path], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and f"{len(cases)} cases, 0 mismatches" in out.stdout, out.stdout + out.stderr


def walk_slice(firsts, off, good, target, count):
    """rtable.hip's findBucket and outward walk restated: the node slice [lo, hi) it selects from."""
    f = [bytes(x) for x in firsts]
    nb = len(f)
    gpre = np.concatenate([[0], np.cumsum([int(np.count_nonzero(good[off[b]: off[b + 1]])) for b in range(nb)])])
    j = max([b for b in range(1, nb) if f[b] <= bytes(target)], default=0)
    rmax = max(j, nb - j)
    rs = next(r for r in range(1, rmax + 1) if r >= rmax or gpre[min(nb, j + r)] - gpre[max(0, j - r)] >= count)
    return int(off[max(0, j - rs)]), int(off[min(nb, j + rs)])


def test_walk_rule_matches_the_reference_walk():
    """The smallest r whose bucket range holds `count` good nodes (else the whole table) is where
    the reference's round-by-round walk stops: the closest good nodes of that slice are the
    oracle's answer -- on grown tables and on runs of empty buckets longer than 64."""
    cases = RC.synthetic()
    for cluster in (False, True):
        _, firsts, off, nodes, tg = RC.grown(cluster)
        cases += [RC.case(f"grown_{cluster}_{fr}", firsts, off, nodes, RC.good_mask(nodes.shape[0], fr), tg[::5])
                  for fr in RC.FRACTIONS]
    for c in cases:
        ints = [int.from_bytes(bytes(r), "big") for r in c["nodes"]]
        for count in c["counts"]:
            want, wcnt = RC.expected(c, count)
            for qi, t in enumerate(c["targets"]):
                lo, hi = walk_slice(c["firsts"], c["off"], c["good"], t, count)
                ti = int.from_bytes(bytes(t), "big")
                got = sorted((ints[i] ^ ti, i) for i in range(lo, hi) if c["good"][i])[:count]
                assert [i for _, i in got] == list(want[qi, : wcnt[qi]]), (c["name"], count, qi)


# mangled-name fragment -> max VGPRs.  Every k_rt instantiation is built for 8 waves / SIMD (one
# wave per target: occupancy is what hides the dependent loads), i.e. at most 64 VGPRs; compiled:
VGPR_CAPS = {
    "k_rtILi0ELj8E": 64,     # 18  indices, K = 8
    "k_rtILi0ELj16E": 64,    # 18  indices, K = 16
    "k_rtILi0ELj32E": 64,    # 21  indices, K = 32
    "k_rtILi1ELj8E": 64,     # 18  reply (count 8 only)
    "k_rtILi2ELj8E": 64,     # 17  closer, K = 8
    "k_rtILi2ELj16E": 64,    # 17  closer, K = 16
    "k_rtILi2ELj32E": 64,    # 20  closer, K = 32
    "k_rt_gpreE": 64,        # 42
}   # (update_good's byte setter: prims.hip, capped in test_ncache_cpu.py)


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_rtable_kernels_no_scratch_and_vgpr_budget():
    out = subprocess.run([HIPCC, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "--cuda-device-only", "-c",
                          os.path.join(CSRC, "rtable.hip"), "-o", os.devnull, "-Rpass-analysis=kernel-resource-usage"],
                         capture_output=True, text=True, cwd=CSRC, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    kern, usage = None, {}
    for line in out.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            kern = m.group(1)
            usage[kern] = {}
            continue
        m = re.search(r"(VGPRs|ScratchSize \[bytes/lane\]): (\d+)", line)
        if m and kern:
            usage[kern][m.group(1).split()[0]] = int(m.group(2))
    assert usage, "no kernel resource remarks parsed"
    spills = {k: v["ScratchSize"] for k, v in usage.items() if v.get("ScratchSize", 0)}
    assert not spills, f"kernels using scratch: {spills}"
    seen = set()
    for k, v in usage.items():
        frags = [f for f in VGPR_CAPS if re.search(rf"\d{f}", k)]
        assert len(frags) == 1, f"{k}: a kernel of rtable.hip without a cap"
        seen.add(frags[0])
        assert v["VGPRs"] <= VGPR_CAPS[frags[0]], f"{k}: {v['VGPRs']} VGPRs > {VGPR_CAPS[frags[0]]}"
    assert seen == set(VGPR_CAPS), f"kernels not found: {set(VGPR_CAPS) - seen}"
