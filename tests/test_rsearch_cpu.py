"""CPU-side checks of the resident searches (dhtgpu_sr_*, opendht_amd/csrc/rsearch.hip): the boundary
(header, exports, binding, null context), the model the GPU tests rely on -- against an independent
Python insertNode, on the case that separates the cache's walk order from distance order, and its
list bound on every case -- the C++ adapter's host path, queues and slot free list against the
oracle, and the kernels' register and scratch budget.  No GPU needed."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import ncache_cases as NC
import opendht_amd
import rsearch_cases as RS
from test_oracle import py_insert_node

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "opendht_amd", "csrc")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
SRS = ["dhtgpu_sr_reset", "dhtgpu_sr_open", "dhtgpu_sr_expire", "dhtgpu_sr_set_state", "dhtgpu_sr_update_state",
       "dhtgpu_sr_set_candidate", "dhtgpu_sr_insert", "dhtgpu_sr_insert_dev", "dhtgpu_sr_refill", "dhtgpu_sr_refill_dev",
       "dhtgpu_sr_status", "dhtgpu_sr_status_dev", "dhtgpu_sr_lists", "dhtgpu_sr_lists_dev"]
EINVAL = -1


def test_header_library_and_binding_agree():
    src = open(os.path.join(ROOT, "include", "dhtgpu.h")).read()
    declared = set(re.findall(r"^int (dhtgpu_sr_[a-z0-9_]+)\(", src, re.M))
    assert declared == set(SRS)
    assert re.search(r"^#define DHTGPU_SR_CAP 64u$", src, re.M) and RS.CAP == 64 and opendht_amd.SR_CAP == 64
    out = subprocess.check_output(["nm", "-D", "--defined-only", opendht_amd.LIB_PATH], text=True)
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    assert set(SRS) <= exported
    assert set(SRS) <= set(opendht_amd.exported_symbols())
    L = opendht_amd.lib()
    for s in SRS:
        assert getattr(L, s).argtypes is not None, s
        assert callable(getattr(opendht_amd.Context, s[len("dhtgpu_"):])), s


def test_null_context_is_einval():
    L = opendht_amd.lib()
    b20 = (ctypes.c_uint8 * 20)()
    u8 = ctypes.cast(b20, ctypes.POINTER(ctypes.c_uint8))
    w = (ctypes.c_uint32 * 64)()
    u32 = ctypes.cast(w, ctypes.POINTER(ctypes.c_uint32))
    o = (ctypes.c_uint64 * 2)()
    u64 = ctypes.cast(o, ctypes.POINTER(ctypes.c_uint64))
    assert L.dhtgpu_sr_reset(None, 4) == EINVAL
    assert L.dhtgpu_sr_open(None, u32, u8, 1) == EINVAL
    assert L.dhtgpu_sr_expire(None, u32, 1) == EINVAL
    assert L.dhtgpu_sr_set_state(None, u8, 1) == EINVAL
    assert L.dhtgpu_sr_update_state(None, u32, u8, 1) == EINVAL
    assert L.dhtgpu_sr_set_candidate(None, u32, u32, u8, 1) == EINVAL
    assert L.dhtgpu_sr_insert(None, u32, 1, u64, u32, u8, u8, u8) == EINVAL
    assert L.dhtgpu_sr_insert_dev(None, None, 0, None, None, None, 0, None, None, None) == EINVAL
    assert L.dhtgpu_sr_refill(None, u32, 1, 14, u32) == EINVAL
    assert L.dhtgpu_sr_refill_dev(None, None, 0, 14, None, None) == EINVAL
    assert L.dhtgpu_sr_status(None, u32, 1, u32) == EINVAL
    assert L.dhtgpu_sr_status_dev(None, None, 0, None, None) == EINVAL
    assert L.dhtgpu_sr_lists(None, u32, 1, u32, u8, u32) == EINVAL
    assert L.dhtgpu_sr_lists_dev(None, None, 0, None, None, None, None) == EINVAL


# ---- the model ------------------------------------------------------------------------------------
class _State:
    """handle -> state byte with the model's default"""
    def __init__(self, d):
        self.d = d

    def __getitem__(self, h):
        return self.d.get(int(h), 0)


class PyModel(RS.Model):
    """The model with its insert replaced by the independent Python insertNode of test_oracle.py
    (big integers, Python lists), handles used directly as node names."""
    def insert(self, slots, ins_off, ins_handle, ins_ids, ins_token=None):
        off = [int(x) for x in ins_off]
        tot = off[-1]
        handle = [int(h) for h in np.asarray(ins_handle).reshape(-1)[:tot]]
        for h, k in zip(handle, RS.as_ids(ins_ids)[:tot]):
            self.ids[h] = bytes(k)
        added = np.zeros(tot, np.uint8)
        st = _State(self.state)
        for j, s in enumerate(slots):
            sl = self.slots[int(s)]
            for i in range(off[j], off[j + 1]):
                a, sl.expired = py_insert_node(self.ids, st, sl.target, sl.row, sl.flags, sl.expired, handle[i],
                                               bool(ins_token[i]) if ins_token is not None else False)
                added[i] = a
        return added


SCRIPTS = RS.all_exact_scripts()


def same_state(a, b, what):
    slots = np.arange(len(a.slots))
    for x, y, nm in zip(a.lists(slots) + (a.status(slots),), b.lists(slots) + (b.status(slots),),
                        ("rows", "flags", "lens", "status")):
        assert np.array_equal(x, y), f"{what}: {nm} differ"


@pytest.mark.parametrize("name", [n for n, s in SCRIPTS if s[0][1] <= 40])
def test_model_matches_python_insert_node(name):
    """Every step of the small-set scripts on the oracle-backed model and on the Python one: the
    same rows, flags, lengths, status words and return values."""
    script = dict(SCRIPTS)[name]
    a, b = RS.Model(), PyModel()
    for k, step in enumerate(script):
        wa, _ = RS.run_step(step, a)
        wb, _ = RS.run_step(step, b)
        assert (wa is None and wb is None) or np.array_equal(wa, wb), f"{name} step {k} {step[0]}: results differ"
        same_state(a, b, f"{name} step {k} {step[0]}")


def test_every_exact_case_stays_under_the_row():
    """No exact case overflows: every list of every script stays within SEARCH_NODES + MAX_BAD = 54
    entries after every step; the pre-fill of the 700-slot shapes leaves lists of 13, 14, 15 and
    >= 50 entries; a second refill of the refill shapes inserts nothing."""
    seen = set()
    for name, script in SCRIPTS:
        m = RS.Model()
        last_refill = None
        for k, step in enumerate(script):
            want, _ = RS.run_step(step, m)
            assert RS.max_len(m) <= RS.LIST_BOUND, f"{name} step {k}: a list of {RS.max_len(m)}"
            assert not any(sl.over for sl in m.slots)
            if name.startswith("insert") and step[0] == "insert" and script[k - 1][0] != "insert" and k < 6:
                seen |= {len(sl.row) for sl in m.slots}     # after the pre-fill
            if step[0] == "refill" and name.startswith("refill"):
                if last_refill is not None:
                    assert not want.any(), f"{name}: the second refill inserted {want}"
                last_refill = want
    assert {13, 14, 15} <= seen and max(seen) >= 50, sorted(seen)


def test_refill_inserts_in_walk_order_not_distance_order():
    """On ncache_cases.non_monotone() a refill of 3 offers the walk's nodes -- the keys 0000.., 1000..,
    1001.. -- where a kernel that sorts the cache by distance would offer 0000.., 1111.., 1110..: the
    lists differ, so such a kernel fails the GPU test."""
    keys, target = NC.non_monotone()
    m = RS.Model()
    for step in RS.non_monotone_script(count=3):
        RS.run_step(step, m)
    key_of = {h: k for k, h in m.nc.map.items()}
    got = [key_of[h][0] >> 4 for h in m.slots[0].row]
    assert sorted(got) == [0x0, 0x8, 0x9]
    acc = np.ones(keys.shape[0], np.uint8)
    skeys = m.nc.sorted()[0]
    by_distance = [skeys[i][0] >> 4 for i in NC.distance_sorted(skeys, acc, target[0], 3)]
    assert sorted(by_distance) == [0x0, 0xE, 0xF]
    t = NC.key_int(target[0])
    assert [NC.key_int(key_of[h]) ^ t for h in m.slots[0].row] == sorted(NC.key_int(key_of[h]) ^ t for h in m.slots[0].row)


# ---- the C++ adapter --------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def rsearch_check(tmp_path_factory):
    """tests/cpp/rsearch_check.cpp built as C++11 with -Wall -Wextra -Werror against mock Search types"""
    exe = str(tmp_path_factory.mktemp("rsearch") / "rsearch_check")
    libdir = os.path.dirname(opendht_amd.LIB_PATH)
    odir = os.path.join(ROOT, "oracle")
    subprocess.check_call(["make", "-s", "-C", odir])
    subprocess.check_call(["g++", "-std=c++11", "-O2", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "rsearch_check.cpp"), "-o", exe, "-L", libdir, "-ldhtgpu",
                           "-L", odir, "-loracle", "-Wl,-rpath," + libdir, "-Wl,-rpath," + odir])
    return exe


def test_adapter_compiles_as_cxx11(rsearch_check):
    assert subprocess.check_output([rsearch_check], text=True).strip() == "built"


def test_adapter_host_path_queues_and_free_list(rsearch_check):
    """What ResidentSearches runs below its device threshold (cached_nodes_host + insertNode)
    against the oracle, its queues and its slot free list."""
    out = subprocess.run([rsearch_check, "--host"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "(host paths): 0 mismatches" in out.stdout, out.stdout + out.stderr


# mangled-name fragment -> max VGPRs.  One wave per search: every kernel is built for 8 waves / SIMD,
# i.e. at most 64 VGPRs, the occupancy step at or above what the compiler reports; compiled:
VGPR_CAPS = {
    "k_sr_insertE": 64,       # 32
    "k_sr_refillE": 64,       # 43  the walk's two windows + the row
    "k_sr_openE": 64,         # 20
    "k_sr_expireE": 64,       # 4
    "k_sr_candidateE": 64,    # 5
    "k_sr_statusE": 64,       # 6
    "k_sr_listsE": 64,        # 6
}   # (update_state's byte setter: prims.hip, capped in test_ncache_cpu.py)


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_rsearch_kernels_no_scratch_and_vgpr_budget():
    out = subprocess.run([HIPCC, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "--cuda-device-only", "-c",
                          os.path.join(CSRC, "rsearch.hip"), "-o", os.devnull, "-Rpass-analysis=kernel-resource-usage"],
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
        assert len(frags) == 1, f"{k}: a kernel of rsearch.hip without a cap"
        seen.add(frags[0])
        assert v["VGPRs"] <= VGPR_CAPS[frags[0]], f"{k}: {v['VGPRs']} VGPRs > {VGPR_CAPS[frags[0]]}"
    assert seen == set(VGPR_CAPS), f"kernels not found: {set(VGPR_CAPS) - seen}"
