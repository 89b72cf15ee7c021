"""CPU-side checks of the resident NodeCache (dhtgpu_nc_*, opendht_amd/csrc/ncache.hip): the boundary
(header, exports, binding, argument errors), the C++ adapter's host path and slot bookkeeping
against the oracle, the model the GPU tests rely on checked against itself, and the kernels'
register and scratch budget.  No GPU needed."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import ncache_cases as NC
import opendht_amd
import oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "opendht_amd", "csrc")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
NCS = ["dhtgpu_nc_set", "dhtgpu_nc_insert", "dhtgpu_nc_erase", "dhtgpu_nc_update_accept", "dhtgpu_nc_set_accept",
       "dhtgpu_nc_size", "dhtgpu_nc_export", "dhtgpu_nc_nodes_dev", "dhtgpu_nc_nodes"]
EINVAL = -1


def test_header_library_and_binding_agree():
    src = open(os.path.join(ROOT, "include", "dhtgpu.h")).read()
    declared = set(re.findall(r"^int (dhtgpu_nc_[a-z0-9_]+)\(", src, re.M))
    assert declared == set(NCS)
    assert re.search(r"^#define DHTGPU_NC_MAX_HANDLE \(1u << 28\)$", src, re.M) and NC.MAX_HANDLE == 1 << 28
    out = subprocess.check_output(["nm", "-D", "--defined-only", opendht_amd.LIB_PATH], text=True)
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    assert set(NCS) <= exported
    assert set(NCS) <= set(opendht_amd.exported_symbols())
    L = opendht_amd.lib()
    for s in NCS:
        assert getattr(L, s).argtypes is not None, s
    for m in ("nc_set", "nc_insert", "nc_erase", "nc_update_accept", "nc_set_accept", "nc_size", "nc_export",
              "nc_nodes", "nc_nodes_dev"):
        assert callable(getattr(opendht_amd.Context, m)), m


def test_null_context_is_einval():
    L = opendht_amd.lib()
    b20 = (ctypes.c_uint8 * 20)()
    u8 = ctypes.cast(b20, ctypes.POINTER(ctypes.c_uint8))
    w = (ctypes.c_uint32 * 16)()
    u32 = ctypes.cast(w, ctypes.POINTER(ctypes.c_uint32))
    n = ctypes.c_uint64(0)
    assert L.dhtgpu_nc_set(None, u8, None, 1) == EINVAL
    assert L.dhtgpu_nc_insert(None, u8, u32, None, 1, None) == EINVAL
    assert L.dhtgpu_nc_erase(None, u8, 1, None) == EINVAL
    assert L.dhtgpu_nc_update_accept(None, u32, u8, 1) == EINVAL
    assert L.dhtgpu_nc_set_accept(None, u8, 1) == EINVAL
    assert L.dhtgpu_nc_size(None, ctypes.byref(n)) == EINVAL
    assert L.dhtgpu_nc_export(None, u8, u32) == EINVAL
    assert L.dhtgpu_nc_nodes(None, u8, 1, 8, u32, u32) == EINVAL
    assert L.dhtgpu_nc_nodes_dev(None, None, 0, 0, 8, None, None, None) == EINVAL


@pytest.fixture(scope="module")
def ncache_check(tmp_path_factory):
    """tests/cpp/ncache_check.cpp built as C++11 with -Wall -Wextra -Werror against the mock map shape"""
    exe = str(tmp_path_factory.mktemp("ncache") / "ncache_check")
    libdir = os.path.dirname(opendht_amd.LIB_PATH)
    odir = os.path.join(ROOT, "oracle")
    subprocess.check_call(["make", "-s", "-C", odir])
    subprocess.check_call(["g++", "-std=c++11", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "ncache_check.cpp"), "-o", exe, "-L", libdir, "-ldhtgpu",
                           "-L", odir, "-loracle", "-Wl,-rpath," + libdir, "-Wl,-rpath," + odir])
    return exe


def test_adapter_compiles_as_cxx11(ncache_check):
    assert subprocess.check_output([ncache_check], text=True).strip() == "built"


def test_adapter_host_path_and_slot_bookkeeping(ncache_check):
    """What ResidentCache runs below its device threshold (the host walk, expired weak_ptrs
    included) against the oracle, and its slots and free list through insert, erase, re-insert
    into a freed slot."""
    out = subprocess.run([ncache_check, "--host"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "(host paths): 0 mismatches" in out.stdout, out.stdout + out.stderr


# ---- the model against itself ---------------------------------------------------------------------
def py_walk(keys, accept, target, count):
    """NodeCache::getCachedNodes (src/node_cache.cpp:42-74) restated in Python over sorted keys:
    sorted positions in walk order"""
    ints = [NC.key_int(k) for k in keys]
    t = NC.key_int(target)
    n = len(ints)
    nxt = next((i for i, k in enumerate(ints) if k >= t), n)
    prv = nxt - 1
    out = []
    while len(out) < count and (nxt < n or prv >= 0):
        if prv < 0:
            it, nxt = nxt, nxt + 1
        elif nxt >= n:
            it, prv = prv, prv - 1
        elif ints[prv] ^ t < ints[nxt] ^ t:
            it, prv = prv, prv - 1
        else:
            it, nxt = nxt, nxt + 1
        if accept[it]:
            out.append(it)
    return out


def test_non_monotone_case_separates_walk_from_distance_sort():
    """On the 4-bit-prefix keys the oracle's row is the head-comparison walk (0000, 1000, 1001, ...),
    which a sort by XOR distance does not give: a sort-based kernel fails the GPU test."""
    keys, target = NC.non_monotone()
    model = NC.Model()
    model.set(keys)
    skeys, sh = model.sorted()
    acc = np.ones(len(sh), np.uint8)
    for count in (3, 8, 32):
        want, wcnt = model.expected(target, count)
        walk = py_walk(skeys, acc, target[0], count)
        assert list(want[0, : wcnt[0]]) == [int(sh[i]) for i in walk]
        assert walk[:3] == [0, 1, 2]
        assert NC.distance_sorted(skeys, acc, target[0], count) != walk
    assert NC.distance_sorted(skeys, acc, target[0], 3) == [0, len(sh) - 1, len(sh) - 2]


def test_model_lookup_matches_the_python_walk():
    """model.expected (the oracle + the handle map) against the Python restatement: random keys with
    permuted handles, clustered keys, every accept kind"""
    keys = O.gen_ids(41, 300)
    handles = (np.random.default_rng(1).permutation(900)[:300] + 5).astype(np.uint32)
    ckeys, ctargets = NC.clustered()
    for ks, hs, tg in ((keys, handles, NC.targets_for(keys, 2)), (ckeys, None, ctargets)):
        model = NC.Model()
        model.set(ks, hs)
        skeys, sh = model.sorted()
        for kind in NC.ACCEPTS:
            model.acc = NC.accept_handles(kind, sh)
            acc = [int(h) in model.acc for h in sh]
            for count in (1, 14):
                want, wcnt = model.expected(tg, count)
                for qi, t in enumerate(tg):
                    walk = py_walk(skeys, acc, t, count)
                    assert list(want[qi, : wcnt[qi]]) == [int(sh[i]) for i in walk], (kind, count, qi)
                    assert (want[qi, wcnt[qi]:] == NC.NONE).all()


def test_model_mutations():
    """emplace / erase in batch order: a present key keeps its handle and its accept bit, of equal
    keys in a batch the first wins, a repeated erase finds nothing"""
    keys = O.gen_ids(42, 10)
    model = NC.Model()
    model.set(keys[:4])
    model.update_accept([1], 0)
    ids = np.stack([keys[1], keys[5], keys[5], keys[6]])
    new = model.insert(ids, [50, 51, 52, 53], [1, 0, 1, 1])
    assert list(new) == [0, 1, 0, 1]
    assert model.map[bytes(keys[1])] == 1 and model.map[bytes(keys[5])] == 51
    assert 1 not in model.acc and 51 not in model.acc and 53 in model.acc and 50 not in model.acc
    found = model.erase(np.stack([keys[0], keys[9], keys[0]]))
    assert list(found) == [1, 0, 0]
    skeys, sh = model.sorted()
    assert [bytes(k) for k in skeys] == sorted(bytes(k) for k in keys[[1, 2, 3, 5, 6]])
    empty = NC.Model()
    out, cnt = empty.expected(keys[:2], 8)
    assert (out == NC.NONE).all() and not cnt.any()
    ids, handles, accept = NC.mutation_batch(model, 63, 3, 100)
    assert bytes(ids[62]) == bytes(ids[0]) and not ids[1].any() and (ids[2] == 0xFF).all()
    assert sum(bytes(k) in model.map for k in ids) >= 1


# mangled-name fragment -> max VGPRs.  One wave per target (k_nc) and streaming passes: every
# kernel is built for 8 waves / SIMD, i.e. at most 64 VGPRs, the next occupancy step above what
# the compiler reports; compiled:
VGPR_CAPS = {
    "k_ncE": 64,              # 33  the lookup
    "k_nc_rankILb0E": 64,     # 20  insert
    "k_nc_rankILb1E": 64,     # 20  erase
    "k_nc_compactE": 64,      # 14
    "k_nc_mergeILb0E": 64,    # 16  insert
    "k_nc_mergeILb1E": 64,    # 11  erase
    "k_nc_handlesE": 64,      # 6
    "k_nc_bits_packE": 64,    # 15
}
# the shared primitives' kernels (prims.hip), which took over the scan of the block counts and the
# indexed setters of the nc, rt and sr families under the same cap
PRIMS_VGPR_CAPS = {
    "k_scan_rowsIjE": 64,     # 12  u32 totals
    "k_scan_rowsIyE": 64,     # 12  u64 totals
    "k_bits_updateE": 64,     # 9
    "k_bytes_updateE": 64,    # 8
}


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_ncache_kernels_no_scratch_and_vgpr_budget():
    check_unit_budget("ncache.hip", VGPR_CAPS)


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_prims_kernels_no_scratch_and_vgpr_budget():
    check_unit_budget("prims.hip", PRIMS_VGPR_CAPS)


def check_unit_budget(unit, caps):
    out = subprocess.run([HIPCC, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "--cuda-device-only", "-c",
                          os.path.join(CSRC, unit), "-o", os.devnull, "-Rpass-analysis=kernel-resource-usage"],
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
        frags = [f for f in caps if re.search(rf"\d{f}", k)]
        assert len(frags) == 1, f"{k}: a kernel of {unit} without a cap"
        seen.add(frags[0])
        assert v["VGPRs"] <= caps[frags[0]], f"{k}: {v['VGPRs']} VGPRs > {caps[frags[0]]}"
    assert seen == set(caps), f"kernels not found: {set(caps) - seen}"
