"""CPU-side checks of the growing resident routing table (dhtgpu_rtg_*, opendht_amd/csrc/rtgrow.hip):
the boundary (header, exports, binding, a NULL context), the Python model of tests/rtgrow_cases.py
pinned to the oracle's table in the all-good regime, the model's state rules on hand-made rows, the
kernels' register, scratch and LDS budget, and the C++ adapter's host paths.  No GPU needed."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import opendht_amd
import oracle as O
import rtgrow_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "opendht_amd", "csrc")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
RTG = ["dhtgpu_rtg_on_new_node", "dhtgpu_rtg_expire", "dhtgpu_rtg_set_state", "dhtgpu_rtg_update_state",
       "dhtgpu_rtg_size", "dhtgpu_rtg_export"]
EINVAL = -1


def test_header_library_and_binding_agree():
    src = open(os.path.join(ROOT, "include", "dhtgpu.h")).read()
    declared = set(re.findall(r"^int (dhtgpu_rtg_[a-z0-9_]+)\(", src, re.M))
    assert declared == set(RTG)
    out = subprocess.check_output(["nm", "-D", "--defined-only", opendht_amd.LIB_PATH], text=True)
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    assert set(RTG) <= exported
    assert set(RTG) <= set(opendht_amd.exported_symbols())
    L = opendht_amd.lib()
    for s in RTG:
        assert getattr(L, s).argtypes is not None, s
    for m in ("rtg_on_new_node", "rtg_expire", "rtg_set_state", "rtg_update_state", "rtg_size", "rtg_export"):
        assert callable(getattr(opendht_amd.Context, m)), m
    for name, val in (("NONE", 0), ("KNOWN", 1), ("PLACED", 2), ("REPLACED", 3), ("FULL", 4), ("UNAPPLIED", 5)):
        assert re.search(rf"^#define DHTGPU_RTG_{name} {val}\b", src, re.M), name
        assert getattr(opendht_amd, "RTG_" + name) == val == getattr(C, "RTG_" + name)
    assert re.search(r"^#define DHTGPU_RTG_MAX_HANDLE 65536u", src, re.M) and opendht_amd.RTG_MAX_HANDLE == 65536


def test_null_context_is_einval():
    L = opendht_amd.lib()
    b20 = (ctypes.c_uint8 * 20)()
    u8 = ctypes.cast(b20, ctypes.POINTER(ctypes.c_uint8))
    w = (ctypes.c_uint32 * 16)()
    u32 = ctypes.cast(w, ctypes.POINTER(ctypes.c_uint32))
    assert L.dhtgpu_rtg_on_new_node(None, u8, u32, u8, None, 1, 0, u8, u32, u32) == EINVAL
    assert L.dhtgpu_rtg_expire(None, u32, u32) == EINVAL
    assert L.dhtgpu_rtg_set_state(None, u8, 1) == EINVAL
    assert L.dhtgpu_rtg_update_state(None, u32, u8, 1) == EINVAL
    assert L.dhtgpu_rtg_size(None, u32, u32) == EINVAL
    assert L.dhtgpu_rtg_export(None, u8, u32, u8, u32, u8) == EINVAL


# ---- the model is pinned by the oracle ------------------------------------------------------------
def model_equals_oracle(myid, ids, client):
    res, (firsts, off, nodes) = C.oracle_run(myid, ids, client)
    m = C.Model(myid, client)
    got, aux = m.batch(ids, np.arange(ids.shape[0]))
    assert set(got.tolist()) <= {C.RTG_PLACED, C.RTG_FULL} and np.all(aux == C.NONE)
    assert np.array_equal((got == C.RTG_PLACED).astype(np.uint8), res)
    f, o, x, h, st = m.export()
    assert np.array_equal(f, firsts) and np.array_equal(o, off) and np.array_equal(x, nodes)
    assert [bytes(ids[j]) for j in h] == [bytes(r) for r in nodes]
    assert np.diff(off).max() <= 8
    assert m.stat() == (firsts.shape[0], nodes.shape[0], firsts.shape[0] - 1)
    return firsts.shape[0], nodes.shape[0]


@pytest.mark.parametrize("client", [0, 1])
@pytest.mark.parametrize("n", C.SIZES)
def test_model_equals_oracle_on_uniform_ids(client, n):
    shapes = [model_equals_oracle(*C.uniform(seed, n), client) for seed in C.SEEDS]
    nbs, nns = C.SHAPES[(client, n)]
    assert tuple(s[0] for s in shapes) == nbs and tuple(s[1] for s in shapes) == nns


def test_the_client_runs_cross_a_round_of_find_bucket():
    assert all(nb > 64 for nb in C.SHAPES[(1, 2000)][0])


@pytest.mark.parametrize("client", [0, 1])
@pytest.mark.parametrize("shuffle", [False, True])
def test_model_equals_oracle_on_the_deep_chain(client, shuffle):
    myid, ids = C.deep_chain(shuffle=shuffle)
    if client:
        ids = np.concatenate([ids, O.gen_ids(1, 2000)])
    nb, nn = model_equals_oracle(myid, ids, client)
    assert nb > 128


# ---- the model's state rules, on rows small enough to check by eye ---------------------------------
def test_model_state_rules():
    myid = bytes([0x80] + [0] * 19)
    far = [bytes([i + 1] + [0] * 19) for i in range(9)]          # the other side of bit 0
    m = C.Model(myid)
    for h in range(8):
        assert m.on_new_node(far[h], h, C.EXPIRED if h in (6, 2) else C.GOOD) == (C.RTG_PLACED, C.NONE)
    assert m.buckets == [[7, 6, 5, 4, 3, 2, 1, 0]]
    assert m.on_new_node(far[8], 8) == (C.RTG_REPLACED, 6) and m.buckets == [[7, 8, 5, 4, 3, 2, 1, 0]]
    assert m.on_new_node(far[6], 9, 0) == (C.RTG_REPLACED, 2) and m.buckets == [[7, 8, 5, 4, 3, 9, 1, 0]]
    assert 6 not in m.ids and 2 not in m.state
    assert m.on_new_node(far[6], 9) == (C.RTG_KNOWN, C.NONE)
    # node 9 is not good, but the table has one bucket: the split goes ahead, and reverses the row
    assert m.on_new_node(bytes([0xC0] + [0] * 19), 10) == (C.RTG_PLACED, C.NONE)
    assert m.firsts == [bytes(20), myid] and m.buckets == [[0, 1, 9, 3, 4, 5, 8, 7], [10]]
    # a full bucket that is not mine: FULL, the ping pick is the first not-good node without a pending message
    assert m.on_new_node(far[2], 11) == (C.RTG_FULL, 9)
    m.update_state([9, 3], [C.PENDING, 0])
    assert m.on_new_node(far[2], 11) == (C.RTG_FULL, 3)
    m.update_state([3], [C.PENDING])
    assert m.on_new_node(far[2], 11) == (C.RTG_FULL, C.NONE)
    m.update_state([4], [C.EXPIRED])
    assert m.expire() == [4] and m.buckets[0] == [0, 1, 9, 3, 5, 8, 7] and m.stat() == (2, 8, 1)
    # dubious blocks the split of my bucket once there are two buckets
    mine = [bytes([0x80 | (0x40 >> k)] + [h] + [0] * 18) for k, h in zip((0, 0, 0, 1, 1, 2, 2), range(20, 27))]
    for h, x in zip(range(20, 27), mine):
        assert m.on_new_node(x, h, C.GOOD if h != 23 else 0) == (C.RTG_PLACED, C.NONE)
    assert len(m.buckets[1]) == 8
    assert m.on_new_node(bytes([0x81] + [0] * 19), 30) == (C.RTG_FULL, 23) and m.stat()[0] == 2
    m.update_good([23], [1])
    assert m.on_new_node(bytes([0x81] + [0] * 19), 30) == (C.RTG_PLACED, C.NONE) and m.stat()[0] > 2


def test_model_stops_at_256_buckets():
    firsts = np.zeros((256, 20), np.uint8)
    firsts[:, 0] = np.arange(256)
    myid = np.array([77] + [1] * 19, np.uint8)
    nodes = np.zeros((8, 20), np.uint8)
    nodes[:, 0] = 77
    nodes[:, 1] = np.arange(8)
    off = np.zeros(257, np.uint32)
    off[78:] = 8
    m = C.Model.from_table(myid, firsts, off, nodes)
    x = np.zeros((3, 20), np.uint8)
    x[:, 0] = (5, 77, 6)
    x[:, 2] = 9
    res, aux = m.batch(x, [100, 101, 102])
    assert res.tolist() == [C.RTG_PLACED, C.RTG_UNAPPLIED, C.RTG_UNAPPLIED] and m.stat() == (256, 9, 0)


# ---- the kernels' budget --------------------------------------------------------------------------
# mangled-name fragment -> max VGPRs, each a few registers above the figure this compile prints
# (beside it).  The two table kernels run as one workgroup, so their cap guards against a spill, not
# for occupancy; the three one-thread-per-entry kernels keep 8 waves / SIMD.
VGPR_CAPS = {
    "k_rtgILb0E": 64,          # 59  onNewNode batch
    "k_rtgILb1E": 36,          # 31  expireBuckets
    "k_rtg_set_stateE": 12,    # 6
    "k_rtg_updateE": 12,       # 6
    "k_rtg_handlesE": 10,      # 4
}
LDS_MAX = 160 * 1024           # one gfx950 workgroup; the table kernels hold 100,416 B


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_rtgrow_kernels_no_scratch_lds_and_vgpr_budget():
    out = subprocess.run([HIPCC, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "--cuda-device-only", "-c",
                          os.path.join(CSRC, "rtgrow.hip"), "-o", os.devnull, "-Rpass-analysis=kernel-resource-usage"],
                         capture_output=True, text=True, cwd=CSRC, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    kern, usage = None, {}
    for line in out.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            kern = m.group(1)
            usage[kern] = {}
            continue
        m = re.search(r"(VGPRs|ScratchSize \[bytes/lane\]|LDS Size \[bytes/block\]): (\d+)", line)
        if m and kern:
            usage[kern][m.group(1).split()[0]] = int(m.group(2))
    assert usage, "no kernel resource remarks parsed"
    spills = {k: v["ScratchSize"] for k, v in usage.items() if v.get("ScratchSize", 0)}
    assert not spills, f"kernels using scratch: {spills}"
    seen = set()
    for k, v in usage.items():
        frags = [f for f in VGPR_CAPS if re.search(rf"\d{f}", k)]
        assert len(frags) == 1, f"{k}: a kernel of rtgrow.hip without a cap"
        seen.add(frags[0])
        assert v["VGPRs"] <= VGPR_CAPS[frags[0]], f"{k}: {v['VGPRs']} VGPRs > {VGPR_CAPS[frags[0]]}"
        assert v["LDS"] <= LDS_MAX, f"{k}: {v['LDS']} B of LDS"
    assert seen == set(VGPR_CAPS), f"kernels not found: {set(VGPR_CAPS) - seen}"
    assert max(v["LDS"] for v in usage.values()) > 64 * 1024   # the table kernels' LDS is static: the remark counts it


# ---- the C++ adapter --------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def rtgrow_check(tmp_path_factory):
    """tests/cpp/rtgrow_check.cpp built as C++11 with -Wall -Wextra -Werror against the mock table shape"""
    exe = str(tmp_path_factory.mktemp("rtgrow") / "rtgrow_check")
    libdir = os.path.dirname(opendht_amd.LIB_PATH)
    odir = os.path.join(ROOT, "oracle")
    subprocess.check_call(["make", "-s", "-C", odir])
    subprocess.check_call(["g++", "-std=c++11", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "rtgrow_check.cpp"), "-o", exe, "-L", libdir, "-ldhtgpu",
                           "-L", odir, "-loracle", "-Wl,-rpath," + libdir, "-Wl,-rpath," + odir])
    return exe


def test_adapter_compiles_as_cxx11(rtgrow_check):
    assert subprocess.check_output([rtgrow_check], text=True).strip() == "built"


@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_adapter_host_table_agrees_with_the_model(rtgrow_check, tmp_path, seed):
    """The mock table that stands for the caller's own in the adapter check (onNewNode, split,
    expireBuckets written after the reference in C++) gives the model's results and the model's
    table on a random walk: what the device is compared with in --run is the model's behaviour."""
    myid, ops = C.random_walk(seed, steps=40)
    client = seed % 2
    m = C.Model(myid, client)
    blob = [np.uint32(client).tobytes(), bytes(myid)]
    want, nops = [], 0
    for op in ops:
        if op[0] == "new":
            res, aux = m.batch(op[1], op[2], op[3])
            for j in range(len(res)):
                blob.append(b"\0" + bytes(op[1][j]) + np.uint32(op[2][j]).tobytes() + bytes([op[3][j]]))
                want.append(f"new {res[j]} {-1 if aux[j] == C.NONE else aux[j]}")
                nops += 1
        elif op[0] == "expire":
            m.expire()
            blob.append(b"\1")
            want.append("expire")
            nops += 1
        elif op[0] == "update":
            m.update_state(op[1], op[2])
            for h, v in zip(op[1], op[2]):
                blob.append(b"\2" + np.uint32(h).tobytes() + bytes([v]))
                nops += 1
    blob.insert(2, np.uint32(nops).tobytes())
    for first, row in zip(m.firsts, m.buckets):
        want.append(" ".join([first.hex()] + [f"{h}:{m.state[h]}" for h in row]))
    path = str(tmp_path / "ops.bin")
    open(path, "wb").write(b"".join(blob))
    out = subprocess.run([rtgrow_check, "--host", path], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    assert out.stdout.split("\n")[:-1] == want
