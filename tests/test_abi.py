"""CPU-side checks of the drop-in boundary: libdhtgpu.so loads and exports every
entry point include/dhtgpu.h declares (no compute calls -- no GPU here)."""
import ctypes
import os
import re
import subprocess

import pytest

import cpp_check
import ncache_cases
import opendht_amd
import rsearch_cases
import rtgrow_cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header_symbols():
    src = open(os.path.join(ROOT, "include", "dhtgpu.h")).read()
    return sorted(set(re.findall(r"\b(dhtgpu_[a-z0-9_]+)\s*\(", src)))


def test_library_built():
    assert os.path.exists(opendht_amd.LIB_PATH), "run __graft_entry__.build() first"


def test_exports_match_header():
    syms = header_symbols()
    assert len(syms) >= 15
    out = subprocess.check_output(["nm", "-D", "--defined-only", opendht_amd.LIB_PATH], text=True)
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    missing = [s for s in syms if s not in exported]
    assert not missing, missing
    assert sorted(opendht_amd.exported_symbols()) == syms


def test_ctypes_load_and_strerror():
    L = opendht_amd.lib()
    for s in header_symbols():
        assert hasattr(L, s)
    assert L.dhtgpu_strerror(0) == b"ok"
    assert L.dhtgpu_strerror(-5).startswith(b"id set holds duplicate")


@pytest.fixture(scope="module")
def adapter_check(tmp_path_factory):
    return cpp_check.build("adapter", tmp_path_factory.mktemp("adapter"))


def test_cpp_adapter_header_compiles(adapter_check):
    """The C++11 host adapter (include/dhtgpu.hpp) compiles as C++11 against a
    reference-shaped mock table (tests/cpp/adapter_check.cpp)."""
    assert subprocess.check_output([adapter_check], text=True).strip() == "built"


def test_cpp_adapter_host_walks(adapter_check):
    """The adapter's host walks -- what a single findClosestNodes / getCachedNodes runs below the
    device threshold -- give the oracle's nodes in the oracle's order (no GPU needed)."""
    cpp_check.run(adapter_check, ["--host"], "adapter_check (host walks)", 120)


# ---- header, exports and binding, family by family ------------------------------------------------
# family -> (prefix, entry points without "dhtgpu_", pinned #defines: name -> (text in the header, value)).
# Under a prefix the header declares exactly these names; every entry point is exported, bound with
# argument types, and has a Context method of its name.  (accept: no prefix of its own.)
FAMILIES = {
    "accept": (None, ["set_accept", "set_accept_bits_dev", "update_accept", "num_accepted", "write_ids"], {}),
    "rt": ("rt_", ["rt_set", "rt_set_good", "rt_update_good", "rt_find_closest_dev", "rt_find_closest", "rt_reply_dev",
                   "rt_reply", "rt_closer_dev", "rt_closer"], {}),
    "rtg": ("rtg_", ["rtg_on_new_node", "rtg_expire", "rtg_set_state", "rtg_update_state", "rtg_size", "rtg_export"],
            {"RTG_NONE": ("0", 0), "RTG_KNOWN": ("1", 1), "RTG_PLACED": ("2", 2), "RTG_REPLACED": ("3", 3),
             "RTG_FULL": ("4", 4), "RTG_UNAPPLIED": ("5", 5), "RTG_MAX_HANDLE": ("65536u", 65536)}),
    "nc": ("nc_", ["nc_set", "nc_insert", "nc_erase", "nc_update_accept", "nc_set_accept", "nc_size", "nc_export",
                   "nc_nodes_dev", "nc_nodes"], {"NC_MAX_HANDLE": ("(1u << 28)", 1 << 28)}),
    "ncr": ("ncr_", ["ncr_find", "ncr_find_dev", "ncr_get_nodes", "ncr_extract"], {}),
    "sr": ("sr_", ["sr_reset", "sr_open", "sr_expire", "sr_set_state", "sr_update_state", "sr_set_candidate", "sr_insert",
                   "sr_insert_dev", "sr_refill", "sr_refill_dev", "sr_status", "sr_status_dev", "sr_lists",
                   "sr_lists_dev"], {"SR_CAP": ("64u", 64)}),
    "srm": ("srm_", ["srm_set", "srm_set_done", "srm_offer", "srm_offer_dev", "srm_export"], {}),
}
# the Python mirrors of the pinned values: the binding's and the case modules'
MIRRORS = {"RTG_MAX_HANDLE": [opendht_amd.RTG_MAX_HANDLE], "NC_MAX_HANDLE": [ncache_cases.MAX_HANDLE],
           "SR_CAP": [opendht_amd.SR_CAP, rsearch_cases.CAP]}
MIRRORS.update({"RTG_" + r: [getattr(opendht_amd, "RTG_" + r), getattr(rtgrow_cases, "RTG_" + r)]
                for r in ("NONE", "KNOWN", "PLACED", "REPLACED", "FULL", "UNAPPLIED")})


@pytest.mark.parametrize("family", list(FAMILIES))
def test_header_library_and_binding_agree(family):
    prefix, short, defines = FAMILIES[family]
    names = {"dhtgpu_" + s for s in short}
    src = open(os.path.join(ROOT, "include", "dhtgpu.h")).read()
    out = subprocess.check_output(["nm", "-D", "--defined-only", opendht_amd.LIB_PATH], text=True)
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    if prefix:
        assert set(re.findall(rf"^int (dhtgpu_{prefix}[a-z0-9_]+)\(", src, re.M)) == names
        assert {s for s in exported if s.startswith("dhtgpu_" + prefix)} == names
        assert {s for s in opendht_amd.exported_symbols() if s.startswith("dhtgpu_" + prefix)} == names
    L = opendht_amd.lib()
    for s in sorted(names):
        assert re.search(rf"\b{s}\s*\(", src), s
        assert s in exported and s in opendht_amd._SIG and hasattr(L, s), s
        assert getattr(L, s).argtypes is not None, s
        method = getattr(opendht_amd.Context, s[len("dhtgpu_"):])
        assert callable(method) or (s == "dhtgpu_num_accepted" and isinstance(method, property)), s
    for name, (text, val) in defines.items():
        assert re.search(rf"^#define DHTGPU_{name} {re.escape(text)}(?: +/\*.*\*/)?$", src, re.M), name
        assert MIRRORS[name] == [val] * len(MIRRORS[name]), name


# ---- a null context ---------------------------------------------------------------------------------
# Entry points that are not asked for DHTGPU_EINVAL on a null context: why.
_NO_CTX = "takes no context"
NO_NULL_CONTEXT_STATUS = {
    "dhtgpu_ctx_destroy": "returns nothing (destroying no context is allowed)",
    "dhtgpu_ctx_stream": "returns the stream, not a status",
    "dhtgpu_num_ids": "returns a count, not a status",
    "dhtgpu_sub_handles_active": "returns a flag, not a status",
    "dhtgpu_batch_plan": "a null context is allowed: the plan of the default configuration (tests/test_route_model.py)",
    "dhtgpu_strerror": _NO_CTX,
    "dhtgpu_device_count": _NO_CTX,
    "dhtgpu_ctx_create": _NO_CTX + ": it makes one",
    "dhtgpu_merge_dev": _NO_CTX + ": its first parameter is a device pointer",
    "dhtgpu_merge_ties_dev": _NO_CTX + ": its first parameter is a device pointer",
    "dhtgpu_pack_dev": _NO_CTX + ": its first parameter is a device pointer",
    "dhtgpu_classify_dev": _NO_CTX + ": its first parameter is a device pointer",
    "dhtgpu_gen_dev": _NO_CTX,
    "dhtgpu_table_depth": _NO_CTX,
}
NULL_CONTEXT_ENTRIES = [n for n in opendht_amd._SIG if n not in NO_NULL_CONTEXT_STATUS]
_INTS = (ctypes.c_int, ctypes.c_uint32, ctypes.c_uint64)


def test_every_entry_point_is_called_with_a_null_context_or_excluded():
    """By the header, not by the binding (where a device pointer and the context are both void*):
    every entry point whose first parameter is the dhtgpu_ctx* and that answers a status is called
    below; an excluded one either takes no context or has its reason, and no exclusion is stale."""
    src = open(os.path.join(ROOT, "include", "dhtgpu.h")).read()
    takes_ctx = set(re.findall(r"\b(dhtgpu_[a-z0-9_]+)\s*\(\s*(?:const\s+)?dhtgpu_ctx\*", src))
    assert set(NO_NULL_CONTEXT_STATUS) <= set(opendht_amd._SIG)
    for n, why in NO_NULL_CONTEXT_STATUS.items():
        assert (n not in takes_ctx) == why.startswith(_NO_CTX), n
    assert set(NULL_CONTEXT_ENTRIES) == {n for n in takes_ctx if n not in NO_NULL_CONTEXT_STATUS}
    assert all(opendht_amd._SIG[n][1] is ctypes.c_int for n in NULL_CONTEXT_ENTRIES)


@pytest.mark.parametrize("name", NULL_CONTEXT_ENTRIES)
def test_null_context_is_einval(name):
    """A null context with otherwise plausible arguments -- a small host buffer for every host pointer,
    1 for every integer, null for every device pointer and stream -- is DHTGPU_EINVAL, before any
    device call (no GPU here)."""
    args, _ = opendht_amd._SIG[name]
    keep, call = [], [None]
    for a in args[1:]:
        if a in _INTS:
            call.append(1)
        elif a is ctypes.c_void_p:
            call.append(None)
        else:   # a host pointer
            keep.append((ctypes.c_uint64 * 64)())
            call.append(ctypes.cast(keep[-1], a))
    assert getattr(opendht_amd.lib(), name)(*call) == opendht_amd.EINVAL


def test_table_depth_vs_oracle():
    """Host-side helper of the C ABI (no device work): RoutingTable::depth."""
    import numpy as np
    import oracle as O
    import opendht_amd
    for seed in (1, 2, 3):
        firsts, _, _ = O.Table(O.gen_ids(seed, 1)[0]).grow(O.gen_ids(seed + 10, 20000)).export()
        for b in range(firsts.shape[0]):
            assert opendht_amd.table_depth(firsts, b) == O.depth(firsts, b)
    assert opendht_amd.table_depth(np.zeros((0, 20), np.uint8), 0) == 0


def test_host_units_keep_their_family_state():
    """The C ABI's host layer is one unit per entry-point family, and a family's
    state in the context is its unit's alone: c->rt in api_rtable.hip, c->sr in api_rsearch.hip,
    c->nc in api_ncache.hip -- but for the one documented crossing, the resident searches' refill,
    which reads nc.valid and nc.view().  Each unit has its static helpers first and then exactly
    one extern "C" block."""
    csrc = os.path.join(ROOT, "opendht_amd", "csrc")
    units = {fn: open(os.path.join(csrc, fn)).read() for fn in sorted(os.listdir(csrc))
             if re.fullmatch(r"api\w*\.hip", fn)}
    assert set(units) == {"api.hip", "api_batch.hip", "api_dht.hip", "api_rtable.hip", "api_ncache.hip", "api_rsearch.hip"}

    def users(member):
        return {fn for fn, src in units.items() if re.search(r"->" + member + r"\b", src)}

    assert users("rt") == {"api_rtable.hip"}
    assert users("sr") == {"api_rsearch.hip"}
    assert users("nc") == {"api_ncache.hip", "api_rsearch.hip"}
    crossing = re.findall(r"->nc\b(.{0,8})", units["api_rsearch.hip"])
    assert crossing and all(re.match(r"\.(valid\b|view\(\))", x) for x in crossing), crossing
    for fn, src in units.items():
        assert src.count('extern "C" {') == 1, fn
        assert src.rstrip().endswith('}  // extern "C"'), fn   # nothing stands behind the block


def test_production_build_has_no_measurement_switches():
    """The shipped library cannot return different nodes (SURVEY §8(b) error contract): the
    sources carry no result-altering measurement macro (#if/#ifdef on a DHT_* name), the Makefile
    takes no extra defines and builds gfx950 only, and DHTGPU_DBG is masked at context creation to
    the diagnostics bits that leave results unchanged (phase stamps; K6 instead of KS for small
    batches -- both exact; tests/test_gpu_parity.py::test_dbg_bits_leave_results_unchanged)."""
    csrc = os.path.join(ROOT, "opendht_amd", "csrc")
    bad = []
    for fn in sorted(os.listdir(csrc)):
        if not fn.endswith((".hip", ".h", ".cpp")):
            continue
        for no, line in enumerate(open(os.path.join(csrc, fn)), 1):
            if re.match(r"\s*#\s*(if|ifdef|ifndef|elif)\b.*\bDHT_[A-Z0-9_]+", line):
                bad.append(f"{fn}:{no}: {line.strip()}")
    assert not bad, bad
    mk = open(os.path.join(csrc, "Makefile")).read()
    assert "EXTRA" not in mk and "$(error" in mk and "ifneq ($(ARCH),gfx950)" in mk
    internal = open(os.path.join(csrc, "dhtgpu_internal.h")).read()
    m = re.search(r"constexpr uint32_t kDbgAllowed = ([^;]+);", internal)
    assert m and m.group(1).replace(" ", "") == "256u|(1u<<23)", m
    api = open(os.path.join(csrc, "api.hip")).read()
    assert re.search(r'getenv\("DHTGPU_DBG"\)\)\s*c->dbg = .*& kDbgAllowed;', api)
    batch = open(os.path.join(csrc, "batch.hip")).read()
    assert "c.dbg & 256u" in batch   # K6 honours the stamp bit only
