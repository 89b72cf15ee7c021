"""CPU-side checks of Dht::searchStep on the resident searches (dhtgpu_srs_*,
opendht_amd/csrc/srstep.hip): literal expectations written from the reference (src/dht.cpp:562-654,
src/search.h) against the model the GPU tests rely on; that every script reaches the edge it is named
for; header, exports and binding of the srs family; the kernels' register and scratch budget (with
rsearch.hip's and srmap.hip's under the wider row); and the C++ adapter's host check.  No GPU needed."""
import os
import re
import subprocess

import numpy as np
import pytest

import cpp_check
import kernel_budget as KB
import opendht_amd
import rsearch_cases as RS
import srstep_cases as SS
from srstep_cases import B_DONE, B_EXPIRED, B_REFILLED, B_SKIPPED, B_SYNCED, E, u32

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NOW = 1000


# ---- literal expectations ---------------------------------------------------------------------------
def one_search(state=None):
    return SS.start(1, 800, state)


def stepped(sc, now=NOW):
    """one step of slot 0 at `now`: (handles sent, out4 row)"""
    sc.add("clock", now)
    send, out4 = sc.add("step", u32([0]), E, 0)
    n = int(out4[0, 0])
    assert (send[0, n:] == SS.NONE).all()
    return [int(h) for h in send[0, :n]], [int(x) for x in out4[0]]


def replied_list(sc, ticks):
    """8 good entries 10..17 at distances 1..8, entry i replied (a token) at ticks[i] and its request completed"""
    for i, t in enumerate(ticks):
        sc.add("clock", t)
        sc.fill(0, [10 + i], [1 + i], token=1)
    sc.add("request", u32([0] * 8), u32(range(10, 18)), 2)


def test_three_good_entries_are_all_asked():
    sc = one_search()
    sc.fill(0, [10, 11, 12], [1, 2, 3])
    assert stepped(sc) == ([10, 11, 12], [3, 3, 0, 0])


def test_six_good_entries_the_first_four_are_asked():
    sc = one_search()
    sc.fill(0, range(10, 16), range(1, 7))
    assert stepped(sc) == ([10, 11, 12, 13], [4, 4, 0, 0])
    assert stepped(sc, NOW + 1) == ([], [0, 4, 0, 0])      # four pending: currentlySolicitedNodeCount() == 4


def test_candidates_are_asked_and_not_counted():
    """[cand, good, cand, good, good, good, good], no node expired: searchSendGetValues goes on until four
    non-bad entries are pending -- entries 0-5"""
    sc = one_search()
    sc.fill(0, range(10, 17), range(1, 8))
    sc.add("candidate", u32([0, 0]), u32([10, 12]), 1)
    assert stepped(sc) == ([10, 11, 12, 13, 14, 15], [6, 4, 0, 0])


def test_synced_search_is_done_and_then_skipped():
    sc = one_search()
    replied_list(sc, [400] * 8)
    assert stepped(sc) == ([], [0, 0, 0, B_SYNCED | B_DONE])      # 400 + 600 >= 1000
    req, tick = sc.model.entries([0])
    assert not req.any() and (tick[0, :8] == 400).all()           # setDone() cleared getStatus
    assert stepped(sc, NOW + 1) == ([], [0, 0, 0, B_SKIPPED | B_DONE])


def test_one_stale_reply_breaks_the_sync_and_is_asked_again():
    sc = one_search()
    replied_list(sc, [400, 400, 400, 400, 400, 399, 400, 400])
    assert stepped(sc) == ([15], [1, 1, 0, 0])                    # 399 + 600 < 1000; the others: now > 1000 fails


def test_empty_list_expires():
    sc = one_search()
    assert stepped(sc) == ([], [0, 0, 0, B_EXPIRED | B_DONE])


BAD = list(range(100, 125))


def bad_state():
    st = np.zeros(200, np.uint8)
    st[BAD] = 1
    return st


def test_25_leading_bad_of_26_expires():
    sc = one_search(bad_state())
    sc.fill(0, BAD + [10], range(1, 27))
    assert sc.model.status([0])[0].tolist() == [26, 25, 25, 0]
    assert stepped(sc) == ([10], [1, 0, 0, B_EXPIRED | B_DONE])   # (the request goes out before the expiry test)
    assert sc.model.status([0])[0].tolist() == [0, 0, 0, 1]


def test_24_entries_all_bad_expires():
    sc = one_search(bad_state())
    sc.fill(0, BAD[:24], range(1, 25))
    assert stepped(sc) == ([], [0, 0, 0, B_EXPIRED | B_DONE])


def test_24_leading_bad_of_30_does_not_expire():
    sc = one_search(bad_state())
    sc.fill(0, BAD[:24] + list(range(10, 16)), range(1, 31))
    assert sc.model.status([0])[0].tolist() == [30, 24, 24, 0]
    assert stepped(sc) == ([10, 11, 12, 13], [4, 4, 0, 0])


# ---- every script reaches its edge ------------------------------------------------------------------
@pytest.fixture(scope="module")
def scripts():
    return dict(SS.all_scripts())


def rows(sc):
    """out4 of every step, flattened: [(slot, out4 row)]"""
    return [(int(s), [int(x) for x in r[1][i]]) for st, r in zip(sc.steps, sc.results) if st[0] == "step"
            for i, s in enumerate(st[1])]


def test_tick_edge_reaches_equality_both_ways(scripts):
    sc = scripts["tick_edge"]
    assert rows(sc) == [(0, [0, 0, 0, B_SYNCED | B_DONE]), (2, [1, 1, 0, 0]),            # now == tick + E
                        (1, [4, 4, 0, 0]), (2, [3, 4, 0, 0]), (0, [0, 0, 0, B_SKIPPED | B_DONE])]   # one tick later
    assert [int(x) for x in SS.steps_of(sc)[0][0][1, :1]] == [10]
    assert set(sc.model.tick[1].values()) == {400} and sc.model.clock == 400 + E + 1


def test_wrap_reaches_the_top_of_the_clock(scripts):
    sc = scripts["wrap"]
    assert sc.model.clock == 0xFFFFFFFF
    assert max(sc.model.tick[0].values()) + E > 0xFFFFFFFF       # a 32-bit sum would wrap
    assert rows(sc) == [(1, [1, 1, 0, 0]), (0, [0, 0, 0, B_SYNCED | B_DONE])]
    assert int(SS.steps_of(sc)[0][0][0, 0]) == 10


def test_sol_goes_from_three_to_four(scripts):
    sc = scripts["sol"]
    assert rows(sc) == [(0, [2, 4, 0, 0]), (0, [0, 4, 0, 0])]
    assert [int(x) for x in SS.steps_of(sc)[0][0][0, :2]] == [11, 13]     # the candidate, then one good entry


def test_refill_edges(scripts):
    sc = scripts["refill"]
    r = rows(sc)
    assert r[0][1][3] == B_REFILLED and r[0][1][2] > 0       # 13 good entries: due
    assert r[1][1][2:] == [0, 0]                              # 14: not
    assert r[2][1][2:] == [14, B_REFILLED]                    # empty
    assert r[3][1][2:] == [0, 0]                              # refill_count 0
    assert r[4][1][2:] == [0, 0] and sc.model.rtick[2] == 1601 and sc.steps[-4][1] == 1000 + E   # refill_tick + E == now
    assert r[5][1][3] == B_REFILLED


def test_expiry_edges(scripts):
    sc = scripts["expiry"]
    assert [x[1][3] for x in rows(sc)] == [5, 5, 5, 0, 0, 37, 37, 37]


def test_travel_moves_marked_entries(scripts):
    """marked entries changed position, a removable node left, and the handle trimmed and inserted
    again inside one batch came back fresh"""
    sc = scripts["travel"]
    m = sc.model
    req, tick = m.entries(np.arange(5))
    assert req.any() and tick.any()
    for s in range(5):
        assert 70 not in m.slots[s].row
    moved = [s for s in range(5) for j, h in enumerate(m.slots[s].row)
             if 10 <= h - 1000 * s < 24 and m.tick[s].get(h) and m.req[s].get(h) and j != h - 1000 * s - 10]
    assert len(set(moved)) == 5
    assert [int(x) for x in sc.notes["before"]] == [(12 + 1) % 3, 304]      # entry 22 of slot 4: req 1, tick 304
    assert list(sc.results[sc.notes["batch"]]) == [1, 1, 1, 1]   # 23 back, 83 trims it, 72 trims 22 and leaves, 22 back
    assert 4022 in m.slots[4].row and m.req[4].get(4022, 0) == 0 and m.tick[4].get(4022, 0) == 0
    assert 4023 not in m.slots[4].row and 4072 not in m.slots[4].row


@pytest.mark.parametrize("name", ["traffic7", "traffic64"])
def test_traffic_reaches_every_leg(scripts, name):
    sc = scripts[name]
    r = rows(sc)
    bits = 0
    for _, o in r:
        bits |= o[3]
    want = B_REFILLED | (B_SYNCED | B_DONE | B_SKIPPED | B_EXPIRED if name == "traffic7" else 0)
    assert bits & want == want, bin(bits)
    assert {len(st[1]) for st in sc.steps if st[0] == "step"} >= {1, 4, 5}
    assert any(o[0] > 0 and o[1] == 4 for _, o in r) and any(0 < o[0] < 4 for _, o in r)
    assert {st[0] for st in sc.steps} >= {"request", "insert", "offer", "step", "clock"}


def test_scripts_stay_exact(scripts):
    """no list outgrows rsearch_cases' bound, at most 64 slots, an nc mirror of at most 256 keys"""
    for name, sc in scripts.items():
        assert RS.max_len(sc.model) <= RS.LIST_BOUND and len(sc.model.slots) <= 64, name
        assert not any(sl.over for sl in sc.model.slots), name
        assert len(sc.model.nc.map) <= 256, name


# ---- header, exports and binding --------------------------------------------------------------------
SRS = ["srs_set_clock", "srs_set_request", "srs_step", "srs_step_dev", "srs_entries", "srs_entries_dev"]


def test_srs_header_library_and_binding_agree():
    names = {"dhtgpu_" + s for s in SRS}
    src = open(os.path.join(ROOT, "include", "dhtgpu.h")).read()
    out = subprocess.check_output(["nm", "-D", "--defined-only", opendht_amd.LIB_PATH], text=True)
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    assert set(re.findall(r"^int (dhtgpu_srs_[a-z0-9_]+)\(", src, re.M)) == names
    assert {s for s in exported if s.startswith("dhtgpu_srs_")} == names
    assert {s for s in opendht_amd.exported_symbols() if s.startswith("dhtgpu_srs_")} == names
    L = opendht_amd.lib()
    for s in sorted(names):
        assert s in opendht_amd._SIG and getattr(L, s).argtypes is not None, s
        assert callable(getattr(opendht_amd.Context, s[len("dhtgpu_"):])), s
    top = src[: src.index("Threading")]   # the header block at the top lists the family
    assert "dhtgpu_srs_step " in top and "dhtgpu_srs_set_clock/_set_request/_entries" in top


# ---- the kernels' budget ------------------------------------------------------------------------------
# One wave per search, 8 waves / SIMD: at most 64 VGPRs and no scratch; compiled:
SRSTEP_CAPS = {
    "k_srs_stepE": 64,       # 46  the row, the refill walk's two windows
    "k_srs_requestE": 64,    # 4
    "k_srs_entriesE": 64,    # 6
}


@pytest.mark.skipif(KB.HIPCC is None, reason="hipcc not installed")
def test_kernel_budget_with_the_wider_row():
    from test_kernel_resources import CAPS
    KB.compile_all(["srstep", "rsearch", "srmap"])
    KB.check("srstep", SRSTEP_CAPS)
    KB.check("rsearch", CAPS["rsearch"])
    KB.check("srmap", CAPS["srmap"])


# ---- the C++ adapter ----------------------------------------------------------------------------------
def test_adapter_compiles_as_cxx11_and_host_check(tmp_path):
    """tests/cpp/srstep_check.cpp: ResidentSearches::noteRequest / stepBatch compile as C++11, and the
    check's struct-based searchStep agrees with its literal cases with no device behind it"""
    exe = cpp_check.build("srstep", tmp_path)
    assert subprocess.check_output([exe], text=True).strip() == "built"
    cpp_check.run(exe, ["--host"], "srstep_check (host paths)", 120)
