"""CPU-side checks of the resident searches (dhtgpu_sr_*, opendht_amd/csrc/rsearch.hip): the model
the GPU tests rely on -- against an independent Python insertNode, on the case that separates the
cache's walk order from distance order, and its list bound on every case -- and the C++ adapter's
host path, queues and slot free list against the oracle.  No GPU needed.  (Header, exports, binding
and a null context: tests/test_abi.py; the kernels' register and scratch budget:
tests/test_kernel_resources.py.)"""
import subprocess

import numpy as np
import pytest

import cpp_check
import ncache_cases as NC
import rsearch_cases as RS
from test_oracle import py_insert_node


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
    return cpp_check.build("rsearch", tmp_path_factory.mktemp("rsearch"))


def test_adapter_compiles_as_cxx11(rsearch_check):
    assert subprocess.check_output([rsearch_check], text=True).strip() == "built"


def test_adapter_host_path_queues_and_free_list(rsearch_check):
    """What ResidentSearches runs below its device threshold (cached_nodes_host + insertNode)
    against the oracle, its queues and its slot free list."""
    cpp_check.run(rsearch_check, ["--host"], "rsearch_check (host paths)", 120)
