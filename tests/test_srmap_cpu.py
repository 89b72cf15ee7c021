"""CPU-side checks of Dht::trySearchInsert over the resident searches' map (dhtgpu_srm_*,
opendht_amd/csrc/srmap.hip): the model the GPU tests rely on against an independent pure-Python walk
over test_oracle.py's insertNode; the equivalence the kernels are built on -- the filter followed by
the walk of the remaining nodes equals the plain sequential walk, on every case, with and without
removable-not-expired nodes; what the cases must contain; and the C++ adapter's host path.  No GPU
needed.  (Header, exports, binding and a null context: tests/test_abi.py; the kernels' register and
scratch budget, rsearch.hip's pinned kernel set included: tests/test_kernel_resources.py.)"""
import subprocess

import numpy as np
import pytest

import cpp_check
import rsearch_cases as RS
import srmap_cases as SM
from test_oracle import py_insert_node


# ---- the model ----------------------------------------------------------------------------------
SCRIPTS = SM.all_scripts()
NAMES = [n for n, _ in SCRIPTS]


def state_of(m):
    slots = np.arange(len(m.slots))
    return m.lists(slots) + (m.status(slots),)


def same_state(a, b, what):
    for x, y, nm in zip(state_of(a), state_of(b), ("rows", "flags", "lens", "status")):
        assert np.array_equal(x, y), f"{what}: {nm} differ"
    assert a.done == b.done and a.order == b.order, what


class _State:
    def __init__(self, d):
        self.d = d

    def __getitem__(self, h):
        return self.d.get(int(h), 0)


def py_offer(model, handles, ids):
    """trySearchInsert written out again: a sorted list of (target, slot), two plain loops and the
    Python insertNode of test_oracle.py on the model's own rows -- no bisect, no oracle."""
    srs = sorted((model.slots[s].target, s) for s in model.order)
    st = _State(model.state)
    cnt = np.zeros(len(handles), np.uint32)
    for j, (h, k) in enumerate(zip([int(x) for x in handles], RS.as_ids(ids))):
        model.ids[h] = bytes(k)
        c = sum(t < bytes(k) for t, _ in srs)
        for idx in (list(range(c, len(srs))), list(range(c - 1, -1, -1))):
            for i in idx:
                s = srs[i][1]
                sl = model.slots[s]
                added, sl.expired = py_insert_node(model.ids, st, sl.target, sl.row, sl.flags, sl.expired, h, False)
                cnt[j] += added
                if not added and not sl.expired and s not in model.done:
                    break
    return cnt


@pytest.mark.parametrize("name", [n for n in NAMES if n not in ("converged", "shape410", "shape453")])
def test_model_matches_python_walk(name):
    """The model's plain walk (the oracle's insertNode) and the pure-Python one: the same counts and
    the same rows, flags, lengths and status words after every offer."""
    a, b = SM.Model(), SM.Model()
    for k, step in enumerate(dict(SCRIPTS)[name]):
        if step[0] == "offer":
            want = a.offer(step[1], step[2], use_filter=False)[0]
            got = py_offer(b, step[1], step[2])
            assert np.array_equal(want, got), f"{name} step {k}: counts differ"
        else:     # (the pre-fills: the oracle on both sides, compared with Python by test_rsearch_cpu.py)
            SM.run_step(step, a)
            SM.run_step(step, b)
        same_state(a, b, f"{name} step {k} {step[0]}")


@pytest.mark.parametrize("name", NAMES)
def test_filter_then_walk_equals_the_plain_walk(name):
    """The equivalence srmap.hip is built on: answering the nodes between two walls up front (count 0,
    the two cuts) and walking the rest in order gives the plain sequential walk's counts, touched mask
    and lists -- on every case, those that draw state 2 (where the hazard rules apply) included."""
    a, b = SM.Model(), SM.Model()
    for k, step in enumerate(dict(SCRIPTS)[name]):
        wa, _ = SM.run_step(step, a, use_filter=True)
        wb, _ = SM.run_step(step, b, use_filter=False)
        what = f"{name} step {k} {step[0]}"
        if step[0] == "offer":
            assert np.array_equal(wa[0], wb[0]) and np.array_equal(wa[1], wb[1]), f"{what}: results differ"
            assert not wa[2][3] and not wb[2][3], f"{what}: an exact case overflowed"
        same_state(a, b, what)
        assert RS.max_len(a) <= RS.LIST_BOUND, f"{what}: a list of {RS.max_len(a)}"


def test_cases_contain_what_they_are_for():
    """converged: the filter answers most nodes; fresh: every node enters every search; skip_run: a
    walk passes nine refusing searches and inserts beyond them; trim_only: the offer changes lengths
    only; the hazards: a state-2 node in the batch disables the filter, a listed one its search."""
    res = {}
    for name in ("converged", "fresh", "skip_run", "trim_only", "hazard_listed", "hazard_batch"):
        m, offers = SM.Model(), []
        for step in dict(SCRIPTS)[name]:
            before = SM.clone(m) if step[0] == "offer" else None
            w, _ = SM.run_step(step, m)
            if step[0] == "offer":
                offers.append((before, w, SM.clone(m)))
        res[name] = offers
    _, (cnt, _, stats), _ = res["converged"][0]
    assert stats[0] > 0.6 * cnt.size and stats[0] + np.count_nonzero(cnt) <= cnt.size and np.count_nonzero(cnt) > 0
    for _, (cnt, _, stats), _ in res["fresh"][:1]:
        assert (cnt == 65).all() and stats[0] == 0 and stats[1] == 65 * 20
    _, (cnt, touched, stats), after = res["skip_run"][0]
    assert (cnt == 3).all() and stats[1] == 12 * cnt.size and bin(int(touched[0])).count("1") == 3
    before, (cnt, _, stats), after = res["trim_only"][0]
    assert not cnt.any() and stats[0] == cnt.size and stats[1] == 0
    assert [len(s.row) for s in before.slots] == [24] * 4 and [len(s.row) for s in after.slots] == [14] * 4
    _, (_, _, stats), _ = res["hazard_listed"][0]
    assert stats[2] == 0 and stats[1] > 0
    _, (_, _, stats), _ = res["hazard_batch"][0]
    assert stats[2] == 1 and stats[0] == 0
    _, (_, _, stats), _ = res["hazard_batch"][1]
    assert stats[2] == 0 and stats[0] > 0


def test_map_order_and_duplicates():
    m = SM.Model()
    m.reset(5)
    t = np.zeros((5, 20), np.uint8)
    t[:, 0] = [9, 3, 200, 3, 0]
    m.open(np.arange(5), t)
    assert m.srm_set([0, 1, 2, 4]) == 0 and m.order == [4, 1, 0, 2]
    assert m.srm_set([0, 1, 3]) == SM.EUNSORTED and m.order is None
    assert m.srm_set([]) == 0 and m.order == []
    assert m.offer([7], t[:1])[2][0] == 1          # no search on either side: filtered


# ---- the C++ adapter --------------------------------------------------------------------------------
def test_adapter_compiles_as_cxx11_and_host_walk(tmp_path):
    """ResidentSearches::offerBatch below its threshold, and with no device behind it: the reference's
    walk on the host map against the oracle, and the pairs it queues."""
    exe = cpp_check.build("srmap", tmp_path)
    assert subprocess.check_output([exe], text=True).strip() == "built"
    cpp_check.run(exe, ["--host"], "srmap_check (host paths)", 120)
