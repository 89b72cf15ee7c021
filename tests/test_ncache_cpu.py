"""CPU-side checks of the resident NodeCache (dhtgpu_nc_*, opendht_amd/csrc/ncache.hip): the C++
adapter's host path and slot bookkeeping against the oracle, and the model the GPU tests rely on
checked against itself.  No GPU needed.  (Header, exports, binding and a null context:
tests/test_abi.py; the kernels' register and scratch budget: tests/test_kernel_resources.py.)"""
import subprocess

import numpy as np
import pytest

import cpp_check
import ncache_cases as NC
import oracle as O


@pytest.fixture(scope="module")
def ncache_check(tmp_path_factory):
    """tests/cpp/ncache_check.cpp built as C++11 with -Wall -Wextra -Werror against the mock map shape"""
    return cpp_check.build("ncache", tmp_path_factory.mktemp("ncache"))


def test_adapter_compiles_as_cxx11(ncache_check):
    assert subprocess.check_output([ncache_check], text=True).strip() == "built"


def test_adapter_host_path_and_slot_bookkeeping(ncache_check):
    """What ResidentCache runs below its device threshold (the host walk, expired weak_ptrs
    included) against the oracle, and its slots and free list through insert, erase, re-insert
    into a freed slot."""
    cpp_check.run(ncache_check, ["--host"], "ncache_check (host paths)", 120)


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
