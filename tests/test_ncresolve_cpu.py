"""CPU-side checks of keys-to-handles over the resident NodeCache (dhtgpu_ncr_*,
opendht_amd/csrc/ncresolve.hip): the model the GPU tests rely on checked against ncache_cases.Model,
the mirrored G-switch constants, and the C++ adapter's host path.  No GPU needed.  (Header, exports,
binding and a null context: tests/test_abi.py; the kernels' register and scratch budget:
tests/test_kernel_resources.py.)"""
import os
import re
import subprocess

import numpy as np
import pytest

import cpp_check
import ncache_cases as NC
import ncresolve_cases as NR
import oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "opendht_amd", "csrc")


# ---- the model against ncache_cases.Model ----------------------------------------------------------
def _models(n=300, seed=61):
    keys = O.gen_ids(seed, n)
    handles = (np.random.default_rng(seed).permutation(3 * n)[:n] + 7).astype(np.uint32)
    a, b = NR.Model(), NC.Model()
    a.nc.set(keys, handles)
    b.set(keys, handles)
    a.nc.update_accept(handles[:40], 0)
    b.update_accept(handles[:40], 0)
    return a, b


def test_model_get_nodes_is_insert_with_the_reported_handles():
    """get_nodes' map and accept set equal Model.insert given, for each key, the handle get_nodes
    reported; the new bytes agree; the free handles go to the new keys in batch order"""
    for m in (1, 4, 63, 257):
        a, b = _models()
        ids, _, accept = NC.mutation_batch(a.nc, m, 5 + m, 0)
        free = NR.free_list(a, m, 9)
        h, new, used = a.get_nodes(ids, free, accept)
        assert used == int(new.sum()) and list(h[new == 1]) == list(free[:used])
        want_new = b.insert(ids, h, accept)
        assert np.array_equal(new, want_new)
        assert a.nc.map == b.map and a.nc.acc == b.acc
        for j, k in enumerate(ids):
            assert a.nc.map[bytes(k)] == h[j]
    a, _ = _models()
    k = O.gen_ids(3, 2)
    h, new, used = a.get_nodes(np.stack([k[0], k[1], k[0]]), [900, 901, 902], [0, 1, 1])
    assert list(h) == [900, 901, 900] and list(new) == [1, 1, 0] and used == 2
    assert 900 not in a.nc.acc and 901 in a.nc.acc   # the first appearance's accept byte wins


def test_model_extract_is_erase_plus_the_handles():
    a, b = _models()
    keys = list(a.nc.map)
    ids = NC.as_ids(np.frombuffer(b"".join([keys[3], keys[9], keys[3]]), np.uint8))
    ids = np.concatenate([ids, O.gen_ids(77, 2)])
    want_h = [a.nc.map[keys[3]], a.nc.map[keys[9]], NR.NONE, NR.NONE, NR.NONE]
    acc_before = set(a.nc.acc)
    h = a.extract(ids)
    found = b.erase(ids)
    assert list(h) == want_h and np.array_equal(found, (h != NR.NONE).astype(np.uint8))
    assert a.nc.map == b.map and a.nc.acc == acc_before


def test_model_find_and_exhaustion():
    a, _ = _models()
    keys = list(a.nc.map)
    ids = np.concatenate([NC.as_ids(np.frombuffer(keys[0] + keys[50], np.uint8)), O.gen_ids(78, 1)])
    h, acc = a.find(ids)
    assert list(h) == [a.nc.map[keys[0]], a.nc.map[keys[50]], NR.NONE]
    assert list(acc) == [a.nc.map[keys[0]] in a.nc.acc, a.nc.map[keys[50]] in a.nc.acc, 0]
    # exhaustion leaves the model untouched and says how many handles the batch needs
    batch = np.concatenate([O.gen_ids(79, 5), ids[:2], O.gen_ids(79, 1)])
    before = (dict(a.nc.map), set(a.nc.acc))
    with pytest.raises(NR.Exhausted) as e:
        a.get_nodes(batch, [1000, 1001, 1002, 1003])
    assert e.value.needed == 5 and (a.nc.map, a.nc.acc) == before
    h, new, used = a.get_nodes(batch, [1000, 1001, 1002, 1003, 1004])
    assert used == 5 and list(new) == [1, 1, 1, 1, 1, 0, 0, 0] and h[7] == 1000


def test_case_builders():
    keys = O.gen_ids(5, 4097)
    for m in NR.FIND_BATCHES:
        p = NR.find_probes(keys, m, 1)
        assert p.shape == (m, 20)
    p = NR.find_probes(keys, 4097, 1)
    have = {bytes(k) for k in p}
    assert bytes(20) in have and b"\xff" * 20 in have and sum(bytes(k) in have for k in keys) > 3000
    ck, cp = NR.clustered_probes()
    held = {bytes(k) for k in ck}
    assert any(bytes(k) in held for k in cp) and any(bytes(k) not in held for k in cp)
    assert all(bytes(k[:16]) == bytes(ck[0, :16]) for k in cp)   # they differ from the keys in word 4 only
    f = NR.free_list(_models()[0], 50, 2)
    assert len(set(f.tolist())) == 50 and not set(f.tolist()) & set(_models()[0].nc.map.values())
    assert list(f) != sorted(f) and max(f) - min(f) > 50
    for g in (NR.G_NARROW, NR.G_WIDE):
        assert {g - 1, g, g + 1, (g + 1) ** 2 - 1, (g + 1) ** 2, (g + 1) ** 2 + 1} <= set(NR.FIND_SIZES)
    assert NR.WIDE_MAX_BATCH in NR.FIND_BATCHES and NR.WIDE_MAX_BATCH + 1 in NR.FIND_BATCHES


def test_mirrored_constants_match_the_library():
    src = open(os.path.join(CSRC, "dhtgpu_internal.h")).read()
    lanes = re.search(r"constexpr uint32_t kNcrWideLanes = (\d+), kNcrNarrowLanes = (\d+);", src)
    switch = re.search(r"constexpr uint32_t kNcrWideMaxBatch = (\d+);", src)
    assert lanes and switch
    assert (int(lanes.group(1)), int(lanes.group(2))) == (NR.G_WIDE, NR.G_NARROW)
    assert int(switch.group(1)) == NR.WIDE_MAX_BATCH
    hpp = open(os.path.join(ROOT, "include", "dhtgpu.hpp")).read()
    mfb = re.search(r"static const size_t kMinResidentFindBatch = (\d+);", hpp)
    assert mfb and int(mfb.group(1)) % 64 == 0


# ---- the C++11 adapter ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ncresolve_check(tmp_path_factory):
    """tests/cpp/ncresolve_check.cpp built as C++11 with -Wall -Wextra -Werror"""
    return cpp_check.build("ncresolve", tmp_path_factory.mktemp("ncresolve"))


def test_adapter_compiles_as_cxx11(ncresolve_check):
    assert subprocess.check_output([ncresolve_check], text=True).strip() == "built"


def test_adapter_host_path_and_bookkeeping(ncresolve_check):
    """slotsOfBatch below its threshold, getNodeBatch's bookkeeping against a std::map restatement of
    dhtgpu_ncr_get_nodes, free-list reuse after noteErase, an expired node made anew in its slot"""
    cpp_check.run(ncresolve_check, ["--host"], "ncresolve_check (host paths)", 120)
