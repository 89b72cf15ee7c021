"""CPU-side checks of the resident routing table (dhtgpu_rt_*, opendht_amd/csrc/rtable.hip): the C++
adapter's host paths against the oracle, the table snapshots the GPU tests rely on, and the
kernel's walk rule restated on the CPU.  No GPU needed.  (Header, exports, binding and a null
context: tests/test_abi.py; the kernels' register and scratch budget: tests/test_kernel_resources.py.)"""
import subprocess

import numpy as np
import pytest

import cpp_check
import rtable_cases as RC


@pytest.fixture(scope="module")
def rtable_check(tmp_path_factory):
    """tests/cpp/rtable_check.cpp built as C++11 with -Wall -Wextra -Werror against the mock table shape"""
    return cpp_check.build("rtable", tmp_path_factory.mktemp("rtable"))


def test_adapter_compiles_as_cxx11(rtable_check):
    assert subprocess.check_output([rtable_check], text=True).strip() == "built"


def test_adapter_host_replies_and_closeness(rtable_check):
    """What ResidentTable runs below its device threshold: replies (findClosestNodes + the packed
    records) and both closeness tests against the oracle on a grown table, af 4 and af 6."""
    cpp_check.run(rtable_check, ["--host"], "rtable_check (host paths)", 120)


def test_oracle_and_host_walk_agree_on_the_synthetic_tables(rtable_check, tmp_path):
    """The GPU tests take the oracle's word on tables no onNewNode grows; here the adapter's
    independent host walk (detail::find_closest_host) gives the same nodes on each of them."""
    cases = RC.synthetic() + RC.ties()
    path = str(tmp_path / "cases.bin")
    RC.dump(cases, path)
    cpp_check.run_for_line(rtable_check, ["--tables", path], f"rtable_check (tables): {len(cases)} cases, 0 mismatches", 300)


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
