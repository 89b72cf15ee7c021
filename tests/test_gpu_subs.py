"""K6 over prefix sub-partitions (route 2) in the forms no other test reaches: sub-partitions
built in index order (the staged F2 over 8 bucket sets, sparse and dense survivors), a sequence of
calls that changes route and k on one context and one workspace slot, a partition shared by three
or more of k_f2_direct's workgroups, and equal ids across the stable sort.  Every case runs on a
fresh context whose ids are made on the device (gen_ids, write_ids for the crafted part), asserts
the route of every call from the plan query, compares the whole batch with the K1 scan (the
independent kernel family) and at most 16 rows plus the crafted ones with the CPU oracle.  The
shapes are those of tests/golden/sub_shapes.txt, whose routes, order and F2 form
tests/test_batch_plan.py pins on the CPU.  Marked gpu."""
import time

import numpy as np
import pytest

import opendht_amd
import oracle as O
import test_gpu_parity as P
from sub_shapes import assert_subs, shape
from test_gpu_scale import _handles_vs_indices

pytestmark = pytest.mark.gpu

NONE = opendht_amd.NONE


def route(c, n, q, k):
    return opendht_amd.batch_plan(n, q, k, ctx=c)["route"]


def assert_route(c, n, q, k, want):
    """Route `want` on this device; as assert_subs, a device that is not the 256-CU one skips."""
    got = route(c, n, q, k)
    if got != want:
        assert opendht_amd.batch_plan(n, q, k, num_cus=256)["route"] == want, (n, q, k)
        pytest.skip(f"n={n} q={q} k={k}: route {got} on this device, {want} only at 256 CUs")


def same_rows(got, cnt, want, wcnt, what):
    bad = np.nonzero((got != want).any(axis=1) | (cnt != wcnt))[0]
    assert bad.size == 0, f"{what}: {bad.size} rows differ, first {bad[:5]}: {got[bad[0]]} vs {want[bad[0]]}"


def oracle_overwritten(seed, n, crafted, tg, k):
    """The exact top-k over the stream gen_ids(seed, n) whose first len(crafted) ids were
    overwritten by `crafted`: the oracle over the crafted ids and the generator-fed oracle over
    the rest of the stream, merged by (160-bit distance, index)."""
    m = crafted.shape[0]
    a, ac = O.topk(crafted, tg, k, threads=16)
    b, bc = O.topk_gen(seed, n - m, tg, k, start=m, threads=16)
    out = np.full((tg.shape[0], k), NONE, dtype=np.uint32)
    cnt = np.zeros(tg.shape[0], dtype=np.uint32)
    for r in range(tg.shape[0]):
        cand = [(O.py_dist(tg[r], crafted[int(i)]), int(i)) for i in a[r, :ac[r]]]
        cand += [(O.py_dist(tg[r], O.gen_ids(seed, 1, start=int(i))[0]), int(i)) for i in b[r, :bc[r]]]
        cand.sort()
        cnt[r] = min(k, len(cand))
        out[r, :cnt[r]] = [i for _, i in cand[:k]]
    return out, cnt


def record_rows(c, tg, k, base, sc, scnt, rows):
    """Record form with an index base: word 2 of every record == the K1 scan's index + base, and on
    `rows` words 0 and 1 == the id's own (read back from the context)."""
    rec = P._ctx_records(c, tg, k, base)
    want = np.where(sc == NONE, sc, sc + np.uint32(base))
    same_rows(rec[..., 2], scnt, want, scnt, f"record indices, k={k}")
    for r in rows:
        for j in range(int(scnt[r])):
            w = c.get_ids(int(sc[r, j]), 1).view(">u4").astype(np.uint32)[0]
            assert tuple(rec[r, j, :2]) == (w[0], w[1]), (k, r, j)


def test_unsorted_sub_partitions():
    """2^27 ids, 36,864 targets: 8 sub-partitions of 4,608 targets each, under 2 % survivors at k = 8,
    1 and 32, so the first call builds them in index order -- the staged F2 reading the descriptor
    table with non-temporal loads, 8 bucket sets (k6_decide.txt: unsorted-k8/-k1/-k32).  Index form,
    record form with idx_base = 1000 and sub-partition handles mapped back on the device, each ==
    the K1 scan on the whole batch and the oracle on 16 rows.  Then 2^18 targets at k = 8 on the same
    context: the sub-partitions stay as built, so the staged F2 runs at dense survivors (~6 %;
    unsorted-then-dense)."""
    t0 = time.perf_counter()
    n, q, _ = shape("unsorted-k8.unsorted")
    seed = 9101
    with opendht_amd.Context(0) as c:
        c.gen_ids(seed, n)
        tg = O.gen_ids(9102, q)
        rows = np.arange(0, q, q // 16)[:16]
        w32, wc32 = O.topk_gen(seed, n, tg[rows], 32, threads=16)
        s32, sc32 = c.topk(tg, 32)   # one scan: the top-k of a smaller k is its rows' first k
        for k in (8, 1, 32):
            assert (n, q, k) == shape(f"unsorted-k{k}.unsorted")
            assert_subs(c, n, q, k)
            got, cnt = c.batch_topk(tg, k)
            sc, scnt = np.ascontiguousarray(s32[:, :k]), np.minimum(sc32, k)
            same_rows(got, cnt, sc, scnt, f"index form vs K1, k={k}")
            same_rows(got[rows], cnt[rows], w32[:, :k], np.minimum(wc32, k), f"index form vs oracle, k={k}")
            record_rows(c, tg, k, 1000, sc, scnt, rows[:4])
            _handles_vs_indices(c, tg, k)
        n2, q2, k2 = shape("unsorted-then-dense.unsorted")
        assert n2 == n
        assert_subs(c, n, q2, k2)
        tg2 = O.gen_ids(9103, q2)
        got, cnt = c.batch_topk(tg2, k2)
        sc, scnt = c.topk(tg2, k2)
        same_rows(got, cnt, sc, scnt, "dense call vs K1")
        rows2 = np.arange(0, q2, q2 // 16)[:16]
        want, wcnt = O.topk_gen(seed, n, tg2[rows2], k2, threads=16)
        same_rows(got[rows2], cnt[rows2], want, wcnt, "dense call vs oracle")
    print(f"test_unsorted_sub_partitions: {time.perf_counter() - t0:.1f} s")


def test_call_sequence_one_workspace_slot():
    """2^26 ids, six calls on one context and its own stream (one workspace slot): sub-partitioned at
    k = 8, one set (another head layout), sub-partitioned at k = 32 (the descriptor table moves), KS,
    one set at k = 3, and the first call again.  Each call's route is asserted, every call == the K1
    scan, 16 rows == the oracle, and the last call's rows are the first's.  A one-set call after a
    sub-partitioned one met stale statistics words, a sub-partitioned call after a change of k a
    stale descriptor table, and a workspace slot's reuse across routes once gave 3 wrong rows of
    262,144 by the order the suite happened to run in: this is that order, fixed."""
    t0 = time.perf_counter()
    n, q, _ = shape("kseq-k8.sorted")
    assert shape("kseq-k32.sorted")[:2] == (n, q)
    seed = 9201
    calls = [(q, 8, opendht_amd.ROUTE_SUBS), (65536, 8, opendht_amd.ROUTE_K6), (q, 32, opendht_amd.ROUTE_SUBS),
             (40, 8, opendht_amd.ROUTE_KS), (65536, 3, opendht_amd.ROUTE_K6), (q, 8, opendht_amd.ROUTE_SUBS)]
    with opendht_amd.Context(0) as c:
        c.gen_ids(seed, n)
        tg = O.gen_ids(9202, q)
        rows = np.arange(0, 40, 40 // 16)[:16]   # rows of every call's batch, the KS call's included
        w32, wc32 = O.topk_gen(seed, n, tg[rows], 32, threads=16)
        for qi, ki, want in calls:
            assert_route(c, n, qi, ki, want)
        s32, sc32 = c.topk(tg, 32)   # one scan: a call's rows are its targets' first k of these
        first = None
        for i, (qi, ki, _) in enumerate(calls):
            got, cnt = c.batch_topk(tg[:qi], ki)
            sc, scnt = s32[:qi, :ki], np.minimum(sc32[:qi], ki)
            same_rows(got, cnt, sc, scnt, f"call {i + 1} (q={qi}, k={ki}) vs K1")
            same_rows(got[rows], cnt[rows], w32[:, :ki], np.minimum(wc32, ki), f"call {i + 1} vs oracle")
            if i == 0:
                first = (got, cnt)
        same_rows(got, cnt, first[0], first[1], "last call vs first call")
    print(f"test_call_sequence_one_workspace_slot: {time.perf_counter() - t0:.1f} s")


def test_partition_shared_by_three_workgroups():
    """2^26 ids, 2^17 targets at k = 8 (sorted sub-partitions, k_f2_direct); ids [0, 2^19) overwritten
    by ids of one 26-bit prefix with hashed low bits.  Sorted, they are one run of 2^19 ids in one
    level-19 cell of sub-partition 1, whose workgroups hold about 2.4e5 ids each: the run fills
    the range of at least one workgroup whose first and last partition are both shared with its
    neighbours (every reservation a global atomic) and part of two more.  1/8 of the targets lie in
    the prefix: their partition overflows its bucket and they take the fallback scan.  The decision
    (direct still taken with the matching span table) is k6_decide.txt's
    subs-one-partition-three-workgroups.  Whole batch == K1 scan; 8 targets inside the prefix and
    8 outside == the oracle."""
    t0 = time.perf_counter()
    n, q, k = shape("kseq-k8.sorted")
    seed, m = 9301, 1 << 19
    crafted = O.gen_ids(9302, m)
    crafted[:, :4] = np.array([0x5B, 0xC4, 0x9A, 0x40], np.uint8) | (crafted[:, :4] & np.array([0, 0, 0, 0x3F], np.uint8))
    assert len(np.unique(crafted, axis=0)) == m
    tg = O.gen_ids(9303, q)
    tg[: q // 8, :4] = np.array([0x5B, 0xC4, 0x9A, 0x40], np.uint8) | (tg[: q // 8, :4] & np.array([0, 0, 0, 0x3F], np.uint8))
    with opendht_amd.Context(0) as c:
        c.gen_ids(seed, n)
        c.write_ids(0, crafted)
        assert_subs(c, n, q, k)
        got, cnt = c.batch_topk(tg, k)
        sc, scnt = c.topk(tg, k)
        same_rows(got, cnt, sc, scnt, "vs K1")
        rows = np.r_[np.arange(0, q // 8, q // 64)[:8], np.arange(q // 8, q, q // 9)[:8]]
        want, wcnt = oracle_overwritten(seed, n, crafted, tg[rows], k)
        assert (want[:8] < m).all() and np.all(wcnt == k)   # the prefix's targets answer from the crafted run
        same_rows(got[rows], cnt[rows], want, wcnt, "vs oracle")
    print(f"test_partition_shared_by_three_workgroups: {time.perf_counter() - t0:.1f} s")


def test_equal_ids_across_the_stable_sort():
    """2^26 ids, 2^17 targets at k = 8 (sorted sub-partitions); ids [0, 2^16) overwritten by copies of
    the stream's ids [2^25, 2^25 + 2^16), and the copies are the first 2^16 targets.  Each such
    target has two ids at distance 0: the sort of the sub-partitions is stable, so the pair keeps
    its index order and the row starts (j, 2^25 + j), lower index first.  Whole batch == K1 scan;
    8 of the copies and 8 other targets == the oracle."""
    t0 = time.perf_counter()
    n, q, k = shape("kseq-k8.sorted")
    seed, m, src = 9401, 1 << 16, 1 << 25
    crafted = O.gen_ids(seed, m, start=src)
    tg = O.gen_ids(9402, q)
    tg[:m] = crafted
    with opendht_amd.Context(0) as c:
        c.gen_ids(seed, n)
        c.write_ids(0, crafted)
        assert_subs(c, n, q, k)
        got, cnt = c.batch_topk(tg, k)
        assert np.all(cnt == k)
        j = np.arange(m, dtype=np.uint32)
        bad = np.nonzero((got[:m, 0] != j) | (got[:m, 1] != j + np.uint32(src)))[0]
        assert bad.size == 0, f"{bad.size} pairs out of index order, first {bad[:5]}: {got[bad[0]]}"
        sc, scnt = c.topk(tg, k)
        same_rows(got, cnt, sc, scnt, "vs K1")
        rows = np.r_[np.arange(0, m, m // 8)[:8], np.arange(m, q, (q - m) // 8)[:8]]
        want, wcnt = oracle_overwritten(seed, n, crafted, tg[rows], k)
        same_rows(got[rows], cnt[rows], want, wcnt, "vs oracle")
    print(f"test_equal_ids_across_the_stable_sort: {time.perf_counter() - t0:.1f} s")
