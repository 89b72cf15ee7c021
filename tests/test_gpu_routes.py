"""K6 route accounting on the device: every constructed case (tests/route_cases.py) at k = 8, 14, 32
against the oracle for the rows and against the routing model (tests/route_model.py) for the
counters dhtgpu_batch_topk_timed returns, in index form, in record form and on a second call; and
the same results through output pointers that are only 4-byte aligned."""
import numpy as np
import pytest

import opendht_amd
import oracle as O
import route_cases as RC
import route_model as M
import test_gpu_parity as P

pytestmark = pytest.mark.gpu

KS = [8, 14, 32]
_want = {}   # (case, k) -> the oracle's rows and counts, computed once


def want_rows(case):
    key = (case.name, case.k)
    if key not in _want:
        idx, cnt = O.topk(case.ids, case.targets, case.k, threads=16)
        if case.shard:   # a prefix shard answers in stream indices
            gidx = case.shard[4]
            idx = np.where(idx == opendht_amd.NONE, idx, gidx[np.minimum(idx, len(gidx) - 1)].astype(np.uint32))
        _want[key] = (idx, cnt)
    return _want[key]


def build_on(c, name, k):
    """The case built from the device's own plan; on a device of another CU count a case whose
    precondition no longer holds is skipped, not failed."""
    try:
        return RC.build(name, k, ctx=c)
    except RC.Precondition as e:
        RC.build(name, k, num_cus=256)   # (fails here when the 256-CU plan itself moved)
        pytest.skip(f"{name} k={k}: this device's plan does not admit the case: {e}")


def load(c, case):
    if case.shard:
        seed, stream, pbits, pval, _ = case.shard
        c.gen_ids_prefix(seed, stream, pbits, pval)
    else:
        c.set_ids(case.ids)
    assert c.num_ids == case.n


def planes(tg, stride, lead=0):
    """Target word planes on the device at `stride`, `lead` words into their buffer."""
    import torch
    q = tg.shape[0]
    w = np.zeros((5, stride), dtype=np.uint32)
    w[:, :q] = tg.view(">u4").reshape(q, 5).astype(np.uint32).T
    buf = torch.zeros(lead + 5 * stride, dtype=torch.int32, device="cuda:0")
    buf[lead:] = torch.from_numpy(w.reshape(-1).view(np.int32)).to("cuda:0")
    return buf


def timed(c, tp, ts, q, k):
    import torch
    idx = torch.full((q, k), -7, dtype=torch.int32, device="cuda:0")
    cnt = torch.full((q,), -7, dtype=torch.int32, device="cuda:0")
    _, fb, sv, wv = c.batch_topk_timed(tp.data_ptr(), ts, q, k, idx.data_ptr(), cnt.data_ptr(), c.stream)
    torch.cuda.synchronize()
    return idx.cpu().numpy().view(np.uint32), cnt.cpu().numpy().view(np.uint32), (fb, sv, wv)


def check_stats(case, st, what):
    e = case.expect
    print(f"{what}: model fallback {e['fallback']} survivors {e['survivors']} wave {e['wave']}; stats4 {st}")
    for key, got in zip(("fallback", "survivors", "wave"), st):
        lo, hi = e[key]
        assert lo <= got <= hi, f"{what}: {key} = {got}, the model says [{lo}, {hi}] (stats4 {st}, plan {case.plan})"


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("name", RC.NAMES)
def test_route_case(name, k):
    """Rows == the oracle's for every target and stats4 within the model's bounds (equal where the
    model is tight); record form with an index base; then the first call again on the same context:
    the same rows, and the same counters where nothing order-dependent happens (within the bounds
    otherwise) -- the bitmap, the counters, the spill count and F2's `lost` push are zero again."""
    with opendht_amd.Context(0) as c:
        case = build_on(c, name, k)
        assert case.plan == opendht_amd.batch_plan(case.n, case.q, k, ctx=c)
        load(c, case)
        q = case.q
        ts = (q + 63) // 64 * 64
        tp = planes(case.targets, ts)
        widx, wcnt = want_rows(case)
        idx, cnt, st = timed(c, tp, ts, q, k)
        bad = np.nonzero((idx != widx).any(axis=1) | (cnt != wcnt))[0]
        assert bad.size == 0, f"{name} k={k}: {bad.size} rows differ, first {bad[:5]}: {idx[bad[0]]} vs {widx[bad[0]]}"
        check_stats(case, st, f"{name} k={k}")
        # record form, stream indices on the shard
        base = 0 if case.shard else 1000
        gidx = case.shard[4].astype(np.int64) if case.shard else np.arange(case.n, dtype=np.int64) + base
        got = P._ctx_records(c, case.targets, k, base)
        rec = P._want_records(case.ids, gidx, case.targets, k)
        badr = np.nonzero((got != rec).any(axis=(1, 2)))[0]
        assert badr.size == 0, f"{name} k={k} records: {badr.size} rows differ, first {badr[:5]}: {got[badr[0]]} vs {rec[badr[0]]}"
        idx2, cnt2, st2 = timed(c, tp, ts, q, k)
        assert np.array_equal(idx2, widx) and np.array_equal(cnt2, wcnt), f"{name} k={k}: the second call's rows differ"
        check_stats(case, st2, f"{name} k={k} second call")
        if M.tight(case.expect):
            assert st2 == st, f"{name} k={k}: second call stats4 {st2}, first {st}"


@pytest.mark.parametrize("k", [8, 32])
@pytest.mark.parametrize("name", ["clean_packed", "w0_ties"])
def test_outputs_four_byte_aligned(name, k):
    """out_idx / out_cnt / out_rec 4 bytes past a 16-byte boundary (F3's word-by-word writer in
    the Exact instantiation, the dword record writer), the target planes 4 bytes past one too at an
    odd stride t_stride = q: the aligned call's results, and the words on either side untouched."""
    import torch
    PAT, LEAD, TAIL = 0x5A5A5A5A, 5, 8
    with opendht_amd.Context(0) as c:
        case = build_on(c, name, k)
        load(c, case)
        q = case.q - 1 if case.q % 2 == 0 else case.q   # odd
        tg = case.targets[:q]
        widx, wcnt = (x[:q] for x in want_rows(case))
        tpa = planes(tg, (q + 63) // 64 * 64)
        aidx, acnt, _ = timed(c, tpa, (q + 63) // 64 * 64, q, k)
        assert np.array_equal(aidx, widx) and np.array_equal(acnt, wcnt)
        arec = P._ctx_records(c, tg, k, 1000)
        tp = planes(tg, q, lead=1)
        tptr = tp.data_ptr() + 4

        def guarded(words):
            b = torch.full((LEAD + words + TAIL,), PAT, dtype=torch.int32, device="cuda:0")
            assert b.data_ptr() % 16 == 0
            return b

        def split(b, words):
            h = b.cpu().numpy().view(np.uint32)
            assert (h[:LEAD] == PAT).all() and (h[LEAD + words:] == PAT).all(), "guard words overwritten"
            return h[LEAD: LEAD + words]
        bi, bc = guarded(q * k), guarded(q)
        c.batch_topk_dev(tptr, q, q, k, bi.data_ptr() + 4 * LEAD, bc.data_ptr() + 4 * LEAD, None, 0, c.stream)
        torch.cuda.synchronize()
        assert np.array_equal(split(bi, q * k).reshape(q, k), aidx), f"{name} k={k}: unaligned index rows differ"
        assert np.array_equal(split(bc, q), acnt)
        br = guarded(q * k * 3)
        c.batch_topk_dev(tptr, q, q, k, None, None, br.data_ptr() + 4 * LEAD, 1000, c.stream)
        torch.cuda.synchronize()
        assert np.array_equal(split(br, q * k * 3).reshape(q, k, 3), arec), f"{name} k={k}: unaligned records differ"
