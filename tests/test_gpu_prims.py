"""GPU checks of the shared workgroup scan (opendht_amd/csrc/prims_dev.h, prims.hip) through the
public entry points that use it, at the smallest sizes where its strip logic can go wrong: the scan
takes 1,024 entries per strip and carries a running total, so each case puts 1, 64, 65 (a wave and
one), 1,024, 1,025 or 2,049 entries through it -- or just past 1,024 where one size is enough.  Every
comparison is exact, against numpy or the project's own models.  Marked gpu: run on the MI355X box."""
import numpy as np
import pytest

import ncache_cases as NC
import oracle as O

pytestmark = pytest.mark.gpu

NONE = 0xFFFFFFFF
SEED = 8600
TILE = 4096                      # ids per select / view / sort tile: one scan entry each
NMAX = 1024 * 8192 + 1           # the index case: 1,025 P0 blocks of 8,192 ids (= 2,049 tiles)


@pytest.fixture(scope="module")
def ctx():
    import opendht_amd
    c = opendht_amd.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def stream():
    """the id stream gen_ids(SEED, NMAX), shared and left unchanged: (NMAX, 20) bytes and (NMAX, 5) words"""
    ids = O.gen_ids(SEED, NMAX)
    return ids, ids.view(">u4").reshape(-1, 5).astype(np.uint32)


@pytest.fixture(scope="module")
def dev_planes():
    """the same stream as device word planes (torch tensor, stride)"""
    import opendht_amd
    import torch
    stride = (NMAX + TILE - 1) // TILE * TILE
    planes = torch.empty(5 * stride, dtype=torch.int32, device=torch.device("cuda", 0))
    assert opendht_amd.lib().dhtgpu_gen_dev(SEED, 0, NMAX, planes.data_ptr(), stride, None) == 0
    torch.cuda.synchronize()
    return planes, stride


def lex_order(words):
    """the lexicographic order of (n, 5) id words; the 64-bit prefixes decide when they are distinct"""
    k = (words[:, 0].astype(np.uint64) << np.uint64(32)) | words[:, 1].astype(np.uint64)
    order = np.argsort(k, kind="stable")
    if (np.diff(k[order]) > 0).all():
        return order
    return np.lexsort((words[:, 4], words[:, 3], words[:, 2], words[:, 1], words[:, 0]))


# ---- the select-prefix scan: one entry per 4,096-id block ------------------------------------------
@pytest.mark.parametrize("pbits", [1, 0])
@pytest.mark.parametrize("L", [1, 64, 65, 1024, 1025, 2049])
def test_select_prefix_scan_lengths(ctx, stream, dev_planes, L, pbits):
    import torch
    ids, words = stream
    planes, stride = dev_planes
    n = (L - 1) * TILE + 1
    dev = torch.device("cuda", 0)
    out = torch.empty(5 * stride, dtype=torch.int32, device=dev)
    gidx = torch.empty(stride, dtype=torch.int32, device=dev)
    m = ctx.select_prefix_dev(planes.data_ptr(), stride, n, pbits, 1 if pbits else 0, out.data_ptr(), stride,
                              gidx.data_ptr())
    sel = np.flatnonzero(ids[:n, 0] >> 7) if pbits else np.arange(n)
    assert m == sel.size
    assert np.array_equal(gidx[:m].cpu().numpy().view(np.uint32), sel.astype(np.uint32))
    got = out.view(5, stride)[:, :m].cpu().numpy().view(np.uint32)
    for w in range(5):
        assert np.array_equal(got[w], words[:n][sel, w]), f"plane {w}"


# ---- the view's scan: one entry per 4,096-id tile --------------------------------------------------
def test_view_scan_past_one_strip(ctx, stream):
    ids, _ = stream
    n = 1024 * TILE + 1   # 1,025 tiles
    mask = np.random.default_rng(1).random(n) < 0.5
    tg = O.gen_ids(SEED + 1, 16)
    ctx.gen_ids(SEED, n)
    ctx.set_accept(mask)
    assert ctx.num_accepted == int(mask.sum())
    sel = np.flatnonzero(mask)
    want, wcnt = O.topk(ids[:n][sel], tg, 8, threads=16)
    want = sel[want].astype(np.uint32)   # (n_acc >= 8: no NONE entries)
    got, cnt = ctx.topk(tg, 8)
    ctx.set_accept(None)
    assert np.array_equal(cnt, wcnt) and np.array_equal(got, want)


# ---- the sort's row scan: one entry per 4,096-id tile and digit ------------------------------------
def test_sort_rowscan_past_one_strip(ctx, stream):
    ids, words = stream
    n = 1024 * TILE + 1   # 1,025 sort tiles
    ctx.cache_set(ids[:n])
    assert np.array_equal(ctx.cache_sorted(), lex_order(words[:n]).astype(np.uint32))


# ---- the NodeCache's scan: one entry per 256 batch keys --------------------------------------------
def test_nc_scan_past_one_strip(ctx, stream):
    ids, _ = stream
    m = 1024 * 256 + 1    # 1,025 blocks
    base = ids[:1000]
    batch = ids[1000: 1000 + m].copy()
    batch[3::8] = base[np.arange(batch[3::8].shape[0]) % 1000]     # resident keys (and their repeats)
    r = batch[5::8].shape[0]
    batch[5::8] = batch[4::8][:r][::-1]                            # repeats of other batch keys, before and after them
    hs = np.arange(2000, 2000 + m, dtype=np.uint32)
    model = NC.Model()
    model.set(base)
    ctx.nc_set(base)
    want = model.insert(batch, hs)
    new = ctx.nc_insert(batch, hs)
    assert 0.2 < 1.0 - want.mean() < 0.3
    assert np.array_equal(new, want)
    gk, gh = ctx.nc_export()
    wk, wh = model.sorted()
    assert np.array_equal(gk, wk) and np.array_equal(gh, wh)
    gone = batch[want == 1][::2]
    assert np.array_equal(ctx.nc_erase(gone), model.erase(gone))
    gk, gh = ctx.nc_export()
    wk, wh = model.sorted()
    assert np.array_equal(gk, wk) and np.array_equal(gh, wh)


# ---- the index build's scans: P0's rows of 1,025 blocks, the bins, P1's and P2's LDS histograms ----
def test_index_scans_past_one_strip(ctx, stream):
    tg = O.gen_ids(SEED + 2, 64)
    ctx.gen_ids(SEED, NMAX)
    ctx.index_build()
    for k in (8, 32):
        want, wcnt = ctx.topk(tg, k)   # K1, the flat scan
        got, cnt = ctx.index_topk(tg, k)
        assert np.array_equal(cnt, wcnt) and np.array_equal(got, want), k
