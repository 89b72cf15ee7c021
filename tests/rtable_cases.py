"""Table snapshots for the resident routing table's tests (tests/test_rtable_cpu.py checks them on
the CPU, tests/test_gpu_rtable.py runs them on the device): grown tables, and synthetic ones that
reach what a grown table never does -- slices of many 64-node steps, walks past 64 rounds, lists
that never fill, 64- and 96-bit ties.  Test infrastructure only."""
import struct

import numpy as np

import oracle as O

COUNTS = (1, 8, 14, 32)
FRACTIONS = (1.0, 0.7, 0.4, 0.0)


def case(name, firsts, off, nodes, good, targets, counts=COUNTS):
    return {"name": name, "firsts": np.ascontiguousarray(firsts, np.uint8), "off": np.ascontiguousarray(off, np.uint32),
            "nodes": np.ascontiguousarray(nodes, np.uint8).reshape(-1, 20), "good": np.ascontiguousarray(good, np.uint8),
            "targets": np.ascontiguousarray(targets, np.uint8), "counts": tuple(counts)}


def grown(cluster):
    """The table of test_find_closest_vs_oracle: (myid, firsts, off, nodes, targets) -- 300 random
    targets, 40 node ids, myid, every bucket first."""
    myid = O.gen_ids(99, 1)[0]
    ids = O.gen_ids(100, 10000)
    if cluster:
        ids[:5000, :3] = myid[:3]
    firsts, off, nodes = O.Table(myid).grow(ids).export()
    tg = np.concatenate([O.gen_ids(101, 300), nodes[:: max(1, nodes.shape[0] // 40)][:40], myid[None, :], firsts])
    return myid, firsts, off, nodes, tg


def good_mask(n, fraction, seed=7):
    return (np.random.default_rng(seed).random(n) < fraction).astype(np.uint8)


def sorted_ids(seed, n=600):
    ids = O.gen_ids(seed, n)
    order = np.lexsort(ids.T[::-1])
    return np.ascontiguousarray(ids[order])


def cut(ids, sizes):
    """Sorted ids cut into buckets of the given sizes: first[0] the zero id, the other firsts the
    buckets' first ids."""
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint32)
    assert off[-1] == ids.shape[0]
    firsts = ids[off[:-1]].copy()
    firsts[0] = 0
    return firsts, off


def sizes_for(nb, n, seed):
    """nb non-empty bucket sizes summing to n"""
    if nb == 1:
        return [n]
    rng = np.random.default_rng(seed)
    cuts = np.sort(rng.choice(np.arange(1, n), nb - 1, replace=False))
    return list(np.diff(np.concatenate([[0], cuts, [n]])))


def edge_targets(ids, firsts, off, seed, buckets=()):
    """random targets, node ids, the zero and the all-ones id, every first (at most 16), and ids
    inside the named buckets"""
    t = [O.gen_ids(seed, 24), ids[:: max(1, ids.shape[0] // 12)][:12], np.zeros((1, 20), np.uint8),
         np.full((1, 20), 255, np.uint8), firsts[:: max(1, firsts.shape[0] // 16)][:16]]
    for b in buckets:
        t.append(ids[off[b]: off[b] + 2])
        t.append(ids[off[b + 1] - 1: off[b + 1]])
    return np.concatenate(t)


def synthetic():
    cases = []
    ids = sorted_ids(4242)
    n = ids.shape[0]
    # one 600-node bucket: ten 64-node steps; every node good, and 70 % of them
    f, off = cut(ids, [n])
    tg = edge_targets(ids, f, off, 1)
    cases.append(case("one_bucket", f, off, ids, np.ones(n, np.uint8), tg))
    cases.append(case("one_bucket_70", f, off, ids, good_mask(n, 0.7, 3), tg))
    # exactly 63 / 64 / 65 good nodes in that bucket
    for g in (63, 64, 65):
        m = np.zeros(n, np.uint8)
        m[np.random.default_rng(g).choice(n, g, replace=False)] = 1
        cases.append(case(f"one_bucket_{g}_good", f, off, ids, m, tg))
    # buckets of 63, 64 and 65 nodes: at count 32 a target inside one is answered from that slice
    f, off = cut(ids, [63, 64, 65, 100, n - 292])
    cases.append(case("slices_63_64_65", f, off, ids, np.ones(n, np.uint8), edge_targets(ids, f, off, 2, (0, 1, 2, 3, 4))))
    # two buckets
    f, off = cut(ids, sizes_for(2, n, 5))
    cases.append(case("two_buckets", f, off, ids, good_mask(n, 0.7, 5), edge_targets(ids, f, off, 3, (0, 1))))
    # 256 buckets; good nodes only in bucket 0 (targets in the last bucket: 255 rounds down), and
    # the mirror image (targets in bucket 0: 255 rounds up)
    f, off = cut(ids, sizes_for(256, n, 6))
    tg = edge_targets(ids, f, off, 4, (0, 100, 255))
    cases.append(case("256_buckets", f, off, ids, good_mask(n, 0.4, 6), tg))
    m = np.zeros(n, np.uint8)
    m[off[0]: off[1]] = 1
    cases.append(case("256_good_in_first", f, off, ids, m, tg))
    m = np.zeros(n, np.uint8)
    m[off[255]: off[256]] = 1
    cases.append(case("256_good_in_last", f, off, ids, m, tg))
    m = np.zeros(n, np.uint8)
    m[off[70]: off[71]] = 1   # 70 rounds up from bucket 0, 185 down from the last
    cases.append(case("256_good_in_70", f, off, ids, m, tg))
    # exactly count and count - 1 good nodes in the whole table
    for nb, (ff, oo) in ((5, cut(ids, sizes_for(5, n, 8))), (256, (f, off))):
        for g in (7, 8, 13, 14, 31, 32):
            m = np.zeros(n, np.uint8)
            m[np.random.default_rng(100 + g).choice(n, g, replace=False)] = 1
            cases.append(case(f"{nb}_buckets_{g}_good", ff, oo, ids, m, edge_targets(ids, ff, oo, 5, (0, nb - 1)),
                              counts=(8, 14, 32)))
    cases.append(case("none_good", f, off, ids, np.zeros(n, np.uint8), tg))
    return cases


def ties():
    """Nodes that share their first 64 (40 of them) and 96 bits (20 of those) with each other and
    with the targets, among ordinary ones; counts 8 and 32."""
    ids = O.gen_ids(777, 300)
    ids[:40, :8] = ids[0, :8]
    ids[:20, :12] = ids[0, :12]
    pre, deep = ids[0, :8].copy(), ids[0, :12].copy()
    ids = np.ascontiguousarray(ids[np.lexsort(ids.T[::-1])])
    assert np.unique(ids, axis=0).shape[0] == ids.shape[0]
    group = ids[(ids[:, :8] == pre).all(1)]
    t64 = O.gen_ids(778, 12)
    t64[:, :8] = pre
    t96 = O.gen_ids(779, 12)
    t96[:, :12] = deep
    tg = np.concatenate([t64, t96, group[:6], O.gen_ids(780, 6)])
    out = []
    for nb in (1, 5):
        f, off = cut(ids, sizes_for(nb, ids.shape[0], 9))
        out.append(case(f"ties_{nb}", f, off, ids, np.ones(ids.shape[0], np.uint8), tg, counts=(8, 32)))
        out.append(case(f"ties_{nb}_70", f, off, ids, good_mask(ids.shape[0], 0.7, 9), tg, counts=(8, 32)))
    return out


def dump(cases, path):
    """The cases as tests/cpp/rtable_check.cpp --tables reads them."""
    with open(path, "wb") as fh:
        for c in cases:
            nb, nn, q = c["firsts"].shape[0], c["nodes"].shape[0], c["targets"].shape[0]
            fh.write(struct.pack("<4I", nb, nn, q, len(c["counts"])))
            fh.write(np.asarray(c["counts"], np.uint32).tobytes())
            for k in ("firsts", "off", "nodes", "good", "targets"):
                fh.write(c[k].tobytes())


def expected(c, count):
    """The oracle's (q, count) rows and (q,) counts for one case."""
    return O.find_closest_batch(c["firsts"], c["off"], c["nodes"], c["good"], c["targets"], count, threads=8)
