"""The sub-partitioned shapes of the GPU tests (tests/golden/sub_shapes.txt, read by
tests/cpp/plan_check.cpp too) and the route assertion every test makes before a call it claims
is sub-partitioned."""
import os

import pytest

import opendht_amd

PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sub_shapes.txt")


def load():
    """[(name, n, q, k, q_build)]: q_build is the q of the call that built the sub-partitions
    (the call itself where the line names none)."""
    out = []
    for line in open(PATH):
        f = line.split()
        if not f or f[0].startswith("#"):
            continue
        n, q, k = int(f[1]), int(f[2]), int(f[3])
        out.append((f[0], n, q, k, int(f[4]) if len(f) > 4 else q))
    return out


SHAPES = {name: (n, q, k) for name, n, q, k, _ in load()}


def shape(name):
    """(n, q, k) of a listed shape."""
    return SHAPES[name]


def assert_subs(ctx, n, q, k):
    """A batch_topk call of q targets at k over n ids on ctx's device is served over prefix
    sub-partitions (n: the ids the call sees -- a mask's view, not the set behind it).  A device of
    another CU count than the 256 the shapes were chosen for may plan the shape as one set: skipped
    there, failed when the 256-CU plan itself has moved."""
    route = opendht_amd.batch_plan(n, q, k, ctx=ctx)["route"]
    if route != opendht_amd.ROUTE_SUBS:
        r256 = opendht_amd.batch_plan(n, q, k, num_cus=256)["route"]
        assert r256 == opendht_amd.ROUTE_SUBS, f"n={n} q={q} k={k}: route {r256} at 256 CUs, not sub-partitioned"
        pytest.skip(f"n={n} q={q} k={k}: route {route} on this device, sub-partitioned only at 256 CUs")
