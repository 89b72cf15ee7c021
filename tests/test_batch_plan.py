"""K6's host planning (opendht_amd/csrc/batch_plan.{h,cpp}) is host-only code: these tests build
and run it on the CPU, with no device.

  * tests/cpp/plan_dump.cpp, linked against the library, prints the plan queries over a grid of
    shapes; tests/golden/k6_plan_grid.txt is a subset of the grid recorded from the revision
    before the planning moved out of batch.hip (the full grid was compared once).
  * tests/cpp/plan_check.cpp, compiled with batch_plan.cpp alone, prints the launch decision
    (decide_batch) for a list of call shapes -- the named ones in full, the grids as one hash per
    group -- and checks, for each, what the kernels rely on; tests/golden/k6_decide.txt was
    recorded from the launch's chooser lifted verbatim.
  * tests/golden/sub_shapes.txt lists the sub-partitioned shapes the GPU tests run; plan_check
    records the route, the split, the order and the decision of each, and the library's own plan
    query must route every one of them to sub-partitions on 256 CUs.
"""
import os
import subprocess

import opendht_amd
import sub_shapes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "opendht_amd", "csrc")
GOLDEN = os.path.join(ROOT, "tests", "golden")
WARN = ["-std=c++17", "-Wall", "-Wextra", "-Werror"]


def test_plan_sources_are_host_only():
    """batch_plan.h / batch_plan.cpp compile as plain C++17 with no ROCm include path."""
    for fn in ("batch_plan.cpp", "batch_plan.h"):
        src = open(os.path.join(CSRC, fn)).read()
        assert "#include <hip" not in src and "dhtgpu_internal.h" not in src, fn
        subprocess.check_call(["g++", *WARN, "-fsyntax-only", "-x", "c++", os.path.join(CSRC, fn)])


def test_plan_grid_matches_recorded(tmp_path):
    exe = str(tmp_path / "plan_dump")
    libdir = os.path.dirname(opendht_amd.LIB_PATH)
    subprocess.check_call(["g++", *WARN, os.path.join(ROOT, "tests", "cpp", "plan_dump.cpp"), "-o", exe,
                           "-L", libdir, "-ldhtgpu", "-Wl,-rpath," + libdir])
    fixture = os.path.join(GOLDEN, "k6_plan_grid.txt")
    want = open(fixture).read()
    got = subprocess.check_output([exe, fixture], text=True)
    assert len(want.splitlines()) > 100
    # the spot values of the cfg-2 shape: plan words 1..13 and batch_bytes
    assert "16777216 65536 8 256 1 0 | 1 | 0 1 19 19 10 20 192 576 8 4096 4 8644 65536 256 0 0 0 | 63313152 " in got
    if got != want:
        bad = [(g, w) for g, w in zip(got.splitlines(), want.splitlines()) if g != w]
        raise AssertionError(f"{len(bad)} grid rows differ (or rows are missing); first: got {bad[:1]}")


def test_launch_decisions_match_recorded_and_invariants_hold(tmp_path):
    exe = str(tmp_path / "plan_check")
    subprocess.check_call(["g++", *WARN, "-O1", "-I", CSRC, os.path.join(ROOT, "tests", "cpp", "plan_check.cpp"),
                           os.path.join(CSRC, "batch_plan.cpp"), "-o", exe])
    run = subprocess.run([exe, os.path.join(GOLDEN, "sub_shapes.txt")], capture_output=True, text=True)
    assert run.returncode == 0, run.stderr[-4000:]   # exit 1: an invariant of the kernels is broken
    want = open(os.path.join(GOLDEN, "k6_decide.txt")).read()
    if run.stdout != want:
        bad = [(g, w) for g, w in zip(run.stdout.splitlines(), want.splitlines()) if g != w]
        raise AssertionError(f"{len(bad)} decisions differ (or rows are missing); first: got {bad[:1]}")
    forms = want.splitlines()[-1].split()   # "F2 forms: direct N narrow N segmented N sparse N dense N"
    assert forms[:2] == ["F2", "forms:"] and all(int(n) > 0 for n in forms[3::2]), forms


def test_listed_shapes_are_sub_partitioned():
    """Every shape of tests/golden/sub_shapes.txt on a 256-CU device: the library's plan query routes
    it to prefix sub-partitions, and its recorded rows (k6_decide.txt) carry that route, the order
    the shape is named for (.sorted / .unsorted) and the F2 that goes with it -- k_f2_direct (form 0)
    and one bucket set over sorted sub-partitions, a staged form read through the descriptor table
    (src 1 or 2) and 8 bucket sets over unsorted ones.  The GPU tests take their shapes from this
    list: when the planner moves, this fails here, on the CPU."""
    rows = open(os.path.join(GOLDEN, "k6_decide.txt")).read().splitlines()
    shapes = sub_shapes.load()
    assert len(shapes) >= 20 and {nm.rsplit(".", 1)[1] for nm, *_ in shapes} == {"sorted", "unsorted"}
    for name, n, q, k, qb in shapes:
        assert opendht_amd.batch_plan(n, q, k, num_cus=256)["route"] == opendht_amd.ROUTE_SUBS, (name, n, q, k)
        head = f"sub-shape {name} n {n} q {q} k {k} q_build {qb} | "
        at = [i for i, r in enumerate(rows) if r.startswith(head)]
        assert len(at) == 1, f"{name}: {len(at)} recorded rows"
        want_sorted = {"sorted": 1, "unsorted": 0}[name.rsplit(".", 1)[1]]
        route, nsub, srt = (int(rows[at[0]].split(" | ")[1].split()[j]) for j in (1, 3, 5))
        assert route == opendht_amd.ROUTE_SUBS and nsub >= 2 and srt == want_sorted, rows[at[0]]
        dec = rows[at[0] + 1]
        assert dec.startswith(f"{name} ") and f" nsub {nsub} q {q} " in dec and f" k {k} " in dec, dec
        plan = dec.split(" | ")[1].split()
        f2 = dec.split(" | ")[2].split()
        form, src, nsets = int(f2[2]), int(f2[4]), int(plan[8])
        assert src in (1, 2), dec
        if want_sorted:
            assert form == 0 and nsets == 1, dec
        else:
            assert form in (1, 2, 3, 4) and nsets == 8, dec
