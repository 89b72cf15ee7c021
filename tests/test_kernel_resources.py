"""Register and scratch budget of every kernel of the library (CPU test: hipcc cross-compiles gfx950).

A kernel that spills to scratch, or whose VGPRs cross an occupancy step, runs several times
slower without any change in its results: round 5's record-form stores inside the fallback scan's
unrolled result loop took F4 from 135 VGPRs to 221 + 752 B of scratch per lane and F4 from 7.5 to
25 us (profiles/r05/g), with every parity test green.  This pins the budget at build time, on the
compile lines of the shipped build (tests/kernel_budget.py).

CAPS: unit -> mangled-name fragment -> max VGPRs.  Every kernel of a unit matches exactly one
fragment, and a new kernel or a new unit without a cap fails.  The occupancy steps of gfx950 are 64,
72, 80, 96, 128, 168 and 256 VGPRs (8, 7, 6, 5, 4, 3, 2 waves / SIMD).  Where no reason is given the
cap is the top of the step in which the compiled count, in the comment beside it, lies."""
import pytest

import kernel_budget as KB

CAPS = {
    # the hot path: the occupancy each kernel is tuned for (measured values in the comments, round 5;
    # beside them the counts under the shipped flags, which give batch.hip's F3 one VGPR more)
    "batch": {
        "k_f2_filterI": 128,         # 109-111 (66-112): 4 waves / SIMD beside its 152 KB of LDS
        "k_f3_answerILi8E": 96,      # 69-78 (70-83) (the k <= 8 instantiations)
        "k_f3_answerILi16E": 168,    # 123-136 (r05), 141-145 with round 6's record word 0 from the stage (124-146): 3 waves / SIMD up to 168
        "k_f3_answerILi32E": 256,    # 221-252
        "k_f4I": 144,                # 139 (141): 3 waves / SIMD
        "k_s1_filterI": 128,         # (50-58)
        "k_s2_answerI": 144,         # (142)
        "k_f2_directI": 64,          # 32
        "k_f1_targetsE": 64,         # 16
        "k_f1_coarseE": 64,          # 28
        "k_f1_fineE": 64,            # 60
        "k_shift_w0E": 64,           # 8
        "k_cell_countE": 64,         # 6
        "k_cell_packE": 64,          # 4
        "k_cell_spansE": 64,         # 42
        "k_handles_to_idxE": 64,     # 14
        "k_idx_to_handlesE": 64,     # 4
        "k_handle_inverseE": 64,     # 10
        "k_fb_handlesE": 64,         # 15
    },
    "scan": {
        "k_merge3I": 64,             # 48-52
        "k_scanI": 128,              # 109
        "k_mergeE": 64,              # 14
        "k_merge_fullI": 64,         # 16-45
        "k_merge_headsI": 64,        # 16-44
        "k_map_idxE": 64,            # 6
        "k_rec3E": 64,               # 12
        "k_tie_wordsE": 64,          # 12
    },
    "table": {
        "k_classifyE": 128,          # K2 99 (120): one 1,024-thread workgroup per CU (4 waves / SIMD)
        "k_cachedE": 64,             # 27
        "k_find_closestILj8E": 64,   # 58
        "k_find_closestILj16E": 96,  # 88
        "k_find_closestILj32E": 168, # 154
    },
    "keys": {
        "k_genE": 64,                # 27
        "k_packE": 64,               # 19
        "k_unpackE": 64,             # 15
        "k_fillE": 64,               # 5
        "k_check_sortedE": 64,       # 14
        "k_sel_countE": 64,          # 8
        "k_sel_compactE": 64,        # 24
    },
    "index": {
        "k_p0_histE": 64,            # 20
        "k_p1_scatterE": 128,        # 120
        "k_p2_bucketsE": 64,         # 40
        "k_queryE": 64,              # 30
    },
    "sort": {
        "k_sort_histE": 64,          # 8
        "k_sort_scatterE": 64,       # 42
        "k_iotaE": 64,               # 4
        "k_adjacent_equalE": 64,     # 10
    },
    "wire": {
        "k_wire_encodeE": 64,        # 19
        "k_wire_decodeE": 64,        # 25
    },
    "crawl": {
        "k_net_sortE": 64,           # 12
        "k_searchE": 128,            # 109
    },
    "search": {
        "k_search_insertE": 64,      # 42
        "k_table_statsE": 64,        # 16
    },
    # The compaction runs on every mask change: it stays within the 4-waves-per-SIMD step (4
    # workgroups of 33 KB of LDS per CU).
    "view": {
        "k_view_compactE": 128,      # 104
        "k_view_packE": 64,          # 25
        "k_view_trimE": 64,          # 2
        "k_view_countE": 64,         # 8
        "k_view_addE": 64,           # 7
    },
    # The shared primitives' kernels, which took over the scan of the block counts and the indexed
    # setters of the nc, rt and sr families (update_good's, update_state's byte setter) under their cap.
    "prims": {
        "k_scan_rowsIjE": 64,        # 12  u32 totals
        "k_scan_rowsIyE": 64,        # 12  u64 totals
        "k_bits_updateE": 64,        # 9
        "k_bytes_updateE": 64,       # 8
    },
    # Every k_rt instantiation is built for 8 waves / SIMD (one wave per target: occupancy is what
    # hides the dependent loads), i.e. at most 64 VGPRs; compiled:
    "rtable": {
        "k_rtILi0ELj8E": 64,         # 18  indices, K = 8
        "k_rtILi0ELj16E": 64,        # 18  indices, K = 16
        "k_rtILi0ELj32E": 64,        # 21  indices, K = 32
        "k_rtILi1ELj8E": 64,         # 18  reply (count 8 only)
        "k_rtILi2ELj8E": 64,         # 17  closer, K = 8
        "k_rtILi2ELj16E": 64,        # 17  closer, K = 16
        "k_rtILi2ELj32E": 64,        # 20  closer, K = 32
        "k_rt_gpreE": 64,            # 42
    },
    # Each a few registers above the figure this compile prints (beside it).  The two table kernels
    # run as one workgroup, so their cap guards against a spill, not for occupancy; the three
    # one-thread-per-entry kernels keep 8 waves / SIMD.  (Their LDS: tests/test_rtgrow_cpu.py.)
    "rtgrow": {
        "k_rtgILb0E": 64,            # 59  onNewNode batch
        "k_rtgILb1E": 36,            # 31  expireBuckets
        "k_rtg_set_stateE": 12,      # 6
        "k_rtg_updateE": 12,         # 6
        "k_rtg_handlesE": 10,        # 4
    },
    # One wave per target (k_nc) and streaming passes: every kernel is built for 8 waves / SIMD, i.e.
    # at most 64 VGPRs, the next occupancy step above what the compiler reports; compiled:
    "ncache": {
        "k_ncE": 64,                 # 33  the lookup
        "k_nc_rankILb0E": 64,        # 20  insert
        "k_nc_rankILb1E": 64,        # 20  erase
        "k_nc_compactE": 64,         # 14
        "k_nc_mergeILb0E": 64,       # 16  insert
        "k_nc_mergeILb1E": 64,       # 11  erase
        "k_nc_handlesE": 64,         # 6
        "k_nc_bits_packE": 64,       # 15
    },
    # The find holds a key, a range and one pivot; the others are streaming passes: every kernel is
    # built for 8 waves / SIMD, i.e. at most 64 VGPRs; compiled:
    "ncresolve": {
        "k_ncr_findILj64EE": 64,     # 24  one wave per key
        "k_ncr_findILj16EE": 64,     # 24  16 lanes per key
        "k_ncr_orderILb1EE": 64,     # 5   the blocks' counts
        "k_ncr_orderILb0EE": 64,     # 14  the positions
        "k_ncr_assignE": 64,         # 22
        "k_ncr_extractE": 64,        # 6
    },
    # One wave per search: every kernel is built for 8 waves / SIMD, i.e. at most 64 VGPRs, the
    # occupancy step at or above what the compiler reports; compiled:
    "rsearch": {
        "k_sr_insertE": 64,          # 32
        "k_sr_refillE": 64,          # 43  the walk's two windows + the row
        "k_sr_openE": 64,            # 20
        "k_sr_expireE": 64,          # 4
        "k_sr_candidateE": 64,       # 5
        "k_sr_statusE": 64,          # 6
        "k_sr_listsE": 64,           # 6
    },
    # The filter and the small kernels are built for 8 waves / SIMD (64 VGPRs); the walk is one
    # workgroup of 8 waves and nothing shares its CU, capped at the same step.
    "srmap": {
        "k_srm_gatherE": 64,         # 13
        "k_srm_orderE": 64,          # 4
        "k_srm_doneE": 64,           # 5
        "k_srm_filterE": 64,         # 19
        "k_srm_walkE": 64,           # 31
    },
}

def test_every_kernel_unit_has_a_budget():
    """CAPS names exactly the Makefile's kernel units (SRCS without api*): a new .hip needs a table"""
    assert sorted(CAPS) == sorted(KB.kernel_units())


@pytest.fixture(scope="module")
def compiled(request):
    """the remarks of the units this session selected, compiled side by side"""
    KB.compile_all([i.callspec.params["unit"] for i in request.session.items
                    if getattr(i, "function", None) is test_no_scratch_and_vgpr_budget])


@pytest.mark.skipif(KB.HIPCC is None, reason="hipcc not installed")
@pytest.mark.parametrize("unit", list(CAPS))
def test_no_scratch_and_vgpr_budget(compiled, unit):
    KB.check(unit, CAPS[unit])
