// batch_plan.h -- what K6's kernels (batch.hip) and its host planning (batch_plan.cpp) share:
// the geometry constants, the two LDS-layout formulas both sides evaluate, the sub-partition
// descriptors, and the plan / layout / launch-decision values.  Host-only C++17: no HIP header,
// so the planning compiles, runs and is tested without a device (tests/cpp/plan_check.cpp).
#ifndef DHTGPU_BATCH_PLAN_H
#define DHTGPU_BATCH_PLAN_H
#include <stddef.h>
#include <stdint.h>

#ifdef __HIPCC__
#define K6_HOST_DEVICE __host__ __device__
#else
#define K6_HOST_DEVICE
#endif

namespace dhtgpu {

// ID-plane geometry: planes are padded to a multiple of kTile ids so that the scan
// kernel can stream whole tiles without bounds checks.
constexpr uint32_t kTile = 4096;
constexpr uint32_t kScanWaves = 8;       // waves per scan workgroup
constexpr uint32_t kScanTargets = 16;    // targets held (wave-uniform) per wave
constexpr uint32_t kLdsBytes = 160 * 1024;   // LDS per CU (gfx950)

inline uint64_t pad_ids(uint64_t n) { return ((n + kTile - 1) / kTile) * kTile; }

constexpr uint32_t kMaxK = 32;                       // = DHTGPU_MAX_K of include/dhtgpu.h
constexpr int kF1Threads = 256;                      // one thread per target
constexpr int kF3Threads = 256;
constexpr uint32_t kF3Cap = 4096;                    // survivors per partition staged in LDS
constexpr uint32_t kMaxLm = 19;                      // 2^19-bit bitmap = 64 KB of LDS in F2
constexpr uint32_t kMaxSubBits = 11;                 // F3 sub-prefix histogram <= 2048 bins
constexpr uint32_t kMaxQ = 1u << 22;                 // targets per call
constexpr uint32_t kTieSlots = 8;                    // deferred-tie slots per F3 partition
// F1's per-target bucket counters tcount[p] sit 256 B apart: their returning atomics execute
// at the memory side, one request per lane (random partitions), and counters packed into one
// 4 KB run would all queue on the same channel.  F2's pcount stays packed: its flush reserves
// consecutive partitions from consecutive lanes, which coalesce into one request per line.
// F2's survivor buckets come in kSets sets, one per XCD (block b uses set b % 8: blocks b and
// b + 8 share an XCD): a counter then takes 32 blocks' reservations instead of 256 (one
// address completes about 88 returning atomics per µs), and a bucket's partial-line runs are
// all written through one XCD's L2, which merges them into whole lines.  F3 gathers a
// partition from its kSets contiguous buckets.
constexpr uint32_t kSets = 8;
constexpr uint32_t kCtrStride = 64;

// F1's two-pass form (batch.hip: k_f1_coarse + k_f1_fine)
constexpr uint32_t kF1aThreads = 1024, kF1aPer = 4, kF1aTargets = kF1aThreads * kF1aPer;
constexpr uint32_t kMaxCoarse = 4096;             // bins (the coarse counters live in the clean head)
constexpr uint32_t kF1bLdsWords = 16384;          // F1b's bitmap words + partition counts (64 KB)
constexpr uint32_t kF1CoarseMinQ = 1u << 17;      // smaller batches: k_f1_targets (at 2^17 F1 is as fast either
                                                  // way, 13.1-13.4 us, and the two-pass form leaves the other call
                                                  // in flight the atomics: prefix rank 0.130-0.135 -> 0.127-0.128 ms)

// F2 (batch.hip: k_f2_filter, k_f2_direct)
constexpr int kF2Threads = 1024;
constexpr uint32_t kF2Sub = 4 * kF2Threads;          // ids per sub-step (one uint4 per thread)
constexpr uint32_t kF2Step = 4 * kF2Sub;             // ids per chunk
constexpr uint32_t kStage = 11264;                   // LDS stage entries (88 KB)
// F2's ring: 2 sub-steps = 32 KB in flight per CU.  A pure 64 MB stream by one 1024-thread
// workgroup per CU (tools/experiments/stream_probe.hip, profiles/r03/experiments) takes
// 13.3 us with 8 (128 KB in flight), 11.7 with 4, 11.1 with 3, 10.3 with 2: a deeper ring only
// queues longer.  F2 at cfg 2: 21.9 us with 4, 21.3 with 3, 20.7 with 2 (round 2: 8, 24.1 us)
constexpr uint32_t kF2Ring = 2;
// Modes: kF2Dense flushes the stage whenever a sub-step could overflow it (one barrier
// per sub-step); kF2Sparse (the plan proved a block's survivors fit the stage) has no
// barrier in the loop and flushes once at the end; kF2Seg is kF2Sparse with a flush every
// a.seg ids (ranges longer than one stage-full: large sub-partitioned sets) -- its own
// instantiation, because the flush inlined in the loop keeps the ring live across it (128
// VGPRs, the whole register file at 16 waves per CU, where kF2Sparse needs 68 and leaves
// room for the other stream's F1 / F4 waves).
// kF2Narrow is kF2Sparse over the 6-B narrow stage (a workgroup's range < 2^16 ids).
constexpr uint32_t kF2Dense = 0, kF2Sparse = 1, kF2Seg = 3, kF2Narrow = 4;
// Src: kF2One -- one set: its descriptor from the kernel arguments, the ring through plain
// global loads; kF2Subs -- several sub-partitions (descriptors read from memory, the ring
// through buffer loads); kF2SubsNT -- the same with non-temporal ring loads, for sets whose w0
// planes exceed the Infinity Cache (kNtBytes): the stream then no longer evicts the survivor
// and target buckets F3 / F4 read next (cfg-3 shard: F2 118 -> 103 us, F3 43 -> 38, F4 19 ->
// 17, profiles/r03/experiments/stream_nt_ab.txt).  A set the cache holds keeps cached loads:
// non-temporal ones re-read it from HBM every call (cfg 2: F2 20.5 -> 22.9 us).
constexpr uint32_t kF2One = 0, kF2Subs = 1, kF2SubsNT = 2;
constexpr uint64_t kNtBytes = 192ull << 20;   // 3/4 of the 256 MB Infinity Cache
constexpr uint32_t kDirParts = 4096;   // k_f2_direct's LDS counters: partitions a range may own (more: global atomics)

// F2's LDS words ahead of its stage (k_f2_filter's layout)
K6_HOST_DEVICE inline uint32_t f2_fixed_words(uint32_t nwords, uint32_t np) {
    return (36 + nwords + np + 1 + 17 + np / 32 + 1 + 3) & ~3u;
}
// F3's LDS words ahead of its stage (k_f3_answer's layout; nsub sort bins)
K6_HOST_DEVICE inline uint32_t f3_words(uint32_t nsub) {
    return (nsub + 1 + 17 + kF3Threads + 1 + 2 + 1) & ~1u;
}

// F4 (batch.hip: k_f4) and KS (k_s1_filter, k_s2_answer)
constexpr uint32_t kFbGroup = kScanWaves * kScanTargets;          // targets per scan role
constexpr uint32_t kFbBlocks = 256;                                // fallback-scan workgroups
constexpr uint32_t kF4IdleGrid = 32;                               // F4's grid after a call that listed no target
constexpr uint32_t kSmallQ = 64;
constexpr uint32_t kSmallCap = 512;                   // candidates per prefix bucket
constexpr uint32_t kSmallFbBlocks = 32;               // K1 fallback scan workgroups (S2's scan roles)

constexpr uint32_t kMaxParts = 1u << 15;
constexpr uint32_t kMaxSubs = 256;            // F2's workgroup -> sub-partition map is u8
constexpr uint32_t kMaxF2Blocks = 65536;

// pf (plan flags): kPlanCells -- the sub-partitions' level-cell_level() id counts (launch_cell_counts)
// are available, which lets the plan mark one level finer with sibling marking (BatchCall::cells);
// kPlanSorted -- the sub-partitions are sorted by prefix (one bucket set per partition, survivors
// of an F2 range clustered in whole cells; BatchCall::sorted)
constexpr uint32_t kPlanCells = 1u, kPlanSorted = 2u;

// One prefix sub-partition of a K6 call's id set (host view; see SubDesc).
struct SubSpec {
    const uint32_t* planes; const uint32_t* w0s;   // unshifted planes; shifted word-0 plane (nullable)
    uint64_t stride, n;
    const uint32_t* gidx; uint32_t base;           // result index map (nullable) or offset
};

// Prefix sub-partitions (dhtgpu_ctx: a set too large for one plan is split by the next
// sub_bits id bits after its shard prefix, each part compacted with its own shifted word-0
// plane): ONE launch sequence serves all of them.  A target's sub-partition is its bits
// [sub_shift, sub_shift + sub_bits); every sub-partition has its own bitmap and its own np
// partitions (global partition = sub * np + p); F2's workgroups are dealt to the
// sub-partitions in proportion to their ids; F3 / F4 read the tie words and map the results
// through the target's sub-partition.  A set that needs no split is the one sub-partition.
struct SubDesc {
    const uint32_t* w0;       // streamed word-0 plane (shifted for shards / sub-partitions)
    const uint32_t* planes;   // unshifted word planes (tie words)
    uint64_t stride, n;
    const uint32_t* gidx;     // result index map (nullable) ...
    uint32_t base;            // ... or offset
    uint32_t lim;             // last 16-B aligned word offset loadable inside w0's allocation
    uint32_t blk0, nblk;      // its F2 workgroups
    uint64_t per_blk;         // F2 ids per workgroup
};

struct BatchPlan {
    uint32_t Lm, b1, Lq, nwords, nblk1, nblk2, stage, sparse, tcap;
    uint32_t sib;    // 1: sibling marking from the set's level-Lm cell counts (Lmin = Lm - 1)
    uint32_t nstage; // F2's narrow stage entries (6 B each; 0: none) -- F2 then leaves room for an F3 workgroup
    uint32_t f3cap;  // F3's LDS stage entries (kF3Cap, or the 6-sigma bound when that buys a 4th workgroup per CU)
    uint32_t scap;   // survivors per (bucket set, partition)
    uint32_t f3cap_wide;   // F3's LDS stage entries when F2 runs its 8-B stage (no narrow stage)
    uint32_t cap6;         // the plan's 6-sigma partition bound (F3 stage entries, <= kF3Cap)
    uint32_t nsets;        // F2 bucket sets per partition: kSets, or 1 over prefix-sorted sub-partitions
    // variance of an F2 range's survivor count per expected survivor: ids of a range are a random
    // sample (1 - f), or -- prefix-sorted sub-partitions -- whole level-Lm cells of mu ids each,
    // marked with probability f ((1 - f) mu + 1: ~30x the binomial at the cfg-3 shard)
    double clump;
    bool fits;   // partitions' survivors fit the F3 stage on uniform ids
    uint64_t per_blk;
};

// workspace: bitmap[nsub][nwords] | ctr[64] | pcount[kSets][NP] | tcount[kMaxParts * kCtrStride] |
// tie_hdr[NP * kTieSlots] | fb done[kFbBlocks] | tie_cnt[NP] -- all-zero between calls -- |
// fb_list[q] | tspill[q] | pstat[NP] | tbuf[NP * tcap] | tie_cand[NP * kTieSlots * 64] |
// pbuf[NP * kSets * scap] | fb rec[kFbBlocks * kFbGroup * k * 6] | sub descriptors | F2 map
// (NP = nsub * np partitions over all sub-partitions)
struct WsLayout {
    size_t ctr, bitmap, pcount, tcount, tie_hdr, fb_done, tie_cnt, ccount, clean;
    size_t fb_list, fb_sub, tspill, pstat, tbuf, tie_cand, pbuf, fb_rec, desc, blk_sub, cbuf, total;
};

// F1's two-pass form (k_f1_coarse + k_f1_fine) for batches of >= kF1CoarseMinQ targets: the
// coarse bins are the finest split (<= b1 and Lm - 5 bits per sub-partition) that keeps >= 512
// targets per bin and >= 16 per (F1a workgroup, bin) -- each reservation a run of >= 128 B (2,048
// bins at 2^20 targets left 2 per run: F1a 34 us, 524 K reservations) -- with F1b's LDS within
// kF1bLdsWords.  c = ~0u: one pass.
struct F1Coarse { uint32_t c, nbins, ccap; };

// What a launch does with its plan once F2's workgroups are dealt (the plan query
// dhtgpu_batch_plan reports the same values): whether some workgroup's range spans more
// than one segment, whether F2 runs the narrow stage, F2's mode among the stage-sorting
// instantiations (the direct form is chosen by decide_batch), the stage entries F2 and
// F3 are given, and whether F1 runs as coarse + fine.
struct BatchRoute {
    bool seg_used, narrow, f1_two_pass;
    uint32_t f2_mode, f2_stage, f3_cap;
    F1Coarse f1c;
};

BatchPlan plan_batch(uint64_t n, uint32_t q, uint32_t k, int num_cus, uint32_t pf = 0);
F1Coarse f1_coarse(const BatchPlan& P, uint32_t nsub, uint32_t q);
WsLayout ws_layout(const BatchPlan& P, uint32_t nsub, uint32_t q, uint32_t k);
size_t f2_lds(const BatchPlan& P, bool narrow = false);
size_t f3_lds(const BatchPlan& P, uint32_t cap);
uint32_t deal_f2_blocks(const BatchPlan& P, const SubSpec* subs, uint32_t nsub, uint32_t q_plan, int num_cus,
                        SubDesc* d, uint32_t* seg);
BatchRoute route_batch(const BatchPlan& P, const SubDesc* hd, uint32_t nsub, uint32_t seg, bool direct, uint32_t q,
                       uint32_t q_plan);
// F4 scratch for a list scan: done counters | split records
size_t list_scan_bytes(uint32_t k);

// K6 per-batch target-prefix filter + exact top-k (no persistent index).
// n: ids of the largest sub-partition (or of the set); q_plan: the targets one sub-partition
// is planned for (q / nsub); nsub: sub-partitions served by the call (1: the set itself).
bool batch_supported(uint64_t n, uint32_t q_plan, uint32_t k, int num_cus, uint32_t nsub = 1, uint32_t pf = 0);
size_t batch_bytes(uint64_t n, uint32_t q, uint32_t q_plan, uint32_t k, int num_cus, uint32_t nsub = 1, uint32_t pf = 0);
// leading workspace bytes that must be zero before a call (the call leaves them zero)
size_t batch_clean_bytes(uint64_t n, uint32_t q_plan, uint32_t k, int num_cus, uint32_t nsub = 1, uint32_t pf = 0);
// offset of the shared counters in the workspace head: their words 0..3 (the call's statistics, read by
// batch_read_stats) stay set after a call, so a head laid out with them elsewhere is zeroed again
size_t batch_ctr_offset(uint64_t n, uint32_t q_plan, uint32_t k, int num_cus, uint32_t nsub = 1, uint32_t pf = 0);
// The routing rules of a call over a set past one plan (api_batch.hip: batch_run, batch_run_subs).
// Sub-partition split of n ids: the smallest s in [1, 8] with 2^s parts of <= 2^24 expected ids.
uint32_t split_bits(uint64_t n);
// the set is served over prefix sub-partitions: no one-set plan accepts the call
bool needs_subs(int num_cus, uint64_t n, uint32_t q, uint32_t k);
// the call that builds the sub-partitions sorts them by prefix: more than 2 % of the ids are
// expected to survive its F2
bool subs_sort_rule(uint64_t n, uint32_t q, uint32_t k);
// KS: batches of at most kSmallQ targets (batch.hip: launch_small_topk)
bool small_supported(uint64_t n, uint32_t q, uint32_t k);
uint32_t small_level(uint64_t n, uint32_t k);   // KS's prefix level Ls
size_t small_bytes();
// words 1..13 of dhtgpu_batch_plan (include/dhtgpu.h) for a one-set K6 call that batch_supported
// accepts: the plan and what launch_batch_topk makes of it, from the launch's own decision
void batch_plan_words(uint64_t n, uint32_t q, uint32_t k, int num_cus, uint32_t* out16);

// Everything launch_batch_topk decides before it touches the workspace, as values.
enum class F2Form : uint32_t { Direct, Narrow, Seg, Sparse, Dense };   // k_f2_direct, or k_f2_filter's Mode
enum class F2Src : uint32_t { One, Subs, SubsNT };                     // kF2One / kF2Subs / kF2SubsNT
struct BatchShape {
    const SubSpec* subs; uint32_t nsub;   // the sub-partitions (one: the set itself)
    uint32_t q, q_plan, k;
    int num_cus;
    uint32_t pf;                          // plan flags
    const uint32_t* spans;                // nullable, host: [nsub][32] cell spans (sorted sub-partitions)
    uint64_t n;                           // ids of the whole set (BatchCall::n)
    uint32_t dbg;                         // the stamp bit (256) or 0
    bool fb_idle;                         // the fallback hint is present and reads 0
};
struct BatchDecision {
    BatchPlan P;              // the plan: the launch's and the workspace layout's
    uint32_t nblk2, seg;      // F2's workgroups; ids per segment (the staged deal's)
    bool direct, nt;          // k_f2_direct; non-temporal ring loads
    uint32_t wwords;          // direct: bitmap window words in LDS per workgroup
    BatchRoute R;
    uint32_t f3_cap;          // F3's stage entries of the launch
    size_t f2_lds, f3_lds;
    F2Form f2_form; F2Src f2_src;
    uint32_t f3_k;            // F3's / F4's K bucket: 8, 16 or 32
    bool f3_diag, f3_exact, f3_subs;
    uint32_t f4_grid;
    uint32_t dbg;             // the stamp bit where the stamp buffers hold the grids
};
// hd: caller-provided SubDesc[kMaxSubs], filled with the sub-partitions' descriptors.  False: the
// call is refused (more F2 workgroups than the map holds).
bool decide_batch(const BatchShape& c, SubDesc* hd, BatchDecision* D);

}  // namespace dhtgpu

#endif  // DHTGPU_BATCH_PLAN_H
