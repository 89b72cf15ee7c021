// plan_check -- K6's launch decision (opendht_amd/csrc/batch_plan.cpp: decide_batch) over a fixed
// list of call shapes, one line per shape, and for every shape the invariants the kernels rely on.
// Compiled together with batch_plan.cpp alone: no library, no HIP, no device.
// tests/test_batch_plan.py compares the output with tests/golden/k6_decide.txt; a broken
// invariant ends the run with exit status 1.  The named shapes print their whole decision; the
// grids print one line per group with the number of shapes and a hash over their decision lines
// (`plan_check -v` prints every line, to find the shape behind a changed hash).
//
// Shapes: the one-set grid; sub-partitioned shapes with span tables (uneven and empty
// sub-partitions, every plan-flag combination); the shapes of bench.py's cfg-3 legs and further
// recorded sets of 2^25 .. 1.25e8 ids, split and planned whatever route the library gives them; span
// tables that refuse k_f2_direct on each of its three conditions; the sub-partitioned shapes the
// GPU tests run (`plan_check [-v] tests/golden/sub_shapes.txt`), each with the route the library
// takes (batch_run's order of decisions), its split and the order its sub-partitions are built
// in; and the constructed sub-partition sizes and span tables of tests/test_gpu_subs.py.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>

#include <stdarg.h>

#include <algorithm>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "batch_plan.h"

using namespace dhtgpu;

static int g_bad = 0;
#define CHECK(cond, ...)                                      \
    do {                                                      \
        if (!(cond)) {                                        \
            fprintf(stderr, "plan_check: %s: ", #cond);       \
            fprintf(stderr, __VA_ARGS__);                     \
            fprintf(stderr, "\n");                            \
            ++g_bad;                                          \
        }                                                     \
    } while (0)

static uint64_t g_rng = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() {   // splitmix64
    uint64_t z = (g_rng += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// the span table of a prefix-sorted sub-partition of n uniform ids: 2^j consecutive ids span about
// 2^j 2^19 / n level-19 cells (times `slack`, plus a few)
static void uniform_spans(uint64_t n, double slack, uint32_t* sp) {
    for (uint32_t j = 0; j < 32; ++j) {
        const double cells = n ? (double)(1ull << j) * 524288.0 / (double)n * slack + 8.0 : 0.0;
        sp[j] = (uint32_t)std::min(cells, 524288.0);
    }
}

// output: a decision line is printed (named shapes, -v) or hashed into the open group
static bool g_verbose = false;
static std::string g_group, g_line;
static uint64_t g_hash = 0;
static uint32_t g_count = 0, g_forms[5] = {0, 0, 0, 0, 0};
static void add(const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_line += buf;
}
static void close_group() {
    if (g_count) printf("%s: %u shapes, hash %016llx\n", g_group.c_str(), g_count, (unsigned long long)g_hash);
    g_count = 0;
}
static void open_group(const std::string& name) {
    close_group();
    g_group = name;
    g_hash = 1469598103934665603ull;
}
static void end_line(bool named) {
    if (named || g_verbose) printf("%s\n", g_line.c_str());
    if (!named) {
        for (char ch : g_line) g_hash = (g_hash ^ (uint8_t)ch) * 1099511628211ull;
        ++g_count;
    }
    g_line.clear();
}

struct Case {
    const char* tag;
    std::vector<uint64_t> n;   // ids per sub-partition
    uint32_t q, q_plan, k;
    int cus;
    uint32_t pf;
    std::vector<uint32_t> spans;   // empty: none
    uint32_t dbg;
    bool fb_idle;
};

static void run(const Case& c, bool named = false) {
    const uint32_t nsub = (uint32_t)c.n.size();
    std::vector<SubSpec> specs(nsub);
    uint64_t n_max = 0, n_all = 0;
    for (uint32_t i = 0; i < nsub; ++i) {
        // (addresses are never read by the planning: a non-null shifted plane marks sub-partitions)
        specs[i] = SubSpec{nullptr, nsub > 1 ? reinterpret_cast<const uint32_t*>(16) : nullptr, pad_ids(c.n[i] ? c.n[i] : 1),
                           c.n[i], nullptr, 0u};
        n_max = std::max(n_max, c.n[i]);
        n_all += c.n[i];
    }
    add("%s n_max %llu nsub %u q %u qp %u k %u cus %d pf %u dbg %u idle %d |", c.tag, (unsigned long long)n_max, nsub, c.q,
           c.q_plan, c.k, c.cus, c.pf, c.dbg, c.fb_idle ? 1 : 0);
    if (!batch_supported(n_max, c.q_plan, c.k, c.cus, nsub, c.pf)) {
        add(" unsupported");
        end_line(named);
        return;
    }
    static SubDesc hd[kMaxSubs];
    BatchDecision D;
    const BatchShape shape{specs.data(), nsub, c.q, c.q_plan, c.k, c.cus, c.pf, c.spans.empty() ? nullptr : c.spans.data(),
                           n_all, c.dbg, c.fb_idle};
    if (!decide_batch(shape, hd, &D)) {
        add(" refused");
        end_line(named);
        return;
    }
    const BatchPlan& P = D.P;
    uint64_t sig = 1469598103934665603ull;
    for (uint32_t i = 0; i < nsub; ++i)
        for (uint64_t v : {(uint64_t)hd[i].blk0, (uint64_t)hd[i].nblk, hd[i].per_blk, (uint64_t)hd[i].lim, hd[i].n})
            sig = (sig ^ v) * 1099511628211ull;
    add(" plan %u %u %u %u %u %u %u %u %u %u %u %u %u %u %u |", P.Lm, P.sib, P.b1, P.Lq, P.nwords, P.tcap, P.scap, P.nsets,
           P.stage, P.nstage, P.sparse, P.f3cap, P.f3cap_wide, P.cap6, P.fits ? 1 : 0);
    add(" f2 form %u src %u blocks %u seg %u wwords %u lds %zu stage %u desc %016llx |", (uint32_t)D.f2_form, (uint32_t)D.f2_src,
           D.nblk2, D.seg, D.wwords, D.f2_lds, D.R.f2_stage, (unsigned long long)sig);
    add(" f1 %d %u %u %u | f3 k %u diag %d exact %d subs %d cap %u lds %zu | f4 %u | dbg %u", D.R.f1_two_pass ? 1 : 0,
           D.R.f1c.c, D.R.f1c.nbins, D.R.f1c.ccap, D.f3_k, D.f3_diag ? 1 : 0, D.f3_exact ? 1 : 0, D.f3_subs ? 1 : 0, D.f3_cap,
           D.f3_lds, D.f4_grid, D.dbg);
    end_line(named);
    ++g_forms[(uint32_t)D.f2_form];

    // ---- what the kernels rely on ----
    CHECK(D.f2_lds <= kLdsBytes && D.f3_lds <= kLdsBytes, "%s: LDS %zu / %zu", c.tag, D.f2_lds, D.f3_lds);
    CHECK(D.nblk2 <= kMaxF2Blocks, "%s: %u F2 workgroups", c.tag, D.nblk2);
    CHECK((D.f2_form == F2Form::Direct) == D.direct, "%s: form", c.tag);
    CHECK(D.f2_form != F2Form::Direct || nsub > 1, "%s: direct over one set", c.tag);
    CHECK((D.f2_src == F2Src::One) == (nsub == 1), "%s: source", c.tag);
    uint32_t blk = 0;
    for (uint32_t i = 0; i < nsub; ++i) {
        const SubDesc& d = hd[i];
        CHECK(d.blk0 == blk, "%s: sub %u starts at %u, not %u", c.tag, i, d.blk0, blk);
        CHECK(d.n == c.n[i], "%s: sub %u ids", c.tag, i);
        CHECK(d.per_blk && d.per_blk % kF2Step == 0, "%s: sub %u range %llu", c.tag, i, (unsigned long long)d.per_blk);
        CHECK((uint64_t)d.nblk * d.per_blk >= d.n && (d.nblk == 0 ? d.n == 0 : (uint64_t)(d.nblk - 1) * d.per_blk < d.n),
              "%s: sub %u: %u ranges of %llu over %llu ids", c.tag, i, d.nblk, (unsigned long long)d.per_blk,
              (unsigned long long)d.n);
        CHECK(d.per_blk <= D.seg || D.f2_form == F2Form::Seg || D.f2_form == F2Form::Dense || D.f2_form == F2Form::Direct ||
                  d.nblk == 0,
              "%s: sub %u: a range past one segment in form %u", c.tag, i, (uint32_t)D.f2_form);
        blk += d.nblk;
    }
    CHECK(blk == D.nblk2, "%s: %u workgroups dealt, %u launched", c.tag, blk, D.nblk2);
    if (D.direct) {
        const uint32_t w = D.wwords;
        CHECK(w >= 64 && w <= 2048 && (w & (w - 1)) == 0 && 2 * w <= P.nwords, "%s: window %u of %u words", c.tag, w, P.nwords);
        CHECK(P.nsets == 1, "%s: direct with %u bucket sets", c.tag, P.nsets);
        // k_f2_direct counts a range's partitions p_first + pl, pl < kDirParts, in LDS: the window
        // direct_window accepted (<= 2,045 words + 3) bounds the level-Lm cells between a range's
        // first and last id, hence the partitions between them, by (cells >> (Lm - b1)) + 1
        for (uint32_t i = 0; i < nsub; ++i) {
            if (!hd[i].nblk) continue;
            uint32_t j = 0;
            while (j < 31 && (1ull << j) < hd[i].per_blk) ++j;
            const uint32_t cells = (c.spans[i * 32 + j] >> (kMaxLm - P.Lm)) + 1;
            CHECK((cells >> (P.Lm - P.b1)) + 1 < kDirParts, "%s: sub %u: a range over %u level-%u cells, partitions of %u",
                  c.tag, i, cells, P.Lm, 1u << (P.Lm - P.b1));
        }
    } else {
        CHECK(D.R.f2_stage >= 1 && f2_fixed_words(P.nwords, 1u << P.b1) * 4 + (size_t)D.R.f2_stage * (D.R.narrow ? 6 : 8) == D.f2_lds,
              "%s: F2 LDS", c.tag);
    }
    const WsLayout L = ws_layout(D.P, nsub, c.q, c.k);
    const size_t off[] = {L.bitmap, L.ctr, L.pcount, L.tcount, L.tie_hdr, L.fb_done, L.tie_cnt, L.ccount, L.clean,
                          L.fb_sub, L.tspill, L.pstat, L.tbuf, L.tie_cand, L.pbuf, L.fb_rec, L.desc, L.blk_sub, L.cbuf};
    CHECK(L.clean == L.fb_list, "%s: clean head ends at %zu, fb_list at %zu", c.tag, L.clean, L.fb_list);
    for (size_t i = 0; i < sizeof off / sizeof off[0]; ++i) {
        CHECK(off[i] % 256 == 0, "%s: layout offset %zu = %zu", c.tag, i, off[i]);
        if (i) CHECK(off[i] > off[i - 1], "%s: layout offsets %zu, %zu", c.tag, off[i - 1], off[i]);
    }
    CHECK(L.cbuf <= L.total && L.total % 256 == 0, "%s: layout end", c.tag);
    CHECK(L.total == batch_bytes(n_max, c.q, c.q_plan, c.k, c.cus, nsub, c.pf), "%s: batch_bytes", c.tag);
    CHECK(L.clean == batch_clean_bytes(n_max, c.q_plan, c.k, c.cus, nsub, c.pf), "%s: batch_clean_bytes", c.tag);
    CHECK(L.ctr == batch_ctr_offset(n_max, c.q_plan, c.k, c.cus, nsub, c.pf), "%s: batch_ctr_offset", c.tag);
}

// a set of n ids split into 2^sb sub-partitions as the library does (uniform ids: n / 2^sb each,
// +- jitter), q targets, sorted or not; spans: uniform tables * slack
static Case subs_case(const char* tag, uint64_t n, uint32_t sb, uint32_t q, uint32_t k, int cus, uint32_t pf, double slack,
                      uint32_t jitter) {
    Case c{tag, {}, q, std::max<uint32_t>(1u, (uint32_t)(((uint64_t)q + (1u << sb) - 1) >> sb)), k, cus, pf, {}, 0u, false};
    const uint32_t S = 1u << sb;
    for (uint32_t i = 0; i < S; ++i) {
        const uint64_t base = n >> sb;
        c.n.push_back(jitter ? base - jitter + rnd() % (2ull * jitter + 1) : base);
    }
    if ((pf & kPlanSorted) && slack > 0.0) {
        c.spans.resize((size_t)S * 32);
        for (uint32_t i = 0; i < S; ++i) uniform_spans(c.n[i], slack, c.spans.data() + (size_t)i * 32);
    }
    return c;
}

// What dhtgpu_batch_plan reports in word 0 (api_batch.hip, batch_run's order of decisions)
static uint32_t route_of(uint64_t n, uint32_t q, uint32_t k, int cus) {
    if (small_supported(n, q, k)) return 0;
    if (needs_subs(cus, n, q, k)) return 2;
    return batch_supported(n, q, k, cus) ? 1 : 3;
}

// tests/golden/sub_shapes.txt: `name n q k [q_build]` per line.  For each shape at 256 CUs: the
// route, the split and whether the sub-partitions are built sorted (by the call itself, or by the
// earlier call of q_build targets), then the decision over even sub-partitions with that order
// (sorted: uniform span tables, as subs_case makes them)
static void listed_shapes(const char* path) {
    std::ifstream in(path);
    if (!in) {
        fprintf(stderr, "plan_check: cannot read %s\n", path);
        ++g_bad;
        return;
    }
    std::string line;
    std::vector<std::string> names;   // (the tags outlive the loop)
    while (std::getline(in, line)) {
        if (line.empty() || line[0] == '#') continue;
        std::istringstream is(line);
        std::string name;
        unsigned long long n = 0;
        uint32_t q = 0, k = 0, qb = 0;
        is >> name >> n >> q >> k;
        if (!(is >> qb)) qb = q;
        CHECK(n && q && k, "%s: malformed line", line.c_str());
        if (!n || !q || !k) continue;
        names.push_back(name);
        const uint32_t sb = split_bits(n);
        const bool sorted = subs_sort_rule(n, qb, k);
        printf("sub-shape %s n %llu q %u k %u q_build %u | route %u nsub %u sorted %d\n", name.c_str(), n, q, k, qb,
               route_of(n, q, k, 256), 1u << sb, sorted ? 1 : 0);
        run(subs_case(names.back().c_str(), n, sb, q, k, 256, kPlanCells | (sorted ? kPlanSorted : 0u), 1.25, 0), true);
    }
}

int main(int argc, char** argv) {
    int arg = 1;
    g_verbose = argc > arg && std::string(argv[arg]) == "-v";
    if (g_verbose) ++arg;
    const char* shapes = argc > arg ? argv[arg] : nullptr;
    // 1. the one-set grid
    const uint64_t ns[] = {1, 5, 40, 1000, 1ull << 15, (1ull << 17) - 1, 1ull << 17, 1ull << 20, (1ull << 24) - 3,
                           1ull << 24, 22400000ull, 1ull << 25, 1ull << 27, (1ull << 31) - 1};
    const uint32_t qs[] = {1, 64, 65, 8192, 65536, (1u << 17) - 1, 1u << 17, 1u << 20, 1u << 22};
    const uint32_t ks[] = {1, 8, 14, 16, 32};
    const int cus[] = {256, 64, 304, 0};
    for (uint64_t n : ns) {
        open_group("one-set grid, n = " + std::to_string(n));
        for (uint32_t q : qs)
            for (uint32_t k : ks)
                for (int cu : cus)
                    if (cu == 256 || cu == 304 || k == 8) run(Case{"one", {n}, q, q, k, cu, 0u, {}, 0u, false});
    }
    close_group();
    // the diagnostics bit and the idle fallback hint (one set)
    for (uint32_t dbg : {0u, 256u})
        for (bool idle : {false, true}) {
            run(Case{"one-flags", {1ull << 24}, 65536, 65536, 8, 256, 0u, {}, dbg, idle}, true);
            run(Case{"one-flags", {1ull << 20}, 1u << 20, 1u << 20, 16, 256, 0u, {}, dbg, idle}, true);
        }
    // 2. bench.py's cfg-3 legs and further recorded sets (uniform ids), split as the library would
    // split them and planned as sub-partitions whichever route it gives the shape (the shapes the
    // tests run, with their routes: 5. below)
    struct { const char* tag; uint64_t n; uint32_t q, k; } known[] = {
        {"cfg3-shard", 1ull << 27, 131072, 8},        {"cfg3-prefix-rank", 125000000ull, 131072, 8},
        {"cfg3-broadcast-rank", 125000000ull, 1u << 20, 8}, {"scale-2p26", 1ull << 26, 1u << 18, 8},
        {"scale-2p26-k16", 1ull << 26, 1u << 18, 16}, {"scale-2p26-k32", 1ull << 26, 1u << 18, 32},
        {"scale-2p25", 1ull << 25, 1u << 18, 8},      {"scale-2p25-k1", 1ull << 25, 1u << 18, 1},
        {"scale-2p25-k20", 1ull << 25, 1u << 18, 20}, {"scale-sibling", 40000000ull, 1u << 19, 8},
        {"scale-sibling", 40000000ull, 1u << 21, 8},
    };
    for (const auto& s : known) {
        uint32_t sb = 1;
        while (sb < 8 && (s.n >> sb) > (1ull << 24)) ++sb;
        // named: 256 CUs, even sub-partitions; hashed: 304 CUs and uneven sub-partitions
        for (uint32_t pf : {kPlanCells, kPlanCells | kPlanSorted}) run(subs_case(s.tag, s.n, sb, s.q, s.k, 256, pf, 1.25, 0), true);
        open_group(std::string(s.tag) + " q " + std::to_string(s.q) + ", 304 CUs / uneven");
        for (int cu : {256, 304})
            for (uint32_t pf : {kPlanCells, kPlanCells | kPlanSorted}) {
                if (cu == 304) run(subs_case(s.tag, s.n, sb, s.q, s.k, cu, pf, 1.25, 0));
                run(subs_case(s.tag, s.n, sb, s.q, s.k, cu, pf, 1.25, 50000));
            }
        close_group();
    }
    // 3. sub-partitioned shapes: every plan-flag combination, uneven and empty sub-partitions
    open_group("drawn sub-partitioned shapes");
    for (uint32_t i = 0; i < 48; ++i) {
        const uint32_t sb = 1 + (uint32_t)(rnd() % 8);
        const uint64_t per = 1ull << (15 + rnd() % 10);
        const uint32_t q = 1u << (8 + rnd() % 14);
        const uint32_t k = ks[rnd() % 5];
        Case c = subs_case("subs", (per + rnd() % per) << sb, sb, q, k, cus[rnd() % 4], (i & 1) ? 3u : (uint32_t)(rnd() % 4), 0.5 + (double)(rnd() % 8),
                           (uint32_t)(per / 4));
        if (i % 5 == 0) c.n[rnd() % c.n.size()] = 0;
        if (i % 7 == 0) c.n[rnd() % c.n.size()] /= 50;
        if ((c.pf & kPlanSorted) && !c.spans.empty())
            for (uint32_t s = 0; s < c.n.size(); ++s) uniform_spans(c.n[s], 1.0 + (double)(i % 4), c.spans.data() + (size_t)s * 32);
        run(c);
    }
    close_group();
    // 4. span tables that refuse k_f2_direct: a window past 2048 words; a window past half the
    // bitmap; more workgroups than the map holds
    {
        Case wide = subs_case("direct-refused-window", 1ull << 27, 3, 131072, 8, 256, kPlanCells | kPlanSorted, 64.0, 0);
        run(wide, true);
        Case all = subs_case("direct-refused-window", 1ull << 27, 3, 131072, 8, 256, kPlanCells | kPlanSorted, 1.0, 0);
        std::fill(all.spans.begin(), all.spans.end(), 524288u);   // clustered ids: a range may span every cell
        run(all, true);
        run(subs_case("direct-refused-half", 1ull << 14, 1, 4096, 8, 256, kPlanCells | kPlanSorted, 1.0, 0), true);
        run(subs_case("direct-refused-half", 1ull << 17, 2, 1u << 14, 8, 256, kPlanSorted, 1.0, 0), true);
        run(subs_case("direct-refused-blocks", ((1ull << 24) - 1) << 7, 7, 1u << 19, 8, 200000, kPlanCells | kPlanSorted, 1.0, 0), true);
        run(subs_case("direct-taken", 1ull << 27, 3, 1u << 20, 8, 256, kPlanCells | kPlanSorted, 1.0, 0), true);
    }
    // 5. the sub-partitioned shapes of the GPU tests
    if (shapes) listed_shapes(shapes);
    // 6. constructed sub-partitions of tests/test_gpu_subs.py and tests/test_gpu_scale.py (2^26 ids,
    // 4 sub-partitions, built sorted)
    {
        const uint32_t pf = kPlanCells | kPlanSorted;
        // ids [0, 2^19) of the stream replaced by 2^19 ids of one 26-bit prefix (sub-partition 1):
        // every sub-partition loses about 2^17 stream ids, the spans are those of the uniform rest (the
        // cluster lies in one level-19 cell) -- direct is still taken, and the cluster's partition is
        // shared by the three or more workgroups whose ranges it fills
        Case wg3 = subs_case("subs-one-partition-three-workgroups", 1ull << 26, 2, 1u << 17, 8, 256, pf, 1.25, 0);
        for (uint32_t i = 0; i < 4; ++i) {
            wg3.n[i] = (1ull << 24) - (1ull << 17);
            uniform_spans(wg3.n[i], 1.25, wg3.spans.data() + (size_t)i * 32);
        }
        wg3.n[1] += 1ull << 19;
        run(wg3, true);
        // ids [0, 2^16) replaced by copies of other stream ids: equal ids, spans unchanged
        run(subs_case("subs-equal-ids", 1ull << 26, 2, 1u << 17, 8, 256, pf, 1.25, 0), true);
        // test_subpartition_with_fewer_than_k_ids: sub-partition 3 emptied down to 5 ids (they span most
        // of its 2^19 cells), its other ids moved into sub-partition 1 -- the window of the 5-id
        // sub-partition's one workgroup is past 2,048 words, so direct is refused: the staged F2 over
        // sorted sub-partitions
        Case few = subs_case("subs-five-id-sub-partition", 1ull << 26, 2, 1u << 18, 8, 256, pf, 1.25, 0);
        few.n[1] = (1ull << 25) - 5;
        few.n[3] = 5;
        uniform_spans(few.n[1], 1.25, few.spans.data() + 32);
        for (uint32_t j = 0; j < 32; ++j) few.spans[3 * 32 + j] = j < 3 ? 150000u * j : 350000u;
        run(few, true);
    }
    printf("F2 forms: direct %u narrow %u segmented %u sparse %u dense %u\n", g_forms[0], g_forms[1], g_forms[2], g_forms[3],
           g_forms[4]);
    if (g_bad) {
        fprintf(stderr, "plan_check: %d invariant(s) broken\n", g_bad);
        return 1;
    }
    return 0;
}
