// api_batch.hip -- the C ABI's K6 and KS entry points (dhtgpu_batch_*, the sub-partition handle
// calls): workspace slots, the prefix sub-partitions of a large set, the route of a call
// (batch_plan.h decides; this unit follows).
#include "api_ctx.h"

// The workspace slot for a call on stream s: the next slot (round-robin) whose last user was s
// (stream order suffices, no wait), else the next unused one, else the next in turn (which
// then waits for its last stream).  Stream-affine, so that up to kBatchDepth streams in flight
// never wait on each other (plain round-robin over 3 streams made every call wait).
static int pick_slot(dhtgpu_ctx* c, hipStream_t s) {
    constexpr int D = dhtgpu_ctx::kBatchDepth;
    int si = -1;
    for (int i = 0; i < D && si < 0; ++i)
        if (c->bslot[(c->bnext + i) % D].last == s) si = (c->bnext + i) % D;
    for (int i = 0; i < D && si < 0; ++i)
        if (!c->bslot[(c->bnext + i) % D].last) si = (c->bnext + i) % D;
    if (si < 0) si = c->bnext;
    c->bnext = (si + 1) % D;
    return si;
}

// A slot last used on another stream: s waits for that stream's work so far (it includes the
// slot's previous call); same stream: stream order suffices.
static int slot_wait(dhtgpu_ctx::BatchSlot& b, hipStream_t s) {
    if (b.last && b.last != s) {
        if (!b.done) DHT_TRY(hipEventCreateWithFlags(&b.done, hipEventDisableTiming));
        DHT_TRY(hipEventRecord(b.done, b.last));
        DHT_TRY(hipStreamWaitEvent(s, b.done, 0));
    }
    return DHTGPU_OK;
}

// The K6 / KS call over one active set: q targets at k, index rows li / lc, the result forms of
// the public call (index form: A's map and idx_base; record form: K6 stores the records itself).
// KS reads the set, target, row and event fields only.
static BatchCall set_call(const dhtgpu_ctx* c, const dhtgpu_ctx::ActiveSet& A, const uint32_t* tp, uint64_t ts, uint32_t q,
                          uint32_t k, uint32_t* li, uint32_t* lc, uint32_t* out_rec, uint32_t idx_base, hipEvent_t* ev) {
    BatchCall bc{};
    bc.planes = A.planes;
    bc.stride = A.stride;
    bc.n = A.n;
    bc.tp = tp;
    bc.ts = ts;
    bc.q = q;
    bc.q_plan = q;
    bc.k = k;
    bc.skip = A.pbits;
    bc.pval = A.pval;
    bc.w0s = A.w0s;
    bc.gidx = out_rec ? nullptr : A.map;
    bc.base = out_rec ? 0u : idx_base;
    bc.out_idx = li;
    bc.out_cnt = lc;
    bc.num_cus = c->num_cus;
    bc.dbg = c->dbg;
    bc.ev = ev;
    bc.out_rec = out_rec;   // every K6 writer of a row stores its records
    bc.rec_gidx = A.map;
    bc.rec_base = idx_base;
    return bc;
}

// One K6 launch sequence on workspace slot `si` (stream s): waits for the slot's previous user
// when that was another stream, cleans the workspace head when needed.
static int batch_slot_run(dhtgpu_ctx* c, int si, BatchCall bc, hipStream_t s, hipEvent_t* ev) {
    dhtgpu_ctx::BatchSlot& b = c->bslot[si];
    if (int r = slot_wait(b, s)) return r;
    uint64_t n_plan = bc.nsub ? 0 : bc.n;   // the plan is the largest sub-partition's
    for (uint32_t i = 0; i < bc.nsub; ++i) n_plan = std::max<uint64_t>(n_plan, bc.subs[i].n);
    const uint32_t nsub = bc.nsub ? bc.nsub : 1u;
    const uint32_t pf = (bc.cells ? kPlanCells : 0u) | (bc.sorted ? kPlanSorted : 0u);
    const size_t need = batch_bytes(n_plan, bc.q, bc.q_plan, bc.k, c->num_cus, nsub, pf);
    const size_t head = batch_clean_bytes(n_plan, bc.q_plan, bc.k, c->num_cus, nsub, pf);
    const size_t ctr_off = batch_ctr_offset(n_plan, bc.q_plan, bc.k, c->num_cus, nsub, pf);
    if (need > b.ws.cap) {   // reallocated: nothing of it is known
        b.zeroed = 0;
        b.desc_sig = 0;
    }
    DHT_TRY(b.ws.ensure(need));
    bc.fb_hint = c->fb_hint.host;
    bc.fb_hint_dev = c->fb_hint.dev;
    // the head is zero after a call but for the statistics words ctr[0..3] (F1 resets them at the
    // start of the next call): a head laid out with its counters elsewhere (another bitmap size --
    // a sub-partitioned call, then a one-set call) would meet them inside another array (a partition
    // count: stale survivors gathered by F3), so it is zeroed again
    if (b.zeroed < head || (b.zeroed && b.ctr_off != ctr_off)) DHT_TRY(hipMemsetAsync(b.ws.p, 0, head, s));
    b.zeroed = 0;   // re-established below once every launch went through
    if (bc.dbg & 256u) {   // phase stamps (zeroed when allocated)
        const bool fresh = !c->stamps.p;
        DHT_TRY(c->stamps.ensure((size_t)3 * 8192 * 16 * 8));
        if (fresh) DHT_TRY(hipMemsetAsync(c->stamps.p, 0, (size_t)3 * 8192 * 16 * 8, s));
        bc.stamps = c->stamps.as<unsigned long long>();
    }
    bc.ws = b.ws.p;
    bc.desc_sig = &b.desc_sig;
    DHT_TRY(launch_batch_topk(bc, s));
    b.last = s;
    b.zeroed = head;   // the call leaves its clean head zero (but for ctr[0..3])
    b.ctr_off = ctr_off;
    c->blast = si;
    c->last_n = n_plan;
    c->last_qp = bc.q_plan;
    c->last_nsub = nsub;
    c->last_pf = pf;
    return DHTGPU_OK;
}

// Build the prefix sub-partitions: the smallest split into 2^s parts of <= 2^24 expected ids
// (s <= 8), each compacted from the context's planes and then sorted by its ids (stable: equal
// ids keep their index order, so index ties break the same way), with its shifted word-0 plane,
// its index maps, its level-19 cell counts and the context's inverse handle map.  Prefix order
// is the layout K6 wants: an F2 workgroup's contiguous range of a sub-partition covers a narrow
// prefix range, so its survivors fall into a few partitions (long, coalesced bucket runs instead
// of a few entries in every partition) and a partition's survivors, results and result-map
// entries sit in a narrow index window (F3's gathers and record words hit lines they share).
static int build_subs(dhtgpu_ctx* c, const dhtgpu_ctx::ActiveSet& A, bool sort) {
    if (c->subs_valid) return DHTGPU_OK;
    c->invalidate_subs();
    const uint32_t sb = split_bits(A.n);
    const uint32_t P = A.pbits + sb;   // prefix bits every id of a sub-partition shares
    if (P > 24) return DHTGPU_ERANGE;
    hipStream_t s = c->stream;
    c->subs.resize((size_t)1 << sb);
    for (uint32_t i = 0; i < (1u << sb); ++i) {
        // (a view: "context-local" below is the view's index)
        PrefixSelect sel{A.planes, A.stride, A.n, P, (A.pval << sb) | i, s};
        unsigned long long m = 0;
        if (int r = sel.count(c, &m)) return r;
        dhtgpu_ctx::SubPart& sp = c->subs[i];
        sp.n = m;
        sp.stride = pad_ids(m ? m : 1);
        DHT_TRY(sp.planes.ensure((size_t)sp.stride * 5 * 4));
        DHT_TRY(sp.map.ensure((size_t)sp.stride * 4));
        DHT_TRY(sp.w0s.ensure((size_t)sp.stride * 4));
        for (int w = 0; w < 5; ++w)   // deterministic padding words (F2 may read them, masked)
            DHT_TRY(launch_fill(sp.planes.as<uint32_t>() + (uint64_t)w * sp.stride + m, sp.stride - m, 0u, s));
        DHT_TRY(sel.compact(sp.planes.as<uint32_t>(), sp.stride, sp.map.as<uint32_t>(), 0));
        if (sort && m > 1) {   // prefix order (stable sort of the compacted ids; perm -> context-local map)
            DevBuf sorted, perm, sscr;
            int unique = 1;
            DHT_TRY(sorted.ensure((size_t)sp.stride * 5 * 4));
            DHT_TRY(perm.ensure((size_t)m * 4));
            DHT_TRY(sscr.ensure(sort_scratch_bytes(m)));
            for (int w = 0; w < 5; ++w)
                DHT_TRY(launch_fill(sorted.as<uint32_t>() + (uint64_t)w * sp.stride + m, sp.stride - m, 0u, s));
            DHT_TRY(launch_sort_ids(sp.planes.as<uint32_t>(), sp.stride, m, sorted.as<uint32_t>(), sp.stride,
                                    perm.as<uint32_t>(), sscr.p, &unique, s));
            DHT_TRY(launch_map_idx(perm.as<uint32_t>(), m, sp.map.as<uint32_t>(), 0, s));
            DHT_TRY(hipMemcpyAsync(sp.map.p, perm.p, (size_t)m * 4, hipMemcpyDeviceToDevice, s));
            DHT_TRY(hipStreamSynchronize(s));
            std::swap(sp.planes, sorted);
        }
        DHT_TRY(launch_shift_w0(sp.planes.as<uint32_t>(), sp.stride, P, sp.w0s.as<uint32_t>(), s));
        if (c->has_gidx) {   // sub -> global stream index, composed once
            DHT_TRY(sp.gmap.ensure((size_t)sp.stride * 4));
            DHT_TRY(hipMemcpyAsync(sp.gmap.p, sp.map.p, (size_t)m * 4, hipMemcpyDeviceToDevice, s));
            DHT_TRY(launch_map_idx(sp.gmap.as<uint32_t>(), m, A.view ? c->acc.gmap.as<uint32_t>() : c->gidx.as<uint32_t>(), 0, s));
        }
    }
    // level-cell_level() id counts of every sub-partition (sibling marking, BatchCall::cells)
    const size_t ncell = (size_t)1 << cell_level();
    DHT_TRY(c->cells.ensure(c->subs.size() * ncell));
    {
        DevBuf cnt;
        DHT_TRY(cnt.ensure(ncell * 4));
        for (size_t i = 0; i < c->subs.size(); ++i)
            DHT_TRY(launch_cell_counts(c->subs[i].w0s.as<uint32_t>(), c->subs[i].n, cnt.as<uint32_t>(),
                                       c->cells.as<uint8_t>() + i * ncell, s));
        for (size_t i = 0; sort && i < c->subs.size(); ++i) {   // window bounds (sorted subs)
            DHT_TRY(launch_cell_spans(c->subs[i].w0s.as<uint32_t>(), c->subs[i].n, cnt.as<uint32_t>(), s));
            DHT_TRY(hipMemcpyAsync(c->subs[i].span, cnt.p, 32 * 4, hipMemcpyDeviceToHost, s));
            DHT_TRY(hipStreamSynchronize(s));
        }
        DHT_TRY(hipStreamSynchronize(s));
        c->spans.assign(sort ? c->subs.size() * 32 : 0, 0u);
        for (size_t i = 0; sort && i < c->subs.size(); ++i)
            std::copy(c->subs[i].span, c->subs[i].span + 32, c->spans.begin() + i * 32);
    }
    DHT_TRY(c->hinv.ensure((size_t)(c->n ? c->n : 1) * 4));
    {
        uint64_t o = 0;
        for (const auto& sp : c->subs) {
            DHT_TRY(launch_handle_inverse(sp.map.as<uint32_t>(), sp.n, (uint32_t)o, c->hinv.as<uint32_t>(), s));
            o += sp.n;
        }
    }
    std::vector<HandleSub> tab(c->subs.size());
    uint64_t off = 0;
    for (size_t i = 0; i < tab.size(); ++i) {
        const dhtgpu_ctx::SubPart& sp = c->subs[i];
        tab[i] = HandleSub{sp.n, sp.map.as<uint32_t>(), c->has_gidx ? sp.gmap.as<uint32_t>() : nullptr, (uint32_t)off, 0u};
        off += sp.n;
    }
    DHT_TRY(c->sub_tab.ensure(tab.size() * sizeof(HandleSub)));
    DHT_TRY(hipMemcpyAsync(c->sub_tab.p, tab.data(), tab.size() * sizeof(HandleSub), hipMemcpyHostToDevice, s));
    DHT_TRY(hipStreamSynchronize(s));
    c->sub_bits = sb;
    c->subs_valid = true;
    c->subs_sorted = sort;
    return DHTGPU_OK;
}

// A K6 call over prefix sub-partitions, all of them in ONE launch sequence.  A target is
// answered from its own sub-partition (F1 routes it by the sub_bits bits after the shard
// prefix): when that holds >= k ids, every id of it is XOR-closer to the target than every id
// outside it, so its top-k is the set's.  Targets whose sub-partition is short of k ids (or
// whose partition overflowed) take F4's scan over the whole set.  A split K6 cannot plan
// (strongly clustered ids: one sub-partition far above 2^24) takes the K1 scan.
static int batch_run_subs(dhtgpu_ctx* c, const dhtgpu_ctx::ActiveSet& A, const uint32_t* tp, uint64_t ts, uint32_t q, uint32_t k, uint32_t* out_idx,
                          uint32_t* out_cnt, uint32_t* out_rec, uint32_t idx_base, hipStream_t s, hipEvent_t* ev) {
    // Prefix-sorted sub-partitions: an F2 range's survivors fall into a few partitions that the
    // range owns, so F2 writes them straight to their buckets with no stage (k_f2_direct: a few KB
    // of LDS, F3 workgroups of the other call in flight beside it) and F3's reads stay inside
    // narrow index windows.  The cfg-3 broadcast rank (2^20 targets on 1.25e8 ids, ~22 % of the
    // ids survive): 1.16 -> 0.43 ms per call; the prefix rank (~3 %): 0.149 -> 0.135 ms, the
    // 2^27-id shard 0.157 -> 0.148-0.152 (profiles/r06/experiments).  Below ~2 % survivors a
    // wave's runs would be one or two entries: index order.  Decided once, by the call that
    // builds them (batch_plan.cpp: subs_sort_rule).
    int r = build_subs(c, A, subs_sort_rule(A.n, q, k));
    if (r) return r;
    const uint32_t sb = c->sub_bits, S = 1u << sb;
    const uint32_t pf = kPlanCells | (c->subs_sorted ? kPlanSorted : 0u);
    const uint32_t P = A.pbits + sb;
    const uint32_t q_plan = std::max<uint32_t>(1u, (uint32_t)(((uint64_t)q + S - 1) >> sb));
    uint64_t n_max = 0;
    for (const auto& sp : c->subs) n_max = std::max<uint64_t>(n_max, sp.n);
    const bool handles = c->sub_handles && !out_rec && !c->acc.has_mask;   // (masked calls return indices)
    if (!batch_supported(n_max, q_plan, k, c->num_cus, S, pf)) {
        if (!handles) return topk_on(c, A, tp, ts, q, k, out_idx, out_cnt, out_rec, idx_base, s);
        // handles on the K1 route: context-local indices (handles go with no mask, so A is the set
        // itself; its global map and the offset are left out), then their handles
        dhtgpu_ctx::ActiveSet L = A;
        L.map = nullptr;
        if ((r = topk_on(c, L, tp, ts, q, k, out_idx, out_cnt, nullptr, 0, s))) return r;
        DHT_TRY(launch_idx_to_handles(c->hinv.as<uint32_t>(), out_idx, (uint64_t)q * k, s));
        return DHTGPU_OK;
    }
    const bool global = !handles && c->has_gidx && c->map_global && !out_rec;
    const int si = pick_slot(c, s);
    dhtgpu_ctx::BatchSlot& b = c->bslot[si];
    uint32_t *li = out_idx, *lc = out_cnt;
    if ((r = local_rows(out_rec, b.out_idx, b.out_cnt, q, k, &li, &lc))) return r;
    std::vector<SubSpec> specs(S);
    uint64_t off = 0;
    for (uint32_t i = 0; i < S; ++i) {
        const dhtgpu_ctx::SubPart& sp = c->subs[i];
        specs[i] = SubSpec{sp.planes.as<uint32_t>(), sp.w0s.as<uint32_t>(), sp.stride, sp.n,
                           handles ? nullptr : global ? sp.gmap.as<uint32_t>() : sp.map.as<uint32_t>(),
                           handles ? (uint32_t)off : 0u};
        off += sp.n;
    }
    // the whole set is F4's scan; the sub-partitions carry their own shifted planes and maps
    BatchCall bc = set_call(c, A, tp, ts, q, k, li, lc, out_rec, idx_base, ev);
    bc.q_plan = q_plan;
    bc.skip = P;
    bc.w0s = nullptr;
    bc.cells = c->cells.as<uint8_t>();
    bc.spans = c->spans.empty() ? nullptr : c->spans.data();
    bc.sorted = c->subs_sorted ? 1u : 0u;
    bc.gidx = global ? A.map : nullptr;   // (else mapped after the call, below)
    bc.base = handles ? kHandleMark : 0u;   // handles: whole-set fallback rows, marked for the pass after F4
    bc.subs = specs.data();
    bc.nsub = S;
    bc.sub_shift = A.pbits;
    bc.sub_bits = sb;
    bc.handles = handles ? 1u : 0u;
    bc.htab = c->sub_tab.as<HandleSub>();
    bc.hinv = c->hinv.as<uint32_t>();
    r = batch_slot_run(c, si, bc, s, ev);
    if (r) return r;
    if (!out_rec && !handles && !global && (idx_base || A.view)) {   // (record form: K6 wrote the records)
        // (a view's sub-partition maps give view indices: through its map to the set's)
        DHT_TRY(launch_map_idx(out_idx, (uint64_t)q * k, A.view ? A.map : nullptr, idx_base, s));
    }
    return DHTGPU_OK;
}

// Batches of at most 64 targets: one pass over word 0 + one workgroup per target prefix (KS).
static int small_run(dhtgpu_ctx* c, const dhtgpu_ctx::ActiveSet& A, const uint32_t* tp, uint64_t ts, uint32_t q, uint32_t k, uint32_t* out_idx,
                     uint32_t* out_cnt, uint32_t* out_rec, uint32_t idx_base, hipStream_t s, hipEvent_t* ev) {
    const int si = pick_slot(c, s);
    dhtgpu_ctx::BatchSlot& b = c->bslot[si];
    if (int r = slot_wait(b, s)) return r;
    if (b.sws.cap < small_bytes()) b.sclean = false;
    DHT_TRY(b.sws.ensure(small_bytes()));
    if (!b.sclean) {
        DHT_TRY(hipMemsetAsync(b.sws.p, 0, small_bytes(), s));
        b.spar = 0;
    }
    b.sclean = true;   // the kernels leave it zero
    uint32_t *li = out_idx, *lc = out_cnt;
    if (int r = local_rows(out_rec, b.out_idx, b.out_cnt, q, k, &li, &lc)) return r;
    const BatchCall bc = set_call(c, A, tp, ts, q, k, li, lc, out_rec, idx_base, ev);
    if (hipError_t e = launch_small_topk(bc, b.sws.p, b.spar, s)) {
        b.sclean = false;   // S1 may have counted into this call's set: the next call re-zeroes it all
        return map_err(e);
    }
    b.spar ^= 1u;
    b.last = s;
    c->last_small = true;
    if (out_rec)   // (KS stores index rows only: the records are made from them)
        DHT_TRY(launch_rec3(li, (uint64_t)q * k, A.planes, A.stride, idx_base, A.map, out_rec, s));
    return DHTGPU_OK;
}

static int batch_run(dhtgpu_ctx* c, const uint32_t* tp, uint64_t ts, uint32_t q, uint32_t k, uint32_t* out_idx,
                     uint32_t* out_cnt, uint32_t* out_rec, uint32_t idx_base, hipStream_t s, hipEvent_t* ev) {
    hipEvent_t evs[8];
    if (!ev && c->has_next_ev) {   // armed by dhtgpu_batch_events: this call only
        for (int i = 0; i < 8; ++i) evs[i] = c->next_ev[i];
        c->has_next_ev = false;
        ev = evs;
    }
    // DHTGPU_DBG bit 2^23: K6 for small batches too (comparison runs; the same exact results)
    dhtgpu_ctx::ActiveSet A;
    if (int r = c->active_set(idx_base, &A)) return r;
    if (A.view && !A.n) {   // every id rejected
        c->last_small = true;   // (no statistics)
        return answer_empty(q, k, out_idx, out_cnt, out_rec, s);
    }
    if (small_supported(A.n, q, k) && !(c->dbg & (1u << 23)))
        return small_run(c, A, tp, ts, q, k, out_idx, out_cnt, out_rec, idx_base, s, ev);
    c->last_small = false;
    if (needs_subs(c->num_cus, A.n, q, k)) return batch_run_subs(c, A, tp, ts, q, k, out_idx, out_cnt, out_rec, idx_base, s, ev);
    if (!batch_supported(A.n, q, k, c->num_cus)) return DHTGPU_ERANGE;
    const int si = pick_slot(c, s);
    dhtgpu_ctx::BatchSlot& b = c->bslot[si];
    uint32_t *li = out_idx, *lc = out_cnt;
    if (int r = local_rows(out_rec, b.out_idx, b.out_cnt, q, k, &li, &lc)) return r;
    return batch_slot_run(c, si, set_call(c, A, tp, ts, q, k, li, lc, out_rec, idx_base, ev), s, ev);
}

extern "C" {

int dhtgpu_batch_topk_dev(dhtgpu_ctx* c, const uint32_t* tp, uint64_t ts, uint32_t q, uint32_t k,
                          uint32_t* out_idx, uint32_t* out_cnt, uint32_t* out_rec, uint32_t idx_base,
                          void* stream) {
    if (int r = check_topk_dev(c, tp, q, k, out_idx, out_cnt, out_rec)) return r;
    if (int r = check_idx_base(c, idx_base)) return r;
    if (!q) return DHTGPU_OK;
    DHT_TRY(c->bind());
    return batch_run(c, tp, ts, q, k, out_idx, out_cnt, out_rec, idx_base,
                     c->stream_or(stream), nullptr);
}

int dhtgpu_batch_events(dhtgpu_ctx* c, void** ev8) {
    if (!c || !ev8) return DHTGPU_EINVAL;
    for (int i = 0; i < 8; ++i) {
        if (!ev8[i]) return DHTGPU_EINVAL;
        c->next_ev[i] = (hipEvent_t)ev8[i];
    }
    c->has_next_ev = true;
    return DHTGPU_OK;
}

int dhtgpu_batch_topk_timed(dhtgpu_ctx* c, const uint32_t* tp, uint64_t ts, uint32_t q, uint32_t k,
                            uint32_t* out_idx, uint32_t* out_cnt, void* stream, float* ms4, uint32_t* stats4) {
    if (!c || !ms4 || k == 0 || k > DHTGPU_MAX_K || !q || !tp || !out_idx || !out_cnt) return DHTGPU_EINVAL;
    if (!c->has_ids) return DHTGPU_ENOIDS;
    DHT_TRY(c->bind());
    hipStream_t s = c->stream_or(stream);
    Events<8> ev;   // start/stop per kernel, recorded by the kernels' own dispatches
    DHT_TRY(ev.create());
    if (int r = batch_run(c, tp, ts, q, k, out_idx, out_cnt, nullptr, 0, s, ev.ev)) return r;
    DHT_TRY(hipStreamSynchronize(s));
    DHT_TRY(hipEventSynchronize(ev.ev[7]));
    for (int i = 0; i < 4; ++i) DHT_TRY(hipEventElapsedTime(&ms4[i], ev.ev[2 * i], ev.ev[2 * i + 1]));
    if (stats4 && c->last_small) {   // the small-batch path keeps no statistics
        for (int i = 0; i < 4; ++i) stats4[i] = 0;
    } else if (stats4) {
        DHT_TRY(batch_read_stats(c->bslot[c->blast].ws.p, c->last_n, q, c->last_qp, k, c->num_cus, stats4, s,
                                 c->last_nsub, c->last_pf));
    }
    return DHTGPU_OK;
}

int dhtgpu_batch_plan(dhtgpu_ctx* c, int num_cus, uint64_t n, uint32_t q, uint32_t k, uint32_t* out16) {
    if (!out16 || k == 0 || k > DHTGPU_MAX_K || !q || !n) return DHTGPU_EINVAL;
    const int cus = c ? c->num_cus : num_cus;
    const uint32_t dbg = c ? c->dbg : 0u;
    for (int i = 0; i < 16; ++i) out16[i] = 0;
    // batch_run's order of decisions
    if (small_supported(n, q, k) && !(dbg & (1u << 23))) {
        out16[0] = 0;
        out16[14] = small_level(n, k);
    } else if (needs_subs(cus, n, q, k)) {
        out16[0] = 2;
    } else if (!batch_supported(n, q, k, cus)) {
        out16[0] = 3;
    } else {
        out16[0] = 1;
        batch_plan_words(n, q, k, cus, out16);
    }
    return DHTGPU_OK;
}

int dhtgpu_batch_topk(dhtgpu_ctx* c, const uint8_t* t20, uint32_t q, uint32_t k, uint32_t* out_idx,
                      uint32_t* out_cnt) {
    if (int r = check_topk_host(c, t20, q, k, out_idx, out_cnt)) return r;
    if (!q) return DHTGPU_OK;
    DHT_TRY(c->bind());
    return host_topk(c, t20, q, k, out_idx, out_cnt, [&](const uint32_t* tp, uint64_t ts, uint32_t* d_idx, uint32_t* d_cnt) {
        return batch_run(c, tp, ts, q, k, d_idx, d_cnt, nullptr, 0, c->stream, nullptr);
    });
}

int dhtgpu_set_sub_handles(dhtgpu_ctx* c, int on) {
    if (!c) return DHTGPU_EINVAL;
    c->sub_handles = on != 0;
    return DHTGPU_OK;
}

int dhtgpu_sub_handles_active(dhtgpu_ctx* c, uint32_t q, uint32_t k) {
    if (!c || !c->has_ids) return 0;
    if (c->acc.has_mask) return 0;   // masked calls return indices
    return c->sub_handles && !(small_supported(c->n, q, k) && !(c->dbg & (1u << 23))) && needs_subs(c->num_cus, c->n, q, k) ? 1 : 0;
}

int dhtgpu_handles_to_indices_dev(dhtgpu_ctx* c, const uint32_t* handles, uint64_t m, uint32_t* out_idx,
                                  uint32_t idx_base, void* stream) {
    if (!c || (m && (!handles || !out_idx))) return DHTGPU_EINVAL;
    if (int r = check_idx_base(c, idx_base)) return r;
    if (!c->subs_valid) return DHTGPU_EINVAL;   // no sub-partitioned call has built the handle space
    if (!m) return DHTGPU_OK;
    DHT_TRY(c->bind());
    const bool global = c->has_gidx && c->map_global;
    DHT_TRY(launch_handles_to_idx(c->sub_tab.as<HandleSub>(), (uint32_t)c->subs.size(), handles, m, out_idx, global,
                                  global ? 0u : idx_base, c->stream_or(stream)));
    return DHTGPU_OK;
}

}  // extern "C"
