// api_rtable.hip -- the C ABI's resident routing table: K1w (dhtgpu_rt_*: upload, the good
// setters, the stream-ordered lookups and replies) and K1g (dhtgpu_rtg_*: growing it on the
// device).  The one unit that touches the context's rt state.
#include "api_ctx.h"

// A grown table's result rows name handles: K1w's positions go through the handle plane on the
// call's stream.  A table that never grew takes no launch.
static int rt_idx_to_handles(dhtgpu_ctx* c, uint32_t* idx, uint64_t m, hipStream_t s) {
    if (!c->rt.grown || !idx) return DHTGPU_OK;
    DHT_TRY(launch_rtg_handles(c->rt.gb[c->rt.gcur].handle, c->rt.v.nn, idx, m, s));
    return DHTGPU_OK;
}

// Argument checks shared by the rt query entry points (tp: the targets, device planes or host bytes).
static int check_rt(const dhtgpu_ctx* c, const void* tp, uint32_t q, uint32_t count, bool outs) {
    if (!c || count == 0 || count > DHTGPU_MAX_K || (q && (!tp || !outs))) return DHTGPU_EINVAL;
    if (!c->rt.valid) return DHTGPU_ENOIDS;
    return DHTGPU_OK;
}

// Blob `which` of the pair, carved (its geometry is fixed, so this allocates once).
static int rtg_carve(dhtgpu_ctx::RTable& t, int which) {
    const size_t sz[] = {(size_t)5 * kRtgBuckets * 4, (size_t)(kRtgBuckets + 1) * 4, (size_t)(kRtgBuckets + 1) * 4, 5 * 4,
                         (size_t)5 * kRtgNodes * 4, kRtgNodes, kRtgNodes, (size_t)kRtgNodes * 4, (size_t)kRtgNodes * 18};
    uint8_t* p[9];
    DHT_TRY(carve(t.g[which], sz, p));
    t.gb[which] = RtgBlob{reinterpret_cast<uint32_t*>(p[0]), reinterpret_cast<uint32_t*>(p[1]), reinterpret_cast<uint32_t*>(p[2]),
                          reinterpret_cast<uint32_t*>(p[3]), reinterpret_cast<uint32_t*>(p[4]), p[5], p[6],
                          reinterpret_cast<uint32_t*>(p[7]), p[8]};
    return DHTGPU_OK;
}

// One mutation: the launch that reads the current table and writes the other blob of the pair.
// `a` null: expireBuckets (d_handles: the removed handles).  The caller reads d_stat[4] and its
// results back, synchronises and calls rtg_adopt.
static int rtg_launch(dhtgpu_ctx* c, const RtgBatch* a, uint32_t* d_handles, uint32_t* d_stat, int* dst) {
    dhtgpu_ctx::RTable& t = c->rt;
    *dst = t.grown ? t.gcur ^ 1 : 0;
    if (int r = rtg_carve(t, *dst)) return r;
    DHT_TRY(t.hmap.ensure((size_t)kRtgMaxHandle * 4));
    if (!t.grown) DHT_TRY(hipMemsetAsync(t.hmap.p, 0xFF, (size_t)kRtgMaxHandle * 4, c->stream));
    const uint32_t* hsrc = t.grown ? t.gb[t.gcur].handle : nullptr;
    const uint8_t* ssrc = t.grown ? t.gb[t.gcur].state : nullptr;
    if (a) DHT_TRY(launch_rtg_insert(t.v, hsrc, ssrc, t.gb[*dst], t.hmap.as<uint32_t>(), *a, d_stat, c->stream));
    else DHT_TRY(launch_rtg_expire(t.v, hsrc, ssrc, t.gb[*dst], t.hmap.as<uint32_t>(), d_handles, d_stat, c->stream));
    return DHTGPU_OK;
}

// The one read-back of a mutation, then the table is what blob dst holds: the view rebuilt from
// {nb, nn} (the kernel wrote the good prefix sums with the planes), the grown flag.
static int rtg_adopt(dhtgpu_ctx* c, int dst, const uint32_t* stat) {
    dhtgpu_ctx::RTable& t = c->rt;
    const RtgBlob& b = t.gb[dst];
    t.gpre = b.gpre;
    t.good = b.good;
    t.v = RtView{stat[0], stat[1], b.fp, b.off, b.gpre, b.np, kRtgNodes, b.good, t.v.alen ? b.tail : nullptr, t.v.alen, b.myid};
    t.gcur = dst;
    t.grown = true;
    t.version = 0;   // no uploaded version names this table any more
    return DHTGPU_OK;
}

// A table that never grew takes its grown form (handle = upload position, state = good) by an empty batch.
static int rtg_ensure_grown(dhtgpu_ctx* c) {
    dhtgpu_ctx::RTable& t = c->rt;
    if (t.grown) return DHTGPU_OK;
    if (!t.rows_ok) return DHTGPU_EINVAL;
    DHT_TRY(t.io.ensure(16));
    uint32_t stat[4] = {};
    int dst = 0;
    const RtgBatch none = {};
    if (int r = rtg_launch(c, &none, nullptr, t.io.as<uint32_t>(), &dst)) return r;
    DHT_TRY(hipMemcpyAsync(stat, t.io.p, 16, hipMemcpyDeviceToHost, c->stream));
    DHT_TRY(hipStreamSynchronize(c->stream));
    return rtg_adopt(c, dst, stat);
}

extern "C" {

// ---- K1w: the resident routing table ---------------------------------------------------------
int dhtgpu_rt_set(dhtgpu_ctx* c, const uint8_t* myid20, uint32_t nb, const uint8_t* firsts20, const uint32_t* off,
                  const uint8_t* node_ids20, const uint8_t* node_tail, uint32_t af, uint64_t version) {
    if (!c || !myid20 || nb > 256 || (nb && (!firsts20 || !off))) return DHTGPU_EINVAL;
    if (node_tail ? (af != 4 && af != 6) : af != 0) return DHTGPU_EINVAL;
    for (uint32_t b = 0; b < nb; ++b)
        if (off[b] > off[b + 1]) return DHTGPU_EINVAL;
    const uint32_t nn = nb ? off[nb] : 0;
    if (nn && !node_ids20) return DHTGPU_EINVAL;
    dhtgpu_ctx::RTable& t = c->rt;
    if (version && t.valid && version == t.version && nb == t.v.nb && nn == t.v.nn) return DHTGPU_OK;
    DHT_TRY(c->bind());
    t.valid = false;
    t.version = 0;
    t.grown = false;   // the grown form goes with the table it grew from
    t.splits = 0;
    t.rows_ok = true;
    for (uint32_t b = 0; b < nb; ++b) t.rows_ok = t.rows_ok && off[b + 1] - off[b] <= 8;
    const uint64_t ns = pad_q(nn ? nn : 1);
    const uint32_t alen = af == 4 ? 4u : af == 6 ? 16u : 0u;
    const std::vector<uint32_t> fp = firsts_planes(firsts20, nb);
    uint32_t my[5];
    for (int w = 0; w < 5; ++w) my[w] = be32(myid20 + 4 * w);
    const uint32_t zero = 0;
    const size_t sz[] = {fp.size() * 4, (size_t)(nb + 1) * 4, (size_t)(nb + 1) * 4, sizeof my,
                         (size_t)ns * 5 * 4, (size_t)ns, (size_t)nn * (alen + 2)};
    uint8_t* p[7];
    DHT_TRY(carve(t.buf, sz, p));
    if (nb) DHT_TRY(hipMemcpyAsync(p[0], fp.data(), sz[0], hipMemcpyHostToDevice, c->stream));
    DHT_TRY(hipMemcpyAsync(p[1], nb ? off : &zero, sz[1], hipMemcpyHostToDevice, c->stream));
    DHT_TRY(hipMemcpyAsync(p[3], my, sizeof my, hipMemcpyHostToDevice, c->stream));
    DHT_TRY(hipMemsetAsync(p[5], 0, (size_t)ns, c->stream));
    if (nn) DHT_TRY(hipMemsetAsync(p[5], 1, nn, c->stream));   // every node starts good
    if (alen && nn) DHT_TRY(hipMemcpyAsync(p[6], node_tail, sz[6], hipMemcpyHostToDevice, c->stream));
    if (int r = upload_ids(c, node_ids20, nn, reinterpret_cast<uint32_t*>(p[4]), ns)) return r;
    t.gpre = reinterpret_cast<uint32_t*>(p[2]);
    t.good = p[5];
    t.v = RtView{nb, nn, reinterpret_cast<const uint32_t*>(p[0]), reinterpret_cast<const uint32_t*>(p[1]), t.gpre,
                 reinterpret_cast<const uint32_t*>(p[4]), ns, t.good, alen ? p[6] : nullptr, alen,
                 reinterpret_cast<const uint32_t*>(p[3])};
    DHT_TRY(launch_rt_gpre(t.v, t.gpre, c->stream));
    DHT_TRY(hipStreamSynchronize(c->stream));
    t.version = version;
    t.valid = true;
    return DHTGPU_OK;
}

int dhtgpu_rt_set_good(dhtgpu_ctx* c, const uint8_t* good) {
    if (!c) return DHTGPU_EINVAL;
    if (!c->rt.valid) return DHTGPU_ENOIDS;
    if (c->rt.grown) return DHTGPU_EINVAL;   // positions mean nothing there: dhtgpu_rtg_set_state
    if (!c->rt.v.nn) return DHTGPU_OK;
    if (!good) return DHTGPU_EINVAL;
    DHT_TRY(c->bind());
    DHT_TRY(hipMemcpyAsync(c->rt.good, good, c->rt.v.nn, hipMemcpyHostToDevice, c->stream));
    DHT_TRY(launch_rt_gpre(c->rt.v, c->rt.gpre, c->stream));
    return DHTGPU_OK;
}

int dhtgpu_rt_update_good(dhtgpu_ctx* c, const uint32_t* idx, const uint8_t* val, uint32_t m) {
    if (!c || (m && (!idx || !val))) return DHTGPU_EINVAL;
    if (!c->rt.valid) return DHTGPU_ENOIDS;
    const uint32_t bound = c->rt.grown ? kRtgMaxHandle : c->rt.v.nn;   // a grown table's idx are handles
    for (uint32_t j = 0; j < m; ++j)
        if (idx[j] >= bound) return DHTGPU_EINVAL;   // nothing applied
    if (!m) return DHTGPU_OK;
    DHT_TRY(c->bind());
    const uint32_t* d_idx;
    const uint8_t* d_val;
    if (int r = stage_idx_val(c, c->staging, idx, val, m, &d_idx, &d_val)) return r;
    if (c->rt.grown)
        DHT_TRY(launch_rtg_update(c->rt.gb[c->rt.gcur], c->rt.hmap.as<uint32_t>(), d_idx, d_val, m, false, c->stream));
    else
        DHT_TRY(launch_bytes_update(c->rt.good, d_idx, d_val, m, true, c->stream));
    DHT_TRY(launch_rt_gpre(c->rt.v, c->rt.gpre, c->stream));
    return DHTGPU_OK;
}

int dhtgpu_rt_find_closest_dev(dhtgpu_ctx* c, const uint32_t* tp, uint64_t ts, uint32_t q, uint32_t count,
                               uint32_t* out_idx, uint32_t* out_cnt, void* stream) {
    if (int r = check_rt(c, tp, q, count, out_idx && out_cnt)) return r;
    if (!q) return DHTGPU_OK;
    DHT_TRY(c->bind());
    DHT_TRY(launch_rt_find(c->rt.v, tp, ts, q, count, out_idx, out_cnt, c->stream_or(stream)));
    return rt_idx_to_handles(c, out_idx, (uint64_t)q * count, c->stream_or(stream));
}

int dhtgpu_rt_reply_dev(dhtgpu_ctx* c, const uint32_t* tp, uint64_t ts, uint32_t q, uint8_t* out, uint32_t* out_len,
                        uint32_t* out_idx, void* stream) {
    if (int r = check_rt(c, tp, q, 8, out && out_len)) return r;
    if (!c->rt.v.tail) return DHTGPU_EINVAL;   // set without tails
    if (!q) return DHTGPU_OK;
    DHT_TRY(c->bind());
    DHT_TRY(launch_rt_reply(c->rt.v, tp, ts, q, out, out_len, out_idx, c->stream_or(stream)));
    return rt_idx_to_handles(c, out_idx, (uint64_t)q * 8, c->stream_or(stream));
}

int dhtgpu_rt_closer_dev(dhtgpu_ctx* c, const uint32_t* tp, uint64_t ts, uint32_t q, uint32_t count, uint32_t min_nodes,
                         uint8_t* out_flag, uint32_t* out_cnt, void* stream) {
    if (int r = check_rt(c, tp, q, count, out_flag != nullptr)) return r;
    if (!q) return DHTGPU_OK;
    DHT_TRY(c->bind());
    DHT_TRY(launch_rt_closer(c->rt.v, tp, ts, q, count, min_nodes, out_flag, out_cnt, c->stream_or(stream)));
    return DHTGPU_OK;
}

int dhtgpu_rt_find_closest(dhtgpu_ctx* c, const uint8_t* t20, uint32_t q, uint32_t count, uint32_t* out_idx,
                           uint32_t* out_cnt) {
    if (int r = check_rt(c, t20, q, count, out_idx && out_cnt)) return r;
    if (!q) return DHTGPU_OK;
    DHT_TRY(c->bind());
    return host_topk(c, t20, q, count, out_idx, out_cnt,
                     [&](const uint32_t* tp, uint64_t ts, uint32_t* d_idx, uint32_t* d_cnt) {
        return dhtgpu_rt_find_closest_dev(c, tp, ts, q, count, d_idx, d_cnt, c->stream);
    });
}

int dhtgpu_rt_reply(dhtgpu_ctx* c, const uint8_t* t20, uint32_t q, uint8_t* out, uint32_t* out_len, uint32_t* out_idx) {
    if (int r = check_rt(c, t20, q, 8, out && out_len)) return r;
    if (!c->rt.v.tail) return DHTGPU_EINVAL;
    if (!q) return DHTGPU_OK;
    DHT_TRY(c->bind());
    const HostOut o[] = {{out, (size_t)q * 8 * (20 + c->rt.v.alen + 2)}, {out_len, (size_t)q * 4},
                         {out_idx, (size_t)q * 8 * 4}};
    return host_rows(c, t20, q, o, [&](const uint32_t* tp, uint64_t ts, uint8_t* const* p) {
        return dhtgpu_rt_reply_dev(c, tp, ts, q, p[0], reinterpret_cast<uint32_t*>(p[1]),
                                   out_idx ? reinterpret_cast<uint32_t*>(p[2]) : nullptr, c->stream);
    });
}

int dhtgpu_rt_closer(dhtgpu_ctx* c, const uint8_t* t20, uint32_t q, uint32_t count, uint32_t min_nodes,
                     uint8_t* out_flag, uint32_t* out_cnt) {
    if (int r = check_rt(c, t20, q, count, out_flag != nullptr)) return r;
    if (!q) return DHTGPU_OK;
    DHT_TRY(c->bind());
    const HostOut o[] = {{out_flag, (size_t)q}, {out_cnt, (size_t)q * 4}};
    return host_rows(c, t20, q, o, [&](const uint32_t* tp, uint64_t ts, uint8_t* const* p) {
        return dhtgpu_rt_closer_dev(c, tp, ts, q, count, min_nodes, p[0],
                                    out_cnt ? reinterpret_cast<uint32_t*>(p[1]) : nullptr, c->stream);
    });
}

// ---- K1g: growing the resident table ------------------------------------------------------------
int dhtgpu_rtg_on_new_node(dhtgpu_ctx* c, const uint8_t* ids20, const uint32_t* handles, const uint8_t* state,
                           const uint8_t* node_tail, uint32_t m, uint32_t flags, uint8_t* out_res, uint32_t* out_aux,
                           uint32_t* out_stat) {
    if (!c || (m && (!ids20 || !handles || !out_res))) return DHTGPU_EINVAL;
    dhtgpu_ctx::RTable& t = c->rt;
    if (!t.valid) return DHTGPU_ENOIDS;
    if (!t.rows_ok || (m && t.v.alen && !node_tail)) return DHTGPU_EINVAL;
    for (uint32_t j = 0; j < m; ++j)
        if (handles[j] >= DHTGPU_RTG_MAX_HANDLE) return DHTGPU_EINVAL;   // nothing applied
    if (!m) {
        if (out_stat) out_stat[0] = t.v.nb, out_stat[1] = t.v.nn, out_stat[2] = t.splits;
        return DHTGPU_OK;
    }
    DHT_TRY(c->bind());
    // One block up -- handles | ids | tails | state -- and one down -- status | aux | results --
    // through one host buffer each way: a flush is a few hundred bytes, and every copy is a round trip.
    const uint32_t rec = t.v.alen ? t.v.alen + 2 : 0;
    const size_t in_off[] = {0, (size_t)m * 4, (size_t)m * 24, (size_t)m * (24 + rec)};
    const size_t in_bytes = (size_t)m * (25 + rec), out_bytes = 16 + (size_t)m * 5;
    const size_t sz[] = {in_bytes, out_bytes};
    uint8_t* p[2];
    DHT_TRY(carve(t.io, sz, p));
    t.hin.resize(in_bytes);
    t.hout.resize(out_bytes);
    uint8_t* h = t.hin.data();
    memcpy(h + in_off[0], handles, (size_t)m * 4);
    memcpy(h + in_off[1], ids20, (size_t)m * 20);
    if (rec) memcpy(h + in_off[2], node_tail, (size_t)m * rec);
    if (state) memcpy(h + in_off[3], state, m);
    DHT_TRY(hipMemcpyAsync(p[0], h, in_bytes, hipMemcpyHostToDevice, c->stream));
    uint32_t* d_stat = reinterpret_cast<uint32_t*>(p[1]);
    const RtgBatch a = {p[0] + in_off[1], reinterpret_cast<const uint32_t*>(p[0]), state ? p[0] + in_off[3] : nullptr,
                        rec ? p[0] + in_off[2] : nullptr, m, flags, t.v.alen, p[1] + 16 + (size_t)m * 4, d_stat + 4};
    int dst = 0;
    if (int r = rtg_launch(c, &a, nullptr, d_stat, &dst)) return r;
    h = t.hout.data();
    DHT_TRY(hipMemcpyAsync(h, p[1], out_bytes, hipMemcpyDeviceToHost, c->stream));
    DHT_TRY(hipStreamSynchronize(c->stream));
    uint32_t stat[4];
    memcpy(stat, h, 16);
    memcpy(out_res, h + 16 + (size_t)m * 4, m);
    if (out_aux) memcpy(out_aux, h + 16, (size_t)m * 4);
    if (int r = rtg_adopt(c, dst, stat)) return r;
    t.splits += stat[2];
    if (out_stat) out_stat[0] = stat[0], out_stat[1] = stat[1], out_stat[2] = t.splits;
    return stat[3] ? DHTGPU_ERANGE : DHTGPU_OK;
}

int dhtgpu_rtg_expire(dhtgpu_ctx* c, uint32_t* out_handles, uint32_t* out_removed) {
    if (!c) return DHTGPU_EINVAL;
    dhtgpu_ctx::RTable& t = c->rt;
    if (!t.valid) return DHTGPU_ENOIDS;
    if (!t.rows_ok) return DHTGPU_EINVAL;
    DHT_TRY(c->bind());
    const uint32_t before = t.v.nn;
    const size_t sz[] = {(size_t)before * 4, 16};
    uint8_t* p[2];
    DHT_TRY(carve(t.io, sz, p));
    uint32_t stat[4] = {};
    int dst = 0;
    if (int r = rtg_launch(c, nullptr, reinterpret_cast<uint32_t*>(p[0]), reinterpret_cast<uint32_t*>(p[1]), &dst)) return r;
    DHT_TRY(hipMemcpyAsync(stat, p[1], 16, hipMemcpyDeviceToHost, c->stream));
    if (out_handles && before) DHT_TRY(hipMemcpyAsync(out_handles, p[0], sz[0], hipMemcpyDeviceToHost, c->stream));
    DHT_TRY(hipStreamSynchronize(c->stream));
    if (int r = rtg_adopt(c, dst, stat)) return r;
    if (out_removed) *out_removed = stat[3];
    return DHTGPU_OK;
}

int dhtgpu_rtg_set_state(dhtgpu_ctx* c, const uint8_t* state_by_handle, uint32_t nh) {
    if (!c || (nh && !state_by_handle) || nh > DHTGPU_RTG_MAX_HANDLE) return DHTGPU_EINVAL;
    dhtgpu_ctx::RTable& t = c->rt;
    if (!t.valid) return DHTGPU_ENOIDS;
    DHT_TRY(c->bind());
    if (int r = rtg_ensure_grown(c)) return r;
    if (!nh || !t.v.nn) return DHTGPU_OK;
    DHT_TRY(t.io.ensure(nh));
    DHT_TRY(hipMemcpyAsync(t.io.p, state_by_handle, nh, hipMemcpyHostToDevice, c->stream));
    DHT_TRY(launch_rtg_set_state(t.gb[t.gcur], t.v.nn, t.io.as<uint8_t>(), nh, c->stream));
    DHT_TRY(launch_rt_gpre(t.v, t.gpre, c->stream));
    return DHTGPU_OK;
}

int dhtgpu_rtg_update_state(dhtgpu_ctx* c, const uint32_t* handles, const uint8_t* val, uint32_t m) {
    if (!c || (m && (!handles || !val))) return DHTGPU_EINVAL;
    dhtgpu_ctx::RTable& t = c->rt;
    if (!t.valid) return DHTGPU_ENOIDS;
    for (uint32_t j = 0; j < m; ++j)
        if (handles[j] >= DHTGPU_RTG_MAX_HANDLE) return DHTGPU_EINVAL;   // nothing applied
    DHT_TRY(c->bind());
    if (int r = rtg_ensure_grown(c)) return r;
    if (!m) return DHTGPU_OK;
    const uint32_t* d_idx;
    const uint8_t* d_val;
    if (int r = stage_idx_val(c, t.io, handles, val, m, &d_idx, &d_val)) return r;
    DHT_TRY(launch_rtg_update(t.gb[t.gcur], t.hmap.as<uint32_t>(), d_idx, d_val, m, true, c->stream));
    DHT_TRY(launch_rt_gpre(t.v, t.gpre, c->stream));
    return DHTGPU_OK;
}

int dhtgpu_rtg_size(dhtgpu_ctx* c, uint32_t* out_nb, uint32_t* out_nn) {
    if (!c) return DHTGPU_EINVAL;
    if (!c->rt.valid) return DHTGPU_ENOIDS;
    if (out_nb) *out_nb = c->rt.v.nb;
    if (out_nn) *out_nn = c->rt.v.nn;
    return DHTGPU_OK;
}

int dhtgpu_rtg_export(dhtgpu_ctx* c, uint8_t* firsts20, uint32_t* bucket_off, uint8_t* ids20, uint32_t* handles,
                      uint8_t* state) {
    if (!c) return DHTGPU_EINVAL;
    dhtgpu_ctx::RTable& t = c->rt;
    if (!t.valid) return DHTGPU_ENOIDS;
    DHT_TRY(c->bind());
    const RtView& v = t.v;
    if (firsts20 && v.nb) {   // the firsts planes (stride nb) back as 20-byte ids
        std::vector<uint32_t> fp((size_t)5 * v.nb);
        DHT_TRY(hipMemcpyAsync(fp.data(), v.fp, fp.size() * 4, hipMemcpyDeviceToHost, c->stream));
        DHT_TRY(hipStreamSynchronize(c->stream));
        for (uint32_t b = 0; b < v.nb; ++b)
            for (int w = 0; w < 5; ++w) {
                const uint32_t x = fp[(size_t)w * v.nb + b];
                uint8_t* o = firsts20 + 20 * (size_t)b + 4 * w;
                o[0] = (uint8_t)(x >> 24), o[1] = (uint8_t)(x >> 16), o[2] = (uint8_t)(x >> 8), o[3] = (uint8_t)x;
            }
    }
    if (bucket_off) DHT_TRY(hipMemcpyAsync(bucket_off, v.off, (size_t)(v.nb + 1) * 4, hipMemcpyDeviceToHost, c->stream));
    if (ids20 && v.nn) {
        DHT_TRY(c->staging.ensure((size_t)v.nn * 20));
        DHT_TRY(launch_unpack(v.np, v.ns, 0, v.nn, c->staging.as<uint8_t>(), c->stream));
        DHT_TRY(hipMemcpyAsync(ids20, c->staging.p, (size_t)v.nn * 20, hipMemcpyDeviceToHost, c->stream));
    }
    if (handles && v.nn) {
        if (t.grown) DHT_TRY(hipMemcpyAsync(handles, t.gb[t.gcur].handle, (size_t)v.nn * 4, hipMemcpyDeviceToHost, c->stream));
        else for (uint32_t i = 0; i < v.nn; ++i) handles[i] = i;
    }
    if (state && v.nn)   // a table that never grew: bit 0 alone
        DHT_TRY(hipMemcpyAsync(state, t.grown ? t.gb[t.gcur].state : v.good, v.nn, hipMemcpyDeviceToHost, c->stream));
    DHT_TRY(hipStreamSynchronize(c->stream));
    if (state && !t.grown)
        for (uint32_t i = 0; i < v.nn; ++i) state[i] = state[i] != 0;
    return DHTGPU_OK;
}

}  // extern "C"
