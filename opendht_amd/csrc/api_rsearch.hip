// api_rsearch.hip -- the C ABI's resident searches: K10w (dhtgpu_sr_*: the searches' node lists,
// insertNode and the fused refill), K10s (dhtgpu_srs_*: searchStep on those lists) and K10m
// (dhtgpu_srm_*: trySearchInsert over their ordered map).  The one unit that touches the context's sr state; of nc it reads valid and view() only.
#include "api_ctx.h"

// every slot names a search; `distinct`: no slot twice
static int sr_check_slots(const dhtgpu_ctx* c, const uint32_t* slots, uint32_t m, bool distinct) {
    for (uint32_t j = 0; j < m; ++j)
        if (slots[j] >= c->sr.nslots) return DHTGPU_EINVAL;
    if (distinct && m > 1) {
        std::vector<uint32_t> s(slots, slots + m);
        std::sort(s.begin(), s.end());
        if (std::adjacent_find(s.begin(), s.end()) != s.end()) return DHTGPU_EINVAL;
    }
    return DHTGPU_OK;
}

// The state array covers handles [0, nh), what it held kept and its new bytes 0: it grows
// geometrically on the context's stream, and the array it replaces is kept until the next growth.
static int sr_state_extent(dhtgpu_ctx* c, uint64_t nh) {
    dhtgpu_ctx::Searches& t = c->sr;
    if (nh <= t.nst) return DHTGPU_OK;
    if (int r = grow_kept(c, t.st, t.st_old, t.nst, (size_t)nh, 4096, DHTGPU_NC_MAX_HANDLE)) return r;
    // (an array that did not grow may hold bytes of an extent dhtgpu_sr_set_state dropped)
    DHT_TRY(hipMemsetAsync(t.st.as<uint8_t>() + t.nst, 0, (size_t)(nh - t.nst), c->stream));
    t.nst = (uint32_t)nh;
    return DHTGPU_OK;
}

// m slots (host) into the head of the staging block p
static int sr_upload_slots(dhtgpu_ctx* c, uint8_t* p, const uint32_t* slots, uint32_t m) {
    DHT_TRY(hipMemcpyAsync(p, slots, (size_t)m * 4, hipMemcpyHostToDevice, c->stream));
    return DHTGPU_OK;
}

// the argument checks every sr call on a slot list shares
static int sr_check(const dhtgpu_ctx* c, const void* slots, uint32_t m) {
    if (!c || (m && !slots)) return DHTGPU_EINVAL;
    if (!c->sr.valid) return DHTGPU_ENOIDS;
    return DHTGPU_OK;
}

// the overflow word of a host insert / refill, read back after the call's other results
static int sr_finish(dhtgpu_ctx* c, const uint32_t* d_over) {
    uint32_t over = 0;
    DHT_TRY(hipMemcpyAsync(&over, d_over, 4, hipMemcpyDeviceToHost, c->stream));
    DHT_TRY(hipStreamSynchronize(c->stream));
    return over ? DHTGPU_ERANGE : DHTGPU_OK;
}

// The offer of m nodes (device arrays) in chunks of kSrmChunk, each a filter and a walk launch on s;
// the mask and the counters are zeroed first.  Neither synchronises nor allocates.
static int srm_offer_on(dhtgpu_ctx* c, const uint32_t* handles, const uint32_t* ip, uint64_t is, uint32_t m,
                        uint32_t* out_cnt, uint32_t* out_touched, uint32_t* out_stats, hipStream_t s) {
    const dhtgpu_ctx::Searches::Map& mp = c->sr.map;
    uint32_t* stats = out_stats ? out_stats : mp.stats();
    DHT_TRY(hipMemsetAsync(stats, 0, 16, s));
    if (out_touched && c->sr.nslots) DHT_TRY(hipMemsetAsync(out_touched, 0, (size_t)((c->sr.nslots + 31) / 32) * 4, s));
    for (uint32_t i = 0; i < m; i += kSrmChunk)
        DHT_TRY(launch_srm_offer(c->sr.view(), mp.view(), mp.arrays(), handles + i, ip + i, is, std::min(kSrmChunk, m - i),
                                 out_cnt + i, out_touched, stats, s));
    return DHTGPU_OK;
}

// the argument checks of both forms of dhtgpu_srs_step
static int srs_step_check(const dhtgpu_ctx* c, const uint32_t* slots, uint32_t m, uint32_t refill_count,
                          const uint32_t* out_send, const uint32_t* out4) {
    if (int r = sr_check(c, slots, m)) return r;
    if (refill_count > DHTGPU_MAX_K || (m && (!out_send || !out4))) return DHTGPU_EINVAL;
    if (c->sr.clock == 0) return DHTGPU_EINVAL;   // no dhtgpu_srs_set_clock yet
    if (refill_count && !c->nc.valid) return DHTGPU_ENOIDS;
    return DHTGPU_OK;
}

// the NodeCache mirror a step's refill leg walks; without one (refill_count 0) it is never read
static NcView srs_nc(const dhtgpu_ctx* c, uint32_t refill_count) {
    return refill_count ? c->nc.view() : NcView{0, nullptr, 0, nullptr, nullptr};
}

extern "C" {

// ---- K10w: the resident searches ---------------------------------------------------------------
int dhtgpu_sr_reset(dhtgpu_ctx* c, uint32_t nslots) {
    if (!c) return DHTGPU_EINVAL;
    if (nslots > (1u << 20)) return DHTGPU_ERANGE;
    DHT_TRY(c->bind());
    dhtgpu_ctx::Searches& t = c->sr;
    t.valid = false;
    t.map.valid = false;
    DHT_TRY(hipStreamSynchronize(c->stream));
    t.st.release();
    t.st_old.release();
    t.nst = 0;
    t.nslots = 0;
    const size_t ns = nslots ? nslots : 1;
    DHT_TRY(t.rows.ensure(ns * DHTGPU_SR_CAP * 6 * 4));
    DHT_TRY(t.tp.ensure(ns * 5 * 4));
    DHT_TRY(t.len.ensure(ns * 4));
    DHT_TRY(t.bits.ensure(ns));
    DHT_TRY(t.tick.ensure(ns * DHTGPU_SR_CAP * 4));
    DHT_TRY(t.rtick.ensure(ns * 4));
    DHT_TRY(hipMemsetAsync(t.tick.p, 0, ns * DHTGPU_SR_CAP * 4, c->stream));
    DHT_TRY(hipMemsetAsync(t.rtick.p, 0, ns * 4, c->stream));
    DHT_TRY(hipMemsetAsync(t.tp.p, 0, ns * 5 * 4, c->stream));
    DHT_TRY(hipMemsetAsync(t.len.p, 0, ns * 4, c->stream));
    DHT_TRY(hipMemsetAsync(t.bits.p, 0, ns, c->stream));
    t.nslots = nslots;
    t.valid = true;
    return DHTGPU_OK;
}

int dhtgpu_sr_open(dhtgpu_ctx* c, const uint32_t* slots, const uint8_t* t20, uint32_t m) {
    if (int r = sr_check(c, slots, m)) return r;
    if (m && !t20) return DHTGPU_EINVAL;
    if (int r = sr_check_slots(c, slots, m, false)) return r;
    c->sr.map.valid = false;   // a slot's target may change: the ordered map is dropped
    if (!m) return DHTGPU_OK;
    DHT_TRY(c->bind());
    DHT_TRY(c->sr.io.ensure((size_t)m * 4));
    if (int r = sr_upload_slots(c, c->sr.io.as<uint8_t>(), slots, m)) return r;
    uint64_t ts = 0;
    DHT_TRY(c->upload_targets(t20, m, &ts));
    DHT_TRY(launch_sr_open(c->sr.view(), c->sr.io.as<uint32_t>(), c->targets.as<uint32_t>(), ts, m, c->stream));
    return DHTGPU_OK;
}

int dhtgpu_sr_expire(dhtgpu_ctx* c, const uint32_t* slots, uint32_t m) {
    if (int r = sr_check(c, slots, m)) return r;
    if (int r = sr_check_slots(c, slots, m, false)) return r;
    if (!m) return DHTGPU_OK;
    DHT_TRY(c->bind());
    DHT_TRY(c->sr.io.ensure((size_t)m * 4));
    if (int r = sr_upload_slots(c, c->sr.io.as<uint8_t>(), slots, m)) return r;
    DHT_TRY(launch_sr_expire(c->sr.view(), c->sr.io.as<uint32_t>(), m, c->stream));
    return DHTGPU_OK;
}

int dhtgpu_sr_set_state(dhtgpu_ctx* c, const uint8_t* state_by_handle, uint32_t nh) {
    if (!c || (nh && !state_by_handle) || nh > DHTGPU_NC_MAX_HANDLE) return DHTGPU_EINVAL;
    if (!c->sr.valid) return DHTGPU_ENOIDS;
    DHT_TRY(c->bind());
    c->sr.nst = 0;   // the array is replaced: nothing of it is kept
    if (int r = sr_state_extent(c, nh)) return r;
    if (nh) DHT_TRY(hipMemcpyAsync(c->sr.st.p, state_by_handle, nh, hipMemcpyHostToDevice, c->stream));
    return DHTGPU_OK;
}

int dhtgpu_sr_update_state(dhtgpu_ctx* c, const uint32_t* handles, const uint8_t* val, uint32_t m) {
    if (!c || (m && (!handles || !val))) return DHTGPU_EINVAL;
    if (!c->sr.valid) return DHTGPU_ENOIDS;
    const uint64_t ext = handle_extent(handles, m);
    if (!ext) return DHTGPU_EINVAL;   // nothing applied
    if (!m) return DHTGPU_OK;
    DHT_TRY(c->bind());
    if (int r = sr_state_extent(c, ext)) return r;
    const uint32_t* d_idx;
    const uint8_t* d_val;
    if (int r = stage_idx_val(c, c->sr.io, handles, val, m, &d_idx, &d_val)) return r;
    DHT_TRY(launch_bytes_update(c->sr.st.as<uint8_t>(), d_idx, d_val, m, false, c->stream));
    return DHTGPU_OK;
}

int dhtgpu_sr_set_candidate(dhtgpu_ctx* c, const uint32_t* slots, const uint32_t* handles, const uint8_t* val,
                            uint32_t m) {
    if (int r = sr_check(c, slots, m)) return r;
    if (m && (!handles || !val)) return DHTGPU_EINVAL;
    if (int r = sr_check_slots(c, slots, m, false)) return r;
    if (!handle_extent(handles, m)) return DHTGPU_EINVAL;
    if (!m) return DHTGPU_OK;
    DHT_TRY(c->bind());
    const size_t sz[] = {(size_t)m * 4, (size_t)m * 4, (size_t)m};
    uint8_t* p[3];
    DHT_TRY(carve(c->sr.io, sz, p));
    if (int r = sr_upload_slots(c, p[0], slots, m)) return r;
    DHT_TRY(hipMemcpyAsync(p[1], handles, sz[1], hipMemcpyHostToDevice, c->stream));
    DHT_TRY(hipMemcpyAsync(p[2], val, sz[2], hipMemcpyHostToDevice, c->stream));
    DHT_TRY(launch_sr_candidate(c->sr.view(), reinterpret_cast<uint32_t*>(p[0]), reinterpret_cast<uint32_t*>(p[1]), p[2],
                                m, c->stream));
    return DHTGPU_OK;
}

int dhtgpu_sr_insert_dev(dhtgpu_ctx* c, const uint32_t* slots, uint32_t m, const uint64_t* ins_off,
                         const uint32_t* ins_handle, const uint32_t* id_planes, uint64_t id_stride,
                         const uint8_t* ins_token, uint8_t* ins_added, void* stream) {
    if (int r = sr_check(c, slots, m)) return r;
    if (m && (!ins_off || !ins_handle || !id_planes)) return DHTGPU_EINVAL;
    if (!m) return DHTGPU_OK;
    DHT_TRY(c->bind());
    DHT_TRY(launch_sr_insert(c->sr.view(), slots, m, ins_off, ins_handle, id_planes, id_stride, ins_token, ins_added,
                             nullptr, c->stream_or(stream)));
    return DHTGPU_OK;
}

int dhtgpu_sr_insert(dhtgpu_ctx* c, const uint32_t* slots, uint32_t m, const uint64_t* ins_off,
                     const uint32_t* ins_handle, const uint8_t* ins_ids20, const uint8_t* ins_token,
                     uint8_t* ins_added) {
    if (int r = sr_check(c, slots, m)) return r;
    if (m && !ins_off) return DHTGPU_EINVAL;
    if (!m) return DHTGPU_OK;
    for (uint32_t j = 0; j < m; ++j)
        if (ins_off[j + 1] < ins_off[j]) return DHTGPU_EINVAL;
    const uint64_t tot = ins_off[m];
    if (tot >= 0xFFFFFFFFull) return DHTGPU_ERANGE;
    if (tot && (!ins_handle || !ins_ids20)) return DHTGPU_EINVAL;
    if (!handle_extent(ins_handle, tot)) return DHTGPU_EINVAL;
    if (int r = sr_check_slots(c, slots, m, true)) return r;
    DHT_TRY(c->bind());
    const uint64_t is = pad_q((uint32_t)(tot ? tot : 1));
    // slots | offsets | handles | id planes | tokens | added | overflow word
    const size_t sz[] = {(size_t)m * 4, ((size_t)m + 1) * 8, (size_t)tot * 4, (size_t)is * 5 * 4, (size_t)tot,
                         (size_t)tot, 4};
    uint8_t* p[7];
    DHT_TRY(carve(c->sr.io, sz, p));
    if (int r = sr_upload_slots(c, p[0], slots, m)) return r;
    DHT_TRY(hipMemcpyAsync(p[1], ins_off, sz[1], hipMemcpyHostToDevice, c->stream));
    if (tot) {
        DHT_TRY(hipMemcpyAsync(p[2], ins_handle, sz[2], hipMemcpyHostToDevice, c->stream));
        if (ins_token) DHT_TRY(hipMemcpyAsync(p[4], ins_token, sz[4], hipMemcpyHostToDevice, c->stream));
        if (int r = upload_ids(c, ins_ids20, tot, reinterpret_cast<uint32_t*>(p[3]), is)) return r;
    }
    DHT_TRY(hipMemsetAsync(p[6], 0, 4, c->stream));
    DHT_TRY(launch_sr_insert(c->sr.view(), reinterpret_cast<uint32_t*>(p[0]), m, reinterpret_cast<uint64_t*>(p[1]),
                             reinterpret_cast<uint32_t*>(p[2]), reinterpret_cast<uint32_t*>(p[3]), is,
                             ins_token ? p[4] : nullptr, p[5], reinterpret_cast<uint32_t*>(p[6]), c->stream));
    if (tot && ins_added) DHT_TRY(hipMemcpyAsync(ins_added, p[5], sz[5], hipMemcpyDeviceToHost, c->stream));
    return sr_finish(c, reinterpret_cast<uint32_t*>(p[6]));
}

int dhtgpu_sr_refill_dev(dhtgpu_ctx* c, const uint32_t* slots, uint32_t m, uint32_t count, uint32_t* out_inserted,
                         void* stream) {
    if (!c || count == 0 || count > DHTGPU_MAX_K || (m && (!slots || !out_inserted))) return DHTGPU_EINVAL;
    if (!c->sr.valid || !c->nc.valid) return DHTGPU_ENOIDS;
    if (!m) return DHTGPU_OK;
    DHT_TRY(c->bind());
    DHT_TRY(launch_sr_refill(c->sr.view(), c->nc.view(), slots, m, count, out_inserted, nullptr, c->stream_or(stream)));
    return DHTGPU_OK;
}

int dhtgpu_sr_refill(dhtgpu_ctx* c, const uint32_t* slots, uint32_t m, uint32_t count, uint32_t* out_inserted) {
    if (!c || count == 0 || count > DHTGPU_MAX_K || (m && (!slots || !out_inserted))) return DHTGPU_EINVAL;
    if (!c->sr.valid || !c->nc.valid) return DHTGPU_ENOIDS;
    if (int r = sr_check_slots(c, slots, m, true)) return r;
    if (!m) return DHTGPU_OK;
    DHT_TRY(c->bind());
    const size_t sz[] = {(size_t)m * 4, (size_t)m * 4, 4};   // slots | inserted | overflow word
    uint8_t* p[3];
    DHT_TRY(carve(c->sr.io, sz, p));
    if (int r = sr_upload_slots(c, p[0], slots, m)) return r;
    DHT_TRY(hipMemsetAsync(p[2], 0, 4, c->stream));
    DHT_TRY(launch_sr_refill(c->sr.view(), c->nc.view(), reinterpret_cast<uint32_t*>(p[0]), m, count,
                             reinterpret_cast<uint32_t*>(p[1]), reinterpret_cast<uint32_t*>(p[2]), c->stream));
    DHT_TRY(hipMemcpyAsync(out_inserted, p[1], sz[1], hipMemcpyDeviceToHost, c->stream));
    return sr_finish(c, reinterpret_cast<uint32_t*>(p[2]));
}

int dhtgpu_sr_status_dev(dhtgpu_ctx* c, const uint32_t* slots, uint32_t m, uint32_t* out4, void* stream) {
    if (int r = sr_check(c, slots, m)) return r;
    if (m && !out4) return DHTGPU_EINVAL;
    if (!m) return DHTGPU_OK;
    DHT_TRY(c->bind());
    DHT_TRY(launch_sr_status(c->sr.view(), slots, m, out4, c->stream_or(stream)));
    return DHTGPU_OK;
}

int dhtgpu_sr_status(dhtgpu_ctx* c, const uint32_t* slots, uint32_t m, uint32_t* out4) {
    if (int r = sr_check(c, slots, m)) return r;
    if (m && !out4) return DHTGPU_EINVAL;
    if (int r = sr_check_slots(c, slots, m, false)) return r;
    if (!m) return DHTGPU_OK;
    DHT_TRY(c->bind());
    const size_t sz[] = {(size_t)m * 4, (size_t)m * 16};
    uint8_t* p[2];
    DHT_TRY(carve(c->sr.io, sz, p));
    if (int r = sr_upload_slots(c, p[0], slots, m)) return r;
    DHT_TRY(launch_sr_status(c->sr.view(), reinterpret_cast<uint32_t*>(p[0]), m, reinterpret_cast<uint32_t*>(p[1]),
                             c->stream));
    DHT_TRY(hipMemcpyAsync(out4, p[1], sz[1], hipMemcpyDeviceToHost, c->stream));
    DHT_TRY(hipStreamSynchronize(c->stream));
    return DHTGPU_OK;
}

int dhtgpu_sr_lists_dev(dhtgpu_ctx* c, const uint32_t* slots, uint32_t m, uint32_t* out_handle, uint8_t* out_flags,
                        uint32_t* out_len, void* stream) {
    if (int r = sr_check(c, slots, m)) return r;
    if (m && !out_handle) return DHTGPU_EINVAL;
    if (!m) return DHTGPU_OK;
    DHT_TRY(c->bind());
    DHT_TRY(launch_sr_lists(c->sr.view(), slots, m, out_handle, out_flags, out_len, c->stream_or(stream)));
    return DHTGPU_OK;
}

int dhtgpu_sr_lists(dhtgpu_ctx* c, const uint32_t* slots, uint32_t m, uint32_t* out_handle, uint8_t* out_flags,
                    uint32_t* out_len) {
    if (int r = sr_check(c, slots, m)) return r;
    if (m && !out_handle) return DHTGPU_EINVAL;
    if (int r = sr_check_slots(c, slots, m, false)) return r;
    if (!m) return DHTGPU_OK;
    DHT_TRY(c->bind());
    const size_t sz[] = {(size_t)m * 4, (size_t)m * DHTGPU_SR_CAP * 4, (size_t)m * DHTGPU_SR_CAP, (size_t)m * 4};
    uint8_t* p[4];
    DHT_TRY(carve(c->sr.io, sz, p));
    if (int r = sr_upload_slots(c, p[0], slots, m)) return r;
    DHT_TRY(launch_sr_lists(c->sr.view(), reinterpret_cast<uint32_t*>(p[0]), m, reinterpret_cast<uint32_t*>(p[1]), p[2],
                            reinterpret_cast<uint32_t*>(p[3]), c->stream));
    DHT_TRY(hipMemcpyAsync(out_handle, p[1], sz[1], hipMemcpyDeviceToHost, c->stream));
    if (out_flags) DHT_TRY(hipMemcpyAsync(out_flags, p[2], sz[2], hipMemcpyDeviceToHost, c->stream));
    if (out_len) DHT_TRY(hipMemcpyAsync(out_len, p[3], sz[3], hipMemcpyDeviceToHost, c->stream));
    DHT_TRY(hipStreamSynchronize(c->stream));
    return DHTGPU_OK;
}

// ---- K10s: Dht::searchStep for find_node searches ------------------------------------------------
int dhtgpu_srs_set_clock(dhtgpu_ctx* c, uint32_t now) {
    if (!c) return DHTGPU_EINVAL;
    if (now == 0) return DHTGPU_ERANGE;   // 0 is "never set"
    c->sr.clock = now;
    return DHTGPU_OK;
}

int dhtgpu_srs_set_request(dhtgpu_ctx* c, const uint32_t* slots, const uint32_t* handles, const uint8_t* val,
                           uint32_t m) {
    if (int r = sr_check(c, slots, m)) return r;
    if (m && (!handles || !val)) return DHTGPU_EINVAL;
    for (uint32_t j = 0; j < m; ++j)
        if (val[j] > 2) return DHTGPU_EINVAL;
    if (int r = sr_check_slots(c, slots, m, false)) return r;
    if (!handle_extent(handles, m)) return DHTGPU_EINVAL;
    if (!m) return DHTGPU_OK;
    DHT_TRY(c->bind());
    const size_t sz[] = {(size_t)m * 4, (size_t)m * 4, (size_t)m};
    uint8_t* p[3];
    DHT_TRY(carve(c->sr.io, sz, p));
    if (int r = sr_upload_slots(c, p[0], slots, m)) return r;
    DHT_TRY(hipMemcpyAsync(p[1], handles, sz[1], hipMemcpyHostToDevice, c->stream));
    DHT_TRY(hipMemcpyAsync(p[2], val, sz[2], hipMemcpyHostToDevice, c->stream));
    DHT_TRY(launch_srs_request(c->sr.view(), reinterpret_cast<uint32_t*>(p[0]), reinterpret_cast<uint32_t*>(p[1]), p[2], m,
                               c->stream));
    return DHTGPU_OK;
}

int dhtgpu_srs_step_dev(dhtgpu_ctx* c, const uint32_t* slots, uint32_t m, uint32_t node_expire, uint32_t refill_count,
                        uint32_t* out_send, uint32_t* out4, void* stream) {
    if (int r = srs_step_check(c, slots, m, refill_count, out_send, out4)) return r;
    if (!m) return DHTGPU_OK;
    DHT_TRY(c->bind());
    DHT_TRY(launch_srs_step(c->sr.view(), srs_nc(c, refill_count), slots, m, node_expire, refill_count, out_send, out4,
                            nullptr, c->stream_or(stream)));
    return DHTGPU_OK;
}

int dhtgpu_srs_step(dhtgpu_ctx* c, const uint32_t* slots, uint32_t m, uint32_t node_expire, uint32_t refill_count,
                    uint32_t* out_send, uint32_t* out4) {
    if (int r = srs_step_check(c, slots, m, refill_count, out_send, out4)) return r;
    if (int r = sr_check_slots(c, slots, m, true)) return r;
    if (!m) return DHTGPU_OK;
    DHT_TRY(c->bind());
    // slots | send rows | out4 | overflow word
    const size_t sz[] = {(size_t)m * 4, (size_t)m * DHTGPU_SR_CAP * 4, (size_t)m * 16, 4};
    uint8_t* p[4];
    DHT_TRY(carve(c->sr.io, sz, p));
    if (int r = sr_upload_slots(c, p[0], slots, m)) return r;
    DHT_TRY(hipMemsetAsync(p[3], 0, 4, c->stream));
    DHT_TRY(launch_srs_step(c->sr.view(), srs_nc(c, refill_count), reinterpret_cast<uint32_t*>(p[0]), m, node_expire,
                            refill_count, reinterpret_cast<uint32_t*>(p[1]), reinterpret_cast<uint32_t*>(p[2]),
                            reinterpret_cast<uint32_t*>(p[3]), c->stream));
    DHT_TRY(hipMemcpyAsync(out_send, p[1], sz[1], hipMemcpyDeviceToHost, c->stream));
    DHT_TRY(hipMemcpyAsync(out4, p[2], sz[2], hipMemcpyDeviceToHost, c->stream));
    return sr_finish(c, reinterpret_cast<uint32_t*>(p[3]));
}

int dhtgpu_srs_entries_dev(dhtgpu_ctx* c, const uint32_t* slots, uint32_t m, uint8_t* out_req, uint32_t* out_tick,
                           void* stream) {
    if (int r = sr_check(c, slots, m)) return r;
    if (!m) return DHTGPU_OK;
    DHT_TRY(c->bind());
    DHT_TRY(launch_srs_entries(c->sr.view(), slots, m, out_req, out_tick, c->stream_or(stream)));
    return DHTGPU_OK;
}

int dhtgpu_srs_entries(dhtgpu_ctx* c, const uint32_t* slots, uint32_t m, uint8_t* out_req, uint32_t* out_tick) {
    if (int r = sr_check(c, slots, m)) return r;
    if (int r = sr_check_slots(c, slots, m, false)) return r;
    if (!m) return DHTGPU_OK;
    DHT_TRY(c->bind());
    const size_t sz[] = {(size_t)m * 4, (size_t)m * DHTGPU_SR_CAP, (size_t)m * DHTGPU_SR_CAP * 4};
    uint8_t* p[3];
    DHT_TRY(carve(c->sr.io, sz, p));
    if (int r = sr_upload_slots(c, p[0], slots, m)) return r;
    DHT_TRY(launch_srs_entries(c->sr.view(), reinterpret_cast<uint32_t*>(p[0]), m, p[1], reinterpret_cast<uint32_t*>(p[2]),
                               c->stream));
    if (out_req) DHT_TRY(hipMemcpyAsync(out_req, p[1], sz[1], hipMemcpyDeviceToHost, c->stream));
    if (out_tick) DHT_TRY(hipMemcpyAsync(out_tick, p[2], sz[2], hipMemcpyDeviceToHost, c->stream));
    DHT_TRY(hipStreamSynchronize(c->stream));
    return DHTGPU_OK;
}

// ---- K10m: Dht::trySearchInsert over the searches' ordered map -------------------------------------
int dhtgpu_srm_set(dhtgpu_ctx* c, const uint32_t* slots, uint32_t ns) {
    if (int r = sr_check(c, slots, ns)) return r;
    if (int r = sr_check_slots(c, slots, ns, true)) return r;
    dhtgpu_ctx::Searches::Map& mp = c->sr.map;
    mp.valid = false;
    DHT_TRY(c->bind());
    DHT_TRY(hipStreamSynchronize(c->stream));   // (an offer in flight reads the buffers replaced below)
    DHT_TRY(mp.work.ensure(kSrmWorkWords * 4));
    DHT_TRY(hipMemsetAsync(mp.work.p, 0, kSrmWorkWords * 4, c->stream));
    mp.ns = ns;
    mp.stride = pad_ids(ns ? ns : 1);
    if (ns) {
        DHT_TRY(mp.in.ensure((size_t)mp.stride * 5 * 4));
        DHT_TRY(mp.planes.ensure((size_t)mp.stride * 5 * 4));
        DHT_TRY(mp.perm.ensure((size_t)mp.stride * 4));
        DHT_TRY(mp.order.ensure((size_t)ns * 4));
        DHT_TRY(c->sort_scratch.ensure(sort_scratch_bytes(ns)));
        DHT_TRY(c->sr.io.ensure((size_t)ns * 4));
        if (int r = sr_upload_slots(c, c->sr.io.as<uint8_t>(), slots, ns)) return r;
        DHT_TRY(launch_srm_gather(c->sr.view(), c->sr.io.as<uint32_t>(), ns, mp.in.as<uint32_t>(), mp.stride, c->stream));
        int unique = 1;
        DHT_TRY(launch_sort_ids(mp.in.as<uint32_t>(), mp.stride, ns, mp.planes.as<uint32_t>(), mp.stride,
                                mp.perm.as<uint32_t>(), c->sort_scratch.p, &unique, c->stream));
        DHT_TRY(hipStreamSynchronize(c->stream));
        if (!unique) return DHTGPU_EUNSORTED;   // a std::map has unique keys: the map stays invalid
        DHT_TRY(launch_srm_order(c->sr.io.as<uint32_t>(), mp.perm.as<uint32_t>(), ns, mp.order.as<uint32_t>(), c->stream));
    }
    mp.valid = true;
    return DHTGPU_OK;
}

int dhtgpu_srm_set_done(dhtgpu_ctx* c, const uint32_t* slots, const uint8_t* val, uint32_t m) {
    if (int r = sr_check(c, slots, m)) return r;
    if (m && !val) return DHTGPU_EINVAL;
    if (int r = sr_check_slots(c, slots, m, false)) return r;
    if (!m) return DHTGPU_OK;
    DHT_TRY(c->bind());
    const uint32_t* d_slots;
    const uint8_t* d_val;
    if (int r = stage_idx_val(c, c->sr.io, slots, val, m, &d_slots, &d_val)) return r;
    DHT_TRY(launch_srm_done(c->sr.view(), d_slots, d_val, m, c->stream));
    return DHTGPU_OK;
}

int dhtgpu_srm_offer_dev(dhtgpu_ctx* c, const uint32_t* handles, const uint32_t* id_planes, uint64_t id_stride,
                         uint32_t m, uint32_t* out_cnt, uint32_t* out_touched, uint32_t* out_stats, void* stream) {
    if (!c || (m && (!handles || !id_planes || !out_cnt))) return DHTGPU_EINVAL;
    if (!c->sr.valid || !c->sr.map.valid) return DHTGPU_ENOIDS;
    if (!m) return DHTGPU_OK;
    DHT_TRY(c->bind());
    return srm_offer_on(c, handles, id_planes, id_stride, m, out_cnt, out_touched, out_stats, c->stream_or(stream));
}

int dhtgpu_srm_offer(dhtgpu_ctx* c, const uint32_t* handles, const uint8_t* ids20, uint32_t m, uint32_t* out_cnt,
                     uint32_t* out_touched, uint32_t* out_stats) {
    if (!c || (m && (!handles || !ids20 || !out_cnt))) return DHTGPU_EINVAL;
    if (!c->sr.valid || !c->sr.map.valid) return DHTGPU_ENOIDS;
    if (!handle_extent(handles, m)) return DHTGPU_EINVAL;
    if (!m) return DHTGPU_OK;
    DHT_TRY(c->bind());
    const uint64_t is = pad_q(m);
    const size_t tw = (size_t)((c->sr.nslots + 31) / 32) * 4;
    // handles | id planes | counts | touched mask | stats
    const size_t sz[] = {(size_t)m * 4, (size_t)is * 5 * 4, (size_t)m * 4, tw ? tw : 4, 16};
    uint8_t* p[5];
    DHT_TRY(carve(c->sr.io, sz, p));
    DHT_TRY(hipMemcpyAsync(p[0], handles, sz[0], hipMemcpyHostToDevice, c->stream));
    if (int r = upload_ids(c, ids20, m, reinterpret_cast<uint32_t*>(p[1]), is)) return r;
    if (int r = srm_offer_on(c, reinterpret_cast<uint32_t*>(p[0]), reinterpret_cast<uint32_t*>(p[1]), is, m,
                             reinterpret_cast<uint32_t*>(p[2]), reinterpret_cast<uint32_t*>(p[3]),
                             reinterpret_cast<uint32_t*>(p[4]), c->stream))
        return r;
    uint32_t stats[4] = {0, 0, 0, 0};
    DHT_TRY(hipMemcpyAsync(out_cnt, p[2], sz[2], hipMemcpyDeviceToHost, c->stream));
    if (out_touched && tw) DHT_TRY(hipMemcpyAsync(out_touched, p[3], tw, hipMemcpyDeviceToHost, c->stream));
    DHT_TRY(hipMemcpyAsync(stats, p[4], 16, hipMemcpyDeviceToHost, c->stream));
    DHT_TRY(hipStreamSynchronize(c->stream));
    if (out_stats) memcpy(out_stats, stats, 16);
    return stats[3] ? DHTGPU_ERANGE : DHTGPU_OK;
}

int dhtgpu_srm_export(dhtgpu_ctx* c, uint32_t* out_slots, uint8_t* out_done, uint32_t* out_ns) {
    if (!c || !out_ns) return DHTGPU_EINVAL;
    if (!c->sr.valid || !c->sr.map.valid) return DHTGPU_ENOIDS;
    const dhtgpu_ctx::Searches::Map& mp = c->sr.map;
    *out_ns = mp.ns;
    if (!mp.ns || (!out_slots && !out_done)) return DHTGPU_OK;
    DHT_TRY(c->bind());
    std::vector<uint32_t> order(mp.ns);
    std::vector<uint8_t> bits(c->sr.nslots);
    DHT_TRY(hipMemcpyAsync(order.data(), mp.order.p, (size_t)mp.ns * 4, hipMemcpyDeviceToHost, c->stream));
    DHT_TRY(hipMemcpyAsync(bits.data(), c->sr.bits.p, c->sr.nslots, hipMemcpyDeviceToHost, c->stream));
    DHT_TRY(hipStreamSynchronize(c->stream));
    for (uint32_t j = 0; j < mp.ns; ++j) {
        if (out_slots) out_slots[j] = order[j];
        if (out_done) out_done[j] = order[j] < c->sr.nslots ? (bits[order[j]] >> 2) & 1u : 0u;
    }
    return DHTGPU_OK;
}

}  // extern "C"
