// api_ncache.hip -- the C ABI's resident NodeCache (K8w, dhtgpu_nc_*; K8r, dhtgpu_ncr_*): the mirror's two buffer
// sets, its accept mask by handle, incremental insert / erase, the stream-ordered lookups, and keys to handles.
// The one unit that changes the context's nc state (the resident searches read its view).
#include "api_ctx.h"

// The accept mask covers handles [0, nh): it grows geometrically, new bits 0, on the context's
// stream.  The mask it replaces is kept until the next growth, for lookups in flight on other streams.
static int nc_mask_ensure(dhtgpu_ctx* c, uint64_t nh) {
    dhtgpu_ctx::NCache& t = c->nc;
    if (int r = grow_kept(c, t.bits, t.bits_old, (size_t)t.words * 4, (size_t)((nh + 31) / 32) * 4, 1024 * 4,
                          DHTGPU_NC_MAX_HANDLE / 32 * 4))
        return r;
    t.words = t.bits.cap / 4;
    return DHTGPU_OK;
}

// Room for `need` keys in buffer set `which` (its contents are not kept), with head-room of a half.
static int nc_room(dhtgpu_ctx* c, int which, uint64_t need) {
    dhtgpu_ctx::NCache& t = c->nc;
    if (t.cap[which] >= need && t.set[which].p) return DHTGPU_OK;
    const uint64_t cap = (std::max<uint64_t>(1024, need + need / 2) + 63) & ~uint64_t(63);
    t.cap[which] = 0;
    DHT_TRY(t.set[which].ensure((size_t)cap * 6 * 4));
    t.cap[which] = cap;
    return DHTGPU_OK;
}

// m keys (host) sorted into out_planes, nc.perm = the permutation; synchronises.
static int nc_sort_batch(dhtgpu_ctx* c, const uint8_t* ids20, uint64_t m, uint32_t* out_planes, uint64_t out_stride,
                         int* unique) {
    dhtgpu_ctx::NCache& t = c->nc;
    const uint64_t ms = pad_ids(m ? m : 1);
    DHT_TRY(t.in.ensure((size_t)ms * 5 * 4));
    DHT_TRY(t.perm.ensure((size_t)ms * 4));
    if (int r = upload_ids(c, ids20, m, t.in.as<uint32_t>(), ms)) return r;
    DHT_TRY(c->sort_scratch.ensure(sort_scratch_bytes(m)));
    DHT_TRY(launch_sort_ids(t.in.as<uint32_t>(), ms, m, out_planes, out_stride, t.perm.as<uint32_t>(), c->sort_scratch.p,
                            unique, c->stream));
    DHT_TRY(hipStreamSynchronize(c->stream));
    return DHTGPU_OK;
}

// What the ncr forms of a mutation add: get_nodes draws its handles from `free` (the first
// min(nfree, m) are uploaded) instead of taking them from the caller; both report handles.
struct NcResolve {
    const uint32_t* free;   // get_nodes: the caller's free handles; extract: null
    uint32_t nfree;
    uint32_t* out_handle;   // [m] host
    uint32_t* out_used;     // nullable
};

// insert / erase (and get_nodes / extract: rs set): sort the batch, rank it, read the kept count
// (and the result bytes, and rs's handles) back, one pass into the other buffer set.
static int nc_mutate(dhtgpu_ctx* c, bool erase, const uint8_t* ids20, const uint32_t* handles, const uint8_t* accept,
                     uint32_t m, uint8_t* out_res, const NcResolve* rs = nullptr) {
    dhtgpu_ctx::NCache& t = c->nc;
    const uint64_t ms = pad_ids(m);
    DHT_TRY(t.sorted.ensure((size_t)ms * 5 * 4));
    int unique = 1;   // repeats inside a batch are allowed
    if (int r = nc_sort_batch(c, ids20, m, t.sorted.as<uint32_t>(), ms, &unique)) return r;
    const size_t nb = ((size_t)m + 255) / 256;   // rank | flag | block counts | their scan | kpos | ksrc | total | result bytes
    const bool draw = rs && !erase;              // ... | get_nodes: order counts | their scan | total | order | free handles
    const uint32_t nup = draw ? std::min(rs->nfree, m) : 0;
    const size_t sz[] = {(size_t)m * 4, (size_t)m * 4, nb * 4, nb * 4, (size_t)m * 4, (size_t)m * 4, 4, (size_t)m,
                         draw ? nb * 4 : size_t(0), draw ? nb * 4 : size_t(0), draw ? size_t(4) : size_t(0),
                         draw ? (size_t)m * 4 : size_t(0), (size_t)nup * 4};
    uint8_t* p[13];
    DHT_TRY(carve(t.work, sz, p));
    uint32_t* rank = reinterpret_cast<uint32_t*>(p[0]);
    uint32_t* flag = reinterpret_cast<uint32_t*>(p[1]);
    uint32_t* kpos = reinterpret_cast<uint32_t*>(p[4]);
    uint32_t* ksrc = reinterpret_cast<uint32_t*>(p[5]);
    if (!erase || rs) DHT_TRY(t.hin.ensure((size_t)m * 4));   // (extract: the freed handles)
    if (!erase) {
        if (draw) {
            if (nup) DHT_TRY(hipMemcpyAsync(p[12], rs->free, (size_t)nup * 4, hipMemcpyHostToDevice, c->stream));
        } else {
            DHT_TRY(hipMemcpyAsync(t.hin.p, handles, (size_t)m * 4, hipMemcpyHostToDevice, c->stream));
        }
        if (accept) {
            DHT_TRY(t.ain.ensure((size_t)m));
            DHT_TRY(hipMemcpyAsync(t.ain.p, accept, (size_t)m, hipMemcpyHostToDevice, c->stream));
        }
    }
    const NcView v = t.view();
    DHT_TRY(launch_nc_rank(erase, v, t.sorted.as<uint32_t>(), ms, t.perm.as<uint32_t>(), m, rank, flag,
                           reinterpret_cast<uint32_t*>(p[2]), reinterpret_cast<uint32_t*>(p[3]), kpos, ksrc,
                           reinterpret_cast<uint32_t*>(p[6]), p[7], c->stream));
    if (draw)
        DHT_TRY(launch_ncr_assign(v, t.sorted.as<uint32_t>(), ms, t.perm.as<uint32_t>(), m, rank, flag, p[7],
                                  reinterpret_cast<uint32_t*>(p[8]), reinterpret_cast<uint32_t*>(p[9]),
                                  reinterpret_cast<uint32_t*>(p[10]), reinterpret_cast<uint32_t*>(p[11]),
                                  reinterpret_cast<uint32_t*>(p[12]), nup, t.hin.as<uint32_t>(), c->stream));
    else if (rs)
        DHT_TRY(launch_ncr_extract(v, t.perm.as<uint32_t>(), rank, flag, m, t.hin.as<uint32_t>(), c->stream));
    uint32_t kept = 0;
    DHT_TRY(hipMemcpyAsync(&kept, p[6], 4, hipMemcpyDeviceToHost, c->stream));
    if (out_res) DHT_TRY(hipMemcpyAsync(out_res, p[7], (size_t)m, hipMemcpyDeviceToHost, c->stream));
    if (rs) DHT_TRY(hipMemcpyAsync(rs->out_handle, t.hin.p, (size_t)m * 4, hipMemcpyDeviceToHost, c->stream));
    DHT_TRY(hipStreamSynchronize(c->stream));
    if (draw) {
        if (rs->out_used) *rs->out_used = kept;
        if (kept > rs->nfree) return DHTGPU_ERANGE;   // nothing applied
    }
    if (!kept) return DHTGPU_OK;
    const int dst = t.cur ^ 1;
    const uint64_t nn = erase ? (uint64_t)t.n - kept : (uint64_t)t.n + kept;
    if (int r = nc_room(c, dst, nn)) return r;
    if (erase) {
        DHT_TRY(launch_nc_erase(v, t.set[dst].as<uint32_t>(), t.cap[dst], kpos, kept, c->stream));
    } else {
        // the mask covers the handles the merge writes: the caller's, or the free handles drawn
        if (int r = nc_mask_ensure(c, draw ? handle_extent(rs->free, kept) : handle_extent(handles, m))) return r;
        DHT_TRY(launch_nc_insert(v, t.set[dst].as<uint32_t>(), t.cap[dst], kpos, ksrc, kept, t.sorted.as<uint32_t>(), ms,
                                 t.perm.as<uint32_t>(), t.hin.as<uint32_t>(), accept ? t.ain.as<uint8_t>() : nullptr,
                                 t.bits.as<uint32_t>(), c->stream));
    }
    DHT_TRY(hipStreamSynchronize(c->stream));
    t.cur = dst;
    t.n = (uint32_t)nn;
    return DHTGPU_OK;
}

extern "C" {

int dhtgpu_nc_set(dhtgpu_ctx* c, const uint8_t* ids20, const uint32_t* handles, uint64_t n) {
    if (!c || (!ids20 && n)) return DHTGPU_EINVAL;
    if (n >= 0xFFFFFFFFull) return DHTGPU_ERANGE;
    if (!handles && n > DHTGPU_NC_MAX_HANDLE) return DHTGPU_EINVAL;
    const uint64_t ext = handles ? handle_extent(handles, n) : std::max<uint64_t>(n, 1);
    if (!ext) return DHTGPU_EINVAL;
    DHT_TRY(c->bind());
    dhtgpu_ctx::NCache& t = c->nc;
    t.valid = false;
    t.n = 0;
    t.cur = 0;
    if (int r = nc_room(c, 0, n)) return r;
    int unique = 1;
    if (int r = nc_sort_batch(c, ids20, n, t.set[0].as<uint32_t>(), t.cap[0], &unique)) return r;
    if (!unique) return DHTGPU_EUNSORTED;
    if (int r = nc_mask_ensure(c, ext)) return r;
    DHT_TRY(hipMemsetAsync(t.bits.p, 0, (size_t)t.words * 4, c->stream));
    if (handles) {
        DHT_TRY(t.hin.ensure((size_t)n * 4 + 4));
        DHT_TRY(hipMemcpyAsync(t.hin.p, handles, (size_t)n * 4, hipMemcpyHostToDevice, c->stream));
    } else {
        if (n) DHT_TRY(hipMemsetAsync(t.bits.p, 0xFF, (size_t)((n + 31) / 32) * 4, c->stream));   // (past n: never read)
    }
    DHT_TRY(launch_nc_handles(t.perm.as<uint32_t>(), handles ? t.hin.as<uint32_t>() : nullptr, (uint32_t)n,
                              t.set[0].as<uint32_t>() + 5 * t.cap[0], t.bits.as<uint32_t>(), c->stream));
    DHT_TRY(hipStreamSynchronize(c->stream));
    t.n = (uint32_t)n;
    t.valid = true;
    return DHTGPU_OK;
}

int dhtgpu_nc_insert(dhtgpu_ctx* c, const uint8_t* ids20, const uint32_t* handles, const uint8_t* accept, uint32_t m,
                     uint8_t* out_new) {
    if (!c || (m && (!ids20 || !handles))) return DHTGPU_EINVAL;
    if (!c->nc.valid) return DHTGPU_ENOIDS;
    if ((uint64_t)c->nc.n + m >= 0xFFFFFFFFull) return DHTGPU_ERANGE;   // (before any array is read)
    if (m && !handle_extent(handles, m)) return DHTGPU_EINVAL;   // nothing applied
    if (!m) return DHTGPU_OK;
    DHT_TRY(c->bind());
    return nc_mutate(c, false, ids20, handles, accept, m, out_new);
}

int dhtgpu_nc_erase(dhtgpu_ctx* c, const uint8_t* ids20, uint32_t m, uint8_t* out_found) {
    if (!c || (m && !ids20)) return DHTGPU_EINVAL;
    if (!c->nc.valid) return DHTGPU_ENOIDS;
    if (!m) return DHTGPU_OK;
    DHT_TRY(c->bind());
    return nc_mutate(c, true, ids20, nullptr, nullptr, m, out_found);
}

int dhtgpu_nc_update_accept(dhtgpu_ctx* c, const uint32_t* handles, const uint8_t* val, uint32_t m) {
    if (!c || (m && (!handles || !val))) return DHTGPU_EINVAL;
    if (!c->nc.valid) return DHTGPU_ENOIDS;
    const uint64_t ext = handle_extent(handles, m);
    if (!ext) return DHTGPU_EINVAL;   // nothing applied
    if (!m) return DHTGPU_OK;
    DHT_TRY(c->bind());
    dhtgpu_ctx::NCache& t = c->nc;
    if (int r = nc_mask_ensure(c, ext)) return r;
    const uint32_t* d_idx;
    const uint8_t* d_val;
    if (int r = stage_idx_val(c, t.hin, handles, val, m, &d_idx, &d_val)) return r;
    DHT_TRY(launch_bits_update(t.bits.as<uint32_t>(), d_idx, d_val, m, c->stream));
    return DHTGPU_OK;
}

int dhtgpu_nc_set_accept(dhtgpu_ctx* c, const uint8_t* accept_by_handle, uint32_t nh) {
    if (!c || (nh && !accept_by_handle) || nh > DHTGPU_NC_MAX_HANDLE) return DHTGPU_EINVAL;
    if (!c->nc.valid) return DHTGPU_ENOIDS;
    if (!nh) return DHTGPU_OK;
    DHT_TRY(c->bind());
    dhtgpu_ctx::NCache& t = c->nc;
    if (int r = nc_mask_ensure(c, nh)) return r;
    DHT_TRY(t.ain.ensure((size_t)nh));
    DHT_TRY(hipMemcpyAsync(t.ain.p, accept_by_handle, (size_t)nh, hipMemcpyHostToDevice, c->stream));
    DHT_TRY(launch_nc_bits_pack(t.ain.as<uint8_t>(), nh, t.bits.as<uint32_t>(), c->stream));
    return DHTGPU_OK;
}

int dhtgpu_nc_size(dhtgpu_ctx* c, uint64_t* out_n) {
    if (!c || !out_n) return DHTGPU_EINVAL;
    if (!c->nc.valid) return DHTGPU_ENOIDS;
    *out_n = c->nc.n;
    return DHTGPU_OK;
}

int dhtgpu_nc_export(dhtgpu_ctx* c, uint8_t* out_ids20, uint32_t* out_handles) {
    if (!c) return DHTGPU_EINVAL;
    if (!c->nc.valid) return DHTGPU_ENOIDS;
    const NcView v = c->nc.view();
    if (!v.n) return DHTGPU_OK;
    DHT_TRY(c->bind());
    if (out_ids20) {
        DHT_TRY(c->nc.in.ensure((size_t)v.n * 20));
        DHT_TRY(launch_unpack(v.kp, v.ks, 0, v.n, c->nc.in.as<uint8_t>(), c->stream));
        DHT_TRY(hipMemcpyAsync(out_ids20, c->nc.in.p, (size_t)v.n * 20, hipMemcpyDeviceToHost, c->stream));
    }
    if (out_handles) DHT_TRY(hipMemcpyAsync(out_handles, v.hp, (size_t)v.n * 4, hipMemcpyDeviceToHost, c->stream));
    DHT_TRY(hipStreamSynchronize(c->stream));
    return DHTGPU_OK;
}

int dhtgpu_nc_nodes_dev(dhtgpu_ctx* c, const uint32_t* tp, uint64_t ts, uint32_t q, uint32_t count, uint32_t* out_handle,
                        uint32_t* out_cnt, void* stream) {
    if (!c || count == 0 || count > DHTGPU_MAX_K || (q && (!tp || !out_handle || !out_cnt))) return DHTGPU_EINVAL;
    if (!c->nc.valid) return DHTGPU_ENOIDS;
    if (!q) return DHTGPU_OK;
    DHT_TRY(c->bind());
    DHT_TRY(launch_nc_nodes(c->nc.view(), tp, ts, q, count, out_handle, out_cnt, c->stream_or(stream)));
    return DHTGPU_OK;
}

int dhtgpu_nc_nodes(dhtgpu_ctx* c, const uint8_t* t20, uint32_t q, uint32_t count, uint32_t* out_handle,
                    uint32_t* out_cnt) {
    if (!c || count == 0 || count > DHTGPU_MAX_K || (q && (!t20 || !out_handle || !out_cnt))) return DHTGPU_EINVAL;
    if (!c->nc.valid) return DHTGPU_ENOIDS;
    if (!q) return DHTGPU_OK;
    DHT_TRY(c->bind());
    return host_topk(c, t20, q, count, out_handle, out_cnt,
                     [&](const uint32_t* tp, uint64_t ts, uint32_t* d_h, uint32_t* d_cnt) {
        return dhtgpu_nc_nodes_dev(c, tp, ts, q, count, d_h, d_cnt, c->stream);
    });
}

int dhtgpu_ncr_find_dev(dhtgpu_ctx* c, const uint32_t* ip, uint64_t is, uint32_t m, uint32_t* out_handle,
                        uint8_t* out_accept, void* stream) {
    if (!c || (m && (!ip || !out_handle || is < m))) return DHTGPU_EINVAL;
    if (!c->nc.valid) return DHTGPU_ENOIDS;
    if (!m) return DHTGPU_OK;
    DHT_TRY(c->bind());
    DHT_TRY(launch_ncr_find(c->nc.view(), c->nc.words, ip, is, m, out_handle, out_accept, c->stream_or(stream)));
    return DHTGPU_OK;
}

int dhtgpu_ncr_find(dhtgpu_ctx* c, const uint8_t* ids20, uint32_t m, uint32_t* out_handle, uint8_t* out_accept) {
    if (!c || (m && (!ids20 || !out_handle))) return DHTGPU_EINVAL;
    if (!c->nc.valid) return DHTGPU_ENOIDS;
    if (!m) return DHTGPU_OK;
    DHT_TRY(c->bind());
    dhtgpu_ctx::NCache& t = c->nc;
    const uint64_t ms = pad_ids(m);
    DHT_TRY(t.in.ensure((size_t)ms * 5 * 4));
    if (int r = upload_ids(c, ids20, m, t.in.as<uint32_t>(), ms)) return r;
    const size_t sz[] = {(size_t)m * 4, (size_t)m};
    uint8_t* p[2];
    DHT_TRY(carve(t.work, sz, p));
    if (int r = dhtgpu_ncr_find_dev(c, t.in.as<uint32_t>(), ms, m, reinterpret_cast<uint32_t*>(p[0]),
                                    out_accept ? p[1] : nullptr, c->stream))
        return r;
    DHT_TRY(hipMemcpyAsync(out_handle, p[0], (size_t)m * 4, hipMemcpyDeviceToHost, c->stream));
    if (out_accept) DHT_TRY(hipMemcpyAsync(out_accept, p[1], (size_t)m, hipMemcpyDeviceToHost, c->stream));
    DHT_TRY(hipStreamSynchronize(c->stream));
    return DHTGPU_OK;
}

int dhtgpu_ncr_get_nodes(dhtgpu_ctx* c, const uint8_t* ids20, uint32_t m, const uint32_t* free_handles, uint32_t nfree,
                         const uint8_t* accept, uint32_t* out_handle, uint8_t* out_new, uint32_t* out_used) {
    if (!c || (m && (!ids20 || !out_handle)) || (nfree && !free_handles)) return DHTGPU_EINVAL;
    if (!c->nc.valid) return DHTGPU_ENOIDS;
    if ((uint64_t)c->nc.n + m >= 0xFFFFFFFFull) return DHTGPU_ERANGE;   // (before any array is read)
    if (nfree && !handle_extent(free_handles, nfree)) return DHTGPU_EINVAL;   // nothing applied
    if (out_used) *out_used = 0;
    if (!m) return DHTGPU_OK;
    DHT_TRY(c->bind());
    const NcResolve rs{free_handles, nfree, out_handle, out_used};
    return nc_mutate(c, false, ids20, nullptr, accept, m, out_new, &rs);
}

int dhtgpu_ncr_extract(dhtgpu_ctx* c, const uint8_t* ids20, uint32_t m, uint32_t* out_handle) {
    if (!c || (m && (!ids20 || !out_handle))) return DHTGPU_EINVAL;
    if (!c->nc.valid) return DHTGPU_ENOIDS;
    if (!m) return DHTGPU_OK;
    DHT_TRY(c->bind());
    const NcResolve rs{nullptr, 0, out_handle, nullptr};
    return nc_mutate(c, true, ids20, nullptr, nullptr, m, nullptr, &rs);
}

}  // extern "C"
