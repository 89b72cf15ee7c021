// api_dht.hip -- the C ABI's one-shot reference interfaces (a table snapshot, the caches, the
// wire format, Search::insertNode, table statistics: everything they need comes with the call)
// and the crawl model.
#include "api_ctx.h"

// Sort n ids (planes, stride) into `out` (sorted planes + permutation); synchronises.
static int sort_into(dhtgpu_ctx* c, const uint32_t* planes, uint64_t stride, uint64_t n, dhtgpu_ctx::SortedSet& out) {
    out.valid = false;
    out.n = n;
    out.stride = pad_ids(n ? n : 1);
    DHT_TRY(out.planes.ensure((size_t)out.stride * 5 * 4));
    DHT_TRY(out.perm.ensure((size_t)out.stride * 4));
    DHT_TRY(c->sort_scratch.ensure(sort_scratch_bytes(n)));
    int unique = 1;
    DHT_TRY(launch_sort_ids(planes, stride, n, out.planes.as<uint32_t>(), out.stride, out.perm.as<uint32_t>(),
                            c->sort_scratch.p, &unique, c->stream));
    DHT_TRY(hipStreamSynchronize(c->stream));
    if (c->sort_scratch.cap > ((size_t)1 << 30)) c->sort_scratch.release();   // large sorts: do not keep GBs
    out.unique = unique != 0;
    out.valid = true;
    return DHTGPU_OK;
}

// The getCachedNodes walk of q targets over a sorted set (perm nullable), accept[] in caller order.
static int cached_walk(dhtgpu_ctx* c, const uint32_t* planes, uint64_t stride, uint64_t n, const uint32_t* perm,
                       const uint8_t* accept, const uint8_t* t20, uint32_t q, uint32_t count, const uint32_t* gidx,
                       uint32_t* out_idx, uint32_t* out_cnt) {
    uint8_t* d_acc = nullptr;
    if (accept && n) {
        DHT_TRY(c->cache_acc.ensure((size_t)n + 16));
        d_acc = c->cache_acc.as<uint8_t>();
        DHT_TRY(hipMemcpyAsync(d_acc, accept, (size_t)n, hipMemcpyHostToDevice, c->stream));
    }
    return host_topk(c, t20, q, count, out_idx, out_cnt,
                     [&](const uint32_t* tp, uint64_t ts, uint32_t* d_idx, uint32_t* d_cnt) -> int {
        DHT_TRY(launch_cached(planes, stride, n, perm, d_acc, tp, ts, q, count, d_idx, d_cnt, c->stream));
        if (gidx) DHT_TRY(launch_map_idx(d_idx, (uint64_t)q * count, gidx, 0, c->stream));
        return DHTGPU_OK;
    });
}

static int buffer_nodes_impl(dhtgpu_ctx* c, const uint32_t* planes, uint64_t stride, uint64_t n,
                             const uint8_t* node_tail, uint32_t af, const uint8_t* t20, uint32_t q,
                             const uint32_t* cand, uint32_t nc, uint8_t* out, uint32_t* out_len, size_t lead) {
    // every candidate must name a node (the kernel reads its planes and tail)
    for (size_t i = 0; i < (size_t)q * nc; ++i)
        if (cand[i] != DHTGPU_NONE && cand[i] >= n) return DHTGPU_EINVAL;
    const uint32_t alen = af == 4 ? 4u : 16u, rec = 20 + alen + 2;
    const size_t tl = (size_t)n * (alen + 2), cl = (size_t)q * nc * 4, ol = (size_t)q * 8 * rec, ll = (size_t)q * 4;
    DHT_TRY(c->wire.ensure(wire_bytes(lead, n, alen, q, nc)));
    uint8_t* base = c->wire.as<uint8_t>() + lead;
    uint8_t* d_tail = base;
    uint32_t* d_cand = reinterpret_cast<uint32_t*>(base + al256(tl));
    uint8_t* d_out = base + al256(tl) + al256(cl);
    uint32_t* d_len = reinterpret_cast<uint32_t*>(d_out + al256(ol));
    if (tl) DHT_TRY(hipMemcpyAsync(d_tail, node_tail, tl, hipMemcpyHostToDevice, c->stream));
    if (cl) DHT_TRY(hipMemcpyAsync(d_cand, cand, cl, hipMemcpyHostToDevice, c->stream));
    uint64_t ts = 0;
    DHT_TRY(c->upload_targets(t20, q, &ts));
    DHT_TRY(launch_wire_encode(planes, stride, d_tail, alen, c->targets.as<uint32_t>(), ts, q, d_cand, nc, d_out,
                               d_len, c->stream));
    DHT_TRY(hipMemcpyAsync(out, d_out, ol, hipMemcpyDeviceToHost, c->stream));
    DHT_TRY(hipMemcpyAsync(out_len, d_len, ll, hipMemcpyDeviceToHost, c->stream));
    DHT_TRY(hipStreamSynchronize(c->stream));
    return DHTGPU_OK;
}

extern "C" {

int dhtgpu_find_closest(dhtgpu_ctx* c, uint32_t nb, const uint8_t* firsts20, const uint32_t* off,
                        const uint8_t* node_ids20, const uint8_t* good, const uint8_t* t20,
                        uint32_t q, uint32_t count, uint32_t* out_idx, uint32_t* out_cnt) {
    if (!c || count == 0 || count > DHTGPU_MAX_K) return DHTGPU_EINVAL;
    if (q && (!t20 || !out_idx || !out_cnt)) return DHTGPU_EINVAL;
    if (nb > 256 || (nb && (!firsts20 || !off))) return DHTGPU_EINVAL;
    if (!q) return DHTGPU_OK;
    if (nb == 0) {   // empty table: empty result (src/routing_table.cpp:116)
        for (uint32_t i = 0; i < q; ++i) {
            out_cnt[i] = 0;
            for (uint32_t r = 0; r < count; ++r) out_idx[(size_t)i * count + r] = DHTGPU_NONE;
        }
        return DHTGPU_OK;
    }
    const uint32_t nn = off[nb];
    if (nn && (!node_ids20 || !good)) return DHTGPU_EINVAL;
    for (uint32_t b = 0; b < nb; ++b)
        if (off[b] > off[b + 1]) return DHTGPU_EINVAL;
    DHT_TRY(c->bind());
    // host snapshot -> one device blob: firsts planes | off | gcnt | node planes | good
    const uint64_t ns = pad_q(nn ? nn : 1);
    const std::vector<uint32_t> fp = firsts_planes(firsts20, nb);
    std::vector<uint32_t> gcnt(nb);
    for (uint32_t b = 0; b < nb; ++b) {
        uint32_t g = 0;
        for (uint32_t i = off[b]; i < off[b + 1]; ++i) g += good[i] != 0;
        gcnt[b] = g;
    }
    const size_t o_fp = 0, o_off = o_fp + fp.size() * 4, o_g = o_off + (size_t)(nb + 1) * 4,
                 o_np = (o_g + (size_t)nb * 4 + 15) & ~size_t(15), o_good = o_np + (size_t)ns * 5 * 4,
                 total = o_good + nn + 16;
    DHT_TRY(c->aux.ensure(total));
    uint8_t* base = c->aux.as<uint8_t>();
    DHT_TRY(hipMemcpyAsync(base + o_fp, fp.data(), fp.size() * 4, hipMemcpyHostToDevice, c->stream));
    DHT_TRY(hipMemcpyAsync(base + o_off, off, (size_t)(nb + 1) * 4, hipMemcpyHostToDevice, c->stream));
    DHT_TRY(hipMemcpyAsync(base + o_g, gcnt.data(), (size_t)nb * 4, hipMemcpyHostToDevice, c->stream));
    if (nn) {
        DHT_TRY(hipMemcpyAsync(base + o_good, good, nn, hipMemcpyHostToDevice, c->stream));
        DHT_TRY(c->staging.ensure((size_t)std::max<uint64_t>(nn, q) * 20));
        DHT_TRY(hipMemcpyAsync(c->staging.p, node_ids20, (size_t)nn * 20, hipMemcpyHostToDevice, c->stream));
        DHT_TRY(launch_pack(c->staging.as<uint8_t>(), nn, (uint32_t*)(base + o_np), ns, c->stream));
        DHT_TRY(hipStreamSynchronize(c->stream));   // staging reused for targets
    }
    return host_topk(c, t20, q, count, out_idx, out_cnt,
                     [&](const uint32_t* tp, uint64_t ts, uint32_t* d_idx, uint32_t* d_cnt) -> int {
        DHT_TRY(launch_find_closest(nb, (const uint32_t*)(base + o_fp), (const uint32_t*)(base + o_off),
                                    (const uint32_t*)(base + o_g), (const uint32_t*)(base + o_np), ns,
                                    base + o_good, tp, ts, q, count, d_idx, d_cnt, c->stream));
        return DHTGPU_OK;
    });
}

int dhtgpu_classify_dev(const uint32_t* planes, uint64_t stride, uint64_t n, uint32_t nb,
                        const uint32_t* d_fp, const uint32_t* myid_words, uint8_t* out_bucket,
                        unsigned long long* d_hist, void* stream) {
    if (!d_fp || !myid_words || !d_hist || nb == 0 || nb > 256 || (n && !planes)) return DHTGPU_EINVAL;
    DHT_TRY(launch_classify(planes, stride, n, nb, d_fp, myid_words, out_bucket, d_hist, (hipStream_t)stream));
    return DHTGPU_OK;
}

int dhtgpu_classify(dhtgpu_ctx* c, uint32_t nb, const uint8_t* firsts20, const uint8_t* myid20,
                    uint8_t* out_bucket, uint64_t* hist161) {
    if (!c || !firsts20 || !myid20 || !hist161 || nb == 0 || nb > 256) return DHTGPU_EINVAL;
    if (!c->has_ids) return DHTGPU_ENOIDS;
    DHT_TRY(c->bind());
    const std::vector<uint32_t> fp = firsts_planes(firsts20, nb);
    uint32_t my[5];
    for (int w = 0; w < 5; ++w) my[w] = be32(myid20 + 4 * w);
    DHT_TRY(c->aux.ensure(fp.size() * 4 + 161 * 8 + 64));
    uint8_t* base = c->aux.as<uint8_t>();
    unsigned long long* d_hist = (unsigned long long*)(base + ((fp.size() * 4 + 15) & ~size_t(15)));
    DHT_TRY(hipMemcpyAsync(base, fp.data(), fp.size() * 4, hipMemcpyHostToDevice, c->stream));
    DHT_TRY(hipMemsetAsync(d_hist, 0, 161 * 8, c->stream));
    uint8_t* d_bucket = nullptr;
    if (out_bucket && c->n) {
        DHT_TRY(c->aux2.ensure((size_t)c->n + 16));
        d_bucket = c->aux2.as<uint8_t>();
    }
    DHT_TRY(launch_classify(c->planes.as<uint32_t>(), c->stride, c->n, nb, (const uint32_t*)base, my,
                            d_bucket, d_hist, c->stream));
    if (d_bucket) DHT_TRY(hipMemcpyAsync(out_bucket, d_bucket, (size_t)c->n, hipMemcpyDeviceToHost, c->stream));
    DHT_TRY(hipMemcpyAsync(hist161, d_hist, 161 * 8, hipMemcpyDeviceToHost, c->stream));
    DHT_TRY(hipStreamSynchronize(c->stream));
    return DHTGPU_OK;
}

int dhtgpu_cached_nodes(dhtgpu_ctx* c, const uint8_t* accept, const uint8_t* t20, uint32_t q,
                        uint32_t count, uint32_t* out_idx, uint32_t* out_cnt) {
    if (int r = check_topk_host(c, t20, q, count, out_idx, out_cnt)) return r;
    DHT_TRY(c->bind());
    if (c->sorted) {
        if (!q) return DHTGPU_OK;
        return cached_walk(c, c->planes.as<uint32_t>(), c->stride, c->n, nullptr, accept, t20, q, count, c->out_map(),
                           out_idx, out_cnt);
    }
    // an unsorted upload: walk its lexicographically sorted view (built once per id set)
    if (!c->sview.valid) {
        int r = sort_into(c, c->planes.as<uint32_t>(), c->stride, c->n, c->sview);
        if (r) return r;
    }
    if (!c->sview.unique) return DHTGPU_EUNSORTED;
    if (!q) return DHTGPU_OK;
    return cached_walk(c, c->sview.planes.as<uint32_t>(), c->sview.stride, c->n, c->sview.perm.as<uint32_t>(), accept,
                       t20, q, count, c->out_map(), out_idx, out_cnt);
}

int dhtgpu_cache_set(dhtgpu_ctx* c, const uint8_t* ids20, uint64_t n, uint64_t version) {
    if (!c || (!ids20 && n)) return DHTGPU_EINVAL;
    if (n >= 0xFFFFFFFFull) return DHTGPU_ERANGE;
    if (version && c->cache.valid && version == c->cache_version && n == c->cache.n) return DHTGPU_OK;
    DHT_TRY(c->bind());
    c->cache.valid = false;
    c->cache_version = 0;
    const uint64_t st = pad_ids(n ? n : 1);
    DHT_TRY(c->cache_in.ensure((size_t)st * 5 * 4));
    int r = upload_ids(c, ids20, n, c->cache_in.as<uint32_t>(), st);
    if (r) return r;
    if ((r = sort_into(c, c->cache_in.as<uint32_t>(), st, n, c->cache))) return r;
    if (!c->cache.unique) {
        c->cache.valid = false;
        return DHTGPU_EUNSORTED;
    }
    c->cache_version = version;
    return DHTGPU_OK;
}

int dhtgpu_cache_nodes(dhtgpu_ctx* c, const uint8_t* accept, const uint8_t* t20, uint32_t q, uint32_t count,
                       uint32_t* out_idx, uint32_t* out_cnt) {
    if (!c || count == 0 || count > DHTGPU_MAX_K || (q && (!t20 || !out_idx || !out_cnt))) return DHTGPU_EINVAL;
    if (!c->cache.valid) return DHTGPU_ENOIDS;
    if (!q) return DHTGPU_OK;
    DHT_TRY(c->bind());
    return cached_walk(c, c->cache.planes.as<uint32_t>(), c->cache.stride, c->cache.n, c->cache.perm.as<uint32_t>(),
                       accept, t20, q, count, nullptr, out_idx, out_cnt);
}

int dhtgpu_cache_sorted(dhtgpu_ctx* c, uint32_t* perm) {
    if (!c || (!perm && c->cache.n)) return DHTGPU_EINVAL;
    if (!c->cache.valid) return DHTGPU_ENOIDS;
    if (!c->cache.n) return DHTGPU_OK;
    DHT_TRY(c->bind());
    DHT_TRY(hipMemcpyAsync(perm, c->cache.perm.p, (size_t)c->cache.n * 4, hipMemcpyDeviceToHost, c->stream));
    DHT_TRY(hipStreamSynchronize(c->stream));
    return DHTGPU_OK;
}

// ---- a11 / f4: compact node wire format ------------------------------------------------

int dhtgpu_buffer_nodes_dev(dhtgpu_ctx* c, const uint8_t* node_tail, uint32_t af, const uint32_t* tp, uint64_t ts,
                            uint32_t q, const uint32_t* cand, uint32_t nc, uint8_t* out, uint32_t* out_len,
                            void* stream) {
    if (!c || (af != 4 && af != 6) || nc > 64) return DHTGPU_EINVAL;
    if (q && (!tp || !out || !out_len || (nc && (!cand || !node_tail)))) return DHTGPU_EINVAL;
    if (!c->has_ids) return DHTGPU_ENOIDS;
    if (!q) return DHTGPU_OK;
    DHT_TRY(c->bind());
    DHT_TRY(launch_wire_encode(c->planes.as<uint32_t>(), c->stride, node_tail, af == 4 ? 4u : 16u, tp, ts, q, cand,
                               nc, out, out_len, c->stream_or(stream)));
    return DHTGPU_OK;
}

int dhtgpu_buffer_nodes(dhtgpu_ctx* c, const uint8_t* node_tail, uint32_t af, const uint8_t* t20, uint32_t q,
                        const uint32_t* cand, uint32_t nc, uint8_t* out, uint32_t* out_len) {
    if (!c || (af != 4 && af != 6) || nc > 64) return DHTGPU_EINVAL;
    if (q && (!t20 || !out || !out_len || (nc && (!cand || !node_tail)))) return DHTGPU_EINVAL;
    if (!c->has_ids) return DHTGPU_ENOIDS;
    if (!q) return DHTGPU_OK;
    DHT_TRY(c->bind());
    return buffer_nodes_impl(c, c->planes.as<uint32_t>(), c->stride, c->n, node_tail, af, t20, q, cand, nc, out,
                             out_len, 0);
}

int dhtgpu_buffer_nodes_ids(dhtgpu_ctx* c, const uint8_t* node_ids20, const uint8_t* node_tail, uint32_t nn,
                            uint32_t af, const uint8_t* t20, uint32_t q, const uint32_t* cand, uint32_t nc,
                            uint8_t* out, uint32_t* out_len) {
    if (!c || (af != 4 && af != 6) || nc > 64) return DHTGPU_EINVAL;
    if (q && (!t20 || !out || !out_len || (nc && (!cand || !node_tail)))) return DHTGPU_EINVAL;
    if (nn && (!node_ids20 || !node_tail)) return DHTGPU_EINVAL;
    if (!q) return DHTGPU_OK;
    DHT_TRY(c->bind());
    // the nodes' planes lead the wire scratch (sized for the whole call first: ensure() may
    // reallocate); the context's id set is left alone
    const uint64_t ns = pad_q(nn ? nn : 1);
    const size_t lead = al256((size_t)ns * 5 * 4);
    DHT_TRY(c->wire.ensure(wire_bytes(lead, nn, af == 4 ? 4u : 16u, q, nc)));
    if (nn) {
        DHT_TRY(c->staging.ensure((size_t)nn * 20));
        DHT_TRY(hipMemcpyAsync(c->staging.p, node_ids20, (size_t)nn * 20, hipMemcpyHostToDevice, c->stream));
        DHT_TRY(launch_pack(c->staging.as<uint8_t>(), nn, c->wire.as<uint32_t>(), ns, c->stream));
        DHT_TRY(hipStreamSynchronize(c->stream));   // staging is reused for the targets
    }
    return buffer_nodes_impl(c, c->wire.as<uint32_t>(), ns, nn, node_tail, af, t20, q, cand, nc, out, out_len, lead);
}

int dhtgpu_deserialize_nodes(dhtgpu_ctx* c, uint32_t af, const uint8_t* myid20, const uint8_t* blob,
                             const uint64_t* msg_off, uint32_t m, const uint8_t* from_af, const uint8_t* from_addr,
                             uint8_t* out_ids20, uint8_t* out_tail, uint8_t* out_status, uint8_t* msg_status,
                             uint32_t* out_nrec) {
    if (!c || (af != 4 && af != 6) || !myid20 || !out_nrec) return DHTGPU_EINVAL;
    if (m && (!msg_off || !from_af || !from_addr || !msg_status)) return DHTGPU_EINVAL;
    *out_nrec = 0;
    if (!m) return DHTGPU_OK;
    const uint32_t alen = af == 4 ? 4u : 16u, rl = 20 + alen + 2;
    // per-message record ranges; a length that is not a whole number of records is the
    // reference's WRONG_NODE_INFO_BUF_LEN (the message's nodes are not used)
    std::vector<uint32_t> rs((size_t)m + 1, 0);
    for (uint32_t i = 0; i < m; ++i) {
        if (msg_off[i + 1] < msg_off[i]) return DHTGPU_EINVAL;
        const uint64_t len = msg_off[i + 1] - msg_off[i];
        msg_status[i] = len % rl ? 1 : 0;
        const uint64_t nr = len % rl ? 0 : len / rl;
        if ((uint64_t)rs[i] + nr > 0xFFFFFFF0ull) return DHTGPU_ERANGE;
        rs[i + 1] = rs[i] + (uint32_t)nr;
    }
    const uint32_t nrec = rs[m];
    *out_nrec = nrec;
    if (!nrec) return DHTGPU_OK;
    if (!blob || !out_ids20 || !out_tail || !out_status) return DHTGPU_EINVAL;
    DHT_TRY(c->bind());
    const uint64_t blen = msg_off[m];
    const size_t sz[] = {(size_t)blen, ((size_t)m + 1) * 8, ((size_t)m + 1) * 4, 32, m, (size_t)m * 16,
                         (size_t)nrec * 20, (size_t)nrec * (alen + 2), nrec};
    uint8_t* p[9];
    DHT_TRY(carve(c->wire, sz, p));
    DHT_TRY(hipMemcpyAsync(p[0], blob, sz[0], hipMemcpyHostToDevice, c->stream));
    DHT_TRY(hipMemcpyAsync(p[1], msg_off, sz[1], hipMemcpyHostToDevice, c->stream));
    DHT_TRY(hipMemcpyAsync(p[2], rs.data(), sz[2], hipMemcpyHostToDevice, c->stream));
    DHT_TRY(hipMemcpyAsync(p[3], myid20, 20, hipMemcpyHostToDevice, c->stream));
    DHT_TRY(hipMemcpyAsync(p[4], from_af, sz[4], hipMemcpyHostToDevice, c->stream));
    DHT_TRY(hipMemcpyAsync(p[5], from_addr, sz[5], hipMemcpyHostToDevice, c->stream));
    DHT_TRY(launch_wire_decode(p[0], reinterpret_cast<const uint64_t*>(p[1]), reinterpret_cast<const uint32_t*>(p[2]),
                               m, nrec, af, p[3], p[4], p[5], p[6], p[7], p[8], c->stream));
    DHT_TRY(hipMemcpyAsync(out_ids20, p[6], sz[6], hipMemcpyDeviceToHost, c->stream));
    DHT_TRY(hipMemcpyAsync(out_tail, p[7], sz[7], hipMemcpyDeviceToHost, c->stream));
    DHT_TRY(hipMemcpyAsync(out_status, p[8], sz[8], hipMemcpyDeviceToHost, c->stream));
    DHT_TRY(hipStreamSynchronize(c->stream));
    return DHTGPU_OK;
}

// RoutingTable::depth (src/routing_table.cpp:100-107) over a table snapshot: one more than
// the larger lowbit (infohash.h:132-143) of the bucket's first and of the next bucket's.
int dhtgpu_table_depth(uint32_t nb, const uint8_t* firsts20, uint32_t b, uint32_t* out_depth) {
    if (!out_depth || (nb && !firsts20) || (nb && b >= nb)) return DHTGPU_EINVAL;
    *out_depth = 0;
    if (!nb) return DHTGPU_OK;
    auto lowbit = [](const uint8_t* h) -> int {
        int i = 19;
        while (i >= 0 && h[i] == 0) --i;
        if (i < 0) return -1;
        int j = 7;
        while (((h[i] >> (7 - j)) & 1) == 0) --j;
        return 8 * i + j;
    };
    const int bit1 = lowbit(firsts20 + 20 * (size_t)b);
    const int bit2 = b + 1 < nb ? lowbit(firsts20 + 20 * (size_t)(b + 1)) : -1;
    *out_depth = (uint32_t)(std::max(bit1, bit2) + 1);
    return DHTGPU_OK;
}

// ---- a10: Search::insertNode, batched ---------------------------------------------------------
int dhtgpu_search_insert(dhtgpu_ctx* c, const uint8_t* node_ids20, const uint8_t* node_state, uint32_t nn,
                         const uint8_t* t20, uint32_t q, uint32_t cap, uint32_t* list_node, uint8_t* list_flags,
                         uint32_t* list_len, uint8_t* search_expired, const uint64_t* ins_off, const uint32_t* ins_node,
                         const uint8_t* ins_token, uint8_t* ins_added) {
    if (!c || cap == 0 || cap > 4096) return DHTGPU_EINVAL;
    if (q && (!t20 || !list_node || !list_flags || !list_len || !search_expired || !ins_off)) return DHTGPU_EINVAL;
    if (!q) return DHTGPU_OK;
    const uint64_t m = ins_off[q];
    if (m && (!ins_node || !ins_token || !ins_added)) return DHTGPU_EINVAL;
    if (nn && (!node_ids20 || !node_state)) return DHTGPU_EINVAL;
    for (uint32_t i = 0; i < q; ++i) {   // every index the kernel follows must name a node
        if (ins_off[i + 1] < ins_off[i] || list_len[i] > cap) return DHTGPU_EINVAL;
        for (uint32_t j = 0; j < list_len[i]; ++j)
            if (list_node[(size_t)i * cap + j] >= nn) return DHTGPU_EINVAL;
    }
    for (uint64_t i = 0; i < m; ++i)
        if (ins_node[i] >= nn) return DHTGPU_EINVAL;
    DHT_TRY(c->bind());
    const uint64_t ns = pad_q(nn ? nn : 1);
    const size_t sz[] = {(size_t)ns * 20, (size_t)nn, (size_t)q * cap * 4, (size_t)q * cap, (size_t)q * 4, (size_t)q,
                         ((size_t)q + 1) * 8, (size_t)m * 4, (size_t)m, (size_t)m, 16};
    uint8_t* p[11];
    DHT_TRY(carve(c->srch, sz, p));
    if (nn) {
        DHT_TRY(c->staging.ensure((size_t)nn * 20));
        DHT_TRY(hipMemcpyAsync(c->staging.p, node_ids20, (size_t)nn * 20, hipMemcpyHostToDevice, c->stream));
        DHT_TRY(launch_pack(c->staging.as<uint8_t>(), nn, reinterpret_cast<uint32_t*>(p[0]), ns, c->stream));
        DHT_TRY(hipMemcpyAsync(p[1], node_state, nn, hipMemcpyHostToDevice, c->stream));
        DHT_TRY(hipStreamSynchronize(c->stream));   // staging is reused for the targets
    }
    DHT_TRY(hipMemcpyAsync(p[2], list_node, sz[2], hipMemcpyHostToDevice, c->stream));
    DHT_TRY(hipMemcpyAsync(p[3], list_flags, sz[3], hipMemcpyHostToDevice, c->stream));
    DHT_TRY(hipMemcpyAsync(p[4], list_len, sz[4], hipMemcpyHostToDevice, c->stream));
    DHT_TRY(hipMemcpyAsync(p[5], search_expired, sz[5], hipMemcpyHostToDevice, c->stream));
    DHT_TRY(hipMemcpyAsync(p[6], ins_off, sz[6], hipMemcpyHostToDevice, c->stream));
    if (m) {
        DHT_TRY(hipMemcpyAsync(p[7], ins_node, sz[7], hipMemcpyHostToDevice, c->stream));
        DHT_TRY(hipMemcpyAsync(p[8], ins_token, sz[8], hipMemcpyHostToDevice, c->stream));
    }
    DHT_TRY(hipMemsetAsync(p[10], 0, 4, c->stream));
    uint64_t ts = 0;
    DHT_TRY(c->upload_targets(t20, q, &ts));
    DHT_TRY(launch_search_insert(reinterpret_cast<uint32_t*>(p[0]), ns, p[1], c->targets.as<uint32_t>(), ts, q, cap,
                                 reinterpret_cast<uint32_t*>(p[2]), p[3], reinterpret_cast<uint32_t*>(p[4]), p[5],
                                 reinterpret_cast<const uint64_t*>(p[6]), reinterpret_cast<const uint32_t*>(p[7]), p[8],
                                 p[9], reinterpret_cast<uint32_t*>(p[10]), c->stream));
    uint32_t overflow = 0;
    DHT_TRY(hipMemcpyAsync(&overflow, p[10], 4, hipMemcpyDeviceToHost, c->stream));
    DHT_TRY(hipMemcpyAsync(list_node, p[2], sz[2], hipMemcpyDeviceToHost, c->stream));
    DHT_TRY(hipMemcpyAsync(list_flags, p[3], sz[3], hipMemcpyDeviceToHost, c->stream));
    DHT_TRY(hipMemcpyAsync(list_len, p[4], sz[4], hipMemcpyDeviceToHost, c->stream));
    DHT_TRY(hipMemcpyAsync(search_expired, p[5], sz[5], hipMemcpyDeviceToHost, c->stream));
    if (m) DHT_TRY(hipMemcpyAsync(ins_added, p[9], sz[9], hipMemcpyDeviceToHost, c->stream));
    DHT_TRY(hipStreamSynchronize(c->stream));
    return overflow ? DHTGPU_ERANGE : DHTGPU_OK;
}

// ---- a4 / a6: InfoHash::lowbit and RoutingTable::depth of every bucket ---------------------------
int dhtgpu_table_stats(dhtgpu_ctx* c, uint32_t nb, const uint8_t* firsts20, int32_t* out_lowbit, uint32_t* out_depth) {
    if (!c || (nb && (!firsts20 || !out_lowbit || !out_depth))) return DHTGPU_EINVAL;
    if (!nb) return DHTGPU_OK;
    DHT_TRY(c->bind());
    const std::vector<uint32_t> fp = firsts_planes(firsts20, nb);
    const size_t a = al256(fp.size() * 4), bsz = al256((size_t)nb * 4);
    DHT_TRY(c->srch.ensure(a + 2 * bsz));
    uint8_t* base = c->srch.as<uint8_t>();
    DHT_TRY(hipMemcpyAsync(base, fp.data(), fp.size() * 4, hipMemcpyHostToDevice, c->stream));
    DHT_TRY(launch_table_stats(reinterpret_cast<uint32_t*>(base), nb, reinterpret_cast<int32_t*>(base + a),
                               reinterpret_cast<uint32_t*>(base + a + bsz), c->stream));
    DHT_TRY(hipMemcpyAsync(out_lowbit, base + a, (size_t)nb * 4, hipMemcpyDeviceToHost, c->stream));
    DHT_TRY(hipMemcpyAsync(out_depth, base + a + bsz, (size_t)nb * 4, hipMemcpyDeviceToHost, c->stream));
    DHT_TRY(hipStreamSynchronize(c->stream));
    return DHTGPU_OK;
}

// ---- f3: crawl replay (iterative searches over a synthetic network) ----------------------
int dhtgpu_net_prepare(dhtgpu_ctx* c, const uint8_t* dead, uint64_t table_seed) {
    if (!c) return DHTGPU_EINVAL;
    if (!c->has_ids || !c->n) return DHTGPU_ENOIDS;
    if (c->has_gidx) return DHTGPU_EINVAL;   // the network is the whole uploaded id set
    DHT_TRY(c->bind());
    // (the whole set's index whatever the accept mask says: the model has its own dead mask)
    int r = index_build_on(c->full_set(), c->stream, nullptr);
    if (r) return r;
    DHT_TRY(c->net_sorted.ensure((size_t)c->n * 8));
    DHT_TRY(launch_net_sort(c->index.p, c->n, c->index_B, c->net_sorted.as<uint2>(), c->stream));
    c->net_has_dead = dead != nullptr;
    if (dead) {
        DHT_TRY(c->net_dead.ensure((size_t)c->n));
        DHT_TRY(hipMemcpyAsync(c->net_dead.p, dead, (size_t)c->n, hipMemcpyHostToDevice, c->stream));
    }
    DHT_TRY(hipStreamSynchronize(c->stream));
    c->net_seed = table_seed;
    c->net_valid = true;
    return DHTGPU_OK;
}

int dhtgpu_set_search_alpha(dhtgpu_ctx* c, uint32_t alpha) {
    if (!c || alpha < 1 || alpha > 8) return DHTGPU_EINVAL;
    c->search_alpha = alpha;
    return DHTGPU_OK;
}

int dhtgpu_search_batch_dev(dhtgpu_ctx* c, const uint32_t* tp, uint64_t ts, uint32_t q, const uint32_t* searchers,
                            uint32_t max_rounds, uint32_t* out_idx, uint8_t* out_flags, uint32_t* out_len,
                            uint32_t* out_rounds, uint32_t* out_queries, void* stream) {
    if (!c || (q && (!tp || !searchers || !out_idx || !out_flags || !out_len || !out_rounds || !out_queries)))
        return DHTGPU_EINVAL;
    if (!c->net_valid || !c->index_valid) return DHTGPU_ENOIDS;
    if (!q) return DHTGPU_OK;
    DHT_TRY(c->bind());
    DHT_TRY(launch_search(c->planes.as<uint32_t>(), c->stride, c->net_sorted.as<uint2>(), c->index.p, c->n,
                          c->index_B, c->net_has_dead ? c->net_dead.as<uint8_t>() : nullptr, c->net_seed, tp, ts, q,
                          searchers, max_rounds, c->search_alpha, out_idx, out_flags, out_len, out_rounds, out_queries,
                          c->stream_or(stream)));
    return DHTGPU_OK;
}

int dhtgpu_search_batch(dhtgpu_ctx* c, const uint8_t* t20, uint32_t q, const uint32_t* searchers, uint32_t max_rounds,
                        uint32_t* out_idx, uint8_t* out_flags, uint32_t* out_len, uint32_t* out_rounds,
                        uint32_t* out_queries) {
    if (!c || (q && (!t20 || !searchers || !out_idx || !out_flags || !out_len || !out_rounds || !out_queries)))
        return DHTGPU_EINVAL;
    if (!c->net_valid) return DHTGPU_ENOIDS;
    if (!q) return DHTGPU_OK;
    for (uint32_t i = 0; i < q; ++i)
        if (searchers[i] >= c->n) return DHTGPU_EINVAL;
    DHT_TRY(c->bind());
    const size_t L = search_list_cap();
    const size_t sz[] = {(size_t)q * 4, (size_t)q * L * 4, (size_t)q * L, (size_t)q * 4, (size_t)q * 4, (size_t)q * 4};
    uint8_t* p[6];
    DHT_TRY(carve(c->net_io, sz, p));
    uint64_t ts = 0;
    DHT_TRY(c->upload_targets(t20, q, &ts));
    DHT_TRY(hipMemcpyAsync(p[0], searchers, sz[0], hipMemcpyHostToDevice, c->stream));
    int r = dhtgpu_search_batch_dev(c, c->targets.as<uint32_t>(), ts, q, (const uint32_t*)p[0], max_rounds,
                                    (uint32_t*)p[1], p[2], (uint32_t*)p[3], (uint32_t*)p[4], (uint32_t*)p[5], c->stream);
    if (r) return r;
    DHT_TRY(hipMemcpyAsync(out_idx, p[1], sz[1], hipMemcpyDeviceToHost, c->stream));
    DHT_TRY(hipMemcpyAsync(out_flags, p[2], sz[2], hipMemcpyDeviceToHost, c->stream));
    DHT_TRY(hipMemcpyAsync(out_len, p[3], sz[3], hipMemcpyDeviceToHost, c->stream));
    DHT_TRY(hipMemcpyAsync(out_rounds, p[4], sz[4], hipMemcpyDeviceToHost, c->stream));
    DHT_TRY(hipMemcpyAsync(out_queries, p[5], sz[5], hipMemcpyDeviceToHost, c->stream));
    DHT_TRY(hipStreamSynchronize(c->stream));
    return DHTGPU_OK;
}

}  // extern "C"
