// api.hip -- the libdhtgpu C ABI (include/dhtgpu.h), first of its host units: the
// lifecycle and id-set calls, the accept mask, K1 and K4, and the one definition of every helper
// that api_ctx.h declares.  Like every api unit it converts between the boundary's 20-byte
// big-endian ids and the device word-plane layout, checks arguments, sizes workspaces and issues
// the launch wrappers of dhtgpu_internal.h; launches no kernel itself and never throws across the ABI.
#include "api_ctx.h"

namespace dhtgpu::host {

int map_err(hipError_t e) {
    if (e == hipSuccess) return DHTGPU_OK;
    if (e == hipErrorOutOfMemory || e == hipErrorMemoryAllocation) return DHTGPU_ENOMEM;
    return DHTGPU_EDEVICE;
}

bool verbose() {
    static const bool v = getenv("DHTGPU_VERBOSE") != nullptr;
    return v;
}

std::vector<uint32_t> firsts_planes(const uint8_t* firsts20, uint32_t nb) {
    std::vector<uint32_t> fp((size_t)5 * nb);
    for (uint32_t b = 0; b < nb; ++b)
        for (int w = 0; w < 5; ++w) fp[(size_t)w * nb + b] = be32(firsts20 + 20 * (size_t)b + 4 * w);
    return fp;
}

// an all-rejected mask: every row empty (stream-ordered)
int answer_empty(uint32_t q, uint32_t k, uint32_t* out_idx, uint32_t* out_cnt, uint32_t* out_rec, hipStream_t s) {
    if (out_idx) DHT_TRY(launch_fill(out_idx, (uint64_t)q * k, DHTGPU_NONE, s));
    if (out_cnt) DHT_TRY(launch_fill(out_cnt, q, 0u, s));
    if (out_rec) DHT_TRY(launch_fill(out_rec, (uint64_t)q * k * 3, DHTGPU_NONE, s));
    return DHTGPU_OK;
}

// ---- sequences shared by several entry points -----------------------------------------------
// n 20-byte ids (host) into the word planes at dst (stride), 2^22 ids (80 MB) of staging at a time.
int upload_ids(dhtgpu_ctx* c, const uint8_t* ids20, uint64_t n, uint32_t* dst, uint64_t stride) {
    const uint64_t chunk = 1ull << 22;
    DHT_TRY(c->staging.ensure((size_t)std::min<uint64_t>(n ? n : 1, chunk) * 20));
    for (uint64_t i = 0; i < n; i += chunk) {
        const uint64_t m = std::min(chunk, n - i);
        DHT_TRY(hipMemcpyAsync(c->staging.p, ids20 + i * 20, (size_t)m * 20, hipMemcpyHostToDevice, c->stream));
        DHT_TRY(launch_pack(c->staging.as<uint8_t>(), m, dst + i, stride, c->stream));
        DHT_TRY(hipStreamSynchronize(c->stream));   // staging is reused
    }
    return DHTGPU_OK;
}

// An indexed update's arguments: m indices and m bytes (host) laid into buf and copied in on the
// context's stream; d_idx / d_val = where they are.  The caller owns buf and the synchronisation.
int stage_idx_val(dhtgpu_ctx* c, DevBuf& buf, const uint32_t* idx, const uint8_t* val, uint64_t m,
                  const uint32_t** d_idx, const uint8_t** d_val) {
    const size_t sz[] = {(size_t)m * 4, (size_t)m};
    uint8_t* p[2];
    DHT_TRY(carve(buf, sz, p));
    DHT_TRY(hipMemcpyAsync(p[0], idx, sz[0], hipMemcpyHostToDevice, c->stream));
    DHT_TRY(hipMemcpyAsync(p[1], val, sz[1], hipMemcpyHostToDevice, c->stream));
    *d_idx = reinterpret_cast<const uint32_t*>(p[0]);
    *d_val = p[1];
    return DHTGPU_OK;
}

// A by-handle array grown to hold `need` bytes: geometrically from `floor`, bounded by `most`; its
// first `live` bytes kept and the rest 0, on the context's stream.  The buffer it replaces is parked
// in `old` until the next growth, for calls in flight on other streams.
int grow_kept(dhtgpu_ctx* c, DevBuf& cur, DevBuf& old, size_t live, size_t need, size_t floor, size_t most) {
    if (need <= cur.cap) return DHTGPU_OK;
    const size_t cap = std::min(std::max(need, std::max(2 * cur.cap, floor)), most);
    DevBuf nb;
    DHT_TRY(nb.ensure(cap));
    if (live) DHT_TRY(hipMemcpyAsync(nb.p, cur.p, live, hipMemcpyDeviceToDevice, c->stream));
    DHT_TRY(hipMemsetAsync(nb.as<uint8_t>() + live, 0, cap - live, c->stream));
    old = std::move(cur);   // (old's previous buffer goes with nb)
    cur = std::move(nb);
    return DHTGPU_OK;
}

// Where a call's local index rows go: the caller's rows, or -- record form, where the records are
// made from the rows -- scratch rows of their own.
int local_rows(uint32_t* out_rec, DevBuf& idx, DevBuf& cnt, uint32_t q, uint32_t k, uint32_t** li, uint32_t** lc) {
    if (!out_rec) return DHTGPU_OK;
    DHT_TRY(idx.ensure((size_t)q * k * 4));
    DHT_TRY(cnt.ensure((size_t)q * 4));
    *li = idx.as<uint32_t>();
    *lc = cnt.as<uint32_t>();
    return DHTGPU_OK;
}

// Argument checks of the top-k calls: the _dev forms (index rows or records) and the host forms.
int check_topk_dev(const dhtgpu_ctx* c, const uint32_t* tp, uint32_t q, uint32_t k, const uint32_t* out_idx,
                   const uint32_t* out_cnt, const uint32_t* out_rec) {
    if (!c || k == 0 || k > DHTGPU_MAX_K || (q && !tp)) return DHTGPU_EINVAL;
    if (!out_rec && (!out_idx || !out_cnt)) return DHTGPU_EINVAL;
    if (!c->has_ids) return DHTGPU_ENOIDS;
    return DHTGPU_OK;
}

// The idx_base rule of include/dhtgpu.h: every index idx_base + i, i < n, is a uint32 below
// DHTGPU_NONE.  n is the context's id count (the index space), whatever an accept mask hides.
int check_idx_base(const dhtgpu_ctx* c, uint32_t idx_base) {
    return (uint64_t)idx_base + c->n > 0xFFFFFFFFull ? DHTGPU_ERANGE : DHTGPU_OK;
}

int check_topk_host(const dhtgpu_ctx* c, const uint8_t* t20, uint32_t q, uint32_t k, const uint32_t* out_idx,
                    const uint32_t* out_cnt) {
    if (!c || k == 0 || k > DHTGPU_MAX_K || (q && (!t20 || !out_idx || !out_cnt))) return DHTGPU_EINVAL;
    if (!c->has_ids) return DHTGPU_ENOIDS;
    return DHTGPU_OK;
}

// K1 over an active set (checked arguments, q > 0)
int topk_on(dhtgpu_ctx* c, const dhtgpu_ctx::ActiveSet& A, const uint32_t* tp, uint64_t ts, uint32_t q, uint32_t k,
            uint32_t* out_idx, uint32_t* out_cnt, uint32_t* out_rec, uint32_t idx_base, hipStream_t s) {
    if (A.view && !A.n) return answer_empty(q, k, out_idx, out_cnt, out_rec, s);
    const ScanPlan p = plan_scan(A.n, q, k, c->num_cus);
    const uint32_t* gidx = A.map;
    const bool one = p.splits == 1 || A.n == 0;
    if (one && !out_rec) {   // one pass writes the final form directly
        DHT_TRY(launch_scan(A.planes, A.stride, A.n, p, tp, ts, q, k, out_idx, out_cnt, out_rec, gidx, idx_base, s));
        return DHTGPU_OK;
    }
    // local indices (merged over id-range splits when the batch is too small to fill the
    // chip), then turned into candidate records or mapped to the final form
    uint32_t *li = out_idx, *lc = out_cnt;
    if (int r = local_rows(out_rec, c->out_idx, c->out_cnt, q, k, &li, &lc)) return r;
    if (one) {
        DHT_TRY(launch_scan(A.planes, A.stride, A.n, p, tp, ts, q, k, li, lc, nullptr, nullptr, 0, s));
    } else {
        DHT_TRY(c->rec.ensure((size_t)p.splits * q * k * 6 * 4));
        DHT_TRY(launch_scan(A.planes, A.stride, A.n, p, tp, ts, q, k, nullptr, nullptr, c->rec.as<uint32_t>(), nullptr, 0,
                            s));
        DHT_TRY(launch_merge(c->rec.as<uint32_t>(), p.splits, q, k, tp, ts, k, li, lc, s));
    }
    if (out_rec)
        DHT_TRY(launch_rec3(li, (uint64_t)q * k, A.planes, A.stride, idx_base, gidx, out_rec, s));
    else
        DHT_TRY(launch_map_idx(li, (uint64_t)q * k, gidx, idx_base, s));
    return DHTGPU_OK;
}

// the K4 index over an active set (the id set's own index, or the view's)
int index_build_on(const dhtgpu_ctx::ActiveSet& A, hipStream_t s, hipEvent_t* ev) {
    const uint32_t B = index_bits(A.n);
    *A.index_valid = false;
    DHT_TRY(A.index->ensure(index_bytes(A.n, B)));
    DHT_TRY(launch_index_build(A.planes, A.stride, A.n, B, A.index->p, s, ev));
    *A.index_B = B;
    *A.index_valid = true;
    return DHTGPU_OK;
}

}  // namespace dhtgpu::host

// Rebuild the accept mask's view when its bits (or the ids under it) changed: count (V1 + V2, one
// host sync for the total, which sizes every view buffer), then the compaction (V3).  The view
// meets what the kernels assume of an id set: stride pad_ids(n), zeroed padding, w0s of the full
// stride.  A mask that accepts every id builds no view.  Everything derived from the previous view
// (sub-partitions, the view's index, the fallback hint, the idx_base map) is dropped.
static int ensure_view(dhtgpu_ctx* c) {
    dhtgpu_ctx::Accept& a = c->acc;
    if (!a.has_mask || !a.stale) return DHTGPU_OK;
    hipStream_t s = c->stream;
    if (a.bits_stream && a.bits_stream != s) DHT_TRY(hipStreamSynchronize(a.bits_stream));
    a.bits_stream = nullptr;
    const uint64_t ntiles = c->stride / kTile;
    DHT_TRY(a.toff.ensure((size_t)(ntiles + 4) * 4 + 16));
    unsigned long long* d_total = a.toff.as<unsigned long long>();
    uint32_t* toff = a.toff.as<uint32_t>() + 4;
    DHT_TRY(launch_view_count(a.bits.as<uint32_t>(), c->stride, toff, d_total, s));
    unsigned long long m = 0;
    DHT_TRY(hipMemcpyAsync(&m, d_total, 8, hipMemcpyDeviceToHost, s));
    DHT_TRY(hipStreamSynchronize(s));
    const bool was = a.active;
    a.active = false;   // (until the new view stands)
    a.bmap_valid = false;
    a.index_valid = false;
    if (was || m < c->n) c->invalidate_subs();
    if (m > c->n) return DHTGPU_EDEVICE;   // (bits past n are cleared by every setter)
    a.n = m;
    if (m < c->n) {
        a.stride = pad_ids(m ? m : 1);
        const bool shard = c->shard_pbits != 0, glob = c->has_gidx;
        DHT_TRY(a.planes.ensure((size_t)a.stride * 5 * 4));
        DHT_TRY(a.map.ensure((size_t)a.stride * 4));
        if (shard) DHT_TRY(a.w0s.ensure((size_t)a.stride * 4));
        if (glob) DHT_TRY(a.gmap.ensure((size_t)a.stride * 4));
        for (int w = 0; w < 5; ++w)
            DHT_TRY(launch_fill(a.planes.as<uint32_t>() + (uint64_t)w * a.stride + m, a.stride - m, 0u, s));
        if (shard) DHT_TRY(launch_fill(a.w0s.as<uint32_t>() + m, a.stride - m, 0u, s));
        if (m)
            DHT_TRY(launch_view_compact(c->planes.as<uint32_t>(), c->stride, a.bits.as<uint32_t>(), toff,
                                        a.planes.as<uint32_t>(), a.stride, a.map.as<uint32_t>(),
                                        shard ? a.w0s.as<uint32_t>() : nullptr, c->shard_pbits,
                                        glob ? c->gidx.as<uint32_t>() : nullptr, glob ? a.gmap.as<uint32_t>() : nullptr, s));
        DHT_TRY(hipStreamSynchronize(s));   // calls on other streams read the view
        a.active = true;
    }
    a.stale = false;
    return DHTGPU_OK;
}

int dhtgpu_ctx::active_set(uint32_t idx_base, ActiveSet* out) {
    int r = ensure_view(this);
    if (r) return r;
    if (!acc.active) {
        *out = full_set();
        return DHTGPU_OK;
    }
    const uint32_t* m = acc.map.as<uint32_t>();
    if (has_gidx && map_global) {
        m = acc.gmap.as<uint32_t>();
    } else if (idx_base) {   // a map and an offset at once: map + idx_base, cached per base
        if (!acc.bmap_valid || acc.bmap_base != idx_base) {
            acc.bmap_valid = false;
            DHT_TRY(acc.bmap.ensure((size_t)acc.stride * 4));
            DHT_TRY(launch_view_add(acc.map.as<uint32_t>(), acc.n, idx_base, acc.bmap.as<uint32_t>(), stream));
            DHT_TRY(hipStreamSynchronize(stream));   // read by calls on any stream
            acc.bmap_base = idx_base;
            acc.bmap_valid = true;
        }
        m = acc.bmap.as<uint32_t>();
    }
    *out = ActiveSet{acc.planes.as<uint32_t>(), acc.stride, acc.n, m, shard_pbits ? acc.w0s.as<uint32_t>() : nullptr,
                     shard_pbits, shard_pval, true, &acc.index, &acc.index_B, &acc.index_valid};
    return DHTGPU_OK;
}

static int finish_ids(dhtgpu_ctx* c, uint64_t n) {
    // zero the padding so tile streaming reads deterministic words
    const uint64_t s = c->stride;
    for (int w = 0; w < 5; ++w)
        DHT_TRY(launch_fill(c->planes.as<uint32_t>() + (uint64_t)w * s + n, s - n, 0u, c->stream));
    DHT_TRY(c->aux.ensure(16));
    DHT_TRY(hipMemsetAsync(c->aux.p, 0, 4, c->stream));
    DHT_TRY(launch_check_sorted(c->planes.as<uint32_t>(), s, n, c->aux.as<uint32_t>(), c->stream));
    uint32_t flag = 0;
    DHT_TRY(hipMemcpyAsync(&flag, c->aux.p, 4, hipMemcpyDeviceToHost, c->stream));
    DHT_TRY(hipStreamSynchronize(c->stream));
    c->n = n;
    c->sorted = flag == 0;
    c->has_ids = true;
    return DHTGPU_OK;
}

static int alloc_ids(dhtgpu_ctx* c, uint64_t n) {
    if (n >= 0xFFFFFFFFull) return DHTGPU_ERANGE;
    c->has_ids = false;
    c->index_valid = false;
    c->net_valid = false;
    c->shard_pbits = 0;
    c->shard_pval = 0;
    c->has_gidx = false;
    c->clear_accept();   // a new id set: every id accepted
    c->invalidate_subs();
    c->sview.valid = false;
    c->stride = pad_ids(n ? n : 1);
    DHT_TRY(c->planes.ensure((size_t)c->stride * 5 * 4));
    return DHTGPU_OK;
}

// the mask buffer at the size the view kernels read unchecked, all zero
static int mask_alloc(dhtgpu_ctx* c, hipStream_t s) {
    const size_t bytes = (size_t)view_mask_words(c->stride) * 4;
    DHT_TRY(c->acc.bits.ensure(bytes));
    DHT_TRY(hipMemsetAsync(c->acc.bits.p, 0, bytes, s));
    return DHTGPU_OK;
}

extern "C" {

const char* dhtgpu_strerror(int code) {
    switch (code) {
        case DHTGPU_OK: return "ok";
        case DHTGPU_EINVAL: return "invalid argument";
        case DHTGPU_ENOMEM: return "device out of memory";
        case DHTGPU_EDEVICE: return "HIP device or kernel error";
        case DHTGPU_ENOIDS: return "no id set uploaded";
        case DHTGPU_EUNSORTED: return "id set holds duplicate ids (NodeCache keys are unique)";
        case DHTGPU_ERANGE: return "size out of range";
        default: return "unknown error";
    }
}

int dhtgpu_device_count(int* out) {
    if (!out) return DHTGPU_EINVAL;
    *out = 0;
    DHT_TRY(hipGetDeviceCount(out));
    return DHTGPU_OK;
}

int dhtgpu_ctx_create(int device, dhtgpu_ctx** out) {
    if (!out) return DHTGPU_EINVAL;
    *out = nullptr;
    int nd = 0;
    DHT_TRY(hipGetDeviceCount(&nd));
    if (device < 0 || device >= nd) return DHTGPU_EINVAL;
    auto* c = new (std::nothrow) dhtgpu_ctx;
    if (!c) return DHTGPU_ENOMEM;
    c->device = device;
    hipError_t e = c->bind();
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&c->stream.h, hipStreamNonBlocking);
    if (const char* d = getenv("DHTGPU_DBG")) c->dbg = (uint32_t)strtoul(d, nullptr, 0) & kDbgAllowed;
    if (e == hipSuccess) {
        hipDeviceProp_t prop;
        if (hipGetDeviceProperties(&prop, device) == hipSuccess) c->num_cus = prop.multiProcessorCount;
    }
    if (e == hipSuccess) {   // F4's fallback-list hint: mapped, coherent host memory (F4 stores it system-scope)
        void* h = nullptr;
        e = hipHostMalloc(&h, 64, hipHostMallocMapped | hipHostMallocCoherent);
        if (e == hipSuccess) {
            c->fb_hint.host = static_cast<uint32_t*>(h);
            *c->fb_hint.host = 1u;   // unknown: assume a fallback list (full-size grid)
            void* d = nullptr;
            e = hipHostGetDevicePointer(&d, h, 0);
            c->fb_hint.dev = static_cast<uint32_t*>(d);
        }
    }
    if (e != hipSuccess) {
        dhtgpu_ctx_destroy(c);
        return map_err(e);
    }
    *out = c;
    return DHTGPU_OK;
}

void dhtgpu_ctx_destroy(dhtgpu_ctx* c) {
    if (!c) return;
    (void)c->bind();
    delete c;
}

void* dhtgpu_ctx_stream(dhtgpu_ctx* c) { return c ? (void*)c->stream.h : nullptr; }

uint64_t dhtgpu_num_ids(const dhtgpu_ctx* c) { return c && c->has_ids ? c->n : 0; }

int dhtgpu_set_ids(dhtgpu_ctx* c, const uint8_t* ids20, uint64_t n) {
    if (!c || (!ids20 && n)) return DHTGPU_EINVAL;
    DHT_TRY(c->bind());
    int r = alloc_ids(c, n);
    if (r) return r;
    if ((r = upload_ids(c, ids20, n, c->planes.as<uint32_t>(), c->stride))) return r;
    return finish_ids(c, n);
}

int dhtgpu_gen_ids(dhtgpu_ctx* c, uint64_t seed, uint64_t start, uint64_t n) {
    if (!c) return DHTGPU_EINVAL;
    DHT_TRY(c->bind());
    int r = alloc_ids(c, n);
    if (r) return r;
    DHT_TRY(launch_gen(seed, start, n, c->planes.as<uint32_t>(), c->stride, c->stream));
    return finish_ids(c, n);
}

int dhtgpu_gen_ids_prefix(dhtgpu_ctx* c, uint64_t seed, uint64_t start, uint64_t n, uint32_t pbits,
                          uint32_t pval) {
    if (!c || pbits > 16 || (pbits < 32 && pval >= (1u << pbits))) return DHTGPU_EINVAL;
    if (n >= 0xFFFFFFFFull || start + n > 0xFFFFFFFFull) return DHTGPU_ERANGE;
    DHT_TRY(c->bind());
    // the whole stream is generated into scratch, then the shard is compacted in order
    const uint64_t gs = pad_ids(n ? n : 1);
    DHT_TRY(c->staging.ensure((size_t)gs * 5 * 4));
    uint32_t* gen = c->staging.as<uint32_t>();
    DHT_TRY(launch_gen(seed, start, n, gen, gs, c->stream));
    PrefixSelect sel{gen, gs, n, pbits, pval, c->stream};
    unsigned long long m = 0;
    int r = sel.count(c, &m);
    if (r) return r;
    if ((r = alloc_ids(c, m))) return r;
    DHT_TRY(c->gidx.ensure((size_t)(m ? m : 1) * 4));
    DHT_TRY(sel.compact(c->planes.as<uint32_t>(), c->stride, c->gidx.as<uint32_t>(), start));
    r = finish_ids(c, m);
    if (r) return r;
    // the generation scratch (20 B per id of the whole stream) is not kept: a device may
    // hold several shard contexts of one large stream
    DHT_TRY(hipStreamSynchronize(c->stream));
    if (c->staging.cap > ((size_t)1 << 28)) c->staging.release();
    if (c->aux.cap > ((size_t)1 << 28)) c->aux.release();
    c->has_gidx = true;
    if (pbits) {
        DHT_TRY(c->w0s.ensure((size_t)c->stride * 4));
        DHT_TRY(launch_shift_w0(c->planes.as<uint32_t>(), c->stride, pbits, c->w0s.as<uint32_t>(), c->stream));
        c->shard_pbits = pbits;
        c->shard_pval = pval;
    }
    return DHTGPU_OK;
}

int dhtgpu_set_global_indices(dhtgpu_ctx* c, int on) {
    if (!c) return DHTGPU_EINVAL;
    c->map_global = on != 0;
    return DHTGPU_OK;
}

// measurement only (not in include/): the phase-stamp buffer of DHTGPU_DBG=256 runs
int dhtgpu_debug_stamps(dhtgpu_ctx* c, void** dev_ptr, uint64_t* bytes) {
    if (!c || !dev_ptr || !bytes) return DHTGPU_EINVAL;
    *dev_ptr = c->stamps.p;
    *bytes = c->stamps.cap;
    return 0;
}

// ---- accept mask ----------------------------------------------------------------------------
int dhtgpu_set_accept(dhtgpu_ctx* c, const uint8_t* accept) {
    if (!c) return DHTGPU_EINVAL;
    if (!c->has_ids) return DHTGPU_ENOIDS;
    DHT_TRY(c->bind());
    if (!accept) {   // every id accepted again: the view and what was built from it go
        DHT_TRY(hipStreamSynchronize(c->stream));
        c->clear_accept();
        return DHTGPU_OK;
    }
    hipStream_t s = c->stream;
    int r = mask_alloc(c, s);
    if (r) return r;
    // bytes -> bits on the device, 2^22 ids of staging at a time (whole mask words per chunk)
    const uint64_t chunk = 1ull << 22;
    DHT_TRY(c->staging.ensure((size_t)std::min<uint64_t>(c->stride, chunk)));
    for (uint64_t i = 0; i < c->n; i += chunk) {
        const uint64_t m = std::min(chunk, c->n - i), words = (m + 31) / 32;
        if (m < words * 32) DHT_TRY(hipMemsetAsync(c->staging.as<uint8_t>() + m, 0, (size_t)(words * 32 - m), s));
        DHT_TRY(hipMemcpyAsync(c->staging.p, accept + i, (size_t)m, hipMemcpyHostToDevice, s));
        DHT_TRY(launch_view_pack(c->staging.as<uint8_t>(), words, c->acc.bits.as<uint32_t>() + i / 32, s));
        DHT_TRY(hipStreamSynchronize(s));   // staging is reused; accept[] is the caller's again
    }
    c->acc.bits_stream = nullptr;
    c->acc.has_mask = true;
    c->acc.stale = true;
    return DHTGPU_OK;
}

int dhtgpu_set_accept_bits_dev(dhtgpu_ctx* c, const uint32_t* bits, void* stream) {
    if (!c || !bits) return DHTGPU_EINVAL;
    if (!c->has_ids) return DHTGPU_ENOIDS;
    DHT_TRY(c->bind());
    hipStream_t s = c->stream_or(stream);
    int r = mask_alloc(c, s);
    if (r) return r;
    DHT_TRY(hipMemcpyAsync(c->acc.bits.p, bits, (size_t)((c->n + 31) / 32) * 4, hipMemcpyDeviceToDevice, s));
    DHT_TRY(launch_view_trim(c->acc.bits.as<uint32_t>(), c->n, s));
    c->acc.bits_stream = s;   // the rebuild waits for this copy
    c->acc.has_mask = true;
    c->acc.stale = true;
    return DHTGPU_OK;
}

int dhtgpu_update_accept(dhtgpu_ctx* c, const uint32_t* idx, const uint8_t* val, uint64_t m) {
    if (!c || (m && (!idx || !val))) return DHTGPU_EINVAL;
    if (!c->has_ids) return DHTGPU_ENOIDS;
    for (uint64_t j = 0; j < m; ++j)
        if (idx[j] >= c->n) return DHTGPU_EINVAL;   // nothing applied
    if (!m) return DHTGPU_OK;
    DHT_TRY(c->bind());
    hipStream_t s = c->stream;
    if (c->acc.bits_stream && c->acc.bits_stream != s) DHT_TRY(hipStreamSynchronize(c->acc.bits_stream));
    c->acc.bits_stream = nullptr;
    if (!c->acc.has_mask) {   // no mask yet: start from every id accepted
        int r = mask_alloc(c, s);
        if (r) return r;
        DHT_TRY(launch_fill(c->acc.bits.as<uint32_t>(), (c->n + 31) / 32, 0xFFFFFFFFu, s));
        DHT_TRY(launch_view_trim(c->acc.bits.as<uint32_t>(), c->n, s));
    }
    const uint32_t* d_idx;
    const uint8_t* d_val;
    if (int r = stage_idx_val(c, c->staging, idx, val, m, &d_idx, &d_val)) return r;
    DHT_TRY(launch_bits_update(c->acc.bits.as<uint32_t>(), d_idx, d_val, m, s));
    DHT_TRY(hipStreamSynchronize(s));   // idx / val are the caller's again
    c->acc.has_mask = true;
    c->acc.stale = true;
    return DHTGPU_OK;
}

int dhtgpu_num_accepted(dhtgpu_ctx* c, uint64_t* out) {
    if (!c || !out) return DHTGPU_EINVAL;
    if (!c->has_ids) return DHTGPU_ENOIDS;
    DHT_TRY(c->bind());
    int r = ensure_view(c);
    if (r) return r;
    *out = c->acc.active ? c->acc.n : c->n;
    return DHTGPU_OK;
}

int dhtgpu_write_ids(dhtgpu_ctx* c, uint64_t first, const uint8_t* ids20, uint64_t m) {
    if (!c || (!ids20 && m)) return DHTGPU_EINVAL;
    if (!c->has_ids) return DHTGPU_ENOIDS;
    if (c->has_gidx) return DHTGPU_EINVAL;   // a prefix shard's ids share its prefix
    if (first > c->n || m > c->n - first) return DHTGPU_ERANGE;
    if (!m) return DHTGPU_OK;
    DHT_TRY(c->bind());
    // everything derived from the ids goes: the lexicographic view, both K4 indices, the
    // sub-partitions, the crawl model and the mask's view (the mask itself stays)
    c->sview.valid = false;
    c->index_valid = false;
    c->acc.index_valid = false;
    c->net_valid = false;
    c->invalidate_subs();
    if (c->acc.has_mask) c->acc.stale = true;
    if (int r = upload_ids(c, ids20, m, c->planes.as<uint32_t>() + first, c->stride)) return r;
    return finish_ids(c, c->n);   // (padding untouched) the sorted / unique flag again
}

int dhtgpu_select_prefix_dev(dhtgpu_ctx* c, const uint32_t* planes, uint64_t stride, uint64_t n, uint32_t pbits,
                             uint32_t pval, uint32_t* out_planes, uint64_t out_stride, uint32_t* out_gidx,
                             uint64_t* out_count, void* stream) {
    if (!c || !out_count || pbits > 16 || (pbits < 32 && pval >= (1u << pbits))) return DHTGPU_EINVAL;
    if (n && (!planes || !out_planes)) return DHTGPU_EINVAL;
    DHT_TRY(c->bind());
    hipStream_t s = c->stream_or(stream);
    PrefixSelect sel{planes, stride, n, pbits, pval, s};
    unsigned long long m = 0;
    if (int r = sel.count(c, &m)) return r;
    if (m > out_stride) return DHTGPU_ERANGE;
    DHT_TRY(sel.compact(out_planes, out_stride, out_gidx, 0));
    DHT_TRY(hipStreamSynchronize(s));
    *out_count = m;
    return DHTGPU_OK;
}

int dhtgpu_get_ids(dhtgpu_ctx* c, uint64_t first, uint64_t n, uint8_t* out20) {
    if (!c || (!out20 && n)) return DHTGPU_EINVAL;
    if (!c->has_ids) return DHTGPU_ENOIDS;
    if (first > c->n || n > c->n - first) return DHTGPU_ERANGE;
    if (!n) return DHTGPU_OK;
    DHT_TRY(c->bind());
    DHT_TRY(c->staging.ensure((size_t)n * 20));
    DHT_TRY(launch_unpack(c->planes.as<uint32_t>(), c->stride, first, n, c->staging.as<uint8_t>(), c->stream));
    DHT_TRY(hipMemcpyAsync(out20, c->staging.p, (size_t)n * 20, hipMemcpyDeviceToHost, c->stream));
    DHT_TRY(hipStreamSynchronize(c->stream));
    return DHTGPU_OK;
}

int dhtgpu_ids_dev(dhtgpu_ctx* c, const uint32_t** planes, uint64_t* stride) {
    if (!c || !planes || !stride) return DHTGPU_EINVAL;
    if (!c->has_ids) return DHTGPU_ENOIDS;
    *planes = c->planes.as<uint32_t>();
    *stride = c->stride;
    return DHTGPU_OK;
}

// ---- K1 -------------------------------------------------------------------------------------
int dhtgpu_topk_dev(dhtgpu_ctx* c, const uint32_t* tp, uint64_t ts, uint32_t q, uint32_t k,
                    uint32_t* out_idx, uint32_t* out_cnt, uint32_t* out_rec, uint32_t idx_base,
                    void* stream) {
    if (int r = check_topk_dev(c, tp, q, k, out_idx, out_cnt, out_rec)) return r;
    if (int r = check_idx_base(c, idx_base)) return r;
    if (!q) return DHTGPU_OK;
    DHT_TRY(c->bind());
    dhtgpu_ctx::ActiveSet A;
    if (int r = c->active_set(idx_base, &A)) return r;
    return topk_on(c, A, tp, ts, q, k, out_idx, out_cnt, out_rec, idx_base, c->stream_or(stream));
}

int dhtgpu_merge_dev(const uint32_t* rec, uint32_t lists, uint32_t q, uint32_t k_in,
                     const uint32_t* tp, uint64_t ts, uint32_t k, uint32_t* out_idx,
                     uint32_t* out_cnt, uint32_t* ties, uint32_t tie_cap, void* stream) {
    if (!rec || !tp || !out_idx || !out_cnt || k == 0 || k > DHTGPU_MAX_K || lists == 0 || k_in == 0 ||
        k_in > DHTGPU_MAX_K)
        return DHTGPU_EINVAL;
    if (lists > DHTGPU_MAX_LISTS) return DHTGPU_ERANGE;
    if (lists > 1 && !ties) return DHTGPU_EINVAL;   // cross-list ties must be listed
    if (!q) return DHTGPU_OK;
    DHT_TRY(launch_merge3(rec, lists, q, k_in, tp, ts, k, out_idx, out_cnt, ties, tie_cap, (hipStream_t)stream));
    return DHTGPU_OK;
}

int dhtgpu_tie_words_dev(dhtgpu_ctx* c, const uint32_t* rec, uint32_t q, uint32_t k, uint32_t idx_base,
                         const uint32_t* ties, uint32_t tie_cap, uint32_t row_base, uint32_t* out_words,
                         void* stream) {
    if (!c || !rec || !out_words || k == 0 || k > DHTGPU_MAX_K) return DHTGPU_EINVAL;
    if (!c->has_ids) return DHTGPU_ENOIDS;
    if (int r = check_idx_base(c, idx_base)) return r;
    if (!q) return DHTGPU_OK;
    DHT_TRY(c->bind());
    hipStream_t s = c->stream_or(stream);
    // records name ids by global index: the prefix shard's ascending map, else idx_base + local
    const uint32_t* gmap = c->out_map();
    DHT_TRY(launch_tie_words(rec, q, k, ties, tie_cap, row_base, c->planes.as<uint32_t>(), c->stride, c->n, gmap,
                             gmap ? 0u : idx_base, out_words, s));
    return DHTGPU_OK;
}

int dhtgpu_merge_ties_dev(const uint32_t* rec, const uint32_t* words, uint32_t lists, uint32_t q, uint32_t k_in,
                          const uint32_t* tp, uint64_t ts, uint32_t k, const uint32_t* ties, uint32_t tie_cap,
                          uint32_t* out_idx, uint32_t* out_cnt, void* stream) {
    if (!rec || !words || !tp || !out_idx || !out_cnt || k == 0 || k > DHTGPU_MAX_K || lists == 0 || k_in == 0 ||
        k_in > DHTGPU_MAX_K)
        return DHTGPU_EINVAL;
    if (lists > DHTGPU_MAX_LISTS) return DHTGPU_ERANGE;
    if (!q || (ties && !tie_cap)) return DHTGPU_OK;
    DHT_TRY(launch_merge_full(rec, words, lists, q, k_in, tp, ts, k, ties, tie_cap, out_idx, out_cnt,
                              (hipStream_t)stream));
    return DHTGPU_OK;
}

int dhtgpu_pack_dev(const uint8_t* ids20, uint64_t n, uint32_t* planes, uint64_t stride, void* stream) {
    if ((!ids20 || !planes) && n) return DHTGPU_EINVAL;
    if (stride < n) return DHTGPU_EINVAL;
    DHT_TRY(launch_pack(ids20, n, planes, stride, (hipStream_t)stream));
    return DHTGPU_OK;
}

int dhtgpu_gen_dev(uint64_t seed, uint64_t start, uint64_t n, uint32_t* planes, uint64_t stride,
                   void* stream) {
    if (!planes && n) return DHTGPU_EINVAL;
    if (stride < n) return DHTGPU_EINVAL;
    DHT_TRY(launch_gen(seed, start, n, planes, stride, (hipStream_t)stream));
    return DHTGPU_OK;
}

int dhtgpu_topk(dhtgpu_ctx* c, const uint8_t* t20, uint32_t q, uint32_t k, uint32_t* out_idx,
                uint32_t* out_cnt) {
    if (int r = check_topk_host(c, t20, q, k, out_idx, out_cnt)) return r;
    if (!q) return DHTGPU_OK;
    DHT_TRY(c->bind());
    return host_topk(c, t20, q, k, out_idx, out_cnt, [&](const uint32_t* tp, uint64_t ts, uint32_t* d_idx, uint32_t* d_cnt) {
        return dhtgpu_topk_dev(c, tp, ts, q, k, d_idx, d_cnt, nullptr, 0, c->stream);
    });
}

// ---- K4 -------------------------------------------------------------------------------------
int dhtgpu_index_build(dhtgpu_ctx* c, void* stream) {
    if (!c) return DHTGPU_EINVAL;
    if (!c->has_ids) return DHTGPU_ENOIDS;
    DHT_TRY(c->bind());
    hipStream_t s = c->stream_or(stream);
    dhtgpu_ctx::ActiveSet A;
    if (int r = c->active_set(0, &A)) return r;
    if (A.view && !A.n) return DHTGPU_OK;   // every id rejected: queries answer empty rows
    return index_build_on(A, s, nullptr);
}

int dhtgpu_index_build_timed(dhtgpu_ctx* c, void* stream, float* ms4) {
    if (!c || !ms4) return DHTGPU_EINVAL;
    if (!c->has_ids) return DHTGPU_ENOIDS;
    DHT_TRY(c->bind());
    hipStream_t s = c->stream_or(stream);
    dhtgpu_ctx::ActiveSet A;
    if (int r = c->active_set(0, &A)) return r;
    Events<5> ev;
    DHT_TRY(ev.create());
    if (int r = index_build_on(A, s, ev.ev)) return r;
    DHT_TRY(hipEventSynchronize(ev.ev[4]));
    for (int i = 0; i < 4; ++i) DHT_TRY(hipEventElapsedTime(&ms4[i], ev.ev[i], ev.ev[i + 1]));
    return DHTGPU_OK;
}

int dhtgpu_index_topk_dev(dhtgpu_ctx* c, const uint32_t* tp, uint64_t ts, uint32_t q, uint32_t k,
                          uint32_t* out_idx, uint32_t* out_cnt, uint32_t* out_rec, uint32_t idx_base,
                          void* stream) {
    if (int r = check_topk_dev(c, tp, q, k, out_idx, out_cnt, out_rec)) return r;
    if (int r = check_idx_base(c, idx_base)) return r;
    if (!c->acc.has_mask && !c->index_valid) return DHTGPU_ENOIDS;
    if (!q) return DHTGPU_OK;
    DHT_TRY(c->bind());
    hipStream_t s = c->stream_or(stream);
    dhtgpu_ctx::ActiveSet A;
    if (int r = c->active_set(idx_base, &A)) return r;
    if (A.view && !A.n) return answer_empty(q, k, out_idx, out_cnt, out_rec, s);
    if (!*A.index_valid) {   // under a mask the index is built by its first query (stream-ordered, on s)
        if (!c->acc.has_mask) return DHTGPU_ENOIDS;
        if (int r = index_build_on(A, s, nullptr)) return r;
    }
    const uint32_t* gidx = A.map;
    uint32_t *li = out_idx, *lc = out_cnt;   // (record form: candidate records for a cross-shard merge)
    if (int r = local_rows(out_rec, c->out_idx, c->out_cnt, q, k, &li, &lc)) return r;
    DHT_TRY(launch_index_query(A.index->p, A.n, *A.index_B, A.planes, A.stride, tp, ts, q, k, li, lc, s));
    if (out_rec)
        DHT_TRY(launch_rec3(li, (uint64_t)q * k, A.planes, A.stride, idx_base, gidx, out_rec, s));
    else
        DHT_TRY(launch_map_idx(li, (uint64_t)q * k, gidx, idx_base, s));
    return DHTGPU_OK;
}

int dhtgpu_index_topk(dhtgpu_ctx* c, const uint8_t* t20, uint32_t q, uint32_t k, uint32_t* out_idx,
                      uint32_t* out_cnt) {
    if (int r = check_topk_host(c, t20, q, k, out_idx, out_cnt)) return r;
    if (!q) return DHTGPU_OK;
    DHT_TRY(c->bind());
    if (!c->acc.has_mask && !c->index_valid) {   // (a view's index: built by the query below)
        int r = dhtgpu_index_build(c, c->stream);
        if (r) return r;
    }
    return host_topk(c, t20, q, k, out_idx, out_cnt, [&](const uint32_t* tp, uint64_t ts, uint32_t* d_idx, uint32_t* d_cnt) {
        return dhtgpu_index_topk_dev(c, tp, ts, q, k, d_idx, d_cnt, nullptr, 0, c->stream);
    });
}

}  // extern "C"
