// api.hip -- the libdhtgpu C ABI (include/dhtgpu.h): the host side of every dhtgpu_* entry
// point.  Converts between the boundary's 20-byte big-endian ids and the device word-plane
// layout, checks arguments, sizes workspaces and issues the launch wrappers of
// dhtgpu_internal.h; launches no kernel itself and never throws across the ABI.
// Ownership: a DevBuf frees its device memory when it is destroyed, and the context's stream
// and mapped hint are owners declared before every buffer, so deleting a dhtgpu_ctx releases
// everything in order and an early return leaks nothing.
// Layout: owners and the context; helpers shared by several entry points (each sequence stands
// once); then the entry points by family -- id set, accept mask, K1, K4, K6, table, caches,
// wire format, searches, the resident routing table, the resident NodeCache, the resident searches and their
// ordered map, crawl model.
#include <hip/hip_runtime.h>
#include <cstdio>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <new>
#include <utility>
#include <vector>

#include "../../include/dhtgpu.h"
#include "dhtgpu_internal.h"

using namespace dhtgpu;

namespace {

// Device memory, owned: freed on destruction, move-only.
struct DevBuf {
    void* p = nullptr;
    size_t cap = 0;
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    DevBuf(DevBuf&& o) noexcept { *this = std::move(o); }
    DevBuf& operator=(DevBuf&& o) noexcept {   // (what this held goes with o)
        std::swap(p, o.p);
        std::swap(cap, o.cap);
        return *this;
    }
    ~DevBuf() { release(); }
    hipError_t ensure(size_t bytes) {
        if (bytes <= cap) return hipSuccess;
        if (p) (void)hipFree(p);
        p = nullptr;
        cap = 0;
        hipError_t e = hipMalloc(&p, bytes ? bytes : 16);
        if (e == hipSuccess) cap = bytes;
        return e;
    }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr;
        cap = 0;
    }
    template <class T>
    T* as() const { return static_cast<T*>(p); }
};

// The context's stream, owned (reads as the hipStream_t it holds).
struct Stream {
    hipStream_t h = nullptr;
    Stream() = default;
    Stream(const Stream&) = delete;
    Stream& operator=(const Stream&) = delete;
    ~Stream() {
        if (h) (void)hipStreamDestroy(h);
    }
    operator hipStream_t() const { return h; }
};

// F4's fallback-list hint: mapped, coherent host memory (F4 stores it system-scope), owned.
struct MappedHint {
    uint32_t* host = nullptr;
    uint32_t* dev = nullptr;   // its device address
    MappedHint() = default;
    MappedHint(const MappedHint&) = delete;
    MappedHint& operator=(const MappedHint&) = delete;
    ~MappedHint() {
        if (host) (void)hipHostFree(host);
    }
};

// N timing events, owned (created together; a creation that fails part-way leaks none).
template <int N>
struct Events {
    hipEvent_t ev[N] = {};
    Events() = default;
    Events(const Events&) = delete;
    Events& operator=(const Events&) = delete;
    ~Events() {
        for (hipEvent_t e : ev)
            if (e) (void)hipEventDestroy(e);
    }
    hipError_t create() {
        for (hipEvent_t& e : ev)
            if (hipError_t r = hipEventCreate(&e)) return r;
        return hipSuccess;
    }
};

int map_err(hipError_t e) {
    if (e == hipSuccess) return DHTGPU_OK;
    if (e == hipErrorOutOfMemory || e == hipErrorMemoryAllocation) return DHTGPU_ENOMEM;
    return DHTGPU_EDEVICE;
}

// DHTGPU_VERBOSE: name the failing HIP call on stderr (diagnostics; read once)
bool verbose() {
    static const bool v = getenv("DHTGPU_VERBOSE") != nullptr;
    return v;
}

#define DHT_TRY(expr)                                                                                  \
    do {                                                                                               \
        hipError_t _e = (expr);                                                                        \
        if (_e != hipSuccess) {                                                                        \
            if (verbose()) fprintf(stderr, "dhtgpu: %s at %s:%d: %s\n", hipGetErrorString(_e), __FILE__, __LINE__, #expr); \
            return map_err(_e);                                                                        \
        }                                                                                              \
    } while (0)

uint32_t pad_q(uint32_t q) { return (q + 63) & ~63u; }
inline size_t al256(size_t b) { return (b + 255) & ~size_t(255); }

// Lay N blocks of sz[i] bytes out in buf, each 256-byte aligned: p[i] = block i.
template <size_t N>
hipError_t carve(DevBuf& buf, const size_t (&sz)[N], uint8_t* (&p)[N]) {
    size_t tot = 0;
    for (size_t x : sz) tot += al256(x);
    if (hipError_t e = buf.ensure(tot)) return e;
    uint8_t* w = buf.as<uint8_t>();
    for (size_t i = 0; i < N; ++i) {
        p[i] = w;
        w += al256(sz[i]);
    }
    return hipSuccess;
}

// Wire scratch behind `lead` bytes: n nodes' tails | q * nc candidates | q * 8 records | q lengths.
size_t wire_bytes(size_t lead, uint64_t n, uint32_t alen, uint32_t q, uint32_t nc) {
    return lead + al256((size_t)n * (alen + 2)) + al256((size_t)q * nc * 4) + al256((size_t)q * 8 * (20 + alen + 2)) +
           al256((size_t)q * 4) + 256;
}

// one big-endian word of an id at the boundary
inline uint32_t be32(const uint8_t* p) {
    return ((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) | ((uint32_t)p[2] << 8) | p[3];
}

// nb bucket firsts (20-byte ids) as word planes: fp[w * nb + b]
std::vector<uint32_t> firsts_planes(const uint8_t* firsts20, uint32_t nb) {
    std::vector<uint32_t> fp((size_t)5 * nb);
    for (uint32_t b = 0; b < nb; ++b)
        for (int w = 0; w < 5; ++w) fp[(size_t)w * nb + b] = be32(firsts20 + 20 * (size_t)b + 4 * w);
    return fp;
}

}  // namespace

struct dhtgpu_ctx {
    int device = 0;
    int num_cus = 256;
    // Members are destroyed in reverse order, after the destructor's body: every buffer below is
    // freed first, then the mapped hint, the stream last.
    Stream stream;
    // fallback-list length of the context's last completed K6 call, written by F4 (a hint read
    // without any sync: it sizes the next call's fallback-scan grid)
    MappedHint fb_hint;
    DevBuf planes;          // 5 * stride u32
    uint64_t n = 0, stride = 0;
    bool sorted = false;
    DevBuf staging;         // host<->device byte staging
    DevBuf targets;         // 5 * tstride u32
    DevBuf out_idx, out_cnt, rec, aux, aux2, aux3;
    bool has_ids = false;
    DevBuf gidx;            // shard -> global index map (dhtgpu_gen_ids_prefix), else unused
    bool has_gidx = false;
    bool map_global = true;  // prefix shard results: global stream indices (else shard-local)
    const uint32_t* out_map() const { return has_gidx && map_global ? gidx.as<uint32_t>() : nullptr; }
    uint32_t shard_pbits = 0;   // prefix shard: every id shares its top shard_pbits bits
    DevBuf w0s;                 // prefix shard: word 0 shifted left by shard_pbits (stride u32)
    DevBuf index;           // K4 workspace: entries | directory | partition scratch
    uint32_t index_B = 0;
    bool index_valid = false;
    DevBuf wire;            // wire-format staging (tails, candidates, blobs)
    DevBuf net_sorted;      // crawl model: {w0, index} in node order (index rebuilt by net_prepare)
    DevBuf net_dead;        // crawl model: dead mask (n bytes) or empty
    DevBuf net_io;          // crawl model: search-batch staging
    uint64_t net_seed = 0;
    bool net_valid = false, net_has_dead = false;
    // K6 workspaces: kBatchDepth slots used round-robin, so that up to kBatchDepth calls issued
    // on different streams run concurrently (one batch's latency-bound F3/F4 overlaps the next
    // batch's HBM-bound F2).  A call on a slot last used on another stream first waits for
    // that stream's work so far (an event recorded there at switch time, so calls that stay on
    // one stream pay nothing); calls on one stream keep plain stream order.
    struct BatchSlot {
        DevBuf ws;              // workspace; its zero-between-calls head (bitmap, counters) stays clean
        DevBuf out_idx, out_cnt;   // record mode: local results before the record conversion
        DevBuf sws;             // small-batch path workspace (zero between calls once cleaned)
        size_t zeroed = 0;      // leading workspace bytes known zero (the last call's clean head) ...
        size_t ctr_off = 0;     // ... but for the statistics words at this offset (batch_ctr_offset)
        uint64_t desc_sig = 0;  // sub-partition descriptors held by the workspace (launch_batch_topk)
        bool sclean = false;
        uint32_t spar = 0;      // small-batch path: the counter set its next call uses
        hipEvent_t done = nullptr;
        hipStream_t last = nullptr;
    };
    static constexpr int kBatchDepth = 4;
    BatchSlot bslot[kBatchDepth];
    int bnext = 0, blast = 0;
    bool last_small = false;   // the last K6-API call took the small-batch path
    uint64_t last_n = 0;       // ... else its plan: largest sub-partition, planned targets, sub-partitions
    uint32_t last_qp = 0, last_nsub = 1;
    uint32_t last_pf = 0;
    // Prefix sub-partitions of a large id set (built on the first K6 call K6 cannot plan in
    // one piece, e.g. the 2^27-id cfg-3 shard): the ids whose next sub_bits bits (after the
    // shard's own prefix) equal i, compacted in order, with their shifted word-0 plane; one K6
    // launch sequence then serves all of them.
    struct SubPart {
        DevBuf planes, map, gmap, w0s;   // planes: 5 * stride u32; map: sub -> ctx-local; gmap: sub -> global
        uint64_t n = 0, stride = 0;
        uint32_t span[32] = {};          // launch_cell_spans of w0s (host copy): F2's window bound
    };
    std::vector<SubPart> subs;
    std::vector<uint32_t> spans;   // [subs][32] the sub-partitions' span tables (BatchCall::spans)
    DevBuf cells;            // [subs][1 << cell_level()] u8 id counts per level-cell_level() prefix (F1's sibling rule)
    DevBuf hinv;             // [n] context-local index -> sub-partition handle
    uint32_t sub_bits = 0;
    bool subs_valid = false;
    bool subs_sorted = false;   // the sub-partitions are sorted by prefix (decided by the call that built them)
    // dhtgpu_set_sub_handles: sub-partitioned calls return handles (a sub-partition's offset +
    // its compacted index), no index-map read per result; sub_tab maps them back on request
    bool sub_handles = false;
    DevBuf sub_tab;   // HandleSub[subs.size()], built with the sub-partitions
    uint32_t shard_pval = 0;
    // lexicographically sorted views (sort.hip): of the main set when it was uploaded unsorted
    // (built on the first cached_nodes call), and the NodeCache mirror (dhtgpu_cache_set)
    struct SortedSet {
        DevBuf planes, perm;
        uint64_t n = 0, stride = 0;
        bool valid = false, unique = true;
    };
    SortedSet sview, cache;
    uint64_t cache_version = 0;
    DevBuf cache_in, sort_scratch, cache_acc;
    DevBuf srch;            // search_insert / table_stats staging
    // Resident routing table (dhtgpu_rt_set ...): one blob -- firsts planes | off | good prefix
    // sums | myid | node planes | good bytes | tails -- and the kernels' view of it.  Private to
    // the rt entry points: the k-NN id set, the accept mask and the cache mirror know nothing of it.
    struct RTable {
        DevBuf buf;
        RtView v = {};
        uint32_t* gpre = nullptr;   // v.gpre / v.good, writable (the good setters)
        uint8_t* good = nullptr;
        bool valid = false;
        uint64_t version = 0;
        // K1g (dhtgpu_rtg_*): the grown form, built by the first rtg mutation and dropped by
        // dhtgpu_rt_set.  A pair of fixed-geometry blobs (RtgBlob) -- a mutation reads the current
        // one (or buf, the first time) and writes the other, so readers in flight on other streams
        // keep theirs -- and the handle -> position map.  v then views g[gcur].
        DevBuf g[2];
        RtgBlob gb[2] = {};
        int gcur = 0;
        bool grown = false;
        bool rows_ok = false;       // every bucket of the upload holds at most 8 nodes
        uint32_t splits = 0;        // splits since the upload
        DevBuf hmap;                // [kRtgMaxHandle] position by handle, DHT_NONE = not resident
        DevBuf io;                  // a mutation's arguments and results
        std::vector<uint8_t> hin, hout;   // ... packed on the host: one copy each way
    } rt;
    // Resident NodeCache (dhtgpu_nc_set ...): two buffer sets of six planes (five key words + the
    // handle), each with head-room -- a mutation reads set[cur] and writes the other -- and the
    // accept mask by handle, which always covers every handle the mirror holds.  Private to the
    // nc entry points, staging included.
    struct NCache {
        DevBuf set[2];
        uint64_t cap[2] = {0, 0};   // keys a set holds = its planes' stride
        int cur = 0;
        uint32_t n = 0;
        DevBuf bits, bits_old;      // bits_old: the mask before its last growth (calls in flight may read it)
        uint64_t words = 0;
        DevBuf in, sorted, perm, hin, ain, work;   // a batch: planes as uploaded, sorted, its permutation, handles, accept bytes
        bool valid = false;
        NcView view() const {
            const uint32_t* p = set[cur].as<uint32_t>();
            return NcView{n, p, cap[cur], p + 5 * cap[cur], bits.as<uint32_t>()};
        }
    } nc;
    // Resident searches (dhtgpu_sr_reset ...): the rows' six entry planes, the slots' targets,
    // lengths and bits bytes, and the node state bytes by handle (grown geometrically; the array
    // before its last growth is kept for calls in flight on other streams).  Private to the sr
    // entry points, staging included; refill reads the nc mirror through nc.view().
    struct Searches {
        DevBuf rows, tp, len, bits;
        uint32_t nslots = 0;
        DevBuf st, st_old;
        uint32_t nst = 0;           // the state array's extent
        DevBuf io;                  // host forms: argument and result staging
        bool valid = false;
        SrView view() const {
            return SrView{nslots, rows.as<uint32_t>(), (uint64_t)nslots * DHTGPU_SR_CAP, tp.as<uint32_t>(),
                          len.as<uint32_t>(), bits.as<uint8_t>(), st.as<uint8_t>(), nst};
        }
        // K10m (dhtgpu_srm_*): the searches' ordered map -- the mapped slots in target order and the
        // sorted target planes -- and an offer's work arrays, all sized by dhtgpu_srm_set so that an
        // offer allocates nothing.  Dropped by dhtgpu_sr_reset and dhtgpu_sr_open.
        struct Map {
            DevBuf in, planes, perm, order, work;
            uint32_t ns = 0;
            uint64_t stride = 0;
            bool valid = false;
            SrmView view() const { return SrmView{ns, order.as<uint32_t>(), planes.as<uint32_t>(), stride}; }
            // work: pos | flag | offs | list | trim x 4 | hazard word, the call's own stats
            SrmWork arrays() const {
                uint32_t* w = work.as<uint32_t>();
                return SrmWork{w, w + kSrmChunk, w + 2 * kSrmChunk, w + 3 * kSrmChunk, w + 4 * kSrmChunk,
                               w + 8 * (size_t)kSrmChunk};
            }
            uint32_t* stats() const { return work.as<uint32_t>() + 8 * (size_t)kSrmChunk + 4; }
        } map;
    } sr;
    // diagnostics: DHTGPU_DBG, the library's one diagnostics switch, read once at creation and
    // masked to kDbgAllowed -- bit 256: per-block phase stamps of F2 / F3 printed to stderr;
    // bit 2^23: K6 instead of KS for batches of <= 64 targets (both exact).  Neither changes a
    // result; every other bit is ignored (the result-altering measurement ablations of earlier
    // rounds are not in this library: DESIGN.md §5d)
    uint32_t dbg = 0;
    uint32_t search_alpha = 4;   // crawl model: requests per search round (MAX_REQUESTED_SEARCH_NODES)
    hipEvent_t next_ev[8] = {};   // dhtgpu_batch_events: the next K6 call records its kernels here
    bool has_next_ev = false;
    DevBuf stamps;
    // Accept mask (dhtgpu_set_accept ...): a bitmask over the set and its live view -- the accepted
    // ids compacted in index order into planes of their own, with the view -> set index map.  The
    // setters store bits and mark the view stale; the next k-NN call (or dhtgpu_num_accepted)
    // rebuilds it once (view.hip).  The k-NN paths read the set through active_set(): the view when
    // a mask rejects at least one id, else the set itself.
    struct Accept {
        DevBuf bits;             // view_mask_words(stride) words, zero past n
        bool has_mask = false;
        bool stale = false;      // bits changed (or the ids did) since the view was built
        hipStream_t bits_stream = nullptr;   // dhtgpu_set_accept_bits_dev: the stream its copy is ordered on
        bool active = false;     // the view is in use: a mask is set and rejects at least one id
        DevBuf planes, map, w0s, gmap;   // 5 * stride u32; view -> set; shifted word 0; view -> global stream
        uint64_t n = 0, stride = 0;
        DevBuf bmap;             // map + bmap_base (a plain context's idx_base != 0), built on first use
        uint32_t bmap_base = 0;
        bool bmap_valid = false;
        DevBuf index;            // the view's own K4 index (the set's stays valid for the crawl model)
        uint32_t index_B = 0;
        bool index_valid = false;
        DevBuf toff;             // tile offsets + total (build scratch)
    } acc;
    // What a k-NN call answers from: the id set, or the accept mask's view of it.
    struct ActiveSet {
        const uint32_t* planes; uint64_t stride, n;
        const uint32_t* map;     // result index map (nullable: index + idx_base); a view's carries idx_base
        const uint32_t* w0s;     // prefix shard: shifted word-0 plane (else nullptr)
        uint32_t pbits, pval;    // prefix shard: shard_pbits / shard_pval
        bool view;
        DevBuf* index; uint32_t* index_B; bool* index_valid;   // the K4 index over these ids
    };
    int active_set(uint32_t idx_base, ActiveSet* out);   // brings the view up to date (may synchronise)
    // the id set itself, whatever the accept mask says
    ActiveSet full_set() {
        return ActiveSet{planes.as<uint32_t>(), stride, n, out_map(), shard_pbits ? w0s.as<uint32_t>() : nullptr,
                         shard_pbits, shard_pval, false, &index, &index_B, &index_valid};
    }
    void clear_accept() {
        const bool was = acc.active;
        acc = Accept{};
        if (was) invalidate_subs();   // they were built from the view
    }

    hipError_t bind() { return hipSetDevice(device); }
    // the stream of a call: the caller's, else the context's
    hipStream_t stream_or(void* s) const { return s ? (hipStream_t)s : stream.h; }
    void invalidate_subs() {
        subs_valid = false;
        if (fb_hint.host) *fb_hint.host = 1u;   // a new set or split: the next call's list length is unknown
        subs.clear();
        sub_tab.release();
        cells.release();
        hinv.release();
        sub_bits = 0;
    }

    // Work in flight ends before anything is freed: the context's stream and every slot's last
    // foreign stream.  The members then go as declared above (the caller has bound the device).
    ~dhtgpu_ctx() {
        if (stream.h) (void)hipStreamSynchronize(stream.h);
        for (auto& b : bslot) {
            if (b.last && b.last != stream.h) (void)hipStreamSynchronize(b.last);
            if (b.done) (void)hipEventDestroy(b.done);
        }
    }

    // upload q targets (20-byte big-endian, host) into target planes; returns stride
    hipError_t upload_targets(const uint8_t* t20, uint32_t q, uint64_t* ts) {
        const uint64_t s = pad_q(q);
        hipError_t e = staging.ensure((size_t)q * 20);
        if (e != hipSuccess) return e;
        if ((e = targets.ensure((size_t)s * 5 * 4)) != hipSuccess) return e;
        if ((e = hipMemcpyAsync(staging.p, t20, (size_t)q * 20, hipMemcpyHostToDevice, stream)) != hipSuccess) return e;
        if ((e = launch_pack(staging.as<uint8_t>(), q, targets.as<uint32_t>(), s, stream)) != hipSuccess) return e;
        *ts = s;
        return hipSuccess;
    }
};

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

// an all-rejected mask: every row empty (stream-ordered)
static int answer_empty(uint32_t q, uint32_t k, uint32_t* out_idx, uint32_t* out_cnt, uint32_t* out_rec, hipStream_t s) {
    if (out_idx) DHT_TRY(launch_fill(out_idx, (uint64_t)q * k, DHTGPU_NONE, s));
    if (out_cnt) DHT_TRY(launch_fill(out_cnt, q, 0u, s));
    if (out_rec) DHT_TRY(launch_fill(out_rec, (uint64_t)q * k * 3, DHTGPU_NONE, s));
    return DHTGPU_OK;
}

// ---- sequences shared by several entry points -----------------------------------------------
// n 20-byte ids (host) into the word planes at dst (stride), 2^22 ids (80 MB) of staging at a time.
static int upload_ids(dhtgpu_ctx* c, const uint8_t* ids20, uint64_t n, uint32_t* dst, uint64_t stride) {
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
static int stage_idx_val(dhtgpu_ctx* c, DevBuf& buf, const uint32_t* idx, const uint8_t* val, uint64_t m,
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
static int grow_kept(dhtgpu_ctx* c, DevBuf& cur, DevBuf& old, size_t live, size_t need, size_t floor, size_t most) {
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

// The ids of a set that carry a prefix, in two passes over scratch carved from the context's aux:
// count() (one host sync for the total, which sizes the caller's output), then compact().
namespace {
struct PrefixSelect {
    const uint32_t* planes; uint64_t stride, n;
    uint32_t pbits, pval;
    hipStream_t s;
    unsigned long long* d_total = nullptr;
    uint32_t* scratch = nullptr;
    int count(dhtgpu_ctx* c, unsigned long long* m) {
        DHT_TRY(c->aux.ensure((size_t)select_scratch_words(n) * 4 + 16));
        d_total = reinterpret_cast<unsigned long long*>(c->aux.as<uint8_t>());
        scratch = reinterpret_cast<uint32_t*>(c->aux.as<uint8_t>() + 8);
        DHT_TRY(launch_select_prefix(planes, stride, n, pbits, pval, scratch, d_total, nullptr, 0, nullptr, 0, s));
        DHT_TRY(hipMemcpyAsync(m, d_total, 8, hipMemcpyDeviceToHost, s));
        DHT_TRY(hipStreamSynchronize(s));
        return DHTGPU_OK;
    }
    // out_idx (nullable): base + the set index of every selected id
    hipError_t compact(uint32_t* out_planes, uint64_t out_stride, uint32_t* out_idx, uint64_t base) const {
        return launch_select_prefix(planes, stride, n, pbits, pval, scratch, d_total, out_planes, out_stride, out_idx,
                                    base, s);
    }
};
}  // namespace

// Where a call's local index rows go: the caller's rows, or -- record form, where the records are
// made from the rows -- scratch rows of their own.
static int local_rows(uint32_t* out_rec, DevBuf& idx, DevBuf& cnt, uint32_t q, uint32_t k, uint32_t** li, uint32_t** lc) {
    if (!out_rec) return DHTGPU_OK;
    DHT_TRY(idx.ensure((size_t)q * k * 4));
    DHT_TRY(cnt.ensure((size_t)q * 4));
    *li = idx.as<uint32_t>();
    *lc = cnt.as<uint32_t>();
    return DHTGPU_OK;
}

// The host form of a top-k call: upload the targets, run(target planes, stride, device rows,
// device counts) on the context's stream, copy the rows back, synchronise.
template <class Run>
static int host_topk(dhtgpu_ctx* c, const uint8_t* t20, uint32_t q, uint32_t k, uint32_t* out_idx, uint32_t* out_cnt,
                     Run run) {
    uint64_t ts = 0;
    DHT_TRY(c->upload_targets(t20, q, &ts));
    DHT_TRY(c->aux2.ensure((size_t)q * k * 4));
    DHT_TRY(c->aux3.ensure((size_t)q * 4));
    if (int r = run(c->targets.as<uint32_t>(), ts, c->aux2.as<uint32_t>(), c->aux3.as<uint32_t>())) return r;
    DHT_TRY(hipMemcpyAsync(out_idx, c->aux2.p, (size_t)q * k * 4, hipMemcpyDeviceToHost, c->stream));
    DHT_TRY(hipMemcpyAsync(out_cnt, c->aux3.p, (size_t)q * 4, hipMemcpyDeviceToHost, c->stream));
    DHT_TRY(hipStreamSynchronize(c->stream));
    return DHTGPU_OK;
}

// The same sequence for entry points whose results are not index rows: N device blocks carved out
// of aux2, filled by run(tp, ts, p) on the context's stream and copied to the host pointers that
// are set (a null one names an output the caller did not ask for).
struct HostOut {
    void* host;
    size_t bytes;
};
template <size_t N, class Run>
static int host_rows(dhtgpu_ctx* c, const uint8_t* t20, uint32_t q, const HostOut (&o)[N], Run run) {
    uint64_t ts = 0;
    DHT_TRY(c->upload_targets(t20, q, &ts));
    size_t sz[N];
    uint8_t* p[N];
    for (size_t i = 0; i < N; ++i) sz[i] = o[i].bytes;
    DHT_TRY(carve(c->aux2, sz, p));
    if (int r = run(c->targets.as<uint32_t>(), ts, p)) return r;
    for (size_t i = 0; i < N; ++i)
        if (o[i].host) DHT_TRY(hipMemcpyAsync(o[i].host, p[i], sz[i], hipMemcpyDeviceToHost, c->stream));
    DHT_TRY(hipStreamSynchronize(c->stream));
    return DHTGPU_OK;
}

// Argument checks of the top-k calls: the _dev forms (index rows or records) and the host forms.
static int check_topk_dev(const dhtgpu_ctx* c, const uint32_t* tp, uint32_t q, uint32_t k, const uint32_t* out_idx,
                          const uint32_t* out_cnt, const uint32_t* out_rec) {
    if (!c || k == 0 || k > DHTGPU_MAX_K || (q && !tp)) return DHTGPU_EINVAL;
    if (!out_rec && (!out_idx || !out_cnt)) return DHTGPU_EINVAL;
    if (!c->has_ids) return DHTGPU_ENOIDS;
    return DHTGPU_OK;
}

static int check_topk_host(const dhtgpu_ctx* c, const uint8_t* t20, uint32_t q, uint32_t k, const uint32_t* out_idx,
                           const uint32_t* out_cnt) {
    if (!c || k == 0 || k > DHTGPU_MAX_K || (q && (!t20 || !out_idx || !out_cnt))) return DHTGPU_EINVAL;
    if (!c->has_ids) return DHTGPU_ENOIDS;
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

int dhtgpu_set_sub_handles(dhtgpu_ctx* c, int on) {
    if (!c) return DHTGPU_EINVAL;
    c->sub_handles = on != 0;
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
// the mask buffer at the size the view kernels read unchecked, all zero
static int mask_alloc(dhtgpu_ctx* c, hipStream_t s) {
    const size_t bytes = (size_t)view_mask_words(c->stride) * 4;
    DHT_TRY(c->acc.bits.ensure(bytes));
    DHT_TRY(hipMemsetAsync(c->acc.bits.p, 0, bytes, s));
    return DHTGPU_OK;
}

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

int dhtgpu_sub_handles_active(dhtgpu_ctx* c, uint32_t q, uint32_t k) {
    if (!c || !c->has_ids) return 0;
    if (c->acc.has_mask) return 0;   // masked calls return indices
    return c->sub_handles && !(small_supported(c->n, q, k) && !(c->dbg & (1u << 23))) && needs_subs(c->num_cus, c->n, q, k) ? 1 : 0;
}

int dhtgpu_handles_to_indices_dev(dhtgpu_ctx* c, const uint32_t* handles, uint64_t m, uint32_t* out_idx,
                                  uint32_t idx_base, void* stream) {
    if (!c || (m && (!handles || !out_idx))) return DHTGPU_EINVAL;
    if (!c->subs_valid) return DHTGPU_EINVAL;   // no sub-partitioned call has built the handle space
    if (!m) return DHTGPU_OK;
    DHT_TRY(c->bind());
    const bool global = c->has_gidx && c->map_global;
    DHT_TRY(launch_handles_to_idx(c->sub_tab.as<HandleSub>(), (uint32_t)c->subs.size(), handles, m, out_idx, global,
                                  global ? 0u : idx_base, c->stream_or(stream)));
    return DHTGPU_OK;
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

// K1 over an active set (checked arguments, q > 0)
static int topk_on(dhtgpu_ctx* c, const dhtgpu_ctx::ActiveSet& A, const uint32_t* tp, uint64_t ts, uint32_t q, uint32_t k,
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

int dhtgpu_topk_dev(dhtgpu_ctx* c, const uint32_t* tp, uint64_t ts, uint32_t q, uint32_t k,
                    uint32_t* out_idx, uint32_t* out_cnt, uint32_t* out_rec, uint32_t idx_base,
                    void* stream) {
    if (int r = check_topk_dev(c, tp, q, k, out_idx, out_cnt, out_rec)) return r;
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

// the K4 index over an active set (the id set's own index, or the view's)
static int index_build_on(const dhtgpu_ctx::ActiveSet& A, hipStream_t s, hipEvent_t* ev) {
    const uint32_t B = index_bits(A.n);
    *A.index_valid = false;
    DHT_TRY(A.index->ensure(index_bytes(A.n, B)));
    DHT_TRY(launch_index_build(A.planes, A.stride, A.n, B, A.index->p, s, ev));
    *A.index_B = B;
    *A.index_valid = true;
    return DHTGPU_OK;
}

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

// ---- K6 -------------------------------------------------------------------------------------
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

int dhtgpu_batch_topk_dev(dhtgpu_ctx* c, const uint32_t* tp, uint64_t ts, uint32_t q, uint32_t k,
                          uint32_t* out_idx, uint32_t* out_cnt, uint32_t* out_rec, uint32_t idx_base,
                          void* stream) {
    if (int r = check_topk_dev(c, tp, q, k, out_idx, out_cnt, out_rec)) return r;
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
}  // extern "C"

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

// ---- K8w: the resident NodeCache --------------------------------------------------------------
}  // extern "C"

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

// 1 + the largest of m handles; 0 when one is at or over the bound
static uint64_t nc_handle_extent(const uint32_t* handles, uint64_t m) {
    uint64_t ext = 1;
    for (uint64_t j = 0; j < m; ++j) {
        if (handles[j] >= DHTGPU_NC_MAX_HANDLE) return 0;
        ext = std::max<uint64_t>(ext, (uint64_t)handles[j] + 1);
    }
    return ext;
}

// insert / erase: sort the batch, rank it, read the kept count (and the result bytes) back, one
// pass into the other buffer set.
static int nc_mutate(dhtgpu_ctx* c, bool erase, const uint8_t* ids20, const uint32_t* handles, const uint8_t* accept,
                     uint32_t m, uint8_t* out_res) {
    dhtgpu_ctx::NCache& t = c->nc;
    const uint64_t ms = pad_ids(m);
    DHT_TRY(t.sorted.ensure((size_t)ms * 5 * 4));
    int unique = 1;   // repeats inside a batch are allowed
    if (int r = nc_sort_batch(c, ids20, m, t.sorted.as<uint32_t>(), ms, &unique)) return r;
    const size_t nb = ((size_t)m + 255) / 256;   // rank | flag | block counts | their scan | kpos | ksrc | total | result bytes
    const size_t sz[] = {(size_t)m * 4, (size_t)m * 4, nb * 4, nb * 4, (size_t)m * 4, (size_t)m * 4, 4, (size_t)m};
    uint8_t* p[8];
    DHT_TRY(carve(t.work, sz, p));
    uint32_t* kpos = reinterpret_cast<uint32_t*>(p[4]);
    uint32_t* ksrc = reinterpret_cast<uint32_t*>(p[5]);
    if (!erase) {
        DHT_TRY(t.hin.ensure((size_t)m * 4));
        DHT_TRY(hipMemcpyAsync(t.hin.p, handles, (size_t)m * 4, hipMemcpyHostToDevice, c->stream));
        if (accept) {
            DHT_TRY(t.ain.ensure((size_t)m));
            DHT_TRY(hipMemcpyAsync(t.ain.p, accept, (size_t)m, hipMemcpyHostToDevice, c->stream));
        }
    }
    const NcView v = t.view();
    DHT_TRY(launch_nc_rank(erase, v, t.sorted.as<uint32_t>(), ms, t.perm.as<uint32_t>(), m,
                           reinterpret_cast<uint32_t*>(p[0]), reinterpret_cast<uint32_t*>(p[1]),
                           reinterpret_cast<uint32_t*>(p[2]), reinterpret_cast<uint32_t*>(p[3]), kpos, ksrc,
                           reinterpret_cast<uint32_t*>(p[6]), p[7], c->stream));
    uint32_t kept = 0;
    DHT_TRY(hipMemcpyAsync(&kept, p[6], 4, hipMemcpyDeviceToHost, c->stream));
    if (out_res) DHT_TRY(hipMemcpyAsync(out_res, p[7], (size_t)m, hipMemcpyDeviceToHost, c->stream));
    DHT_TRY(hipStreamSynchronize(c->stream));
    if (!kept) return DHTGPU_OK;
    const int dst = t.cur ^ 1;
    const uint64_t nn = erase ? (uint64_t)t.n - kept : (uint64_t)t.n + kept;
    if (int r = nc_room(c, dst, nn)) return r;
    if (erase) {
        DHT_TRY(launch_nc_erase(v, t.set[dst].as<uint32_t>(), t.cap[dst], kpos, kept, c->stream));
    } else {
        if (int r = nc_mask_ensure(c, nc_handle_extent(handles, m))) return r;
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
    const uint64_t ext = handles ? nc_handle_extent(handles, n) : std::max<uint64_t>(n, 1);
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
    if (m && !nc_handle_extent(handles, m)) return DHTGPU_EINVAL;   // nothing applied
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
    const uint64_t ext = nc_handle_extent(handles, m);
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

// ---- K10w: the resident searches ---------------------------------------------------------------
}  // extern "C"

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

extern "C" {

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
    const uint64_t ext = nc_handle_extent(handles, m);
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
    if (!nc_handle_extent(handles, m)) return DHTGPU_EINVAL;
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
    if (!nc_handle_extent(ins_handle, tot)) return DHTGPU_EINVAL;
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

// ---- K10m: Dht::trySearchInsert over the searches' ordered map -------------------------------------
}  // extern "C"

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

extern "C" {

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
    if (!nc_handle_extent(handles, m)) return DHTGPU_EINVAL;
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
