// api_ctx.h -- what the host units of the C ABI (api*.hip) share; private, not installed.  The
// owners, the context, and the helpers more than one unit calls: templates, one-liners and the one
// host loop that measured hot stand here, every other helper is declared here and defined once, in api.hip.
// Ownership: a DevBuf frees its device memory when it is destroyed, and the context's stream
// and mapped hint are owners declared before every buffer, so deleting a dhtgpu_ctx releases
// everything in order and an early return leaks nothing.
#pragma once
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

using namespace dhtgpu;   // (this header is the api units' alone: each of them would say the same)

// Named, not anonymous: the owners are members of dhtgpu_ctx, one type across all units.
namespace dhtgpu::host {

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

int map_err(hipError_t e);
// DHTGPU_VERBOSE: name the failing HIP call on stderr (diagnostics; read once)
bool verbose();

#define DHT_TRY(expr)                                                                                  \
    do {                                                                                               \
        hipError_t _e = (expr);                                                                        \
        if (_e != hipSuccess) {                                                                        \
            if (dhtgpu::host::verbose()) fprintf(stderr, "dhtgpu: %s at %s:%d: %s\n", hipGetErrorString(_e), __FILE__, __LINE__, #expr); \
            return dhtgpu::host::map_err(_e);                                                          \
        }                                                                                              \
    } while (0)

inline uint32_t pad_q(uint32_t q) { return (q + 63) & ~63u; }
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
inline size_t wire_bytes(size_t lead, uint64_t n, uint32_t alen, uint32_t q, uint32_t nc) {
    return lead + al256((size_t)n * (alen + 2)) + al256((size_t)q * nc * 4) + al256((size_t)q * 8 * (20 + alen + 2)) +
           al256((size_t)q * 4) + 256;
}

// one big-endian word of an id at the boundary
inline uint32_t be32(const uint8_t* p) {
    return ((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) | ((uint32_t)p[2] << 8) | p[3];
}

// 1 + the largest of m handles; 0 when one is at or over the bound (the NodeCache's: the resident
// searches' handles are cache slots).
// Inline, as the static function it was could be: it walks whole batches (65,536 handles in nc_bench), and the
// two comparisons made with it out of line both read nc_insert slower, if by no more than processes differ (§5o).
inline uint64_t handle_extent(const uint32_t* handles, uint64_t m) {
    uint64_t ext = 1;
    for (uint64_t j = 0; j < m; ++j) {
        if (handles[j] >= DHTGPU_NC_MAX_HANDLE) return 0;
        ext = std::max<uint64_t>(ext, (uint64_t)handles[j] + 1);
    }
    return ext;
}

// nb bucket firsts (20-byte ids) as word planes: fp[w * nb + b]
std::vector<uint32_t> firsts_planes(const uint8_t* firsts20, uint32_t nb);

}  // namespace dhtgpu::host

using namespace dhtgpu::host;

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
        DevBuf tick, rtick;         // the entries' last_get_reply plane; refill_time per slot
        uint32_t clock = 0;         // dhtgpu_srs_set_clock: passed by value to every launch, 0 until set
        uint32_t nslots = 0;
        DevBuf st, st_old;
        uint32_t nst = 0;           // the state array's extent
        DevBuf io;                  // host forms: argument and result staging
        bool valid = false;
        SrView view() const {
            return SrView{nslots, rows.as<uint32_t>(), (uint64_t)nslots * DHTGPU_SR_CAP, tp.as<uint32_t>(),
                          len.as<uint32_t>(), bits.as<uint8_t>(), st.as<uint8_t>(), nst,
                          tick.as<uint32_t>(), rtick.as<uint32_t>(), clock};
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

namespace dhtgpu::host {

// The sequences several units share (api.hip; each is described where it is defined).
int answer_empty(uint32_t q, uint32_t k, uint32_t* out_idx, uint32_t* out_cnt, uint32_t* out_rec, hipStream_t s);
int upload_ids(dhtgpu_ctx* c, const uint8_t* ids20, uint64_t n, uint32_t* dst, uint64_t stride);
int stage_idx_val(dhtgpu_ctx* c, DevBuf& buf, const uint32_t* idx, const uint8_t* val, uint64_t m,
                  const uint32_t** d_idx, const uint8_t** d_val);
int grow_kept(dhtgpu_ctx* c, DevBuf& cur, DevBuf& old, size_t live, size_t need, size_t floor, size_t most);
int local_rows(uint32_t* out_rec, DevBuf& idx, DevBuf& cnt, uint32_t q, uint32_t k, uint32_t** li, uint32_t** lc);
int check_topk_dev(const dhtgpu_ctx* c, const uint32_t* tp, uint32_t q, uint32_t k, const uint32_t* out_idx,
                   const uint32_t* out_cnt, const uint32_t* out_rec);
int check_idx_base(const dhtgpu_ctx* c, uint32_t idx_base);
int check_topk_host(const dhtgpu_ctx* c, const uint8_t* t20, uint32_t q, uint32_t k, const uint32_t* out_idx,
                    const uint32_t* out_cnt);
// K1 over an active set (K6 falls back to it) and the K4 index build (the crawl model's, too)
int topk_on(dhtgpu_ctx* c, const dhtgpu_ctx::ActiveSet& A, const uint32_t* tp, uint64_t ts, uint32_t q, uint32_t k,
            uint32_t* out_idx, uint32_t* out_cnt, uint32_t* out_rec, uint32_t idx_base, hipStream_t s);
int index_build_on(const dhtgpu_ctx::ActiveSet& A, hipStream_t s, hipEvent_t* ev);

// The ids of a set that carry a prefix, in two passes over scratch carved from the context's aux:
// count() (one host sync for the total, which sizes the caller's output), then compact().
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

// The host form of a top-k call: upload the targets, run(target planes, stride, device rows,
// device counts) on the context's stream, copy the rows back, synchronise.
template <class Run>
int host_topk(dhtgpu_ctx* c, const uint8_t* t20, uint32_t q, uint32_t k, uint32_t* out_idx, uint32_t* out_cnt,
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
int host_rows(dhtgpu_ctx* c, const uint8_t* t20, uint32_t q, const HostOut (&o)[N], Run run) {
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

}  // namespace dhtgpu::host
