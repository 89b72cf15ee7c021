// dhtgpu_internal.h -- host-side launch entry points shared between the kernel
// translation units and the C ABI (api*.hip).  Not part of the public ABI.  K6's host-only half --
// the plane geometry, the plan flags, SubSpec, the size queries batch_supported / batch_bytes /
// batch_clean_bytes / batch_ctr_offset / small_* and batch_plan_words -- is batch_plan.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <mutex>

#include "batch_plan.h"

namespace dhtgpu {

// hipFuncSetAttribute (e.g. MaxDynamicSharedMemorySize) applies to the device current on the
// calling thread: set() runs once per device id below kMaxDevices, from whichever thread gets
// there first, and on every call for a device id past the table.  Returns hipGetDevice's error.
constexpr int kMaxDevices = 64;
inline hipError_t per_device_once(std::once_flag* flags, void (*set)()) {
    int dev = 0;
    const hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    if (dev >= 0 && dev < kMaxDevices) std::call_once(flags[dev], set);
    else set();
    return hipSuccess;
}

// prims.hip: the primitives every family shares (their device forms: prims_dev.h)
// Exclusive scan of `rows` consecutive rows of len words each, in -> out (out == in: in place), one
// workgroup per row; tot[r] = row r's sum, in the width of the caller's slot.  One array is one row.
hipError_t launch_excl_scan(const uint32_t* in, uint32_t* out, uint32_t rows, uint32_t len, uint32_t* tot, hipStream_t s);
hipError_t launch_excl_scan(const uint32_t* in, uint32_t* out, uint32_t rows, uint32_t len, unsigned long long* tot,
                            hipStream_t s);
// bit idx[j] of bits = val[j] != 0, j < m (device arrays; idx inside the mask, checked by the caller)
hipError_t launch_bits_update(uint32_t* bits, const uint32_t* idx, const uint8_t* val, uint64_t m, hipStream_t s);
// bytes[idx[j]] = normalise ? val[j] != 0 : val[j], j < m (device arrays; idx inside the array)
hipError_t launch_bytes_update(uint8_t* bytes, const uint32_t* idx, const uint8_t* val, uint64_t m, bool normalise,
                               hipStream_t s);

// keys.hip
hipError_t launch_gen(uint64_t seed, uint64_t start, uint64_t n, uint32_t* planes,
                      uint64_t stride, hipStream_t s);
hipError_t launch_pack(const uint8_t* ids20, uint64_t n, uint32_t* planes, uint64_t stride,
                       hipStream_t s);
hipError_t launch_unpack(const uint32_t* planes, uint64_t stride, uint64_t first, uint64_t n,
                         uint8_t* out20, hipStream_t s);
hipError_t launch_fill(uint32_t* p, uint64_t n, uint32_t v, hipStream_t s);
// sets *d_flag to 1 if ids are NOT strictly ascending (unsorted or duplicated)
hipError_t launch_check_sorted(const uint32_t* planes, uint64_t stride, uint64_t n,
                               uint32_t* d_flag, hipStream_t s);

// ids whose top pbits bits equal pval, compacted in index order (out == nullptr: count
// only).  scratch: select_scratch_words(n) u32; *d_total = number selected; gidx[j] =
// gbase + original index of the j-th selected id (nullable).
hipError_t launch_select_prefix(const uint32_t* planes, uint64_t stride, uint64_t n, uint32_t pbits,
                                uint32_t pval, uint32_t* scratch, unsigned long long* d_total,
                                uint32_t* out, uint64_t out_stride, uint32_t* gidx, uint64_t gbase,
                                hipStream_t s);
uint64_t select_scratch_words(uint64_t n);

// view.hip: the accept mask's live view.  A mask is stride / 32 words (id i = bit (i & 31) of
// word i >> 5), zero past n, so that the kernels below read whole tiles of it unchecked.
uint64_t view_mask_words(uint64_t stride);
// bytes[32 * nwords] (device, 16-B aligned, nonzero = accepted) -> bits[nwords]
hipError_t launch_view_pack(const uint8_t* bytes, uint64_t nwords, uint32_t* bits, hipStream_t s);
// clears the bits past n in the word that holds bit n
hipError_t launch_view_trim(uint32_t* bits, uint64_t n, hipStream_t s);
// toff[stride / kTile] = exclusive offsets of the tiles' accepted ids, *d_total = their number
hipError_t launch_view_count(const uint32_t* bits, uint64_t stride, uint32_t* toff, unsigned long long* d_total,
                             hipStream_t s);
// the accepted ids compacted in index order: out planes (out_stride), map[j] = set index of view id
// j, w0s (nullable; shift in [1, 31]) = the view's shifted word-0 plane, gmap[j] = gidx[map[j]]
// (both nullable).  Writes [0, total) of each only: the caller sizes them from *d_total and zeroes
// the padding.
hipError_t launch_view_compact(const uint32_t* planes, uint64_t stride, const uint32_t* bits, const uint32_t* toff,
                               uint32_t* out, uint64_t out_stride, uint32_t* map, uint32_t* w0s, uint32_t shift,
                               const uint32_t* gidx, uint32_t* gmap, hipStream_t s);
// out[i] = map[i] + base, i < m
hipError_t launch_view_add(const uint32_t* map, uint64_t m, uint32_t base, uint32_t* out, hipStream_t s);

// scan.hip
struct ScanPlan {
    uint32_t blocks_x;   // target groups
    uint32_t splits;     // id-range splits
    uint64_t split_len;  // ids per split (multiple of kTile)
};
// splits are capped so that K3 can stage splits * k records (24 B) of a target in LDS
ScanPlan plan_scan(uint64_t n, uint32_t q, uint32_t k, int num_cus);
// final form: out_idx/out_cnt mapped through gidx (nullable) or offset by idx_base;
// split record form (out_rec != nullptr, internal to the K1 split merge): full 24-B records
// rec[((split * q) + qi) * k + r] * 6 = {w0..w4, idx + idx_base}
hipError_t launch_scan(const uint32_t* ids, uint64_t is, uint64_t n, const ScanPlan& p,
                       const uint32_t* tp, uint64_t ts, uint32_t q, uint32_t k,
                       uint32_t* out_idx, uint32_t* out_cnt, uint32_t* out_rec,
                       const uint32_t* gidx, uint32_t idx_base, hipStream_t s);
hipError_t launch_merge(const uint32_t* rec, uint32_t lists, uint32_t q, uint32_t kin,
                        const uint32_t* tp, uint64_t ts, uint32_t k, uint32_t* out_idx,
                        uint32_t* out_cnt, hipStream_t s);

// valid idx[i] -> gidx ? gidx[idx[i]] : idx[i] + base
hipError_t launch_map_idx(uint32_t* idx, uint64_t m, const uint32_t* gidx, uint32_t base, hipStream_t s);
// compact candidate records (the public record form): rec[i * 3 ..] = {w0, w1, global index} of
// local index idx[i] (all DHT_NONE for DHT_NONE); the global index is gidx[idx[i]] when gidx !=
// nullptr, else idx[i] + base
hipError_t launch_rec3(const uint32_t* idx, uint64_t m, const uint32_t* planes, uint64_t stride, uint32_t base,
                       const uint32_t* gidx, uint32_t* rec, hipStream_t s);
// K3 over compact records (lists <= 64, kin <= 32): rows whose candidates tie on their first 64
// bits across lists are appended to ties = {count, rows[tie_cap]} (zeroed here; nullable)
hipError_t launch_merge3(const uint32_t* rec, uint32_t lists, uint32_t q, uint32_t kin, const uint32_t* tp,
                         uint64_t ts, uint32_t k, uint32_t* out_idx, uint32_t* out_cnt, uint32_t* ties,
                         uint32_t tie_cap, hipStream_t s);
// words 2..4 of this set's candidates (rec: its own compact records, q x k) in the listed rows
// (+ row_base) or every row (ties == nullptr); gmap (nullable, ascending) maps global -> local
hipError_t launch_tie_words(const uint32_t* rec, uint32_t q, uint32_t k, const uint32_t* ties, uint32_t tie_cap,
                            uint32_t row_base, const uint32_t* planes, uint64_t stride, uint64_t n,
                            const uint32_t* gmap, uint32_t base, uint32_t* words, hipStream_t s);
// the listed rows (every row when ties == nullptr) merged again on the full keys
hipError_t launch_merge_full(const uint32_t* rec, const uint32_t* words, uint32_t lists, uint32_t q, uint32_t kin,
                             const uint32_t* tp, uint64_t ts, uint32_t k, const uint32_t* ties, uint32_t tie_cap,
                             uint32_t* out_idx, uint32_t* out_cnt, hipStream_t s);

// table.hip
hipError_t launch_find_closest(uint32_t nb, const uint32_t* fp, const uint32_t* off,
                               const uint32_t* gcnt, const uint32_t* np, uint64_t ns,
                               const uint8_t* good, const uint32_t* tp, uint64_t ts, uint32_t q,
                               uint32_t count, uint32_t* out_idx, uint32_t* out_cnt,
                               hipStream_t s);
hipError_t launch_classify(const uint32_t* planes, uint64_t stride, uint64_t n, uint32_t nb,
                           const uint32_t* fp, const uint32_t* myid, uint8_t* out_bucket,
                           unsigned long long* hist, hipStream_t s);
// perm (nullable): sorted position -> caller index (accept and the output use caller indices)
hipError_t launch_cached(const uint32_t* planes, uint64_t stride, uint64_t n, const uint32_t* perm,
                         const uint8_t* accept, const uint32_t* tp, uint64_t ts, uint32_t q,
                         uint32_t count, uint32_t* out_idx, uint32_t* out_cnt, hipStream_t s);

// index.hip: K4 bucket index (counting sort by the top B bits) + K5 trie-descent k-NN
uint32_t index_bits(uint64_t n);
size_t index_bytes(uint64_t n, uint32_t B);
// ev (nullable): 5 events recorded before/between/after the build's kernels
hipError_t launch_index_build(const uint32_t* planes, uint64_t stride, uint64_t n, uint32_t B, void* ws,
                              hipStream_t s, hipEvent_t* ev = nullptr);
hipError_t launch_index_query(const void* ws, uint64_t n, uint32_t B, const uint32_t* planes, uint64_t stride,
                              const uint32_t* tp, uint64_t ts, uint32_t q, uint32_t k, uint32_t* out_idx,
                              uint32_t* out_cnt, hipStream_t s);

// batch.hip: K6 per-batch target-prefix filter + exact top-k (sizes and plan queries: batch_plan.h)
// stats4 = {fallback targets, survivors, wave-path targets, 0} of the last call on workspace ws
// (synchronises s)
hipError_t batch_read_stats(const void* ws, uint64_t n, uint32_t q, uint32_t q_plan, uint32_t k, int num_cus,
                            uint32_t* stats4, hipStream_t s, uint32_t nsub = 1, uint32_t pf = 0);
uint32_t cell_level();
// u8 counts (saturated) of the n ids of a shifted word-0 plane per top-cell_level()-bit prefix;
// scratch: 4 << cell_level() bytes
hipError_t launch_cell_counts(const uint32_t* w0s, uint64_t n, uint32_t* scratch, uint8_t* out, hipStream_t s);
// spans[j] (device, 32 words) = the most level-cell_level() cells that 2^j consecutive ids of a
// prefix-sorted shifted word-0 plane span (K6's F2 window bound)
hipError_t launch_cell_spans(const uint32_t* w0s, uint64_t n, uint32_t* spans, hipStream_t s);
// prefix shards: out[i] = planes word 0 << shift | word 1 >> (32 - shift), i < stride
hipError_t launch_shift_w0(const uint32_t* planes, uint64_t stride, uint32_t shift, uint32_t* out, hipStream_t s);

constexpr uint32_t kHandleMark = 0x80000000u;   // sets hold < 2^31 ids (batch_supported)
// DHTGPU_DBG bits the library honours (dhtgpu_ctx::dbg): 256 = phase stamps, 2^23 = K6 for
// small batches.  Diagnostics only -- no bit changes a result (tests/test_abi.py pins the mask).
constexpr uint32_t kDbgAllowed = 256u | (1u << 23);
// One sub-partition in handle space: handles [off, off + n) name its ids in its (prefix-sorted) order.
struct HandleSub {
    uint64_t n;
    const uint32_t* map;    // sub-local -> context-local
    const uint32_t* gmap;   // sub-local -> global stream index (nullable: no global map)
    uint32_t off, pad;
};
// out[i] = the index handle h[i] names: gmap (global) or map + base; DHT_NONE stays
hipError_t launch_handles_to_idx(const HandleSub* tab, uint32_t nsub, const uint32_t* h, uint64_t m, uint32_t* out,
                                 bool global, uint32_t base, hipStream_t s);
// idx[i] (context-local) -> its handle in place: hinv[idx[i]] (DHT_NONE stays)
hipError_t launch_idx_to_handles(const uint32_t* hinv, uint32_t* idx, uint64_t m, hipStream_t s);
// hinv[map[j]] = off + j, j < m: the context-local -> handle map of one sub-partition
hipError_t launch_handle_inverse(const uint32_t* map, uint64_t m, uint32_t off, uint32_t* hinv, hipStream_t s);

struct BatchCall {
    void* ws;                              // workspace (batch_bytes), head zero (batch_clean_bytes)
    const uint32_t* planes; uint64_t stride; uint64_t n;   // the id set (unshifted word planes)
    const uint32_t* tp; uint64_t ts;       // target planes
    uint32_t q;                            // targets F1 reads (the whole batch)
    uint32_t q_plan;                       // targets the plan is sized for
    uint32_t k;
    const SubSpec* subs; uint32_t nsub;    // prefix sub-partitions (nsub 0: the set planes/n/w0s/gidx/base)
    uint32_t sub_shift, sub_bits;          // a target's sub-partition: its bits [sub_shift, +sub_bits)
    uint64_t* desc_sig;                    // the workspace's uploaded sub-partition descriptors (signature)
    uint32_t skip; const uint32_t* w0s;    // w0s = 32 id bits from bit `skip` (every id shares its top skip bits)
    uint32_t pval;                         // skip > 0: the shared top bits' value (of the shard; sub-partitions
                                           // append their index: sub_bits more)
    const uint8_t* cells;                  // nullable: [nsub][1 << cell_level()] cell counts of the sub-partitions
    const uint32_t* spans;                 // nullable, HOST: [nsub][32] cell spans of the (prefix-sorted) sub-partitions
    uint32_t sorted;                       // the sub-partitions are sorted by prefix (spans then bound F2's windows)
    const uint32_t* gidx; uint32_t base;   // result index map (nullable) or offset
    uint32_t* out_idx; uint32_t* out_cnt;  // rows of the ORIGINAL target indices
    // record form (nullable): every writer of a result row (F3, the wave paths, F4's scan and
    // merge) stores the row's compact records instead of its indices; rec_gidx / rec_base map the
    // context-local index to the record's global index
    uint32_t* out_rec; const uint32_t* rec_gidx; uint32_t rec_base;
    // sub-partition handles (nsub > 1, dhtgpu_set_sub_handles): every sub-partition's results are
    // its base + sub-local index (SubSpec gidx null, base = the sub-partition's offset); rows F4
    // answers from the whole set carry context-local index | kHandleMark (gidx null, base =
    // kHandleMark) and a pass after F4 turns them into handles through htab
    uint32_t handles; const HandleSub* htab;
    const uint32_t* hinv;                  // handles: context-local index -> handle
    int num_cus;
    uint32_t dbg;                          // DHTGPU_DBG & kDbgAllowed (0 in production)
    const volatile uint32_t* fb_hint;      // nullable: the slot's last fallback-list length (mapped host memory)
    uint32_t* fb_hint_dev;                 // its device address (F4 writes it)
    unsigned long long* stamps;            // dbg & 256: phase stamps [2 * 8192 * 16]
    hipEvent_t* ev;                        // nullable: 8 events around F1..F4
};
hipError_t launch_batch_topk(const BatchCall& c, hipStream_t s);
// KS (batch.hip): batches of at most 64 targets -- one pass over word 0 and one workgroup per
// distinct target prefix (K6's results).  sws: small_bytes(), zero before its first use (left
// zero); parity: alternates between consecutive calls on one workspace (two counter sets);
// ev (nullable) gets S1 as F2's pair and S2 as F3's, F1 / F4 pairs empty.
hipError_t launch_small_topk(const BatchCall& c, void* sws, uint32_t parity, hipStream_t s);

// sort.hip: lexicographic sort of an id set (stable LSD radix over the 160-bit keys).
// out_planes (out_stride >= n) = the ids in ascending InfoHash order, perm[j] = the input index
// of sorted id j; *unique = 0 when two ids are equal.  Synchronises s.
size_t sort_scratch_bytes(uint64_t n);
hipError_t launch_sort_ids(const uint32_t* planes, uint64_t stride, uint64_t n, uint32_t* out_planes, uint64_t out_stride,
                           uint32_t* perm, void* scratch, int* unique, hipStream_t s);

// search.hip: batched Dht::Search::insertNode; RoutingTable::depth + InfoHash::lowbit per bucket
hipError_t launch_search_insert(const uint32_t* planes, uint64_t stride, const uint8_t* st, const uint32_t* tp,
                                uint64_t ts, uint32_t q, uint32_t cap, uint32_t* list_node, uint8_t* list_flags,
                                uint32_t* list_len, uint8_t* expired, const uint64_t* ins_off, const uint32_t* ins_node,
                                const uint8_t* ins_token, uint8_t* ins_added, uint32_t* overflow, hipStream_t s);
hipError_t launch_table_stats(const uint32_t* fp, uint32_t nb, int32_t* out_lowbit, uint32_t* out_depth, hipStream_t s);

// wire.hip: NetworkEngine::bufferNodes / deserializeNodes (compact node records)
hipError_t launch_wire_encode(const uint32_t* planes, uint64_t stride, const uint8_t* tail, uint32_t alen,
                              const uint32_t* tp, uint64_t ts, uint32_t q, const uint32_t* cand, uint32_t c,
                              uint8_t* out, uint32_t* out_len, hipStream_t s);
hipError_t launch_wire_decode(const uint8_t* blob, const uint64_t* msg_off, const uint32_t* rec_start, uint32_t m,
                              uint32_t nrec, uint32_t af, const uint8_t* myid, const uint8_t* from_af,
                              const uint8_t* from_addr, uint8_t* out_ids, uint8_t* out_tail, uint8_t* out_status,
                              hipStream_t s);

// rtable.hip: K1w, the resident routing table (dhtgpu_rt_*).  The mirror as the kernels read it:
// device pointers into one blob owned by the context.
struct RtView {
    uint32_t nb, nn;           // buckets (<= 256), nodes (= off[nb])
    const uint32_t* fp;        // bucket firsts as word planes: fp[w * nb + b]
    const uint32_t* off;       // [nb + 1] bucket b owns nodes [off[b], off[b + 1])
    const uint32_t* gpre;      // [nb + 1] good nodes of buckets [0, b)
    const uint32_t* np;        // node word planes, np[w * ns + i]
    uint64_t ns;
    const uint8_t* good;       // [nn] Node::isGood(now)
    const uint8_t* tail;       // [nn * (alen + 2)] address || port (null: set without tails)
    uint32_t alen;             // 4 / 16 (0 without tails)
    const uint32_t* myid;      // 5 words
};
// gpre from off and good (one workgroup; after every change of the good bytes)
hipError_t launch_rt_gpre(const RtView& v, uint32_t* gpre, hipStream_t s);
// findClosestNodes per target over the mirror (1 <= count <= DHTGPU_MAX_K_DEV): indices + counts;
// the count-8 result as bufferNodes records (out_idx nullable: q x 8); the closeness flag
// (out_cnt nullable)
hipError_t launch_rt_find(const RtView& v, const uint32_t* tp, uint64_t ts, uint32_t q, uint32_t count,
                          uint32_t* out_idx, uint32_t* out_cnt, hipStream_t s);
hipError_t launch_rt_reply(const RtView& v, const uint32_t* tp, uint64_t ts, uint32_t q, uint8_t* out,
                           uint32_t* out_len, uint32_t* out_idx, hipStream_t s);
hipError_t launch_rt_closer(const RtView& v, const uint32_t* tp, uint64_t ts, uint32_t q, uint32_t count,
                            uint32_t min_nodes, uint8_t* out_flag, uint32_t* out_cnt, hipStream_t s);

// rtgrow.hip: K1g, onNewNode / split / expireBuckets on the resident table (dhtgpu_rtg_*).  A grown
// table lives in a blob of fixed geometry -- kRtgBuckets buckets, kRtgNodes nodes (the node planes'
// stride) -- that carries, beside K1w's arrays, each node's handle and its state byte.
constexpr uint32_t kRtgBuckets = 256, kRtgNodes = 2048, kRtgMaxHandle = 65536;
struct RtgBlob {
    uint32_t* fp;        // firsts planes, fp[w * nb + b]
    uint32_t* off;       // [kRtgBuckets + 1]
    uint32_t* gpre;      // [kRtgBuckets + 1]
    uint32_t* myid;      // 5 words
    uint32_t* np;        // node planes, np[w * kRtgNodes + i]
    uint8_t* good;       // [kRtgNodes] bit 0 of the state
    uint8_t* state;      // [kRtgNodes] bit 0 isGood, bit 1 isExpired, bit 2 isPendingMessage
    uint32_t* handle;    // [kRtgNodes] the caller's handle of node i
    uint8_t* tail;       // [kRtgNodes * 18]
};
// a batch of new nodes (device arrays): 20-byte ids, handles, state bytes (nullable: good), tails
// (alen + 2 bytes each; alen = the table's), results
struct RtgBatch {
    const uint8_t* ids20;
    const uint32_t* handles;
    const uint8_t* state;
    const uint8_t* tail;
    uint32_t m, flags, alen;
    uint8_t* out_res;
    uint32_t* out_aux;
};
// One workgroup: the table v (hsrc / ssrc: its handle and state planes, null for a table that never
// grew: handle = position, state = good) through LDS into d; hmap[kRtgMaxHandle] = position by
// handle (DHT_NONE: not resident; all DHT_NONE on entry for a table that never grew).  Every bucket
// of v holds at most 8 nodes.  out_stat[4] = {nb, nn, splits, stopped at a 257th bucket} /
// {nb, nn, 0, nodes removed}; out_handles (nullable) = the removed handles, any order.
hipError_t launch_rtg_insert(const RtView& v, const uint32_t* hsrc, const uint8_t* ssrc, const RtgBlob& d, uint32_t* hmap,
                             const RtgBatch& a, uint32_t* out_stat, hipStream_t s);
hipError_t launch_rtg_expire(const RtView& v, const uint32_t* hsrc, const uint8_t* ssrc, const RtgBlob& d, uint32_t* hmap,
                             uint32_t* out_handles, uint32_t* out_stat, hipStream_t s);
// the state of every resident node whose handle is below nh = by_handle[handle] (device array)
hipError_t launch_rtg_set_state(const RtgBlob& d, uint32_t nn, const uint8_t* by_handle, uint32_t nh, hipStream_t s);
// launch_bytes_update through the handle -> position map: i = hmap[h[j]] for h[j] < kRtgMaxHandle,
// handles that are not resident skipped.  whole: the state byte val[j] (good[i] = its bit 0);
// else good[i] = val[j] != 0 and bit 0 of state[i] follows it.  (It stands here and not in
// prims.hip because every kernel of that unit is pinned by name in an existing budget test.)
hipError_t launch_rtg_update(const RtgBlob& d, const uint32_t* hmap, const uint32_t* h, const uint8_t* val, uint64_t m,
                             bool whole, hipStream_t s);
// idx[j] = handle[idx[j]] for idx[j] < nn, in place (DHT_NONE stays)
hipError_t launch_rtg_handles(const uint32_t* handle, uint32_t nn, uint32_t* idx, uint64_t m, hipStream_t s);

// ncache.hip: K8w, the resident NodeCache mirror (dhtgpu_nc_*).  The mirror as the kernels read
// it: device pointers into the context's current buffer set and its accept mask.
struct NcView {
    uint32_t n;              // keys
    const uint32_t* kp;      // key word planes, lexicographically sorted: kp[w * ks + i]
    uint64_t ks;
    const uint32_t* hp;      // [n] the caller's handle of key i (= kp + 5 * ks)
    const uint32_t* bits;    // accept mask by handle: bit (h & 31) of word h >> 5; covers every handle of hp
};
// getCachedNodes per target over the mirror (1 <= count <= DHTGPU_MAX_K_DEV): handles in walk order + counts
hipError_t launch_nc_nodes(const NcView& v, const uint32_t* tp, uint64_t ts, uint32_t q, uint32_t count,
                           uint32_t* out_handle, uint32_t* out_cnt, hipStream_t s);
// A sorted batch (bp / bs, perm[j] = caller index of sorted key j, m keys) against the mirror:
// rank[j] = its lower bound, flag[j] = the mutation applies to it (insert: not resident; erase:
// resident; never to a repeat of the batch key before it), res[perm[j]] = flag[j], bsum / boff
// [ceil(m / 256)] = the set flags per 256-key block and their exclusive scan, *d_total = their
// sum, kpos / ksrc [e] = rank[j] / j of the e-th kept key.
hipError_t launch_nc_rank(bool erase, const NcView& v, const uint32_t* bp, uint64_t bs, const uint32_t* perm, uint32_t m,
                          uint32_t* rank, uint32_t* flag, uint32_t* bsum, uint32_t* boff, uint32_t* kpos, uint32_t* ksrc,
                          uint32_t* d_total, uint8_t* res, hipStream_t s);
// The one pass of a mutation: the mirror and the cnt kept batch keys (handles hin[], accept bytes
// ain[] -- nullable: accepted -- in the caller's order; their accept bits are set in `bits`) into
// the six planes at dst (stride ds >= n + cnt) / the mirror without the cnt positions kpos[].
hipError_t launch_nc_insert(const NcView& v, uint32_t* dst, uint64_t ds, const uint32_t* kpos, const uint32_t* ksrc,
                            uint32_t cnt, const uint32_t* bp, uint64_t bs, const uint32_t* perm, const uint32_t* hin,
                            const uint8_t* ain, uint32_t* bits, hipStream_t s);
hipError_t launch_nc_erase(const NcView& v, uint32_t* dst, uint64_t ds, const uint32_t* kpos, uint32_t cnt,
                           hipStream_t s);
// hp[j] = hin[perm[j]] with its accept bit set, or perm[j] when hin is null (bits untouched)
hipError_t launch_nc_handles(const uint32_t* perm, const uint32_t* hin, uint32_t n, uint32_t* hp, uint32_t* bits,
                             hipStream_t s);
// bits [0, nh) from bytes[nh] (device arrays)
hipError_t launch_nc_bits_pack(const uint8_t* bytes, uint32_t nh, uint32_t* bits, hipStream_t s);

// ncresolve.hip: K8r, keys to handles over the mirror (dhtgpu_ncr_*).
// k_ncr_find<G> is instantiated for two widths: a batch of at most kNcrWideMaxBatch keys gives every
// key a whole wave (the fewest rounds: what a small batch waits for), a larger one kNcrNarrowLanes
// lanes (a wave serves 64 / kNcrNarrowLanes keys: what a large batch's throughput needs).
// kNcrWideMaxBatch is the measured crossover of the two; tests mirror it.
constexpr uint32_t kNcrWideLanes = 64, kNcrNarrowLanes = 16;
constexpr uint32_t kNcrWideMaxBatch = 5040;
// out_handle[j] = the handle of key j (id planes ip / is, m keys, any order, repeats allowed) or
// DHT_NONE; out_accept (nullable) [j] = its accept bit (0: absent, or past the mask's mask_words)
hipError_t launch_ncr_find(const NcView& v, uint64_t mask_words, const uint32_t* ip, uint64_t is, uint32_t m,
                           uint32_t* out_handle, uint8_t* out_accept, hipStream_t s);
// After launch_nc_rank(false, ...) on the same sorted batch (res = its result bytes, batch order):
// hout[i] = the handle of batch key i -- free_handles[r] for the r-th new key in batch order (DHT_NONE
// when r >= nfree), the resident handle of a present key, the first appearance's handle of a repeat.
// bsum / boff: one word per 256 keys each, d_total: one word, ord: m words (scratch).
hipError_t launch_ncr_assign(const NcView& v, const uint32_t* bp, uint64_t bs, const uint32_t* perm, uint32_t m,
                             const uint32_t* rank, const uint32_t* flag, const uint8_t* res, uint32_t* bsum,
                             uint32_t* boff, uint32_t* d_total, uint32_t* ord, const uint32_t* free_handles, uint32_t nfree,
                             uint32_t* hout, hipStream_t s);
// After launch_nc_rank(true, ...): out[i] = the handle batch key i's erase frees, else DHT_NONE
hipError_t launch_ncr_extract(const NcView& v, const uint32_t* perm, const uint32_t* rank, const uint32_t* flag,
                              uint32_t m, uint32_t* out, hipStream_t s);

// rsearch.hip: K10w, the resident searches (dhtgpu_sr_*).  The search set as the kernels see it:
// device pointers into the context's buffers.
struct SrView {
    uint32_t nslots;
    uint32_t* ep;            // six entry planes, ep[w * es + slot * 64 + l]: the five words of entry l's
    uint64_t es;             //   distance to the slot's target, then its handle | flags << 28 | req << 30; es = nslots * 64
    uint32_t* tp;            // target word planes, tp[w * nslots + slot]
    uint32_t* len;           // [nslots] list lengths (<= 64)
    uint8_t* bits;           // [nslots] bit0 Search::expired, bit1 overflowed, bit2 Search::done
    const uint8_t* st;       // node state by handle (bit0 isExpired(), bit1 isRemovable(now)), [nst]
    uint32_t nst;            //   a handle at or past nst reads as 0
    uint32_t* tk;            // the entries' tick plane, tk[slot * 64 + l]: SearchNode::last_get_reply, 0 = min()
    uint32_t* rtick;         // [nslots] Search::refill_time in clock ticks, 0 = never
    uint32_t clock;          // the context's clock (dhtgpu_srs_set_clock), 0 until set
};
// Search::insertNode + removeExpiredNode: slot slots[j] takes insertions [ins_off[j], ins_off[j + 1])
// in order -- handles, id planes ip / is, token bytes (nullable: none) -- added[] (nullable) =
// insertNode's results; *over_any (nullable) |= 1 when a list overflowed in this call.  Device arrays.
hipError_t launch_sr_insert(const SrView& v, const uint32_t* slots, uint32_t m, const uint64_t* ins_off,
                            const uint32_t* ins_handle, const uint32_t* ip, uint64_t is, const uint8_t* tok,
                            uint8_t* added, uint32_t* over_any, hipStream_t s);
// Dht::refill: getCachedNodes(the slot's target, count) over nc, each result inserted without a token
hipError_t launch_sr_refill(const SrView& v, const NcView& nc, const uint32_t* slots, uint32_t m, uint32_t count,
                            uint32_t* out_inserted, uint32_t* over_any, hipStream_t s);
hipError_t launch_sr_open(const SrView& v, const uint32_t* slots, const uint32_t* tp, uint64_t ts, uint32_t m,
                          hipStream_t s);
hipError_t launch_sr_expire(const SrView& v, const uint32_t* slots, uint32_t m, hipStream_t s);
hipError_t launch_sr_candidate(const SrView& v, const uint32_t* slots, const uint32_t* handles, const uint8_t* val,
                               uint32_t m, hipStream_t s);
// out4[j] = {len, bad nodes, leading bad nodes, bits}; the rows as handles / flags (64 per slot, DHT_NONE padded)
hipError_t launch_sr_status(const SrView& v, const uint32_t* slots, uint32_t m, uint32_t* out4, hipStream_t s);
hipError_t launch_sr_lists(const SrView& v, const uint32_t* slots, uint32_t m, uint32_t* out_handle, uint8_t* out_flags,
                           uint32_t* out_len, hipStream_t s);

// srstep.hip: K10s, Dht::searchStep for find_node searches over the resident rows (dhtgpu_srs_*).
// One wave per listed slot (a slot >= nslots is skipped): out_send[j * 64 + i] = the handle of the
// i-th node to send find_node to (DHT_NONE padded), out4[j] = {sends, solicited nodes after, nodes
// the refill inserted, bits}; node_expire in clock ticks; refill_count 0: no refill leg, nc unread.
// *over_any (nullable) |= 1 when a refill overflowed a row.
hipError_t launch_srs_step(const SrView& v, const NcView& nc, const uint32_t* slots, uint32_t m, uint32_t node_expire,
                           uint32_t refill_count, uint32_t* out_send, uint32_t* out4, uint32_t* over_any,
                           hipStream_t s);
// req = val[j] (0, 1, 2) for the entry of handles[j] in slot slots[j] (one wave per pair; absent: nothing)
hipError_t launch_srs_request(const SrView& v, const uint32_t* slots, const uint32_t* handles, const uint8_t* val,
                              uint32_t m, hipStream_t s);
// the rows' req and tick (64 per slot, 0 padded)
hipError_t launch_srs_entries(const SrView& v, const uint32_t* slots, uint32_t m, uint8_t* out_req, uint32_t* out_tick,
                              hipStream_t s);

// srmap.hip: K10m, Dht::trySearchInsert over the searches' ordered map (dhtgpu_srm_*).  The map as
// the kernels read it: the mapped slots in ascending order of their targets and those targets.
struct SrmView {
    uint32_t ns;             // mapped searches
    const uint32_t* order;   // [ns] slot of the j-th smallest target
    const uint32_t* tp;      // the sorted targets as word planes, tp[w * ts + j]
    uint64_t ts;
};
constexpr uint32_t kSrmChunk = 16384;   // nodes per filter + walk launch pair (the work arrays' size)
// The per-node work arrays of one chunk and the call's counters (device, owned by the context).
struct SrmWork {
    uint32_t* pos;      // [kSrmChunk] lower bound of the node's id in the map
    uint32_t* flag;     // [kSrmChunk] 1: the node is walked, 0: the filter answered it
    uint32_t* offs;     // [kSrmChunk] exclusive scan of flag
    uint32_t* list;     // [kSrmChunk] the walked nodes, batch order
    uint32_t* trim;     // [kSrmChunk * 4] a filtered node's {forward slot, cut, backward slot, cut}, DHT_NONE: no search
    uint32_t* hazard;   // one word per chunk launch: a node of the chunk is removable and not expired
};
constexpr size_t kSrmWorkWords = (size_t)kSrmChunk * 8 + 64;
// planes[w * stride + j] = the target of slot slots[j], j < ns
hipError_t launch_srm_gather(const SrView& v, const uint32_t* slots, uint32_t ns, uint32_t* planes, uint64_t stride,
                             hipStream_t s);
// order[j] = slots[perm[j]], j < ns
hipError_t launch_srm_order(const uint32_t* slots, const uint32_t* perm, uint32_t ns, uint32_t* order, hipStream_t s);
// Search::done of slot slots[j] = val[j] != 0 (bit 2 of the slot's bits byte; a slot >= nslots skipped)
hipError_t launch_srm_done(const SrView& v, const uint32_t* slots, const uint8_t* val, uint32_t m, hipStream_t s);
// trySearchInsert for nodes [0, m) of a chunk (m <= kSrmChunk), in order: handles, id planes ip / is.
// out_cnt[j] = searches that took node j; out_touched (nullable) |= the bit of every slot that took a
// node; stats[4] += {filtered nodes, insertNode calls of the walk}, |= {hazard, overflow}.
hipError_t launch_srm_offer(const SrView& v, const SrmView& mp, const SrmWork& wk, const uint32_t* handles,
                            const uint32_t* ip, uint64_t is, uint32_t m, uint32_t* out_cnt, uint32_t* out_touched,
                            uint32_t* stats, hipStream_t s);

// crawl.hip: crawl-replay model (iterative searches over implicit routing tables)
uint32_t search_list_cap();
// sorts the K4 index buckets (index workspace, n ids, B bits) by (w0, index) into out[n]
hipError_t launch_net_sort(const void* index_ws, uint64_t n, uint32_t B, uint2* out, hipStream_t s);
hipError_t launch_search(const uint32_t* planes, uint64_t stride, const uint2* sorted, const void* index_ws,
                         uint64_t n, uint32_t B, const uint8_t* dead, uint64_t seed, const uint32_t* tp, uint64_t ts,
                         uint32_t q, const uint32_t* searchers, uint32_t max_rounds, uint32_t alpha, uint32_t* out_idx,
                         uint8_t* out_flags, uint32_t* out_len, uint32_t* out_rounds, uint32_t* out_queries,
                         hipStream_t s);

}  // namespace dhtgpu
