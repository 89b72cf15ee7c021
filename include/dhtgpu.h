/*
 * dhtgpu.h -- C ABI of libdhtgpu, the MI355X (gfx950) engine for OpenDHT's
 * XOR-closest-node lookup.
 *
 * Plain C: pointers and sizes only, integer status codes, no exceptions and no
 * callbacks cross this boundary.  Node IDs cross it as 20-byte big-endian
 * arrays, byte-for-byte dht::InfoHash::data() (include/opendht/infohash.h:263,
 * HASH_LEN = 20 at :267).  Results are INDICES into the ID array the caller
 * uploaded last; the caller maps them back to its Sp<Node>.
 *
 * Reference interfaces replaced (paths relative to the OpenDHT tree):
 *   dhtgpu_topk            std::partial_sort(ids, k, InfoHash::xorCmp)          (SURVEY §8 a12,
 *                          include/opendht/infohash.h:179-194) -- the flat exact k-NN
 *                          behind findClosestNodesBatch(targets[], k)
 *   dhtgpu_find_closest    RoutingTable::findClosestNodes(id, now, count)
 *                          (include/opendht/routing_table.h:56, src/routing_table.cpp:110-150)
 *   dhtgpu_cached_nodes    NodeCache::getCachedNodes(id, af, count)
 *                          (include/opendht/node_cache.h:31, src/node_cache.cpp:42-74)
 *   dhtgpu_classify        RoutingTable::findBucket (src/routing_table.cpp:153-166) +
 *                          InfoHash::commonBits (include/opendht/infohash.h:154-176)
 *   dhtgpu_table_depth     RoutingTable::depth (src/routing_table.cpp:100-107)
 *   dhtgpu_buffer_nodes    NetworkEngine::bufferNodes (src/network_engine.cpp:1003-1032)
 *   dhtgpu_deserialize_nodes  NetworkEngine::deserializeNodes (src/network_engine.cpp:849-887)
 *   dhtgpu_search_batch    Dht::Search node refresh: Search::insertNode (src/search.h:636-722)
 *                          driven by find_node rounds (crawl replay, tools/dhtscanner.cpp)
 *   dhtgpu_search_insert   Search::insertNode (src/search.h:636-722) itself, batched over searches
 *   dhtgpu_table_stats     InfoHash::lowbit + RoutingTable::depth of every bucket, on the device
 *   dhtgpu_cache_set/_nodes  NodeCache's map (node_cache.h:43) sorted on the device + getCachedNodes
 *   dhtgpu_rt_set/_set_good  the RoutingTable itself (include/opendht/routing_table.h:45-94) kept on
 *                          the device between calls, with the Node::isGood(now) snapshot
 *   dhtgpu_rt_reply        Dht::onFindNode (src/dht.cpp:2128-2138) / onGetValues' (:2141-2161) answer:
 *                          findClosestNodes(target, now, TARGET_NODES) + bufferNodes, fused
 *   dhtgpu_rt_closer       the closeness tests of Dht::maintainStorage (src/dht.cpp:1862-1879) and
 *                          Dht::onAnnounce (:2293-2294): findClosestNodes + xorCmp(nodes.back(), myid)
 *   dhtgpu_nc_set/_insert/_erase  NodeCache's map (node_cache.h:43) resident on the device, changed
 *                          incrementally (NodeMap::getNode, clearBadNodes: src/node_cache.cpp:87-123)
 *   dhtgpu_nc_nodes        NodeCache::getCachedNodes (src/node_cache.cpp:42-74) over it, one wave per target
 *   dhtgpu_ncr_find/_get_nodes/_extract  NodeMap::getNode (src/node_cache.cpp:87-111) in batches over it: ids to
 *                          handles, absent ids emplaced under the caller's free handles, erase that reports its handle
 *   dhtgpu_sr_insert       Search::insertNode (src/search.h:636-722) over node lists resident on the device,
 *                          one wave per search
 *   dhtgpu_sr_refill       Dht::refill (src/dht.cpp:656-677): getCachedNodes over the nc mirror + insertNode, fused
 *   dhtgpu_sr_status       Search::getNumberOfBadNodes / getNumberOfConsecutiveBadNodes (src/search.h:516-530)
 *   dhtgpu_srs_step        Dht::searchStep (src/dht.cpp:562-654) of a find_node search over those lists: refill,
 *                          isSynced / setDone, the next find_node targets, expiry
 *   dhtgpu_srs_set_clock/_set_request/_entries  its clock, the request state of an entry, the entries' state
 *
 * Threading (mirrors the reference, src/dhtrunner.cpp:115-150): one context per
 * thread, or external locking; every host-pointer call is synchronous.
 * The *_dev entry points take device pointers and a hipStream_t (void*), are
 * stream-ordered and do not synchronise (for batch/bench/multi-GPU use).  A stream passed
 * to a context must outlive it: a later call that moves a workspace slot to another stream
 * records an event on the slot's previous stream, and dhtgpu_ctx_destroy synchronises the
 * streams the slots last used.
 *
 * Host arrays: every host array passed to an entry point -- those of the setters that do not
 * synchronise included (dhtgpu_update_accept, dhtgpu_rt_update_good / _set_good,
 * dhtgpu_nc_update_accept / _set_accept, dhtgpu_sr_update_state / _set_state / _open / _expire /
 * _set_candidate) -- is the caller's again when the call returns, PROVIDED it lies in ordinary
 * (pageable) host memory: stack, heap, std::vector.  The library reads such an array with
 * hipMemcpyAsync into its own staging on the context's stream, and HIP performs that copy
 * synchronously with respect to the host when the host side is not pinned; the kernels then read
 * the staging, never the caller's memory, and back-to-back setters reuse one staging buffer in
 * stream order (a growth of it frees the old one only after the device has drained).  An array in
 * pinned memory (hipHostMalloc, hipHostRegister) is read stream-ordered instead: it must stay
 * unchanged until the context's stream has passed the call, i.e. until any synchronising call of
 * the context or a hipStreamSynchronize(dhtgpu_ctx_stream(ctx)) has returned.
 */
#ifndef DHTGPU_H
#define DHTGPU_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DHTGPU_HASH_LEN 20u
#define DHTGPU_WORDS 5u              /* a 160-bit id = 5 big-endian u32 words */
#define DHTGPU_MAX_K 32u             /* largest k / count served */
#define DHTGPU_NONE 0xFFFFFFFFu      /* index padding for short results */
#define DHTGPU_REC_WORDS 3u          /* candidate record: {w0, w1, global index} (12 B) */
#define DHTGPU_MAX_LISTS 64u         /* candidate lists one merge takes (ranks of a sharded lookup) */

enum {
    DHTGPU_OK = 0,
    DHTGPU_EINVAL = -1,              /* bad argument (null pointer, k == 0 or > DHTGPU_MAX_K, ...) */
    DHTGPU_ENOMEM = -2,              /* device allocation failed */
    DHTGPU_EDEVICE = -3,             /* HIP runtime / kernel launch error */
    DHTGPU_ENOIDS = -4,              /* no id set uploaded */
    DHTGPU_EUNSORTED = -5,           /* cached_nodes / cache_set: the id set holds duplicate ids */
    DHTGPU_ERANGE = -6               /* size out of range (e.g. more than 2^32-1 ids) */
};

typedef struct dhtgpu_ctx dhtgpu_ctx;

/* ---- context ---------------------------------------------------------------- */
int dhtgpu_ctx_create(int device, dhtgpu_ctx** out);
void dhtgpu_ctx_destroy(dhtgpu_ctx* ctx);
const char* dhtgpu_strerror(int code);
int dhtgpu_device_count(int* out);
/* Device stream used by the synchronous calls (hipStream_t as void*). */
void* dhtgpu_ctx_stream(dhtgpu_ctx* ctx);

/* ---- the id set (the device mirror of the routing table / node cache) --------- */
/* Upload n ids (20-byte big-endian each).  The device keeps them as five u32
 * word planes (struct of arrays).  Also records whether the set is sorted and
 * unique (needed by dhtgpu_cached_nodes). */
int dhtgpu_set_ids(dhtgpu_ctx* ctx, const uint8_t* ids20_be, uint64_t n);
/* Generate n synthetic ids directly in HBM: splitmix64 stream,
 * id i = BE(x(3g)) || BE(x(3g+1)) || top4(BE(x(3g+2))), g = start + i. */
int dhtgpu_gen_ids(dhtgpu_ctx* ctx, uint64_t seed, uint64_t start, uint64_t n);
/* Multi-GPU prefix routing: generate the stream [start, start+n) and keep
 * only the ids whose top pbits bits equal pval, in stream order.  Every result index of
 * the context then refers to the GLOBAL stream (start + i); get_ids/classify use shard
 * order.  pbits <= 16.  start + n <= 2^32 - 1 else DHTGPU_ERANGE: every index is a uint32
 * below DHTGPU_NONE.
 *   The same rule holds for idx_base, the offset that dhtgpu_topk_dev, dhtgpu_index_topk_dev,
 * dhtgpu_batch_topk_dev, dhtgpu_tie_words_dev and dhtgpu_handles_to_indices_dev add to
 * context-local indices: idx_base + n <= 2^32 - 1, n = dhtgpu_num_ids (the index space, whatever
 * an accept mask hides), else the call returns DHTGPU_ERANGE before it launches anything and
 * writes no output.  It is checked on every context, a prefix shard whose global indices leave
 * idx_base unused included.  (dhtgpu_batch_topk_timed takes no idx_base: its indices start at 0.) */
int dhtgpu_gen_ids_prefix(dhtgpu_ctx* ctx, uint64_t seed, uint64_t start, uint64_t n, uint32_t pbits,
                          uint32_t pval);
/* Prefix shard contexts (dhtgpu_gen_ids_prefix): on != 0 (the default) makes every
 * lookup return indices into the global stream; on == 0 returns shard-local indices
 * (positions in get_ids order) -- the handle a rank that owns its shard's node table
 * keeps, without the per-result gather through the index map. */
int dhtgpu_set_global_indices(dhtgpu_ctx* ctx, int on);
/* Sets too large for one K6 plan (e.g. a 2^27-id shard) are answered over prefix
 * sub-partitions, compacted copies in id order.  on != 0 makes such calls return
 * sub-partition handles instead of indices: handle = the sub-partition's offset + the id's
 * position in it (one handle per id, in [0, n)), saving the per-result read of the index map
 * (10 us of the cfg-3 shard's 0.15 ms).  Record form (out_rec) is unaffected.
 * dhtgpu_sub_handles_active tells whether a call of q targets at k returns handles (only
 * sub-partitioned calls do); dhtgpu_handles_to_indices_dev maps m handles to the indices the
 * call would have returned (global stream indices per dhtgpu_set_global_indices, else
 * context-local + idx_base); DHTGPU_NONE stays.  The handle space is the one the last
 * sub-partitioned call used (it changes with the id set). */
int dhtgpu_set_sub_handles(dhtgpu_ctx* ctx, int on);
int dhtgpu_sub_handles_active(dhtgpu_ctx* ctx, uint32_t q, uint32_t k);
int dhtgpu_handles_to_indices_dev(dhtgpu_ctx* ctx, const uint32_t* handles, uint64_t m, uint32_t* out_idx,
                                  uint32_t idx_base, void* stream);
/* Accept mask over the resident id set -- Node::isGood / isExpired (src/node.cpp:42-47) for the
 * flat k-NN, the `good` snapshot of dhtgpu_find_closest at the scale of the whole set.  While a
 * mask is set, dhtgpu_topk, dhtgpu_topk_dev, dhtgpu_batch_topk, dhtgpu_batch_topk_dev,
 * dhtgpu_batch_topk_timed, dhtgpu_index_topk and dhtgpu_index_topk_dev return, per target, the k
 * XOR-closest ACCEPTED ids: ascending, equal ids by lower original index, out_cnt = min(k,
 * accepted), DHTGPU_NONE padded, and every index is that of the original set exactly as without a
 * mask (+ idx_base; the global stream index on prefix shards per dhtgpu_set_global_indices; the
 * same in record form, so dhtgpu_tie_words_dev and dhtgpu_merge*_dev need nothing new).  On a
 * prefix shard the mask is indexed by shard-local position (dhtgpu_get_ids order).
 *   The library keeps a live view: the accepted ids compacted in index order on the device (24 B
 * per accepted id, 28 B on prefix shards), which the k-NN kernels answer from unchanged.  The
 * setters only store bits and mark the view stale; the next k-NN call or dhtgpu_num_accepted
 * rebuilds it once (one host synchronisation, whatever number of updates went before), so a
 * stream-ordered caller calls dhtgpu_num_accepted outside its loop.  A mask that accepts every id
 * builds no view (the unmasked path); one that rejects every id answers empty rows.  A view change
 * drops what was built from the view: the sub-partitions of large sets (rebuilt by the next
 * sub-partitioned call) and the view's K4 index (rebuilt by the next index query).  While a mask
 * is set dhtgpu_sub_handles_active returns 0 and sub-partitioned calls return indices.
 *   dhtgpu_set_ids / gen_ids / gen_ids_prefix clear the mask.  Unaffected -- they keep working on
 * the full set, with their own masks where they have one: classify, cached_nodes, cache_*,
 * buffer_nodes* (candidates are original indices, which is what masked lookups return),
 * net_prepare / search_batch*, get_ids, ids_dev, select_prefix_dev.  Like dhtgpu_set_ids, the
 * setters below are not to be called while k-NN calls of the context are in flight.
 *
 * accept[n] (host; nonzero = accepted; NULL = clear the mask: every id accepted again) */
int dhtgpu_set_accept(dhtgpu_ctx* ctx, const uint8_t* accept);
/* device bitmask, ceil(n/32) words, id i = bit (i & 31) of word i >> 5; bits past n ignored; copied
 * stream-ordered */
int dhtgpu_set_accept_bits_dev(dhtgpu_ctx* ctx, const uint32_t* bits, void* stream);
/* flip m entries: accept[idx[j]] = val[j] (host arrays; idx < n else DHTGPU_EINVAL, nothing applied;
 * distinct idx -- of a repeated one, one of its values holds).  With no mask set it starts from
 * every id accepted. */
int dhtgpu_update_accept(dhtgpu_ctx* ctx, const uint32_t* idx, const uint8_t* val, uint64_t m);
/* ids currently accepted (n when no mask is set); brings the view up to date (may synchronise) */
int dhtgpu_num_accepted(dhtgpu_ctx* ctx, uint64_t* out);
/* overwrite ids [first, first+m) in place (slot reuse: mask a dead node off, write the new id into
 * its slot, mask it on); first + m <= n else DHTGPU_ERANGE; prefix-shard contexts: DHTGPU_EINVAL.
 * Keeps the mask; everything derived from the ids is rebuilt on its next use (the sorted / unique
 * state at once; the lexicographic view, the K4 index, the sub-partitions, the view; the crawl
 * model needs dhtgpu_net_prepare again). */
int dhtgpu_write_ids(dhtgpu_ctx* ctx, uint64_t first, const uint8_t* ids20_be, uint64_t m);
uint64_t dhtgpu_num_ids(const dhtgpu_ctx* ctx);
/* Read back ids [first, first+n) as 20-byte big-endian. */
int dhtgpu_get_ids(dhtgpu_ctx* ctx, uint64_t first, uint64_t n, uint8_t* out20_be);
/* Device view of the planes: word j of id i is planes[j*stride + i]. */
int dhtgpu_ids_dev(dhtgpu_ctx* ctx, const uint32_t** planes, uint64_t* stride);

/* ---- K1: flat exact top-k (std::partial_sort over xorCmp) ------------------- */
/* For each of q targets, the k ids closest by XOR distance, ascending; equal ids
 * (not produced by OpenDHT) tie-break by lower index.  out_idx[q*k] (DHTGPU_NONE
 * padded), out_cnt[q] = min(k, n).  1 <= k <= DHTGPU_MAX_K. */
int dhtgpu_topk(dhtgpu_ctx* ctx, const uint8_t* targets20_be, uint32_t q, uint32_t k,
                uint32_t* out_idx, uint32_t* out_cnt);

/* Device form.  Targets as word planes (t_planes[j*t_stride + i]).  Writes either
 * the final indices (out_idx/out_cnt, offset by idx_base) or, if out_rec != NULL,
 * candidate records for a cross-shard merge: out_rec[(qi*k + r)*3 + {w0, w1, idx}] = the
 * first two words of the r-th closest id and its index offset by idx_base (global index
 * of a prefix shard context), ascending in XOR distance; all DHTGPU_NONE for empty slots. */
int dhtgpu_topk_dev(dhtgpu_ctx* ctx, const uint32_t* t_planes, uint64_t t_stride, uint32_t q,
                    uint32_t k, uint32_t* out_idx, uint32_t* out_cnt, uint32_t* out_rec,
                    uint32_t idx_base, void* stream);

/* K3: merge `lists` (<= DHTGPU_MAX_LISTS) candidate-record lists per target,
 * rec[((l*q + qi)*k_in + r)*3] as written by the record forms (each list ascending in XOR
 * distance, DHTGPU_NONE records after its valid ones), into the final top-k.  Used after the
 * RCCL all-gather of per-GPU shards.  The records carry 64 bits of each id: a row where two
 * lists' candidates agree on them (two ids sharing their first 64 bits -- never among the
 * candidates of hash-distributed ids -- or one id sent by two lists) is answered provisionally
 * and appended to ties = {count, rows[tie_cap]} (device, zeroed by this call; may be NULL only
 * when lists == 1); such rows are settled by the second exchange: dhtgpu_tie_words_dev on every
 * shard, then dhtgpu_merge_ties_dev.  Records equal in all five words and the index are one
 * candidate; different ids with equal indices are both kept. */
int dhtgpu_merge_dev(const uint32_t* rec, uint32_t lists, uint32_t q, uint32_t k_in,
                     const uint32_t* t_planes, uint64_t t_stride, uint32_t k,
                     uint32_t* out_idx, uint32_t* out_cnt, uint32_t* ties, uint32_t tie_cap, void* stream);
/* The second exchange's payload from one shard: words 2..4 of this context's candidates
 * (rec: its own q x k records from a record-form call with idx_base) in the rows listed by
 * ties (each row + row_base: the row's place in rec when the merge took a slice of the
 * targets), out_words[(slot*k + r)*3 + {w2, w3, w4}] for slot < min(count, tie_cap); ties ==
 * NULL: every row (slot = row), the fallback when count > tie_cap. */
int dhtgpu_tie_words_dev(dhtgpu_ctx* ctx, const uint32_t* rec, uint32_t q, uint32_t k, uint32_t idx_base,
                         const uint32_t* ties, uint32_t tie_cap, uint32_t row_base, uint32_t* out_words,
                         void* stream);
/* Settle the listed rows (every row when ties == NULL) of a dhtgpu_merge_dev by the full
 * 160-bit keys: words = the lists' tie-word payloads concatenated in list order (each
 * tie_cap x k_in x 3 words, or q x k_in x 3 when ties == NULL). */
int dhtgpu_merge_ties_dev(const uint32_t* rec, const uint32_t* words, uint32_t lists, uint32_t q, uint32_t k_in,
                          const uint32_t* t_planes, uint64_t t_stride, uint32_t k, const uint32_t* ties,
                          uint32_t tie_cap, uint32_t* out_idx, uint32_t* out_cnt, void* stream);

/* Device planes -> the ids whose top pbits bits equal pval, compacted in order into
 * out_planes (out_stride >= count) with out_gidx[j] = original index (nullable);
 * *out_count = number selected.  Synchronises (setup-time helper). */
int dhtgpu_select_prefix_dev(dhtgpu_ctx* ctx, const uint32_t* planes, uint64_t stride, uint64_t n,
                             uint32_t pbits, uint32_t pval, uint32_t* out_planes, uint64_t out_stride,
                             uint32_t* out_gidx, uint64_t* out_count, void* stream);

/* Convert 20-byte big-endian ids (device) into word planes (device). */
int dhtgpu_pack_dev(const uint8_t* ids20_be, uint64_t n, uint32_t* planes, uint64_t stride,
                    void* stream);
/* Generate synthetic ids (same stream as dhtgpu_gen_ids) into device planes. */
int dhtgpu_gen_dev(uint64_t seed, uint64_t start, uint64_t n, uint32_t* planes, uint64_t stride,
                   void* stream);

/* ---- K4/K5: bucket index + trie-descent exact top-k (same results as dhtgpu_topk) ---- */
/* Build (or rebuild) the index over the context's id set: a counting sort of the ids by
 * their top B = clamp(log2(n) - 4, 1, 24) bits into 32-byte records plus a 2^B + 1 entry
 * prefix directory.  Stream-ordered (NULL = the context stream); no host sync. */
int dhtgpu_index_build(dhtgpu_ctx* ctx, void* stream);
/* Diagnostics: the same build with HIP events between its kernels; synchronises and
 * returns per-phase device milliseconds ms4 = {P0 histogram, P0 scans, P1 partition
 * scatter, P2 bucket gather}. */
int dhtgpu_index_build_timed(dhtgpu_ctx* ctx, void* stream, float* ms4);
/* Exact top-k via the index: identical output to dhtgpu_topk_dev -- final indices +
 * counts, or (out_rec != NULL) candidate records for dhtgpu_merge_dev; idx offset by
 * idx_base.  Needs a built index (DHTGPU_ENOIDS otherwise). */
int dhtgpu_index_topk_dev(dhtgpu_ctx* ctx, const uint32_t* t_planes, uint64_t t_stride, uint32_t q,
                          uint32_t k, uint32_t* out_idx, uint32_t* out_cnt, uint32_t* out_rec,
                          uint32_t idx_base, void* stream);
/* Host form: builds the index if the id set changed since the last build, then queries. */
int dhtgpu_index_topk(dhtgpu_ctx* ctx, const uint8_t* targets20_be, uint32_t q, uint32_t k,
                      uint32_t* out_idx, uint32_t* out_cnt);

/* ---- K6: per-batch target-prefix filter + exact top-k (same results as dhtgpu_topk) ---- */
/* Nothing persists between calls: each call streams the id word plane w0 once, keeps only
 * the ids that share the batch targets' level-Lm prefixes (Lm ~ log2(n / 4k)), and answers
 * every target from its complete prefix subtree in LDS; targets whose subtree holds fewer
 * than min(k, n) ids, or whose partition overflows (clustered ids), are answered by the K1
 * scan over all ids inside the same call.  Same output forms as dhtgpu_topk_dev.
 * Large sets (n > 2^24 where one plan cannot cover the batch, e.g. the 2^27-id cfg-3 shard at
 * 131,072 targets): the set is split once into 2^s prefix sub-partitions of <= 2^24 ids (built
 * on the first such call, kept until the set changes: 28 B/id of extra HBM) and every call runs
 * ONE K6 launch sequence over all sub-partitions, each answering the targets of its prefix; a
 * sub-partition with fewer than k ids sends its targets to the K1 scan over the whole set.
 * DHTGPU_ERANGE only when q > 2^22 (or n >= 2^32).
 * Stream-ordered, no host sync (except the one-time sub-partition build).  A context keeps four
 * workspaces and gives each stream its own (the one it last used, else a free one), so calls
 * issued on up to four streams run concurrently (one batch's latency-bound answer phase
 * overlaps the other batches' HBM-bound id streams); a call that must take a workspace last
 * used on another stream (a fifth stream) first waits for that stream.
 * Alignment: out_idx, out_cnt and out_rec need 4-byte alignment only (rows on a 16-byte
 * boundary are stored as whole vectors, others word by word: the same results), and the target
 * planes are read one word at a time, so t_planes needs 4-byte alignment and t_stride may be any
 * value >= q (odd ones included). */
int dhtgpu_batch_topk_dev(dhtgpu_ctx* ctx, const uint32_t* t_planes, uint64_t t_stride, uint32_t q,
                          uint32_t k, uint32_t* out_idx, uint32_t* out_cnt, uint32_t* out_rec,
                          uint32_t idx_base, void* stream);
/* Diagnostics: the same call with a start/stop HIP event pair recorded by each kernel's own
 * dispatch; synchronises and returns per-kernel device milliseconds ms4 = {F1 bucket
 * targets, F2 filter ids, F3 answer, F4 ties + fallback scan} and (nullable) stats4 =
 * {targets answered by the fallback scan, surviving ids, targets answered by an exact wave
 * (w0 ties, large subtrees), 0}.  Sub-partitioned calls: the one launch sequence over all
 * sub-partitions. */
int dhtgpu_batch_topk_timed(dhtgpu_ctx* ctx, const uint32_t* t_planes, uint64_t t_stride, uint32_t q,
                            uint32_t k, uint32_t* out_idx, uint32_t* out_cnt, void* stream, float* ms4,
                            uint32_t* stats4);
/* Diagnostics, host only (no device work; ctx may be NULL): the plan a dhtgpu_batch_topk* call of
 * q targets at k over a set of n ids would run with -- on ctx's device (num_cus ignored), or with
 * ctx == NULL on a device of num_cus compute units.  n is the number of ids the call answers from
 * (the accepted ids while a mask is set).  out[16]:
 *    0  route: 0 = KS small batch, 1 = K6 over one set, 2 = K6 over sub-partitions, 3 = refused
 *              (DHTGPU_ERANGE from the call)
 *    1  Lm, the mark level           2  Lmin, the coarsest level a target answers from
 *    3  b1, partition bits           4  Lq, the deepest level F3 sorts by
 *    5  tcap, targets per partition bucket       6  scap, survivors per (bucket set, partition)
 *    7  nsets, bucket sets per partition         8  F3 stage entries of the launch
 *    9  F2 mode: 0 dense, 1 sparse, 3 segmented, 4 narrow stage
 *   10  F2 stage entries of the launch          11  ids per F2 workgroup
 *   12  F2 workgroups               13  1 when F1 runs as coarse + fine passes
 *   14  KS level Ls (route 0 only)  15  0
 * Words 1..13 are defined for route 1 only (0 otherwise): a sub-partitioned call's plan depends
 * on the sub-partitions built from the set. */
int dhtgpu_batch_plan(dhtgpu_ctx* ctx, int num_cus, uint64_t n, uint32_t q, uint32_t k, uint32_t out[16]);
/* Arm per-kernel timing of the NEXT K6 call on this context without synchronising it:
 * its kernels' own dispatches record start/stop into ev8[0..7] (hipEvent_t as void*, created
 * by the caller with timing enabled) = {F1 start, F1 stop, F2 start, F2 stop, F3 .., F4 ..}
 * (sub-partitioned calls: sub-partition 0's kernels).  For timing kernels inside a timed loop. */
int dhtgpu_batch_events(dhtgpu_ctx* ctx, void** ev8);
/* Host form (synchronous). */
int dhtgpu_batch_topk(dhtgpu_ctx* ctx, const uint8_t* targets20_be, uint32_t q, uint32_t k,
                      uint32_t* out_idx, uint32_t* out_cnt);

/* ---- K1r: RoutingTable::findClosestNodes over a table snapshot ------------------ */
/* Snapshot: nb buckets in list order with firsts20[nb*20] (Bucket::first),
 * bucket_off[nb+1] (bucket b owns nodes [off[b], off[b+1]) of node_ids20), and
 * good[nn] = Node::isGood(now) (src/node.cpp:42-47).  For each target: the
 * min(count, C) XOR-closest good nodes of the contiguous bucket range visited by
 * the reference's outward walk, ascending.  out_idx[q*count] indexes node_ids20. */
int dhtgpu_find_closest(dhtgpu_ctx* ctx, uint32_t nb, const uint8_t* firsts20,
                        const uint32_t* bucket_off, const uint8_t* node_ids20,
                        const uint8_t* good, const uint8_t* targets20_be, uint32_t q,
                        uint32_t count, uint32_t* out_idx, uint32_t* out_cnt);

/* ---- K1w: the resident routing table -------------------------------------------------------- */
/* The table of dhtgpu_find_closest kept on the device between calls, so that a responder's
 * find_node / get answers and the storage closeness tests cross PCIe with their targets only.
 * One table per context (one context per address family), private to the rt entry points: the
 * k-NN id set, the accept mask and the NodeCache mirror are not touched, nor do they touch it.
 *
 * dhtgpu_rt_set uploads a snapshot in bucket list order -- nb <= 256 buckets, firsts20[nb*20]
 * (Bucket::first), bucket_off[nb+1] non-decreasing (bucket b owns nodes [off[b], off[b+1]) of
 * node_ids20), exactly as dhtgpu_find_closest takes them -- together with myid20 (Dht::myid) and,
 * nullable, node_tail: node i's address || port bytes at node_tail[i*(alen+2)], laid out like the
 * node_tail of dhtgpu_buffer_nodes_ids (alen = 4 for af 4, 16 for af 6; af = 0 when node_tail is
 * NULL, and dhtgpu_rt_reply then returns DHTGPU_EINVAL).  Every node starts good.  nb == 0 is a
 * valid, empty table.  version != 0 equal to the last upload's, with the same nb and node count,
 * skips the upload (the rule of dhtgpu_cache_set: the caller bumps it whenever the table changes).
 * Synchronous; like dhtgpu_set_ids it must not be called while rt calls are in flight. */
int dhtgpu_rt_set(dhtgpu_ctx* ctx, const uint8_t* myid20, uint32_t nb, const uint8_t* firsts20,
                  const uint32_t* bucket_off, const uint8_t* node_ids20, const uint8_t* node_tail, uint32_t af,
                  uint64_t version);
/* The Node::isGood(now) snapshot (src/node.cpp:42-47), which changes between calls while the
 * table does not: good[nn] (host; nonzero = good) replaces every bit; dhtgpu_rt_update_good sets
 * good[idx[j]] = val[j] for m entries (host arrays; idx < nn else DHTGPU_EINVAL, nothing applied;
 * distinct idx).  Both run on the context's stream without synchronising it (a device kernel
 * recounts the buckets' good nodes); ordering them against _dev calls issued on other streams is
 * the caller's business, as with the accept setters. */
int dhtgpu_rt_set_good(dhtgpu_ctx* ctx, const uint8_t* good);
int dhtgpu_rt_update_good(dhtgpu_ctx* ctx, const uint32_t* idx, const uint8_t* val, uint32_t m);
/* RoutingTable::findClosestNodes(target, now, count) (src/routing_table.cpp:110-150) for q targets
 * over the resident table and its current good bits: the results of dhtgpu_find_closest --
 * out_idx[q*count] indexes the uploaded nodes, DHTGPU_NONE padded, out_cnt[q]; 1 <= count <=
 * DHTGPU_MAX_K.  One wave per target.  The _dev forms take target planes (t_planes[j*t_stride +
 * i], any t_stride >= q) and device outputs, are stream-ordered (NULL = the context's stream)
 * and neither synchronise nor allocate; an empty table gives out_cnt = 0 and DHTGPU_NONE rows.
 * Every rt query returns DHTGPU_ENOIDS before the first dhtgpu_rt_set. */
int dhtgpu_rt_find_closest_dev(dhtgpu_ctx* ctx, const uint32_t* t_planes, uint64_t t_stride, uint32_t q,
                               uint32_t count, uint32_t* out_idx, uint32_t* out_cnt, void* stream);
int dhtgpu_rt_find_closest(dhtgpu_ctx* ctx, const uint8_t* targets20_be, uint32_t q, uint32_t count,
                           uint32_t* out_idx, uint32_t* out_cnt);
/* The find_node / get reply (Dht::onFindNode, src/dht.cpp:2128-2138; onGetValues, :2141-2161): per
 * target, findClosestNodes(target, now, TARGET_NODES = 8) written as NetworkEngine::bufferNodes
 * (src/network_engine.cpp:1003-1032) writes it -- 26-byte (af 4) / 38-byte (af 6) records at
 * out[qi * 8 * rec ..], out_len[qi] bytes of them (the bytes past out_len[qi] are unspecified).
 * Byte-identical to dhtgpu_rt_find_closest_dev at count 8 followed by dhtgpu_buffer_nodes_ids
 * over the same nodes.  out_idx[q*8] (nullable) also receives the indices. */
int dhtgpu_rt_reply_dev(dhtgpu_ctx* ctx, const uint32_t* t_planes, uint64_t t_stride, uint32_t q, uint8_t* out,
                        uint32_t* out_len, uint32_t* out_idx, void* stream);
int dhtgpu_rt_reply(dhtgpu_ctx* ctx, const uint8_t* targets20_be, uint32_t q, uint8_t* out, uint32_t* out_len,
                    uint32_t* out_idx);
/* The closeness test after findClosestNodes: out_flag[qi] = 1 iff the count-node result holds at
 * least max(min_nodes, 1) nodes and target.xorCmp(last result's id, myid) < 0
 * (include/opendht/infohash.h:179-194), else 0 -- a last node equal to myid gives 0.  count = 8,
 * min_nodes = 1 is Dht::maintainStorage's test when not forced (src/dht.cpp:1862-1879); count =
 * 14, min_nodes = 8 is Dht::onAnnounce's drop test (:2293-2294).  out_flag: u8[q]; out_cnt[q]
 * (nullable) = the result sizes. */
int dhtgpu_rt_closer_dev(dhtgpu_ctx* ctx, const uint32_t* t_planes, uint64_t t_stride, uint32_t q, uint32_t count,
                         uint32_t min_nodes, uint8_t* out_flag, uint32_t* out_cnt, void* stream);
int dhtgpu_rt_closer(dhtgpu_ctx* ctx, const uint8_t* targets20_be, uint32_t q, uint32_t count, uint32_t min_nodes,
                     uint8_t* out_flag, uint32_t* out_cnt);

/* ---- K1g: growing the resident table ---------------------------------------------------------- */
/* RoutingTable::onNewNode (src/routing_table.cpp:204-262, split :87-107 / :176-202) and
 * Dht::expireBuckets (src/dht.cpp:179-192) applied to the resident table on the device, so that a
 * caller without a host table can build one, and one with a host table need not re-pack and
 * upload it for every node that enters a bucket.  All K1w queries go on answering from the result.
 *
 * A node is (id, handle, state byte, tail).  "The same node" is the same handle.  State byte:
 * bit 0 Node::isGood(now), bit 1 isExpired(), bit 2 isPendingMessage(); an expired node is never
 * good (not checked).
 *
 * Handles.  dhtgpu_rt_set is unchanged: a node it uploads has handle = its upload position and
 * state = good.  The first rtg mutation (on_new_node with m > 0, expire, set_state, update_state)
 * turns the table into its grown form.  From then on the out_idx of dhtgpu_rt_find_closest[_dev]
 * and dhtgpu_rt_reply[_dev] are HANDLES -- on a table that never grew these equal the positions, so
 * existing callers see no difference -- and so are the idx of dhtgpu_rt_update_good (idx >=
 * DHTGPU_RTG_MAX_HANDLE: DHTGPU_EINVAL).  dhtgpu_rt_set_good, a positional array, returns
 * DHTGPU_EINVAL on a grown table: dhtgpu_rtg_set_state replaces it.  The next dhtgpu_rt_set drops
 * the grown form, also when its version equals an earlier upload's.
 * A new node's handle (< DHTGPU_RTG_MAX_HANDLE) must differ from every resident handle of another
 * node, and ids are distinct per handle.  The same handle twice in one batch is legal: the second
 * is KNOWN if the first was placed into that bucket.  Handles that are not resident are ignored by
 * the state setters.
 *
 * Limits.  Every bucket of the resident table must hold at most 8 nodes, else DHTGPU_EINVAL (known
 * from bucket_off at dhtgpu_rt_set time; only crafted uploads exceed it, onNewNode never does).
 * nb <= 256 and nn <= 2,048 hold throughout.  An insertion whose split would need a 257th bucket
 * gets DHTGPU_RTG_UNAPPLIED, and so does every insertion after it; the insertions before it stay
 * applied and the call returns DHTGPU_ERANGE.  A table grown by onNewNode from one bucket cannot
 * get there (at most 161 buckets, about 224 in client mode).  A bucket at depth 160 cannot split:
 * the node is FULL.
 *
 * Errors.  DHTGPU_ENOIDS before the first dhtgpu_rt_set.  A handle at or past the bound, or a
 * missing tail array on a table set with tails, gives DHTGPU_EINVAL with nothing applied. */
#define DHTGPU_RTG_NONE 0        /* no bucket (empty table) */
#define DHTGPU_RTG_KNOWN 1       /* handle already in the bucket */
#define DHTGPU_RTG_PLACED 2      /* inserted at the bucket's front */
#define DHTGPU_RTG_REPLACED 3    /* overwrote the first expired node (list order); aux = its handle */
#define DHTGPU_RTG_FULL 4        /* bucket full, node not inserted (the caller may cache it); aux = the ping pick */
#define DHTGPU_RTG_UNAPPLIED 5   /* past a limit, nothing done */
#define DHTGPU_RTG_MAX_HANDLE 65536u
/* flags bit0: RoutingTable::is_client.  ids20[m*20], handles[m], state[m] (nullable: every new node
 * good), node_tail[m*(alen+2)] (required iff the table was set with tails).  Applied in batch
 * order.  out_res[m] = DHTGPU_RTG_*; out_aux[m] (nullable) = the evicted handle (REPLACED), the
 * ping pick of a FULL bucket -- its first node in list order that is not good and has no pending
 * message; the library sends nothing -- or DHTGPU_NONE; out_stat[3] (nullable) = nb, nn and the
 * splits since the upload, after the call.  m == 0 is DHTGPU_OK and changes nothing.  Synchronous,
 * like dhtgpu_nc_insert; not to be called while rt calls are in flight (calls already issued on
 * other streams keep reading the table as it was: it is written to the other blob of a pair). */
int dhtgpu_rtg_on_new_node(dhtgpu_ctx* ctx, const uint8_t* ids20, const uint32_t* handles, const uint8_t* state,
                           const uint8_t* node_tail, uint32_t m, uint32_t flags, uint8_t* out_res, uint32_t* out_aux,
                           uint32_t* out_stat);
/* Dht::expireBuckets: every node whose state says expired leaves its bucket; the survivors keep
 * their order and the buckets stay.  out_handles (nullable; room for the nn before the call)
 * receives the removed handles in no particular order, *out_removed (nullable) their number.
 * Synchronous. */
int dhtgpu_rtg_expire(dhtgpu_ctx* ctx, uint32_t* out_handles, uint32_t* out_removed);
/* The state bytes: set_state gives every resident node with handle < nh the byte
 * state_by_handle[handle] (nh <= DHTGPU_RTG_MAX_HANDLE); update_state sets m of them (distinct
 * handles).  Stream-ordered on the context's stream like dhtgpu_rt_update_good, once the table is
 * in its grown form (the call that turns it synchronises). */
int dhtgpu_rtg_set_state(dhtgpu_ctx* ctx, const uint8_t* state_by_handle, uint32_t nh);
int dhtgpu_rtg_update_state(dhtgpu_ctx* ctx, const uint32_t* handles, const uint8_t* val, uint32_t m);
int dhtgpu_rtg_size(dhtgpu_ctx* ctx, uint32_t* out_nb, uint32_t* out_nn);
/* The resident table back on the host, each array nullable: firsts20[nb*20], bucket_off[nb+1],
 * and per node in bucket list order and in-bucket list order ids20[nn*20], handles[nn], state[nn]
 * -- the arguments of a dhtgpu_rt_set that would upload the same table.  Synchronous. */
int dhtgpu_rtg_export(dhtgpu_ctx* ctx, uint8_t* firsts20, uint32_t* bucket_off, uint8_t* ids20, uint32_t* handles,
                      uint8_t* state);

/* ---- K8w: the resident NodeCache ------------------------------------------------------------- */
/* NodeCache::NodeMap (include/opendht/node_cache.h:43: std::map<InfoHash, weak_ptr<Node>>) kept on
 * the device between calls and changed incrementally, so that a key heard of or dropped costs one
 * pass over the resident keys instead of an upload and a sort of the whole map, and
 * getCachedNodes (src/node_cache.cpp:42-74) crosses PCIe with its targets only.  One mirror per
 * context, private to the nc entry points: the k-NN id set, its accept mask, the dhtgpu_cache_*
 * mirror and the rt table are not touched, nor do they touch it.
 *
 * A key carries a HANDLE, the map's value: a u32 of the caller's choosing below
 * DHTGPU_NC_MAX_HANDLE (its slot number for the weak_ptr<Node>); a handle at or over the bound is
 * DHTGPU_EINVAL and nothing is applied; keeping handles unique is the caller's business.  The
 * ACCEPT bitmask is indexed by handle: a bit is 1 where lock() && !isExpired() && !isClient()
 * holds (src/node_cache.cpp:68-69).  It grows with the handles it is given (32 MB at the bound).
 *
 * dhtgpu_nc_set replaces the mirror with n keys in any order (sorted on the device; handles ==
 * NULL: key i has handle i); every handle given starts accepted, every other bit is cleared.
 * Duplicate keys return DHTGPU_EUNSORTED and leave the mirror invalid, as dhtgpu_cache_set does.
 * n == 0 is a valid, empty mirror. */
#define DHTGPU_NC_MAX_HANDLE (1u << 28)
int dhtgpu_nc_set(dhtgpu_ctx* ctx, const uint8_t* ids20, const uint32_t* handles, uint64_t n);
/* std::map::emplace (NodeMap::getNode, src/node_cache.cpp:99-111) for m keys, applied in batch
 * order: a key already in the map keeps its handle and its accept bit, of equal keys in the batch
 * the first wins; out_new[j] (nullable) = 1 where key j was inserted.  accept[m] (nullable: the
 * new keys are accepted) sets the accept bit of each inserted key's handle.  DHTGPU_ERANGE when
 * n + m >= 2^32 - 1.  dhtgpu_nc_erase is map.erase(key) (NodeMap::getNode(id) :87-97,
 * clearBadNodes :113-123) for m keys in batch order: out_found[j] (nullable) = 1 where key j was
 * erased -- 0 for an absent key and for a repeat of an earlier key of the batch; the handles' accept
 * bits are left as they are.  Both are synchronous (the new size comes back) and run one pass over
 * the resident keys, from one buffer set into the other, with geometric head-room; like
 * dhtgpu_rt_set they must not be issued while nc lookups are in flight. */
int dhtgpu_nc_insert(dhtgpu_ctx* ctx, const uint8_t* ids20, const uint32_t* handles, const uint8_t* accept,
                     uint32_t m, uint8_t* out_new);
int dhtgpu_nc_erase(dhtgpu_ctx* ctx, const uint8_t* ids20, uint32_t m, uint8_t* out_found);
/* The accept bits: bit handles[j] = val[j] != 0 for m handles (distinct; host arrays) /
 * bit h = accept_by_handle[h] != 0 for h < nh, the bits from nh on unchanged.  Both run on the
 * context's stream without synchronising it, like dhtgpu_rt_update_good / dhtgpu_rt_set_good;
 * handles past the mask's extent grow it (new bits are 0). */
int dhtgpu_nc_update_accept(dhtgpu_ctx* ctx, const uint32_t* handles, const uint8_t* val, uint32_t m);
int dhtgpu_nc_set_accept(dhtgpu_ctx* ctx, const uint8_t* accept_by_handle, uint32_t nh);
/* *out_n = the number of keys; the keys (out_ids20[n*20]) and their handles (out_handles[n]) in
 * lexicographic order, either nullable (tests; re-syncing an adapter). */
int dhtgpu_nc_size(dhtgpu_ctx* ctx, uint64_t* out_n);
int dhtgpu_nc_export(dhtgpu_ctx* ctx, uint8_t* out_ids20, uint32_t* out_handles);
/* NodeCache::getCachedNodes(target, af, count) (src/node_cache.cpp:42-74) for q targets over the
 * mirror and its current accept bits: out_handle[q*count] = the accepted keys' handles in the
 * reference's walk order (lower_bound, then the XOR-closer of the two neighbours at every step --
 * not sorted by distance), DHTGPU_NONE padded, out_cnt[q]; 1 <= count <= DHTGPU_MAX_K.  One wave
 * per target.  The _dev form takes target planes (any t_stride >= q) and device outputs, is
 * stream-ordered (NULL = the context's stream) and neither synchronises nor allocates.  Every nc
 * query returns DHTGPU_ENOIDS before the first dhtgpu_nc_set. */
int dhtgpu_nc_nodes_dev(dhtgpu_ctx* ctx, const uint32_t* t_planes, uint64_t t_stride, uint32_t q, uint32_t count,
                        uint32_t* out_handle, uint32_t* out_cnt, void* stream);
int dhtgpu_nc_nodes(dhtgpu_ctx* ctx, const uint8_t* targets20_be, uint32_t q, uint32_t count, uint32_t* out_handle,
                    uint32_t* out_cnt);

/* ---- K8r: keys to handles over the resident NodeCache ------------------------------------------ */
/* What NodeCache::NodeMap::getNode does per node (src/node_cache.cpp:87-111; called for every record
 * of every reply by NetworkEngine::deserializeNodes, src/network_engine.cpp:868, :884), in batches
 * over the K8w mirror, so that the key -> handle map lives in one place: the library resolves ids
 * to handles, emplaces the absent ones under handles drawn from the caller's free list, and says
 * which handle an erase freed.  The dhtgpu_nc_* entry points are unchanged, and these change the
 * mirror exactly as dhtgpu_nc_insert / dhtgpu_nc_erase do.  All four return DHTGPU_ENOIDS before
 * the first dhtgpu_nc_set; m == 0 is a no-op.
 *
 * dhtgpu_ncr_find is NodeMap::find (getNode(id) :87-97 without its erase of an expired entry):
 * out_handle[j] = the handle of key j, DHTGPU_NONE when the mirror does not hold it; out_accept[j]
 * (nullable) = the handle's current accept bit, 0 for an absent key.  Keys may repeat and come in
 * any order.  The host form synchronises.  The _dev form takes id word planes (any id_stride >= m,
 * the layout dhtgpu_srm_offer_dev takes) and device outputs, is stream-ordered (NULL = the
 * context's stream) and neither synchronises nor allocates: a lookup like dhtgpu_nc_nodes_dev,
 * under the same rule against dhtgpu_nc_insert / _erase (and _ncr_get_nodes / _extract) in flight.
 * Its handles can go straight to dhtgpu_sr_insert_dev / dhtgpu_srm_offer_dev. */
int dhtgpu_ncr_find(dhtgpu_ctx* ctx, const uint8_t* ids20, uint32_t m, uint32_t* out_handle, uint8_t* out_accept);
int dhtgpu_ncr_find_dev(dhtgpu_ctx* ctx, const uint32_t* id_planes, uint64_t id_stride, uint32_t m,
                        uint32_t* out_handle, uint8_t* out_accept, void* stream);
/* The emplace of NodeMap::getNode(id, addr, now, confirm, client) (src/node_cache.cpp:99-111) for m
 * keys in batch order.  A key already in the map: out_handle[j] = its handle, out_new[j] = 0, its
 * accept bit untouched.  An absent key at its first appearance takes free_handles[r], r = the
 * number of distinct absent keys before it in the batch: out_new[j] = 1, and the handle's accept
 * bit becomes accept ? accept[j] != 0 : 1.  A later repeat of that key: the same handle,
 * out_new[j] = 0, its accept byte ignored (the first wins, as in dhtgpu_nc_insert).  *out_used =
 * the free handles consumed.  out_new and out_used are nullable.  With more distinct absent keys
 * than nfree it returns DHTGPU_ERANGE with nothing applied -- *out_used = the number needed, the
 * other outputs unspecified.  DHTGPU_ERANGE also when n + m >= 2^32 - 1; a free handle >=
 * DHTGPU_NC_MAX_HANDLE is DHTGPU_EINVAL before any launch; distinct free handles, none of them in
 * use, are the caller's business.  Synchronous.  The mirror that results is the one
 * dhtgpu_nc_insert builds when given, for each key, the handle reported here. */
int dhtgpu_ncr_get_nodes(dhtgpu_ctx* ctx, const uint8_t* ids20, uint32_t m, const uint32_t* free_handles,
                         uint32_t nfree, const uint8_t* accept, uint32_t* out_handle, uint8_t* out_new,
                         uint32_t* out_used);
/* dhtgpu_nc_erase (map.erase(key): getNode(id) :87-97, clearBadNodes :113-123) that says what it
 * freed: out_handle[j] = the erased key's handle, DHTGPU_NONE for an absent key and for a repeat of
 * an earlier key of the batch.  Accept bits are left as they are.  Synchronous. */
int dhtgpu_ncr_extract(dhtgpu_ctx* ctx, const uint8_t* ids20, uint32_t m, uint32_t* out_handle);

/* ---- K10w: the resident searches --------------------------------------------------------------- */
/* The node lists of a node's searches (Dht::Search::nodes, src/search.h; up to MAX_SEARCHES = 16384)
 * kept on the device between calls, so that Search::insertNode (src/search.h:636-722) and a batch
 * of Dht::refill (src/dht.cpp:656-677) run with no list, node table or cache result crossing PCIe.
 * One search set per context, private to the sr entry points.  A search lives in a SLOT in
 * [0, nslots).  A list entry is {handle, 160-bit id, flags}: flags are bit0 candidate and bit1
 * replied, as in dhtgpu_search_insert, and the node's identity is its HANDLE -- the handle space of
 * dhtgpu_nc_*, below DHTGPU_NC_MAX_HANDLE; one handle per id is the caller's business, as it is
 * there.  A row holds DHTGPU_SR_CAP entries; host arrays of rows use that stride and DHTGPU_NONE
 * padding.  Every sr call but dhtgpu_sr_reset returns DHTGPU_ENOIDS before the first reset; a slot
 * >= nslots or a handle >= DHTGPU_NC_MAX_HANDLE in a host array is DHTGPU_EINVAL before any launch
 * (the _dev forms skip such a slot).
 *
 * Ordering: every sr call is ordered on the context's stream (the _dev forms on the stream they
 * are given); insert, refill, status and lists are stream-ordered against each other.  The host
 * forms that return data synchronise; reset, open, expire, set_candidate and the state setters do
 * not.  dhtgpu_nc_insert and dhtgpu_nc_erase stay synchronous and must not be issued while a
 * dhtgpu_sr_refill_dev is in flight on another stream.
 *
 * dhtgpu_sr_reset creates nslots empty searches (nslots <= 2^20, else DHTGPU_ERANGE) and drops any
 * earlier set and the state array.  dhtgpu_sr_open: a new Search in each listed slot -- target
 * set, list empty, expired = 0, overflow bit cleared.  dhtgpu_sr_expire: Search::expire()
 * (src/search.h:560-565), expired = 1 and the list cleared. */
#define DHTGPU_SR_CAP 64u
int dhtgpu_sr_reset(dhtgpu_ctx* ctx, uint32_t nslots);
int dhtgpu_sr_open(dhtgpu_ctx* ctx, const uint32_t* slots, const uint8_t* targets20, uint32_t m);
int dhtgpu_sr_expire(dhtgpu_ctx* ctx, const uint32_t* slots, uint32_t m);
/* Node state, one byte per handle: bit0 Node::isExpired(), bit1 Node::isRemovable(now) -- the
 * node_state of dhtgpu_search_insert, resident.  set replaces the array and its extent nh; update
 * writes m handles (distinct) and grows the array, new bytes 0.  A kernel reads a handle at or past
 * the extent as state 0 (the load is guarded).  Both run on the context's stream without
 * synchronising, like dhtgpu_nc_set_accept / dhtgpu_nc_update_accept. */
int dhtgpu_sr_set_state(dhtgpu_ctx* ctx, const uint8_t* state_by_handle, uint32_t nh);
int dhtgpu_sr_update_state(dhtgpu_ctx* ctx, const uint32_t* handles, const uint8_t* val, uint32_t m);
/* Dht::searchNodeGetExpired's srn->candidate = not over (src/dht.cpp:249-250) for m distinct
 * (slot, handle) pairs: the entry's candidate flag = val[j] != 0; a handle that is not in the
 * slot's list changes nothing. */
int dhtgpu_sr_set_candidate(dhtgpu_ctx* ctx, const uint32_t* slots, const uint32_t* handles, const uint8_t* val,
                            uint32_t m);
/* Search::insertNode (src/search.h:636-722) + removeExpiredNode (:541-551), one wave per search:
 * slot slots[j] takes insertions [ins_off[j], ins_off[j+1]) in order -- handle, id, token byte
 * (ins_token nullable: no tokens) -- and ins_added (nullable) gets insertNode's return values.  The
 * semantics are dhtgpu_search_insert's (trimming that pops the node which just carried a token
 * included), except that "the same node" means "the same handle".  The slots of one call are
 * distinct (host form: DHTGPU_EINVAL otherwise).  An insertion that would make a list longer than
 * DHTGPU_SR_CAP is dropped: the slot's overflow bit is set (until the slot is opened again), the
 * row stays a valid list and the slot's next insertions are applied; the host forms of insert and
 * refill then return DHTGPU_ERANGE after applying everything else, the _dev forms report it through
 * the status bit only.  _dev: every array on the device (ids as word planes, id_stride >= the number
 * of insertions), a stream (NULL = the context's); it neither synchronises nor allocates. */
int dhtgpu_sr_insert(dhtgpu_ctx* ctx, const uint32_t* slots, uint32_t m, const uint64_t* ins_off,
                     const uint32_t* ins_handle, const uint8_t* ins_ids20, const uint8_t* ins_token,
                     uint8_t* ins_added);
int dhtgpu_sr_insert_dev(dhtgpu_ctx* ctx, const uint32_t* slots, uint32_t m, const uint64_t* ins_off,
                         const uint32_t* ins_handle, const uint32_t* id_planes, uint64_t id_stride,
                         const uint8_t* ins_token, uint8_t* ins_added, void* stream);
/* Dht::refill (src/dht.cpp:656-677) for m searches in one launch: getCachedNodes(the slot's
 * target, count) over this context's nc mirror and its current accept bits -- the walk and the
 * walk order of dhtgpu_nc_nodes -- then insertNode(node, no token) for each result in that order;
 * out_inserted[j] = refill's return value.  1 <= count <= DHTGPU_MAX_K (the reference passes
 * SEARCH_NODES = 14); DHTGPU_ENOIDS without an nc mirror. */
int dhtgpu_sr_refill(dhtgpu_ctx* ctx, const uint32_t* slots, uint32_t m, uint32_t count, uint32_t* out_inserted);
int dhtgpu_sr_refill_dev(dhtgpu_ctx* ctx, const uint32_t* slots, uint32_t m, uint32_t count, uint32_t* out_inserted,
                         void* stream);
/* out4[j*4 ..] = {len, getNumberOfBadNodes, getNumberOfConsecutiveBadNodes (src/search.h:516-530,
 * isBad = expired state || candidate), bits: bit0 expired, bit1 overflowed} -- what searchStep's
 * expiry test (src/dht.cpp:641-642) reads. */
int dhtgpu_sr_status(dhtgpu_ctx* ctx, const uint32_t* slots, uint32_t m, uint32_t* out4);
int dhtgpu_sr_status_dev(dhtgpu_ctx* ctx, const uint32_t* slots, uint32_t m, uint32_t* out4, void* stream);
/* The rows, closest first (Search::getNodes order): out_handle[m * DHTGPU_SR_CAP], out_flags
 * (nullable, same shape), out_len[m] (nullable). */
int dhtgpu_sr_lists(dhtgpu_ctx* ctx, const uint32_t* slots, uint32_t m, uint32_t* out_handle, uint8_t* out_flags,
                    uint32_t* out_len);
int dhtgpu_sr_lists_dev(dhtgpu_ctx* ctx, const uint32_t* slots, uint32_t m, uint32_t* out_handle, uint8_t* out_flags,
                        uint32_t* out_len, void* stream);

/* ---- K10s: Dht::searchStep on the resident searches -------------------------------------------- */
/* Dht::searchStep (src/dht.cpp:562-654) for the search with no callbacks, announces or listeners --
 * the find_node search of bootstrap, maintenance and a crawl -- on the rows of dhtgpu_sr_*, one wave
 * per search.  The per-SearchNode state it reads travels with the entry through every insertion,
 * trim and removal of the sr and srm families:
 *   req    the net::Request state of getStatus[ANY_QUERY]: 0 none (erased, expired-and-over and
 *          cancelled alike), 1 pending, 2 completed
 *   tick   SearchNode::last_get_reply in the caller's clock ticks; 0 is time_point::min()
 * and per slot refill_tick, Search::refill_time (0: never).  A newly inserted entry has req 0 and
 * tick 0; dhtgpu_sr_open zeroes refill_tick.  The context holds a CLOCK, 0 until dhtgpu_srs_set_clock
 * (scheduler.time(); now == 0 is DHTGPU_ERANGE; no device work): from then on an insertion that
 * carries a token also sets the entry's tick to the clock (src/search.h:712-718) and every refill
 * sets refill_tick to it (src/dht.cpp:658).
 *
 * dhtgpu_srs_set_request: req = val[j] in {0, 1, 2} (else DHTGPU_EINVAL before any launch) for m
 * (slot, handle) pairs, with dhtgpu_sr_set_candidate's rules: an absent handle changes nothing,
 * stream-ordered, no synchronise.  2 is what the engine does before searchNodeGetDone, 0 is
 * searchNodeGetExpired's erase when over (src/dht.cpp:251-252).
 *
 * dhtgpu_srs_step, per listed search, with now = the clock and E = node_expire (ticks; sums in 64 bits):
 *   1. expired or done on entry: nothing changes, bit `skipped`
 *   2. refill_count != 0 && refill_tick + E < now && len - bad nodes < SEARCH_NODES: Dht::refill as
 *      dhtgpu_sr_refill(count = refill_count) runs it, then refill_tick = now
 *   3. Search::isSynced(now) (src/search.h:734-747) -- each of the first TARGET_NODES = 8 non-bad entries
 *      has replied and tick != 0 && tick + E >= now, and there is one -- then setDone(): done = 1, every
 *      req = 0, nothing is sent
 *   4. otherwise, while fewer than MAX_REQUESTED_SEARCH_NODES = 4 non-bad entries are pending, the
 *      first entry in list order with canGet (src/search.h:139-161 for the one query: the node not
 *      expired and req == 0, or req == 2 and (tick == 0 or now > tick + E)) gets req = 1 and its handle is
 *      appended to out_send[j]; a candidate entry is sent to and not counted
 *   5. leading bad nodes >= min(len, SEARCH_MAX_BAD_NODES = 25): Search::expire() (src/search.h:560-567) --
 *      expired = 1, the list cleared, done = 1.  (dhtgpu_sr_expire itself leaves done alone.)
 * out_send[m * DHTGPU_SR_CAP] rows are DHTGPU_NONE padded; out4[j*4 ..] = {sends, pending non-bad
 * entries after, nodes the refill inserted, bits: bit0 expired after, bit1 overflowed, bit2 done after,
 * bit3 refilled, bit4 synced, bit5 skipped}.  DHTGPU_EINVAL before the first dhtgpu_srs_set_clock.
 * refill_count 0 skips step 2 and needs no nc mirror; 1..DHTGPU_MAX_K needs one, else DHTGPU_ENOIDS.
 * Host form: the slots are distinct (DHTGPU_EINVAL otherwise); on a row overflow DHTGPU_ERANGE after
 * applying everything, as dhtgpu_sr_refill.  _dev: device arrays, a stream (NULL = the context's), a
 * slot >= nslots is skipped (its output rows are not written); neither synchronises nor allocates.
 *
 * dhtgpu_srs_entries: out_req / out_tick [m * DHTGPU_SR_CAP] (either nullable), 0 past a row's end. */
int dhtgpu_srs_set_clock(dhtgpu_ctx* ctx, uint32_t now);
int dhtgpu_srs_set_request(dhtgpu_ctx* ctx, const uint32_t* slots, const uint32_t* handles, const uint8_t* val,
                           uint32_t m);
int dhtgpu_srs_step(dhtgpu_ctx* ctx, const uint32_t* slots, uint32_t m, uint32_t node_expire, uint32_t refill_count,
                    uint32_t* out_send, uint32_t* out4);
int dhtgpu_srs_step_dev(dhtgpu_ctx* ctx, const uint32_t* slots, uint32_t m, uint32_t node_expire,
                        uint32_t refill_count, uint32_t* out_send, uint32_t* out4, void* stream);
int dhtgpu_srs_entries(dhtgpu_ctx* ctx, const uint32_t* slots, uint32_t m, uint8_t* out_req, uint32_t* out_tick);
int dhtgpu_srs_entries_dev(dhtgpu_ctx* ctx, const uint32_t* slots, uint32_t m, uint8_t* out_req, uint32_t* out_tick,
                           void* stream);

/* ---- K10m:Dht::trySearchInsert over the searches' ordered map ---------------------------------- */
/* Dht::trySearchInsert (src/dht.cpp:118-150) for a batch of learned nodes over the resident searches
 * of dhtgpu_sr_*: the reference's searches(af) -- a std::map by target -- is the MAP, a set of slots
 * the library keeps in ascending order of their targets.  For node j of a batch, each taken strictly
 * after node j - 1: c = lower_bound(map, id_j); forward over c, c + 1, ... and then backward over
 * c - 1, c - 2, ...: insertNode(node_j, no token) on the search -- exactly dhtgpu_sr_insert's -- and
 * stop when it returns false on a search that is neither expired (read after the call) nor done.
 *
 * dhtgpu_srm_set: the map is these ns slots, in any order; their targets are gathered and sorted on
 * the device (the 160-bit radix sort of the cache mirror).  A repeated slot or a slot >= nslots is
 * DHTGPU_EINVAL; two slots with equal targets are DHTGPU_EUNSORTED and leave the map invalid; ns = 0
 * is a valid, empty map.  It synchronises.  The map is dropped by dhtgpu_sr_reset and by every
 * dhtgpu_sr_open (a slot's target may have changed); dhtgpu_sr_expire keeps it, as an expired search
 * stays in the reference's map.  offer and export return DHTGPU_ENOIDS without a valid map.
 *
 * dhtgpu_srm_set_done: Search::done of slot slots[j] = val[j] != 0, kept by the slot until it is
 * opened again (a new search is not done); stream-ordered, no synchronise, like
 * dhtgpu_sr_set_candidate.  dhtgpu_sr_status does not report it; dhtgpu_srm_export does.
 *
 * dhtgpu_srm_offer: out_cnt[j] = the number of searches that took node j (trySearchInsert's return
 * value is out_cnt[j] > 0); out_touched (nullable) = a bitmask by slot, ceil(nslots / 32) words,
 * zeroed by the call, a bit set where the slot took at least one node of the batch -- the searches
 * whose next step the caller reschedules; out_stats[4] (nullable) = {nodes answered by the filter
 * without a walk, insertNode calls of the walk, 1 when the batch held a node that is removable and
 * not expired (then no node is filtered), 1 when a row overflowed}.  m = 0 is a no-op.  The host
 * form synchronises and returns DHTGPU_ERANGE after applying everything when a row overflowed, as
 * dhtgpu_sr_insert does; a handle >= DHTGPU_NC_MAX_HANDLE is DHTGPU_EINVAL before any launch.  _dev:
 * every array on the device (ids as word planes, id_stride >= m), a stream (NULL = the context's);
 * it neither synchronises nor allocates and reports overflow through the slots' status bits.  The
 * offers of a context share its work arrays: they are ordered on one stream, or by the caller.
 *
 * dhtgpu_srm_export: the map in target order, out_slots[ns] and out_done[ns] (both nullable; sized
 * by the caller for the ns of the last set), *out_ns = ns.  It synchronises. */
int dhtgpu_srm_set(dhtgpu_ctx* ctx, const uint32_t* slots, uint32_t ns);
int dhtgpu_srm_set_done(dhtgpu_ctx* ctx, const uint32_t* slots, const uint8_t* val, uint32_t m);
int dhtgpu_srm_offer(dhtgpu_ctx* ctx, const uint32_t* handles, const uint8_t* ids20, uint32_t m, uint32_t* out_cnt,
                     uint32_t* out_touched, uint32_t* out_stats);
int dhtgpu_srm_offer_dev(dhtgpu_ctx* ctx, const uint32_t* handles, const uint32_t* id_planes, uint64_t id_stride,
                         uint32_t m, uint32_t* out_cnt, uint32_t* out_touched, uint32_t* out_stats, void* stream);
int dhtgpu_srm_export(dhtgpu_ctx* ctx, uint32_t* out_slots, uint8_t* out_done, uint32_t* out_ns);

/* ---- K2: routing-bucket classification over the context's id set -------------- */
/* out_bucket[n] (nullable) = findBucket(id) index; hist161[161] = histogram of
 * commonBits(id, myid).  nb in [1, 256], firsts sorted ascending (as in the table). */
int dhtgpu_classify(dhtgpu_ctx* ctx, uint32_t nb, const uint8_t* firsts20,
                    const uint8_t* myid20, uint8_t* out_bucket, uint64_t* hist161);
int dhtgpu_classify_dev(const uint32_t* planes, uint64_t stride, uint64_t n, uint32_t nb,
                        const uint32_t* d_first_planes /* 5*nb, word-major */,
                        const uint32_t* myid_words /* host, 5 words */, uint8_t* out_bucket,
                        unsigned long long* d_hist161, void* stream);

/* ---- a8: NodeCache::getCachedNodes walk over the context's id set --------------------- */
/* accept[n] (nullable = all) = lock() && !isExpired() && !isClient().  Output in
 * the reference's walk order (not sorted), indices into the id set.  An id set uploaded
 * unsorted is sorted on the device on the first call (f2: LSD radix over the 160-bit keys,
 * kept until the set changes); DHTGPU_EUNSORTED if it holds duplicate ids. */
int dhtgpu_cached_nodes(dhtgpu_ctx* ctx, const uint8_t* accept, const uint8_t* targets20_be,
                        uint32_t q, uint32_t count, uint32_t* out_idx, uint32_t* out_cnt);

/* ---- f2: the NodeCache mirror (a second, context-private id set) ------------------------ */
/* NodeCache::NodeMap (include/opendht/node_cache.h:43: std::map<InfoHash, weak_ptr<Node>>,
 * src/node_cache.cpp:42-74) as n unique 20-byte keys in the CALLER's order (e.g. a walk of
 * the map, or any order): sorted lexicographically on the device; it does not touch the
 * context's k-NN id set.  version != 0 equal to the last upload's (same n) skips the upload:
 * the caller bumps it whenever the map changes.  DHTGPU_EUNSORTED on duplicate keys. */
int dhtgpu_cache_set(dhtgpu_ctx* ctx, const uint8_t* ids20, uint64_t n, uint64_t version);
/* getCachedNodes(target, af, count) for q targets over the mirror: accept[n] (nullable) and
 * the output indices are in the caller's order of the last dhtgpu_cache_set. */
int dhtgpu_cache_nodes(dhtgpu_ctx* ctx, const uint8_t* accept, const uint8_t* targets20_be, uint32_t q,
                       uint32_t count, uint32_t* out_idx, uint32_t* out_cnt);
/* The mirror's lexicographic order: perm[j] = caller index of the j-th smallest key. */
int dhtgpu_cache_sorted(dhtgpu_ctx* ctx, uint32_t* perm);

/* ---- a6: RoutingTable::depth (src/routing_table.cpp:100-107) over a table snapshot ---- */
/* *out_depth = max(lowbit(first[b]), lowbit(first[b+1])) + 1 (0 for an empty table);
 * table_depth of Dht::getNodesStats (src/dht.cpp:1425-1444) is depth(findBucket(myid)). */
int dhtgpu_table_depth(uint32_t nb, const uint8_t* firsts20, uint32_t b, uint32_t* out_depth);

/* ---- a11 / f4: compact node wire format ---------------------------------------------- */
/* NetworkEngine::bufferNodes(af, id, nodes) (src/network_engine.cpp:1003-1032), batched:
 * for each target, its candidates cand[qi*c .. +c) (indices into the context's id set,
 * DHTGPU_NONE = absent, c <= 64) are sorted by InfoHash::xorCmp to the target, the first
 * SEND_NODES = 8 are kept and written as 26-byte (af 4) / 38-byte (af 6) records
 * id || address || port to out[qi * 8 * rec ..]; out_len[qi] = bytes written.
 * node_tail[i*(alen+2)] = node i's address || port bytes as its sockaddr holds them
 * (network order), alen = 4 / 16.  Equal ids (never in OpenDHT) keep candidate order.
 * Every candidate must be DHTGPU_NONE or < the number of ids: the host form returns
 * DHTGPU_EINVAL otherwise; the _dev form does not check (device pointers). */
int dhtgpu_buffer_nodes_dev(dhtgpu_ctx* ctx, const uint8_t* node_tail, uint32_t af, const uint32_t* t_planes,
                            uint64_t t_stride, uint32_t q, const uint32_t* cand, uint32_t c, uint8_t* out,
                            uint32_t* out_len, void* stream);
int dhtgpu_buffer_nodes(dhtgpu_ctx* ctx, const uint8_t* node_tail, uint32_t af, const uint8_t* targets20,
                        uint32_t q, const uint32_t* cand, uint32_t c, uint8_t* out, uint32_t* out_len);
/* The same over the caller's own nodes: cand indexes node_ids20[nn * 20] / node_tail (the
 * context's id set is not used or changed). */
int dhtgpu_buffer_nodes_ids(dhtgpu_ctx* ctx, const uint8_t* node_ids20, const uint8_t* node_tail, uint32_t nn,
                            uint32_t af, const uint8_t* targets20, uint32_t q, const uint32_t* cand, uint32_t c,
                            uint8_t* out, uint32_t* out_len);
/* NetworkEngine::deserializeNodes (src/network_engine.cpp:849-887), batched over m received
 * n4 (af 4) / n6 (af 6) blobs: message i is blob[msg_off[i] .. msg_off[i+1]), received from
 * from_addr[i*16 ..] (family from_af[i]: 4, 6 or 0).  msg_status[i] = 1 when its length is
 * not a whole number of records (the reference's WRONG_NODE_INFO_BUF_LEN; none of its
 * records is decoded), else 0.  Every record of the other messages is decoded, in order,
 * into out_ids20 / out_tail (address || port after the loopback -> sender rewrite) and
 * out_status: 0 accepted, 1 own id (myid20), 2 martian (NetworkEngine::isMartian).
 * *out_nrec = records decoded (<= msg_off[m] / rec); isNodeBlacklisted stays with the
 * caller. */
int dhtgpu_deserialize_nodes(dhtgpu_ctx* ctx, uint32_t af, const uint8_t* myid20, const uint8_t* blob,
                             const uint64_t* msg_off, uint32_t m, const uint8_t* from_af, const uint8_t* from_addr,
                             uint8_t* out_ids20, uint8_t* out_tail, uint8_t* out_status, uint8_t* msg_status,
                             uint32_t* out_nrec);

/* ---- a10: Dht::Search::insertNode (src/search.h:636-722), batched ------------------------ */
/* q searches (targets20[q]): search s holds list_len[s] <= cap SearchNodes list_node[s*cap ..]
 * (indices into node_ids20[nn * 20], closest first) with list_flags (bit0 candidate, bit1
 * replied) and search_expired[s] (Search::expired).  Its insertions ins_node[ins_off[s] ..
 * ins_off[s+1]) (ins_token != 0: the node replied with a token) are applied in order with the
 * reference's ordering, trimming to SEARCH_NODES = 14 non-bad nodes (isBad = isExpired() ||
 * candidate, :352-354) and removeExpiredNode (:541-551); ins_added = insertNode's result.
 * node_state[nn]: bit0 Node::isExpired(), bit1 Node::isRemovable(now) (node.h:87-89), a
 * snapshot like the good mask of dhtgpu_find_closest.  Lists are updated in place;
 * DHTGPU_ERANGE if a list would outgrow cap (that insertion is dropped). */
int dhtgpu_search_insert(dhtgpu_ctx* ctx, const uint8_t* node_ids20, const uint8_t* node_state, uint32_t nn,
                         const uint8_t* targets20, uint32_t q, uint32_t cap, uint32_t* list_node, uint8_t* list_flags,
                         uint32_t* list_len, uint8_t* search_expired, const uint64_t* ins_off, const uint32_t* ins_node,
                         const uint8_t* ins_token, uint8_t* ins_added);

/* ---- a4 / a6: InfoHash::lowbit (infohash.h:132-143) + RoutingTable::depth per bucket ------ */
/* out_lowbit[b] = lowbit(first[b]) (-1 for the zero id), out_depth[b] = depth of bucket b
 * (src/routing_table.cpp:100-107) for every bucket of a table snapshot, on the device. */
int dhtgpu_table_stats(dhtgpu_ctx* ctx, uint32_t nb, const uint8_t* firsts20, int32_t* out_lowbit, uint32_t* out_depth);

/* ---- f3: crawl replay (BASELINE configs[4]) -------------------------------------------- */
/* The context's id set becomes a synthetic network (model: opendht_amd/csrc/crawl.hip and
 * oracle/crawl_oracle.cpp): node order by (first word, index), implicit k-bucket routing
 * tables sampled with table_seed, dead[n] (host, nullable) marks nodes that never answer.
 * Synchronous. */
int dhtgpu_net_prepare(dhtgpu_ctx* ctx, const uint8_t* dead, uint64_t table_seed);
/* One iterative search per target (Dht::Search, src/search.h: Search::insertNode :636-722,
 * SEARCH_NODES = 14, MAX_REQUESTED_SEARCH_NODES = 4 per round, isSynced :734-747), started
 * by node searchers[qi] from its own routing table.  Per search: the final SearchNode list
 * out_idx[qi*64 ..] (node indices, DHTGPU_NONE padded) with out_flags (bit0 asked, bit1
 * replied, bit2 bad), out_len, rounds run and find_node requests sent. */
int dhtgpu_search_batch(dhtgpu_ctx* ctx, const uint8_t* targets20, uint32_t q, const uint32_t* searchers,
                        uint32_t max_rounds, uint32_t* out_idx, uint8_t* out_flags, uint32_t* out_len,
                        uint32_t* out_rounds, uint32_t* out_queries);
/* Requests a search sends per round (alpha, 1..8) for the following search_batch calls on this
 * context: default 4 = MAX_REQUESTED_SEARCH_NODES (include/opendht/dht.h:321); BASELINE cfg 5
 * states a 3-way alpha. */
int dhtgpu_set_search_alpha(dhtgpu_ctx* ctx, uint32_t alpha);
int dhtgpu_search_batch_dev(dhtgpu_ctx* ctx, const uint32_t* t_planes, uint64_t t_stride, uint32_t q,
                            const uint32_t* searchers, uint32_t max_rounds, uint32_t* out_idx, uint8_t* out_flags,
                            uint32_t* out_len, uint32_t* out_rounds, uint32_t* out_queries, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DHTGPU_H */
