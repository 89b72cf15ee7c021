/*
 * dhtgpu.hpp -- C++11 host adapter over the libdhtgpu C ABI (dhtgpu.h).
 *
 * Drop-in helpers with the reference's signatures and result shapes
 * (paths relative to the OpenDHT tree):
 *
 *   findClosestNodes(ctx, table, id, now, count)          <- RoutingTable::findClosestNodes
 *       (include/opendht/routing_table.h:56, src/routing_table.cpp:110-150)
 *   findClosestNodesBatch(ctx, table, targets, q, now, k)  new batched form (one launch)
 *   getCachedNodes(ctx, map, id, count)                    <- NodeCache::getCachedNodes
 *       (include/opendht/node_cache.h:31, src/node_cache.cpp:42-74)
 *   ClosestIndex                                           flat exact k-NN over a fixed id
 *       set: std::partial_sort(.., InfoHash::xorCmp) (include/opendht/infohash.h:179-194)
 *   bufferNodesBatch(ctx, af6, targets, nodes)             <- NetworkEngine::bufferNodes
 *       (src/network_engine.cpp:1003-1032), batched
 *   ResidentTable                                          the RoutingTable kept on the device:
 *       replyNodesBatch      <- Dht::onFindNode / onGetValues (src/dht.cpp:2128-2161):
 *                               findClosestNodes(target, now, 8) + bufferNodes, fused
 *       closerThanSelfBatch  <- the closeness tests of Dht::maintainStorage (src/dht.cpp:1862-1879)
 *                               and Dht::onAnnounce (:2293-2294)
 *   ResidentCache                                          NodeCache's map kept on the device and
 *       changed incrementally (NodeMap::getNode / clearBadNodes, src/node_cache.cpp:87-123):
 *       getCachedNodesBatch  <- NodeCache::getCachedNodes (src/node_cache.cpp:42-74)
 *
 * The templates are written against the reference's member names only -- a table is a
 * list of buckets with `.first` (InfoHash) and `.nodes` (list of Sp<Node>); a node has
 * `.id`, `isGood(now)`, `isExpired()`, `isClient()`; an InfoHash exposes `data()` (20
 * big-endian bytes) -- so they compile against dht::RoutingTable / NodeCache's map
 * without including OpenDHT headers here.
 *
 * Behaviour: results are identical to the reference (same nodes, same order).  On a
 * device error the helpers throw dhtgpu::Error; they never return different nodes.
 * The caller (single dht_thread, src/dhtrunner.cpp:115-150) owns the Context.
 *
 * Dispatch: a device call costs a fixed ~90 µs (snapshot + PCIe + launches) against
 * ~0.13 µs per findClosestNodes on one CPU core (bench.py find_closest / cpu_baseline), so
 * the helpers answer on the host -- the same walk as the reference body -- below
 * Context::min_device_batch targets (default kMinDeviceBatch = 1024, above the measured
 * crossover of ~740) and only larger batches go to the device.  A single call is therefore
 * as fast as the reference's own (tests/cpp/adapter_check.cpp reports both).  ResidentTable
 * keeps the table on the device, which halves the fixed cost; its thresholds (kMinResidentBatch,
 * kMinResidentReplyBatch) are lower accordingly.
 */
#ifndef DHTGPU_HPP
#define DHTGPU_HPP

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <iterator>
#include <map>
#include <memory>
#include <stdexcept>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

#include "dhtgpu.h"

namespace dhtgpu {

class Error : public std::runtime_error {
public:
    Error(int code, const char* what)
        : std::runtime_error(std::string("libdhtgpu: ") + what + ": " + dhtgpu_strerror(code)), code_(code) {}
    int code() const { return code_; }
private:
    int code_;
};

inline void check(int code, const char* what) {
    if (code != DHTGPU_OK) throw Error(code, what);
}

/* Batches below this many targets are answered on the host (see Dispatch above). */
static const size_t kMinDeviceBatch = 1024;

/* RAII owner of one device context. */
class Context {
public:
    explicit Context(int device = 0) : ctx_(nullptr) { check(dhtgpu_ctx_create(device, &ctx_), "ctx_create"); }
    ~Context() { dhtgpu_ctx_destroy(ctx_); }
    Context(const Context&) = delete;
    Context& operator=(const Context&) = delete;
    dhtgpu_ctx* get() const { return ctx_; }
    size_t min_device_batch = kMinDeviceBatch;   // smallest batch sent to the device
    uint64_t cache_version_ = 0;   // NodeCache mirror: version and size of the last upload
    size_t cache_size_ = 0;
private:
    dhtgpu_ctx* ctx_;
};

namespace detail {
template <class H>
inline void put_id(std::vector<uint8_t>& out, const H& h) {
    const uint8_t* p = h.data();
    out.insert(out.end(), p, p + DHTGPU_HASH_LEN);
}

/* a node's address || port bytes as its sockaddr holds them (network order): the tail of a
 * bufferNodes record (src/network_engine.cpp:1016-1027) */
template <class NodeT>
inline void put_tail(std::vector<uint8_t>& out, const NodeT& nd, bool af_inet6) {
    const uint8_t* a;
    const uint8_t* p;
    size_t alen;
    if (af_inet6) {
        const auto& sin6 = nd.getAddr().getIPv6();
        a = reinterpret_cast<const uint8_t*>(&sin6.sin6_addr);
        p = reinterpret_cast<const uint8_t*>(&sin6.sin6_port);
        alen = 16;
    } else {
        const auto& sin = nd.getAddr().getIPv4();
        a = reinterpret_cast<const uint8_t*>(&sin.sin_addr);
        p = reinterpret_cast<const uint8_t*>(&sin.sin_port);
        alen = 4;
    }
    out.insert(out.end(), a, a + alen);
    out.insert(out.end(), p, p + 2);
}

/* A node's state byte for dhtgpu_rtg_*: bit 0 isGood(now), bit 1 isExpired(), bit 2
 * isPendingMessage().  A node type without the last two (a snapshot-only caller's) gives bit 0. */
template <class NodeT, class TimePoint>
inline auto node_state(const NodeT& n, TimePoint now, int)
    -> decltype((void)n.isExpired(), (void)n.isPendingMessage(), uint8_t()) {
    return (uint8_t)((n.isGood(now) ? 1 : 0) | (n.isExpired() ? 2 : 0) | (n.isPendingMessage() ? 4 : 0));
}
template <class NodeT, class TimePoint>
inline uint8_t node_state(const NodeT& n, TimePoint now, long) {
    return n.isGood(now) ? 1 : 0;
}

/* InfoHash::xorCmp(a, b) < 0 for target t (include/opendht/infohash.h:179-194): at the first
 * byte where a and b differ, the one whose byte XOR t's is smaller is closer. */
inline bool xor_closer(const uint8_t* t, const uint8_t* a, const uint8_t* b) {
    for (unsigned i = 0; i < DHTGPU_HASH_LEN; ++i)
        if (a[i] != b[i]) return (uint8_t)(a[i] ^ t[i]) < (uint8_t)(b[i] ^ t[i]);
    return false;
}

/* The reference's findClosestNodes walk on the host (src/routing_table.cpp:110-150): the
 * target's bucket (findBucket, :153-166: the last whose first <= id), then one bucket on each
 * side per round until `count` good nodes are held, each inserted in xorCmp order. */
template <class Table, class HashT, class TimePoint, class NodePtr>
void find_closest_host(const Table& table, const HashT& id, TimePoint now, size_t count, std::vector<NodePtr>& nodes) {
    nodes.clear();
    const auto begin = table.begin(), end = table.end();
    if (begin == end) return;
    const uint8_t* t = id.data();
    auto b = begin;
    for (;;) {
        auto nx = std::next(b);
        if (nx == end || std::memcmp(t, nx->first.data(), DHTGPU_HASH_LEN) < 0) break;
        b = nx;
    }
    auto insert_bucket = [&](const decltype(*begin)& bk) {
        for (const auto& n : bk.nodes) {
            if (!n->isGood(now)) continue;
            auto here = std::find_if(nodes.begin(), nodes.end(), [&](const NodePtr& o) {
                return xor_closer(t, n->id.data(), o->id.data());
            });
            nodes.insert(here, n);
        }
    };
    auto itn = b;
    auto itp = b == begin ? end : std::prev(b);
    while (nodes.size() < count && (itn != end || itp != end)) {
        if (itn != end) { insert_bucket(*itn); ++itn; }
        if (itp != end) { insert_bucket(*itp); itp = itp == begin ? end : std::prev(itp); }
    }
    if (nodes.size() > count) nodes.resize(count);
}

/* The reference's getCachedNodes walk on the host (src/node_cache.cpp:42-74): out of
 * lower_bound(id), each step takes the XOR-closer of the two neighbours; accepted = lock()
 * succeeds && !isExpired() && !isClient().  O(log N + visited) -- no pass over the map. */
template <class NodeMap, class HashT>
std::vector<std::shared_ptr<typename NodeMap::mapped_type::element_type>>
cached_nodes_host(const NodeMap& c, const HashT& id, size_t count) {
    std::vector<std::shared_ptr<typename NodeMap::mapped_type::element_type>> res;
    const uint8_t* t = id.data();
    auto it_n = c.lower_bound(id);
    auto it_p = it_n;
    const auto end = c.cend();
    auto dec = [&](decltype(it_p)& it) {   // cbegin() -> cend(), else prev()
        auto ret = it;
        it = it == c.cbegin() ? end : std::prev(it);
        return ret;
    };
    if (!c.empty()) dec(it_p);
    while (res.size() < count && (it_n != end || it_p != end)) {
        decltype(it_n) it;
        if (it_p == end) it = it_n++;
        else if (it_n == end) it = dec(it_p);
        else it = xor_closer(t, it_p->first.data(), it_n->first.data()) ? dec(it_p) : it_n++;
        if (auto n = it->second.lock())
            if (!n->isExpired() && !n->isClient()) res.push_back(n);
    }
    return res;
}
/* The find_node / get reply on the host: findClosestNodes(id, now, 8) (already in xorCmp order,
 * so bufferNodes' sort keeps it) packed as id || address || port records. */
template <class Table, class HashT, class TimePoint>
std::vector<uint8_t> reply_nodes_host(const Table& table, const HashT& id, TimePoint now, bool af_inet6) {
    typedef typename std::decay<decltype(*table.begin()->nodes.begin())>::type NodePtr;
    std::vector<NodePtr> nodes;
    find_closest_host(table, id, now, 8, nodes);
    std::vector<uint8_t> out;
    out.reserve(nodes.size() * (af_inet6 ? 38 : 26));
    for (const auto& n : nodes) {
        put_id(out, n->id);
        put_tail(out, *n, af_inet6);
    }
    return out;
}

/* findClosestNodes(id, now, count) holds at least max(min_nodes, 1) nodes and
 * id.xorCmp(nodes.back()->id, myid) < 0 (src/dht.cpp:1862-1879, :2293-2294). */
template <class Table, class HashT, class TimePoint>
bool closer_than_self_host(const Table& table, const HashT& id, TimePoint now, size_t count, size_t min_nodes,
                           const uint8_t* myid) {
    typedef typename std::decay<decltype(*table.begin()->nodes.begin())>::type NodePtr;
    std::vector<NodePtr> nodes;
    find_closest_host(table, id, now, count, nodes);
    return nodes.size() >= (min_nodes ? min_nodes : 1) && xor_closer(id.data(), nodes.back()->id.data(), myid);
}
}  // namespace detail

/* Snapshot of a RoutingTable at time `now`: bucket firsts, per-bucket node ranges,
 * node ids, the isGood(now) mask, and the node handles to map indices back. */
template <class Table, class TimePoint>
struct TableSnapshot {
    typedef typename std::decay<decltype(*std::declval<const Table&>().begin()->nodes.begin())>::type NodePtr;
    std::vector<uint8_t> firsts, ids, good;
    std::vector<uint32_t> off;
    std::vector<NodePtr> nodes;

    TableSnapshot(const Table& table, TimePoint now) {
        for (const auto& b : table) {
            detail::put_id(firsts, b.first);
            off.push_back((uint32_t)nodes.size());
            for (const auto& n : b.nodes) {
                detail::put_id(ids, n->id);
                good.push_back(n->isGood(now) ? 1 : 0);
                nodes.push_back(n);
            }
        }
        off.push_back((uint32_t)nodes.size());
    }
    uint32_t nbuckets() const { return (uint32_t)(firsts.size() / DHTGPU_HASH_LEN); }
};

/* RoutingTable::findClosestNodes for a batch of targets (one device launch). */
template <class Table, class HashT, class TimePoint>
std::vector<std::vector<typename TableSnapshot<Table, TimePoint>::NodePtr>>
findClosestNodesBatch(Context& ctx, const Table& table, const HashT* targets, size_t q, TimePoint now,
                      size_t count) {
    typedef typename TableSnapshot<Table, TimePoint>::NodePtr NodePtr;
    std::vector<std::vector<NodePtr>> res(q);
    if (q == 0 || count == 0) return res;
    if (q < ctx.min_device_batch || count > DHTGPU_MAX_K) {   // the host walk (Dispatch)
        for (size_t i = 0; i < q; ++i) detail::find_closest_host(table, targets[i], now, count, res[i]);
        return res;
    }
    TableSnapshot<Table, TimePoint> snap(table, now);
    std::vector<uint8_t> t;
    t.reserve(q * DHTGPU_HASH_LEN);
    for (size_t i = 0; i < q; ++i) detail::put_id(t, targets[i]);
    std::vector<uint32_t> idx(q * count), cnt(q);
    check(dhtgpu_find_closest(ctx.get(), snap.nbuckets(), snap.firsts.data(), snap.off.data(),
                              snap.ids.empty() ? nullptr : snap.ids.data(),
                              snap.good.empty() ? nullptr : snap.good.data(), t.data(), (uint32_t)q,
                              (uint32_t)count, idx.data(), cnt.data()),
          "find_closest");
    for (size_t i = 0; i < q; ++i) {
        res[i].reserve(cnt[i]);
        for (uint32_t r = 0; r < cnt[i]; ++r) res[i].push_back(snap.nodes[idx[i * count + r]]);
    }
    return res;
}

/* Drop-in for RoutingTable::findClosestNodes(id, now, count): one target is always below
 * the device threshold, so this is the host walk (the reference's cost, no snapshot). */
template <class Table, class HashT, class TimePoint>
std::vector<typename TableSnapshot<Table, TimePoint>::NodePtr>
findClosestNodes(Context& ctx, const Table& table, const HashT& id, TimePoint now, size_t count = 8) {
    if (ctx.min_device_batch > 1) {
        std::vector<typename TableSnapshot<Table, TimePoint>::NodePtr> res;
        detail::find_closest_host(table, id, now, count, res);
        return res;
    }
    return std::move(findClosestNodesBatch(ctx, table, &id, 1, now, count)[0]);
}

/* NodeCache::getCachedNodes over one address family's map (std::map<InfoHash, weak_ptr<Node>>,
 * include/opendht/node_cache.h:43, src/node_cache.cpp:42-74), batched.  The map's keys go to
 * the context's NodeCache mirror (dhtgpu_cache_set: a set of its own, sorted on the device --
 * the context's k-NN id set is not touched); `version` != 0 equal to the previous call's skips
 * that upload (the caller bumps it whenever the map changes).  Accepted = lock() succeeds &&
 * !isExpired() && !isClient(), evaluated at call time; walk order preserved. */
template <class NodeMap, class HashT>
void getCachedNodesRaw(Context& ctx, const NodeMap& map, const HashT* targets, size_t q, size_t count,
                       std::vector<std::shared_ptr<typename NodeMap::mapped_type::element_type>>& locked,
                       std::vector<std::vector<uint32_t>>& out, uint64_t version = 0) {
    std::vector<uint8_t> ids, accept;
    const bool upload = version == 0 || version != ctx.cache_version_ || map.size() != ctx.cache_size_;
    if (upload) ids.reserve(map.size() * DHTGPU_HASH_LEN);
    locked.clear();
    accept.reserve(map.size());
    for (const auto& kv : map) {
        if (upload) detail::put_id(ids, kv.first);
        auto n = kv.second.lock();
        accept.push_back(n && !n->isExpired() && !n->isClient() ? 1 : 0);
        locked.push_back(n);
    }
    if (upload) {
        check(dhtgpu_cache_set(ctx.get(), ids.empty() ? nullptr : ids.data(), map.size(), version), "cache_set");
        ctx.cache_version_ = version;
        ctx.cache_size_ = map.size();
    }
    std::vector<uint8_t> t;
    for (size_t i = 0; i < q; ++i) detail::put_id(t, targets[i]);
    std::vector<uint32_t> idx(q * count), cnt(q);
    out.assign(q, std::vector<uint32_t>());
    if (q == 0) return;
    check(dhtgpu_cache_nodes(ctx.get(), accept.empty() ? nullptr : accept.data(), t.data(), (uint32_t)q,
                             (uint32_t)count, idx.data(), cnt.data()),
          "cache_nodes");
    for (size_t i = 0; i < q; ++i) out[i].assign(idx.begin() + i * count, idx.begin() + i * count + cnt[i]);
}

/* NodeCache::getCachedNodes for a batch of targets.  The device path walks the map once per
 * batch (the accept mask is evaluated at call time, as the reference does per visited entry),
 * so it is taken only when the batch is large against the map (q >= min_device_batch and
 * q >= map.size() / 8: the walk then costs less than 8 entries per target); otherwise each
 * target takes the host walk, O(log N + count). */
template <class NodeMap, class HashT>
std::vector<std::vector<std::shared_ptr<typename NodeMap::mapped_type::element_type>>>
getCachedNodesBatch(Context& ctx, const NodeMap& map, const HashT* targets, size_t q, size_t count,
                    uint64_t version = 0) {
    std::vector<std::vector<std::shared_ptr<typename NodeMap::mapped_type::element_type>>> res(q);
    if (q == 0 || count == 0) return res;
    if (q < ctx.min_device_batch || q < map.size() / 8 || count > DHTGPU_MAX_K) {
        for (size_t i = 0; i < q; ++i) res[i] = detail::cached_nodes_host(map, targets[i], count);
        return res;
    }
    std::vector<std::shared_ptr<typename NodeMap::mapped_type::element_type>> locked;
    std::vector<std::vector<uint32_t>> out;
    getCachedNodesRaw(ctx, map, targets, q, count, locked, out, version);
    for (size_t i = 0; i < q; ++i)
        for (uint32_t j : out[i]) res[i].push_back(locked[j]);
    return res;
}

/* Drop-in for NodeCache::getCachedNodes(id, af, count): one target -- the host walk, as fast
 * as the reference body (no pass over the map, nothing uploaded). */
template <class NodeMap, class HashT>
std::vector<std::shared_ptr<typename NodeMap::mapped_type::element_type>>
getCachedNodes(Context& ctx, const NodeMap& map, const HashT& id, size_t count, uint64_t version = 0) {
    return std::move(getCachedNodesBatch(ctx, map, &id, 1, count, version)[0]);
}

/* Flat exact k-NN over a fixed id set kept resident in HBM (the batched
 * findClosestNodesBatch(targets[], k) of the north star): upload once, query many. */
class ClosestIndex {
public:
    explicit ClosestIndex(Context& ctx) : ctx_(ctx) {}
    template <class HashT>
    void assign(const HashT* ids, size_t n) {
        std::vector<uint8_t> b;
        b.reserve(n * DHTGPU_HASH_LEN);
        for (size_t i = 0; i < n; ++i) detail::put_id(b, ids[i]);
        check(dhtgpu_set_ids(ctx_.get(), b.empty() ? nullptr : b.data(), n), "set_ids");
    }
    /* Accept mask (Node::isGood / isExpired, src/node.cpp:42-47, for the resident set): while one
     * is set, query() returns the closest ACCEPTED ids, as indices into the assigned array.
     * accept[i] != 0 accepts id i; n must be the assigned size. */
    void set_accept(const uint8_t* accept, size_t n) {
        if (!accept || n != dhtgpu_num_ids(ctx_.get())) throw Error(DHTGPU_EINVAL, "set_accept: one byte per id");
        check(dhtgpu_set_accept(ctx_.get(), accept), "set_accept");
    }
    void clear_accept() { check(dhtgpu_set_accept(ctx_.get(), nullptr), "set_accept"); }
    /* accept[idx[j]] = val[j] for m entries (an expired node off, a revived one on) */
    void update_accept(const uint32_t* idx, const uint8_t* val, size_t m) {
        check(dhtgpu_update_accept(ctx_.get(), idx, val, m), "update_accept");
    }
    /* the snapshot rule of findClosestNodesBatch: id i is accepted when nodes[i] &&
     * nodes[i]->isGood(now) (nodes[i] being the node whose id was assigned at i) */
    template <class NodePtr, class TimePoint>
    void set_accept_good(const std::vector<NodePtr>& nodes, TimePoint now) {
        std::vector<uint8_t> a(nodes.size());
        for (size_t i = 0; i < nodes.size(); ++i) a[i] = nodes[i] && nodes[i]->isGood(now) ? 1 : 0;
        static const uint8_t none = 0;
        set_accept(a.empty() ? &none : a.data(), a.size());
    }
    /* overwrite ids [first, first + m) in place (slot reuse: mask the dead node's slot off, write
     * the new id into it, mask it on); the mask is kept */
    template <class HashT>
    void write(size_t first, const HashT* ids, size_t m) {
        std::vector<uint8_t> b;
        b.reserve(m * DHTGPU_HASH_LEN);
        for (size_t i = 0; i < m; ++i) detail::put_id(b, ids[i]);
        check(dhtgpu_write_ids(ctx_.get(), first, b.empty() ? nullptr : b.data(), m), "write_ids");
    }
    /* out[i] = indices of the k ids closest to targets[i], ascending by XOR distance */
    template <class HashT>
    std::vector<std::vector<uint32_t>> query(const HashT* targets, size_t q, size_t k) const {
        std::vector<uint8_t> t;
        t.reserve(q * DHTGPU_HASH_LEN);
        for (size_t i = 0; i < q; ++i) detail::put_id(t, targets[i]);
        std::vector<uint32_t> idx(q * k), cnt(q);
        std::vector<std::vector<uint32_t>> res(q);
        if (q == 0) return res;
        // K6 per-batch prefix filter (large sets run over prefix sub-partitions inside the
        // library); the K1 streaming scan where K6's limits are exceeded (q > 2^22)
        int rc = dhtgpu_batch_topk(ctx_.get(), t.data(), (uint32_t)q, (uint32_t)k, idx.data(), cnt.data());
        if (rc == DHTGPU_ERANGE) rc = dhtgpu_topk(ctx_.get(), t.data(), (uint32_t)q, (uint32_t)k, idx.data(), cnt.data());
        check(rc, "topk");
        for (size_t i = 0; i < q; ++i) res[i].assign(idx.begin() + i * k, idx.begin() + i * k + cnt[i]);
        return res;
    }
private:
    Context& ctx_;
};

/* The routing table resident on the device (dhtgpu_rt_*): the responder path.  Wiring:
 *   assign(table, af, version)   when the table changes (a node added or removed, a bucket
 *                                split): the snapshot rule of TableSnapshot plus every node's
 *                                address || port (af 4 / 6; 0 = no tails, no replies); a version
 *                                != 0 equal to the last one's skips the upload
 *   refresh(table, now)          once per batch: the isGood(now) bits only (by handle, with the
 *                                expired and pending bits, once the mirror has grown)
 *   findClosestNodesBatch / replyNodesBatch / closerThanSelfBatch   the batch itself
 * Between two assigns the mirror follows the table node by node (dhtgpu_rtg_*):
 *   noteNewNode(node, now)       after the caller's own table.onNewNode(node, ...): queues the
 *                                node's id, handle (its slot in the handle -> NodePtr table), state
 *                                byte and tail
 *   noteExpire()                 after Dht::expireBuckets: queues the sweep
 *   flush(table)                 the queue, one device call per run of new nodes or sweep, in order;
 *                                every device path below flushes first.  Evicted and expired handles
 *                                go to a free list.  A queue longer than max_flush_nodes, an
 *                                UNAPPLIED result or a device error falls back to assign(table).
 *   onNewNodeBatch(...)          stand-alone use, no host table: one call, the result codes
 * Batches below min_device_batch (replies: min_reply_batch) targets never touch the device: they
 * run the reference's walk on the table they are given (detail::find_closest_host) and, for replies, pack the records on
 * the host -- neither assign nor refresh is needed for them.  Larger batches answer from the
 * mirror, i.e. from the table as last assigned and refreshed. */
/* Smallest batches answered from the mirror, from the measured crossovers of DESIGN.md §5j
 * (profiles/r10/rtable/rtable_check_run.txt: refresh + the batch call against the host walk, both
 * through this adapter; fixed cost / (host - device cost per target)): replies 59.6 us / (0.250 -
 * 0.051) us = 299 targets; node lists 51.6 us / (0.183 - 0.108) us = 688 -- both paths build the
 * same vectors of node pointers, which is most of either side's cost per target.  The closeness
 * flags were not measured and follow the node lists' threshold. */
static const size_t kMinResidentBatch = 768;
static const size_t kMinResidentReplyBatch = 320;
/* Most queued nodes ResidentTable::flush sends node by node; a longer queue re-assigns the table.
 * From the measured crossover of DESIGN.md §5m (tools/rtgrow_bench.py): a flush costs 39.5 us + 1.19
 * us per node (cfg-1 table; the client table 43.2 + 1.35), the upload of the re-packed table 77.2 us
 * (87.2) whatever the batch: (77.2 - 39.5) / 1.19 = 31.9 nodes (32.5).  The host's re-pack is on
 * top of the upload and was not timed, so the threshold errs towards assign. */
static const size_t kMaxResidentFlush = 32;

template <class Table, class TimePoint>
class ResidentTable {
public:
    typedef typename TableSnapshot<Table, TimePoint>::NodePtr NodePtr;
    template <class HashT>
    ResidentTable(Context& ctx, const HashT& myid)
        : min_device_batch(kMinResidentBatch), min_reply_batch(kMinResidentReplyBatch),
          max_flush_nodes(kMaxResidentFlush), is_client(false), ctx_(ctx), alen_(0), af_(0), grown_(false),
          have_now_(false), now_() {
        std::memcpy(myid_, myid.data(), DHTGPU_HASH_LEN);
    }
    size_t min_device_batch;   // smallest batch answered from the mirror: node lists and closeness flags
    size_t min_reply_batch;    // ... replies
    size_t max_flush_nodes;    // most queued nodes flush() sends node by node; more: assign
    bool is_client;            // RoutingTable::is_client, for the device's split rule

    void assign(const Table& table, unsigned af, uint64_t version = 0) {
        if (af != 0 && af != 4 && af != 6) throw Error(DHTGPU_EINVAL, "ResidentTable::assign: af");
        alen_ = af == 4 ? 4u : af == 6 ? 16u : 0u;
        af_ = af;
        std::vector<uint8_t> firsts, ids, tail;
        std::vector<uint32_t> off;
        nodes_.clear();
        free_.clear();
        slot_of_.clear();
        queue_.clear();   // what was queued is in the table that is uploaded now
        grown_ = false;
        for (const auto& b : table) {
            detail::put_id(firsts, b.first);
            off.push_back((uint32_t)nodes_.size());
            for (const auto& n : b.nodes) {
                detail::put_id(ids, n->id);
                if (alen_) detail::put_tail(tail, *n, af == 6);
                slot_of_[n.get()] = (uint32_t)nodes_.size();
                nodes_.push_back(n);
            }
        }
        off.push_back((uint32_t)nodes_.size());
        resident_.assign(nodes_.size(), 1);   // what is uploaded is resident
        static const uint8_t none[DHTGPU_HASH_LEN] = {0};
        check(dhtgpu_rt_set(ctx_.get(), myid_, (uint32_t)(off.size() - 1), firsts.data(), off.data(),
                            ids.empty() ? nullptr : ids.data(), alen_ ? (tail.empty() ? none : tail.data()) : nullptr,
                            af, version),
              "rt_set");
    }

    /* the isGood(now) bits of the assigned nodes, in the assigned order; on a grown mirror the state
     * bytes of the resident nodes by handle */
    void refresh(const Table& table, TimePoint now) {
        now_ = now;
        have_now_ = true;
        flush(table);
        if (grown_) {
            check(send_states(now), "rtg_set_state");
            return;
        }
        std::vector<uint8_t> good;
        good.reserve(nodes_.size());
        for (const auto& b : table)
            for (const auto& n : b.nodes) good.push_back(n->isGood(now) ? 1 : 0);
        if (good.size() != nodes_.size()) throw Error(DHTGPU_EINVAL, "ResidentTable::refresh: the table changed, assign it");
        check(dhtgpu_rt_set_good(ctx_.get(), good.empty() ? nullptr : good.data()), "rt_set_good");
    }

    template <class HashT>
    std::vector<std::vector<NodePtr>> findClosestNodesBatch(const Table& table, const HashT* targets, size_t q,
                                                            TimePoint now, size_t count) {
        std::vector<std::vector<NodePtr>> res(q);
        if (q == 0 || count == 0) return res;
        if (host(q, count)) {
            for (size_t i = 0; i < q; ++i) detail::find_closest_host(table, targets[i], now, count, res[i]);
            return res;
        }
        flush(table);
        const std::vector<uint8_t> t = pack(targets, q);
        std::vector<uint32_t> idx(q * count), cnt(q);
        check(dhtgpu_rt_find_closest(ctx_.get(), t.data(), (uint32_t)q, (uint32_t)count, idx.data(), cnt.data()),
              "rt_find_closest");
        for (size_t i = 0; i < q; ++i) {
            res[i].reserve(cnt[i]);
            for (uint32_t r = 0; r < cnt[i]; ++r) res[i].push_back(nodes_[idx[i * count + r]]);
        }
        return res;
    }

    /* the find_node / get reply per target: findClosestNodes(target, now, 8) as bufferNodes packs it */
    template <class HashT>
    std::vector<std::vector<uint8_t>> replyNodesBatch(const Table& table, const HashT* targets, size_t q,
                                                      TimePoint now) {
        if (!alen_) throw Error(DHTGPU_EINVAL, "ResidentTable::replyNodesBatch: assigned without an address family");
        const uint32_t rec = 20 + alen_ + 2;
        std::vector<std::vector<uint8_t>> res(q);
        if (q == 0) return res;
        if (q < min_reply_batch) {
            for (size_t i = 0; i < q; ++i) res[i] = detail::reply_nodes_host(table, targets[i], now, alen_ == 16);
            return res;
        }
        flush(table);
        const std::vector<uint8_t> t = pack(targets, q);
        std::vector<uint8_t> out(q * 8 * rec);
        std::vector<uint32_t> len(q);
        check(dhtgpu_rt_reply(ctx_.get(), t.data(), (uint32_t)q, out.data(), len.data(), nullptr), "rt_reply");
        for (size_t i = 0; i < q; ++i) res[i].assign(out.begin() + i * 8 * rec, out.begin() + i * 8 * rec + len[i]);
        return res;
    }

    /* flag[i] = findClosestNodes(targets[i], now, count) holds at least max(min_nodes, 1) nodes and
     * targets[i].xorCmp(nodes.back()->id, myid) < 0: (8, 1) is maintainStorage's test, (14, 8)
     * onAnnounce's */
    template <class HashT>
    std::vector<uint8_t> closerThanSelfBatch(const Table& table, const HashT* targets, size_t q, TimePoint now,
                                             size_t count, size_t min_nodes) {
        std::vector<uint8_t> flag(q, 0);
        if (q == 0 || count == 0) return flag;
        if (host(q, count)) {
            for (size_t i = 0; i < q; ++i)
                flag[i] = detail::closer_than_self_host(table, targets[i], now, count, min_nodes, myid_);
            return flag;
        }
        flush(table);
        const std::vector<uint8_t> t = pack(targets, q);
        check(dhtgpu_rt_closer(ctx_.get(), t.data(), (uint32_t)q, (uint32_t)count, (uint32_t)min_nodes, flag.data(),
                               nullptr),
              "rt_closer");
        return flag;
    }

    /* ---- the mirror follows the table (dhtgpu_rtg_*) ---- */
    void noteNewNode(const NodePtr& node, TimePoint now) {
        Op op;
        op.expire = false;
        std::memcpy(op.id, node->id.data(), DHTGPU_HASH_LEN);
        op.handle = slot(node);
        op.state = detail::node_state(*node, now, 0);
        now_ = now;
        have_now_ = true;
        std::vector<uint8_t> t;
        if (alen_) detail::put_tail(t, *node, alen_ == 16);
        std::memset(op.tail, 0, sizeof op.tail);
        if (!t.empty()) std::memcpy(op.tail, t.data(), t.size());
        queue_.push_back(op);
    }
    void noteExpire() {
        Op op = Op();
        op.expire = true;
        queue_.push_back(op);
    }
    size_t queued() const { return queue_.size(); }
    /* the handle -> node table: what a result index of the mirror names (null: a free handle) */
    const std::vector<NodePtr>& handles() const { return nodes_; }

    void flush(const Table& table) {
        if (queue_.empty()) return;
        size_t news = 0;
        for (const Op& op : queue_) news += op.expire ? 0 : 1;
        bool ok = news <= max_flush_nodes;
        // an uploaded mirror knows its nodes' good bits only: onNewNode and the sweep read the
        // expired and pending bits too, so the first mutation is preceded by the states by handle
        if (ok && !grown_) ok = have_now_ && send_states(now_) == DHTGPU_OK;
        for (size_t b = 0; ok && b < queue_.size();) {
            if (queue_[b].expire) {
                ok = flush_expire();
                ++b;
                continue;
            }
            size_t e = b;
            while (e < queue_.size() && !queue_[e].expire) ++e;
            ok = flush_new(b, e);
            b = e;
        }
        queue_.clear();
        if (!ok) assign(table, af_);
    }

    /* Stand-alone use: m nodes given as ids, caller-owned handles (< DHTGPU_RTG_MAX_HANDLE), state
     * bytes (nullable: good) and tails (alen + 2 bytes each, iff assigned with an address family), applied
     * in order to the mirror as last assigned; returns the DHTGPU_RTG_* codes, aux (nullable) the
     * evicted handles / ping picks.  DHTGPU_ERANGE (a 257th bucket) does not throw: the codes say
     * UNAPPLIED from there on. */
    template <class HashT>
    std::vector<uint8_t> onNewNodeBatch(const HashT* ids, const uint32_t* handles, const uint8_t* state,
                                        const uint8_t* tails, size_t m, std::vector<uint32_t>* aux = nullptr) {
        std::vector<uint8_t> res(m, 0);
        if (!m) return res;
        const std::vector<uint8_t> x = pack(ids, m);
        std::vector<uint32_t> a(m, DHTGPU_NONE);
        const int r = dhtgpu_rtg_on_new_node(ctx_.get(), x.data(), handles, state, tails, (uint32_t)m, is_client ? 1u : 0u,
                                             res.data(), a.data(), nullptr);
        if (r != DHTGPU_ERANGE) check(r, "rtg_on_new_node");
        grown_ = true;
        if (aux) aux->swap(a);
        return res;
    }

private:
    struct Op {
        bool expire;
        uint8_t id[DHTGPU_HASH_LEN];
        uint32_t handle;
        uint8_t state;
        uint8_t tail[18];
    };
    /* the node's handle: the one it holds, else a free one, else a new one */
    uint32_t slot(const NodePtr& node) {
        const auto it = slot_of_.find(node.get());
        if (it != slot_of_.end()) return it->second;
        uint32_t h;
        if (!free_.empty()) {
            h = free_.back();
            free_.pop_back();
            nodes_[h] = node;
        } else {
            h = (uint32_t)nodes_.size();
            nodes_.push_back(node);
        }
        slot_of_[node.get()] = h;
        if (h >= resident_.size()) resident_.resize(h + 1, 0);
        resident_[h] = 0;
        return h;
    }
    void release(uint32_t h) {
        if (h >= nodes_.size() || !nodes_[h]) return;
        slot_of_.erase(nodes_[h].get());
        nodes_[h] = NodePtr();
        if (h < resident_.size()) resident_[h] = 0;
        free_.push_back(h);
    }
    /* one state byte per handle, as of `now` (turns an uploaded mirror into its grown form) */
    int send_states(TimePoint now) {
        std::vector<uint8_t> st(nodes_.size(), 0);
        for (size_t h = 0; h < nodes_.size(); ++h)
            if (nodes_[h]) st[h] = detail::node_state(*nodes_[h], now, 0);
        const int r = dhtgpu_rtg_set_state(ctx_.get(), st.empty() ? nullptr : st.data(), (uint32_t)st.size());
        if (r == DHTGPU_OK) grown_ = true;
        return r;
    }
    bool flush_new(size_t b, size_t e) {
        const size_t m = e - b, rec = alen_ ? alen_ + 2 : 0;
        std::vector<uint8_t> ids, st(m), tails, res(m);
        std::vector<uint32_t> h(m), aux(m);
        for (size_t i = b; i < e; ++i) {
            if (queue_[i].handle >= DHTGPU_RTG_MAX_HANDLE) return false;
            ids.insert(ids.end(), queue_[i].id, queue_[i].id + DHTGPU_HASH_LEN);
            tails.insert(tails.end(), queue_[i].tail, queue_[i].tail + rec);
            h[i - b] = queue_[i].handle;
            st[i - b] = queue_[i].state;
        }
        grown_ = true;
        if (dhtgpu_rtg_on_new_node(ctx_.get(), ids.data(), h.data(), st.data(), rec ? tails.data() : nullptr, (uint32_t)m,
                                   is_client ? 1u : 0u, res.data(), aux.data(), nullptr) != DHTGPU_OK)
            return false;
        for (size_t i = 0; i < m; ++i) {
            if (res[i] == DHTGPU_RTG_UNAPPLIED) return false;
            if (res[i] == DHTGPU_RTG_REPLACED) release(aux[i]);
            if (res[i] == DHTGPU_RTG_PLACED || res[i] == DHTGPU_RTG_REPLACED) resident_[h[i]] = 1;
        }
        for (size_t i = 0; i < m; ++i)   // a node the table did not take keeps no handle
            if (!resident_[h[i]]) release(h[i]);
        return true;
    }
    bool flush_expire() {
        grown_ = true;
        std::vector<uint32_t> gone(nodes_.size() + 1);
        uint32_t n = 0;
        if (dhtgpu_rtg_expire(ctx_.get(), gone.data(), &n) != DHTGPU_OK) return false;
        for (uint32_t i = 0; i < n; ++i) release(gone[i]);
        return true;
    }
    bool host(size_t q, size_t count) const { return q < min_device_batch || count > DHTGPU_MAX_K; }
    template <class HashT>
    static std::vector<uint8_t> pack(const HashT* targets, size_t q) {
        std::vector<uint8_t> t;
        t.reserve(q * DHTGPU_HASH_LEN);
        for (size_t i = 0; i < q; ++i) detail::put_id(t, targets[i]);
        return t;
    }
    Context& ctx_;
    uint8_t myid_[DHTGPU_HASH_LEN];
    uint32_t alen_;
    unsigned af_;
    bool grown_;                               // the mirror took a dhtgpu_rtg_* mutation since the last assign
    bool have_now_;                            // now_ holds the time of the last note or refresh
    TimePoint now_;
    std::vector<NodePtr> nodes_;               // handle -> node (after assign: the upload position)
    std::vector<uint8_t> resident_;            // handle -> the mirror holds it
    std::vector<uint32_t> free_;               // handles of evicted and expired nodes
    std::map<const void*, uint32_t> slot_of_;  // node -> its handle
    std::vector<Op> queue_;
};

/* NodeCache's map resident on the device (dhtgpu_nc_*): the initiator path.  The adapter owns the
 * handle space -- a slot vector of weak_ptr<Node> and a free list; a key's handle is its slot.
 * Wiring:
 *   assign(map)                 once (and to re-sync): the whole map, every slot's accept bit
 *   noteInsert(id, node)        where NodeMap::getNode emplaces (src/node_cache.cpp:99-111); queued
 *   noteErase(id)               where NodeMap::getNode(id) / clearBadNodes erase (:87-97, :113-123); queued
 *   flush()                     the queue as one erase call and one insert call (a key inserted and
 *                               erased again between two flushes never reaches the device)
 *   slotsOfBatch(ids, n)        the handles of n ids (NodeMap::find): the host's key map, or dhtgpu_ncr_find
 *   getNodeBatch(ids, n, make)  NodeMap::getNode(id, addr, ...) for a reply's records: dhtgpu_ncr_get_nodes
 *   refresh()                   once per batch: lock() && !isExpired() && !isClient() of every live
 *                               slot (src/node_cache.cpp:68-69), as one mask upload
 *   getCachedNodesBatch(map, targets, q, count)   the batch itself
 * Batches below min_device_batch targets never touch the device: they run the reference's walk on
 * the map they are given (detail::cached_nodes_host).  Larger batches flush the queue and answer
 * from the mirror, i.e. with the accept bits of the last refresh; a node whose weak_ptr has
 * expired since then is left out of its row. */
/* Smallest batch answered from the mirror, from the crossover measured in DESIGN.md §5k
 * (profiles/r11/ncache/ncache_check_run.txt: refresh + the batch call against the host walk, both
 * through this adapter, 5,994 keys, count 8): the host walk wins at 256 targets (76.2 against 134.3
 * us), the mirror at 512 (180.3 against 199.2 us); the two differences cross at 449 targets.
 * kResidentCacheRebuildRatio: the queue length, as a fraction of the keys held, from which
 * flush() rebuilds the mirror with dhtgpu_nc_set instead of one erase and one insert call
 * (profiles/r11/ncache/nc_bench_large_m.json, 10^6 keys): an insert of 524,288 keys costs 1,248 us
 * against 1,446 us for the rebuild, one of 10^6 keys 2,132 against 1,809 us; the differences cross
 * at 705,000 keys.  The erase crosses at 789,000 keys. */
/* kMinResidentFindBatch: smallest batch of ids slotsOfBatch resolves through dhtgpu_ncr_find
 * instead of the host's key map (profiles/r17/ncresolve/: the host form against m
 * std::map finds over the same 2^20 keys, same session): the map wins at 256 ids (16.3 against 42.3
 * us), the device at 512 (43.6 against 51.5 us); the differences cross at 452 ids, and this is the
 * next multiple of 64 at or above 1.1 x that. */
static const size_t kMinResidentCacheBatch = 512;
static const size_t kMinResidentFindBatch = 512;
static const double kResidentCacheRebuildRatio = 0.705;

/* ResidentCache's handle space, device-free: the slot vector, the free list, the keys held and
 * the operations queued since the last flush. */
template <class NodeT>
class CacheSlots {
public:
    typedef std::shared_ptr<NodeT> NodePtr;
    typedef std::weak_ptr<NodeT> NodeRef;
    struct Key {
        uint8_t b[DHTGPU_HASH_LEN];
        bool operator<(const Key& o) const { return std::memcmp(b, o.b, DHTGPU_HASH_LEN) < 0; }
    };
    template <class HashT>
    static Key key_of(const HashT& id) {
        Key k;
        std::memcpy(k.b, id.data(), DHTGPU_HASH_LEN);
        return k;
    }

    void clear() {
        slots_.clear();
        free_.clear();
        slot_of_.clear();
        ins_.clear();
        era_.clear();
    }
    /* std::map::emplace: a key already held keeps its slot; else the last freed slot, else a new one */
    template <class HashT>
    void noteInsert(const HashT& id, const NodeRef& node) {
        const Key k = key_of(id);
        if (slot_of_.count(k)) return;
        uint32_t h;
        if (!free_.empty()) {
            h = free_.back();
            free_.pop_back();
            slots_[h] = node;
        } else {
            if (slots_.size() >= DHTGPU_NC_MAX_HANDLE) throw Error(DHTGPU_ERANGE, "ResidentCache: out of handles");
            h = (uint32_t)slots_.size();
            slots_.push_back(node);
        }
        slot_of_[k] = h;
        ins_[k] = h;
    }
    /* map.erase(key): the slot goes to the free list; a queued insert of the key leaves the queue */
    template <class HashT>
    void noteErase(const HashT& id) {
        const Key k = key_of(id);
        const auto it = slot_of_.find(k);
        if (it == slot_of_.end()) return;
        slots_[it->second].reset();
        free_.push_back(it->second);
        slot_of_.erase(it);
        if (!ins_.erase(k)) era_.push_back(k);   // (a key never sent needs no erase)
    }
    uint8_t accepted(uint32_t h) const {
        const NodePtr n = slots_[h].lock();
        return n && !n->isExpired() && !n->isClient() ? 1 : 0;
    }
    /* the slot of a key (DHTGPU_NONE: not held) */
    template <class HashT>
    uint32_t slotOf(const HashT& id) const {
        const auto it = slot_of_.find(key_of(id));
        return it == slot_of_.end() ? DHTGPU_NONE : it->second;
    }
    /* slotOf for n keys */
    template <class HashT>
    std::vector<uint32_t> slotsOf(const HashT* ids, size_t n) const {
        std::vector<uint32_t> h(n);
        for (size_t i = 0; i < n; ++i) h[i] = slotOf(ids[i]);
        return h;
    }
    /* The free list dhtgpu_ncr_get_nodes draws from, `count` handles in the order noteInsert would
     * take them: the last freed slot first, then fresh slot numbers (fewer than count at the
     * handle bound). */
    std::vector<uint32_t> offer(size_t count) const {
        std::vector<uint32_t> f;
        f.reserve(count);
        for (size_t i = free_.size(); i > 0 && f.size() < count; --i) f.push_back(free_[i - 1]);
        for (size_t h = slots_.size(); f.size() < count && h < DHTGPU_NC_MAX_HANDLE; ++h) f.push_back((uint32_t)h);
        return f;
    }
    /* What a dhtgpu_ncr_get_nodes call answered for n keys (handle[], is_new[], `used` handles of
     * offer()'s list consumed): the batched NodeMap::getNode(id, addr, ...) on the host side.  A new
     * key's slot takes make_node(j); a key already held returns its node, or, when that has
     * expired, a node made anew in the same slot (src/node_cache.cpp:104-106).  Returns the nodes. */
    template <class HashT, class MakeNode>
    std::vector<NodePtr> adopt(const HashT* ids, size_t n, const uint32_t* handle, const uint8_t* is_new, size_t used,
                               MakeNode make_node) {
        const size_t from_free = used < free_.size() ? used : free_.size();
        free_.resize(free_.size() - from_free);
        slots_.resize(slots_.size() + (used - from_free));
        std::vector<NodePtr> out(n);
        for (size_t j = 0; j < n; ++j) {
            const uint32_t h = handle[j];
            if (is_new[j]) {
                out[j] = make_node(j);
                slots_[h] = out[j];
                slot_of_[key_of(ids[j])] = h;
            } else if (!(out[j] = slots_[h].lock())) {
                out[j] = make_node(j);
                slots_[h] = out[j];
            }
        }
        return out;
    }
    size_t size() const { return slot_of_.size(); }
    size_t pending() const { return ins_.size() + era_.size(); }

    std::vector<NodeRef> slots_;
    std::vector<uint32_t> free_;
    std::map<Key, uint32_t> slot_of_;   // the keys held (queued inserts included)
    std::map<Key, uint32_t> ins_;       // queued inserts
    std::vector<Key> era_;              // queued erases (keys the device holds)
};

template <class NodeMap>
class ResidentCache {
public:
    typedef typename NodeMap::mapped_type::element_type NodeT;
    typedef CacheSlots<NodeT> Slots;
    typedef typename Slots::NodePtr NodePtr;
    typedef typename Slots::NodeRef NodeRef;
    typedef typename Slots::Key Key;
    explicit ResidentCache(Context& ctx)
        : min_device_batch(kMinResidentCacheBatch), rebuild_ratio(kResidentCacheRebuildRatio),
          min_find_batch(kMinResidentFindBatch), max_first_offer((size_t)-1), ctx_(ctx) {}
    size_t min_device_batch;   // smallest batch answered from the mirror
    double rebuild_ratio;      // flush(): queued keys / keys held from which the mirror is rebuilt (0: never)
    size_t min_find_batch;     // smallest batch slotsOfBatch resolves on the device
    size_t max_first_offer;    // most free handles getNodeBatch offers before it knows how many are needed

    void assign(const NodeMap& map) {
        s_.clear();
        for (const auto& kv : map) {
            s_.slot_of_[Slots::key_of(kv.first)] = (uint32_t)s_.slots_.size();
            s_.slots_.push_back(kv.second);
        }
        rebuild();
    }
    template <class HashT>
    void noteInsert(const HashT& id, const NodeRef& node) { s_.noteInsert(id, node); }
    template <class HashT>
    void noteErase(const HashT& id) { s_.noteErase(id); }

    void flush() {
        if (!s_.pending()) return;
        if (rebuild_ratio > 0 && (double)s_.pending() >= rebuild_ratio * (double)s_.size()) {
            s_.ins_.clear();
            s_.era_.clear();
            rebuild();
            return;
        }
        if (!s_.era_.empty()) {
            std::vector<uint8_t> ids;
            ids.reserve(s_.era_.size() * DHTGPU_HASH_LEN);
            for (const Key& k : s_.era_) ids.insert(ids.end(), k.b, k.b + DHTGPU_HASH_LEN);
            check(dhtgpu_nc_erase(ctx_.get(), ids.data(), (uint32_t)s_.era_.size(), nullptr), "nc_erase");
            s_.era_.clear();
        }
        if (!s_.ins_.empty()) {
            std::vector<uint8_t> ids, acc;
            std::vector<uint32_t> handles;
            ids.reserve(s_.ins_.size() * DHTGPU_HASH_LEN);
            for (const auto& kh : s_.ins_) {
                ids.insert(ids.end(), kh.first.b, kh.first.b + DHTGPU_HASH_LEN);
                handles.push_back(kh.second);
                acc.push_back(s_.accepted(kh.second));
            }
            check(dhtgpu_nc_insert(ctx_.get(), ids.data(), handles.data(), acc.data(), (uint32_t)s_.ins_.size(), nullptr),
                  "nc_insert");
            s_.ins_.clear();
        }
    }

    void refresh() {
        if (s_.slots_.empty()) return;
        std::vector<uint8_t> acc(s_.slots_.size());
        for (size_t h = 0; h < acc.size(); ++h) acc[h] = s_.accepted((uint32_t)h);
        check(dhtgpu_nc_set_accept(ctx_.get(), acc.data(), (uint32_t)acc.size()), "nc_set_accept");
    }

    template <class HashT>
    std::vector<std::vector<NodePtr>> getCachedNodesBatch(const NodeMap& map, const HashT* targets, size_t q,
                                                          size_t count) {
        std::vector<std::vector<NodePtr>> res(q);
        if (q == 0 || count == 0) return res;
        if (q < min_device_batch || count > DHTGPU_MAX_K) {
            for (size_t i = 0; i < q; ++i) res[i] = detail::cached_nodes_host(map, targets[i], count);
            return res;
        }
        flush();
        std::vector<uint8_t> t;
        t.reserve(q * DHTGPU_HASH_LEN);
        for (size_t i = 0; i < q; ++i) detail::put_id(t, targets[i]);
        std::vector<uint32_t> h(q * count), cnt(q);
        check(dhtgpu_nc_nodes(ctx_.get(), t.data(), (uint32_t)q, (uint32_t)count, h.data(), cnt.data()), "nc_nodes");
        for (size_t i = 0; i < q; ++i) {
            res[i].reserve(cnt[i]);
            for (uint32_t r = 0; r < cnt[i]; ++r)
                if (NodePtr n = s_.slots_[h[i * count + r]].lock()) res[i].push_back(n);
        }
        return res;
    }

    /* The handles of n ids (DHTGPU_NONE: not held): NodeMap::find in a batch.  Below min_find_batch
     * from the host's key map, from it up flush() then dhtgpu_ncr_find. */
    template <class HashT>
    std::vector<uint32_t> slotsOfBatch(const HashT* ids, size_t n) {
        if (n < min_find_batch) return s_.slotsOf(ids, n);
        flush();
        std::vector<uint8_t> b;
        b.reserve(n * DHTGPU_HASH_LEN);
        for (size_t i = 0; i < n; ++i) detail::put_id(b, ids[i]);
        std::vector<uint32_t> h(n);
        check(dhtgpu_ncr_find(ctx_.get(), b.data(), (uint32_t)n, h.data(), nullptr), "ncr_find");
        return h;
    }

    /* NodeMap::getNode(id, addr, now, confirm, client) (src/node_cache.cpp:99-111) for n ids, where
     * NetworkEngine::deserializeNodes calls it per record (src/network_engine.cpp:868, :884):
     * flushes, resolves and emplaces on the device under the free list (then fresh slot numbers),
     * and creates the Node of every new key through make_node(j) -> shared_ptr<Node>.  A new node
     * that is not acceptable (a client) has its accept bit cleared.  Returns the n nodes. */
    template <class HashT, class MakeNode>
    std::vector<NodePtr> getNodeBatch(const HashT* ids, size_t n, MakeNode make_node) {
        if (n == 0) return std::vector<NodePtr>();
        flush();
        std::vector<uint8_t> b;
        b.reserve(n * DHTGPU_HASH_LEN);
        for (size_t i = 0; i < n; ++i) detail::put_id(b, ids[i]);
        std::vector<uint32_t> h(n);
        std::vector<uint8_t> is_new(n);
        uint32_t used = 0;
        std::vector<uint32_t> offer = s_.offer(n < max_first_offer ? n : max_first_offer);
        for (;;) {
            const int r = dhtgpu_ncr_get_nodes(ctx_.get(), b.data(), (uint32_t)n, offer.empty() ? nullptr : offer.data(),
                                               (uint32_t)offer.size(), nullptr, h.data(), is_new.data(), &used);
            if (r != DHTGPU_ERANGE || used <= offer.size()) {
                check(r, "ncr_get_nodes");
                break;
            }
            offer = s_.offer(used);   // nothing was applied: again with as many as it needs
            if (offer.size() < used) throw Error(DHTGPU_ERANGE, "ResidentCache: out of handles");
        }
        std::vector<NodePtr> out = s_.adopt(ids, n, h.data(), is_new.data(), used, make_node);
        std::vector<uint32_t> rej;
        for (size_t j = 0; j < n; ++j)
            if (is_new[j] && !s_.accepted(h[j])) rej.push_back(h[j]);
        if (!rej.empty()) {
            const std::vector<uint8_t> zero(rej.size(), 0);
            check(dhtgpu_nc_update_accept(ctx_.get(), rej.data(), zero.data(), (uint32_t)rej.size()), "nc_update_accept");
        }
        return out;
    }

    const Slots& slots() const { return s_; }
    Context& context() const { return ctx_; }

private:
    /* the mirror from the keys held: every key with its slot, then every slot's accept bit */
    void rebuild() {
        std::vector<uint8_t> ids;
        std::vector<uint32_t> handles;
        ids.reserve(s_.size() * DHTGPU_HASH_LEN);
        handles.reserve(s_.size());
        for (const auto& kh : s_.slot_of_) {
            ids.insert(ids.end(), kh.first.b, kh.first.b + DHTGPU_HASH_LEN);
            handles.push_back(kh.second);
        }
        check(dhtgpu_nc_set(ctx_.get(), ids.empty() ? nullptr : ids.data(), handles.empty() ? nullptr : handles.data(),
                            s_.size()),
              "nc_set");
        refresh();
    }
    Context& ctx_;
    Slots s_;
};

/* The searches' node lists resident on the device (dhtgpu_sr_*), on top of a ResidentCache: the
 * same context, and a node's handle is its cache slot (every Node of the reference comes out of the
 * NodeCache; what is queued for a node the cache no longer holds at the flush is skipped).  SearchT is the reference's
 * Dht::Search shape: id, expired, nodes (a std::vector of SearchNode{node, candidate, ...},
 * constructible from a shared_ptr<Node>) and insertNode(node, now).  Wiring:
 *   open(id) -> slot            where Dht::search creates a Search; close(slot) where it is dropped
 *                               (closed slots go on a free list, like the cache's)
 *   noteInsert(slot, node, has_token)   where the reply path calls sr->insertNode(node, now, token)
 *   noteCandidate(slot, node, val)      where Dht::searchNodeGetExpired sets srn->candidate
 *   noteRequest(slot, node, state)      where a find_node request completes or is erased (see the method)
 *                               -- all four only queue: no device call before the next flush
 *   stepBatch(slots, q, now_tick, node_expire)   Dht::searchStep for q find_node searches on the
 *                               device; returns the nodes to send find_node to (see the method)
 *   refresh(now)                once per sweep: flushes the queue, then isExpired() | isRemovable(now) << 1
 *                               of every live cache slot, as one upload
 *   refillBatch(searches, slots, q, now)   Dht::refill for q searches; returns the inserted counts
 *   offerBatch(searches, nodes, n, now)    Dht::trySearchInsert for n learned nodes over the host's
 *                               std::map of searches (see the method)
 * Below min_device_batch searches refillBatch runs the reference's body on the host
 * (detail::cached_nodes_host on the map, then sr.insertNode) and queues what it inserted: no device
 * call, so one refill costs what the reference's costs.  From the threshold up it flushes the
 * cache's queue and its own, runs dhtgpu_sr_refill, reads the rows back and reconciles each host
 * Search: nodes becomes the device row in its order, keeping the SearchNode of a node that was
 * listed and making a new one (node->setTime(now)) for a new node; expired is copied.  The device
 * applies queued insertions with the node state of the last refresh.  dhtgpu::Error on a device
 * failure: the caller falls back to the host body as INTEGRATION.md shows. */
/* Smallest batch refilled on the device, from the crossover measured in DESIGN.md §5l
 * (profiles/r12/rsearch/rsearch_check_run.txt: refresh + refillBatch through this adapter against
 * the host body, 6,000 keys, count 14, lists already full): the host body wins at 256 searches
 * (176.7 against 195.7 us), the device at 512 (205.8 against 369.0 us); the two differences cross at
 * 283 searches.  The constant is the next multiple of 64 at or above 1.1 x the crossover (311.3):
 * the margin keeps box-to-box spread from putting the default on the losing side. */
static const size_t kMinResidentRefillBatch = 320;
/* Smallest batch of learned nodes offerBatch sends to the device (dhtgpu_srm_offer), from the
 * crossover measured in DESIGN.md §5n (profiles/r15/srmap/srmap_check_bench.txt: offerBatch through
 * this adapter on the device against the host walk plus the flush of the pairs it queued, 2^20 cached
 * keys, converged lists).  With 1,024 searches the host route wins at 64 nodes (292.4 against 361.2
 * us) and the device at 1,024 (2,178 against 3,394 us): the differences cross at 115 nodes.  With
 * 16,384 searches the host route still wins at 1,024 nodes (2,818 against 3,157 us) and the device at
 * 16,384 (26,970 against 46,930 us): they cross at 1,280.  The constant is the next multiple of 64 at
 * or above 1.1 x the larger crossover (1,408), on the device's side for both map sizes.  On fresh
 * (empty) lists the device lost at both sizes measured (1 and 64 nodes), which this threshold keeps
 * on the host; larger fresh batches were not measured. */
static const size_t kMinResidentOfferBatch = 1408;

template <class NodeMap, class SearchT, class Cache = ResidentCache<NodeMap>>
class ResidentSearches {
public:
    typedef typename Cache::NodePtr NodePtr;
    typedef typename Cache::Key Key;
    typedef typename std::remove_reference<decltype(std::declval<SearchT&>().nodes[0])>::type SearchNodeT;
    /* map: the NodeCache map the host body walks (it outlives this object) */
    ResidentSearches(Cache& cache, const NodeMap& map, uint32_t nslots = 16384)
        : min_device_batch(kMinResidentRefillBatch), min_offer_batch(kMinResidentOfferBatch), cache_(cache), map_(map),
          nslots_(nslots), next_(0), ready_(false), map_version_(1), sent_version_(0) {}
    size_t min_device_batch;   // smallest batch refilled on the device
    size_t min_offer_batch;    // smallest batch of learned nodes offered on the device

    template <class HashT>
    uint32_t open(const HashT& id) {
        uint32_t s;
        if (!free_.empty()) {
            s = free_.back();
            free_.pop_back();
        } else {
            if (next_ >= nslots_) throw Error(DHTGPU_ERANGE, "ResidentSearches: out of slots");
            s = next_++;
        }
        Op op = {kOpen, s, 0, Cache::Slots::key_of(id), NodePtr()};
        log_.push_back(op);
        slot_of_target_[op.key] = s;
        target_of_slot_[s] = op.key;
        ++map_version_;
        return s;
    }
    /* the slot goes to the free list; what was queued for it leaves the queue */
    void close(uint32_t slot) {
        size_t w = 0;
        for (size_t i = 0; i < log_.size(); ++i)
            if (log_[i].kind == kClock || log_[i].slot != slot) log_[w++] = log_[i];
        log_.resize(w);
        free_.push_back(slot);
        const auto t = target_of_slot_.find(slot);
        if (t != target_of_slot_.end()) {
            const auto k = slot_of_target_.find(t->second);
            if (k != slot_of_target_.end() && k->second == slot) slot_of_target_.erase(k);
            target_of_slot_.erase(t);
        }
        ++map_version_;
    }
    void noteInsert(uint32_t slot, const NodePtr& node, bool has_token) {
        Op op = {kInsert, slot, (uint8_t)(has_token ? 1 : 0), Key(), node};
        log_.push_back(op);
    }
    void noteCandidate(uint32_t slot, const NodePtr& node, bool val) {
        Op op = {kCandidate, slot, (uint8_t)(val ? 1 : 0), Key(), node};
        log_.push_back(op);
    }
    /* the request state of the node's entry (0 none, 1 pending, 2 completed): 2 where the engine
     * completes the request before Dht::searchNodeGetDone, 0 where searchNodeGetExpired erases it */
    void noteRequest(uint32_t slot, const NodePtr& node, unsigned state) {
        Op op = {kRequest, slot, (uint8_t)state, Key(), node};
        log_.push_back(op);
    }
    /* scheduler.time() in ticks (> 0) from here on in the queue: the last_get_reply of the replies
     * queued after it.  stepBatch queues its own. */
    void noteClock(uint32_t now_tick) {
        Op op = {kClock, now_tick, 0, Key(), NodePtr()};
        log_.push_back(op);
    }
    size_t pending() const { return log_.size(); }
    size_t freeSlots() const { return free_.size(); }

    /* the queue in order, every run of one kind as one call */
    void flush() {
        ensure();
        size_t i = 0;
        while (i < log_.size()) {
            size_t e = i;
            while (e < log_.size() && log_[e].kind == log_[i].kind) ++e;
            if (log_[i].kind == kOpen) flush_open(i, e);
            else if (log_[i].kind == kInsert) flush_insert(i, e);
            else if (log_[i].kind == kClock) check(dhtgpu_srs_set_clock(ctx(), log_[e - 1].slot), "srs_set_clock");
            else flush_pairs(i, e, log_[i].kind == kRequest);
            i = e;
        }
        log_.clear();
    }

    template <class TimePoint>
    void refresh(TimePoint now) {
        flush();   // what is queued was done under the state the device still holds
        const auto& sl = cache_.slots().slots_;
        if (sl.empty()) return;
        std::vector<uint8_t> st(sl.size());
        for (size_t h = 0; h < st.size(); ++h)
            if (const NodePtr n = sl[h].lock()) st[h] = (uint8_t)((n->isExpired() ? 1 : 0) | (n->isRemovable(now) ? 2 : 0));
        check(dhtgpu_sr_set_state(ctx(), st.data(), (uint32_t)st.size()), "sr_set_state");
    }

    template <class TimePoint>
    std::vector<unsigned> refillBatch(SearchT* const* searches, const uint32_t* slots, size_t q, TimePoint now,
                                      size_t count = 14) {
        std::vector<unsigned> inserted(q, 0);
        if (q == 0) return inserted;
        if (q < min_device_batch || count > DHTGPU_MAX_K) {   // Dht::refill's body
            for (size_t i = 0; i < q; ++i) {
                for (const NodePtr& n : detail::cached_nodes_host(map_, searches[i]->id, count)) {
                    if (searches[i]->insertNode(n, now)) ++inserted[i];
                    noteInsert(slots[i], n, false);
                }
            }
            return inserted;
        }
        cache_.flush();
        flush();
        std::vector<uint32_t> ins(q), rows(q * DHTGPU_SR_CAP), lens(q), st(q * 4);
        const int rc = dhtgpu_sr_refill(ctx(), slots, (uint32_t)q, (uint32_t)count, ins.data());
        if (rc != DHTGPU_ERANGE) check(rc, "sr_refill");   // an overflowed row is still a valid list
        check(dhtgpu_sr_lists(ctx(), slots, (uint32_t)q, rows.data(), nullptr, lens.data()), "sr_lists");
        check(dhtgpu_sr_status(ctx(), slots, (uint32_t)q, st.data()), "sr_status");
        for (size_t i = 0; i < q; ++i) {
            reconcile(*searches[i], &rows[i * DHTGPU_SR_CAP], lens[i], (st[i * 4 + 3] & 1u) != 0, now);
            inserted[i] = ins[i];
        }
        return inserted;
    }

    /* Dht::trySearchInsert (src/dht.cpp:118-150) for n learned nodes, in order.  searches: the
     * reference's searches(af), a std::map<InfoHash, Sp<SearchT>> whose every search was opened here
     * under its key (SearchT::done is read).  Returns trySearchInsert's result per node; touched
     * (nullable) gets the searches that took a node -- those whose nextSearchStep the caller edits to
     * now -- and may name a search more than once.  Below min_offer_batch nodes it runs the
     * reference's walk on the host map and queues every (search, node) the walk called insertNode on.
     * From the threshold up it flushes the queues, sends the map when a search was opened or closed
     * since it was last sent, sends the done bits, runs dhtgpu_srm_offer with the node state of the
     * last refresh, and reconciles the host searches: the rows of those that took a node, and the
     * length of every other one (a refusal only cuts a list's tail).  A batch that cannot go to the
     * device -- a search without a slot, a node the cache does not hold -- and a device error before
     * the offer was issued both fall back to the host walk. */
    template <class SearchMap, class TimePoint>
    std::vector<uint8_t> offerBatch(SearchMap& searches, const NodePtr* nodes, size_t n, TimePoint now,
                                    std::vector<SearchT*>* touched = nullptr) {
        std::vector<uint8_t> res(n, 0);
        if (n == 0) return res;
        if (n >= min_offer_batch) {
            bool sent = false;
            offered_ = false;
            try {
                sent = offer_device(searches, nodes, n, now, res, touched);
            } catch (const Error&) {
                if (offered_) throw;   // the offer was applied: a failing read-back is the caller's
                sent_version_ = 0;
            }
            if (sent) return res;
        }
        for (size_t j = 0; j < n; ++j) res[j] = offer_host(searches, nodes[j], now, touched) ? 1 : 0;
        return res;
    }

    /* What Dht::searchStep decided for one search: the nodes to send find_node to, in list order, and
     * dhtgpu_srs_step's out4 -- pending non-bad entries after, nodes the refill inserted, bits. */
    struct Step {
        std::vector<NodePtr> send;
        uint32_t solicited, inserted, bits;
        bool expired() const { return (bits & 1u) != 0; }
        bool done() const { return (bits & 4u) != 0; }
        bool synced() const { return (bits & 16u) != 0; }
        bool skipped() const { return (bits & 32u) != 0; }
    };
    /* Dht::searchStep (src/dht.cpp:562-654) for q find_node searches whose request state lives with
     * the device (noteRequest): flushes the queues, sets the clock to now_tick (> 0), runs
     * dhtgpu_srs_step and returns its decisions.  The caller sends find_node to every node of
     * Step::send -- the device already holds those requests as pending -- and reports each outcome
     * with noteRequest / noteInsert / noteCandidate.  No host Search is read or written. */
    std::vector<Step> stepBatch(const uint32_t* slots, size_t q, uint32_t now_tick, uint32_t node_expire,
                                uint32_t refill_count = 14) {
        std::vector<Step> res(q);
        if (q == 0) return res;
        cache_.flush();
        noteClock(now_tick);
        flush();
        std::vector<uint32_t> send(q * DHTGPU_SR_CAP), out4(q * 4);
        const int rc = dhtgpu_srs_step(ctx(), slots, (uint32_t)q, node_expire, refill_count, send.data(), out4.data());
        if (rc != DHTGPU_ERANGE) check(rc, "srs_step");   // an overflowed row is still a valid list
        const auto& sl = cache_.slots().slots_;
        for (size_t i = 0; i < q; ++i) {
            for (uint32_t k = 0; k < out4[i * 4]; ++k) {
                const uint32_t h = send[i * DHTGPU_SR_CAP + k];
                if (NodePtr n = h < sl.size() ? sl[h].lock() : NodePtr()) res[i].send.push_back(n);
            }
            res[i].solicited = out4[i * 4 + 1];
            res[i].inserted = out4[i * 4 + 2];
            res[i].bits = out4[i * 4 + 3];
        }
        return res;
    }

private:
    enum Kind { kOpen, kInsert, kCandidate, kRequest, kClock };
    struct Op {
        Kind kind;
        uint32_t slot;  // clock: the tick
        uint8_t val;    // insert: replied with a token; candidate: the flag; request: the state
        Key key;        // open: the target
        NodePtr node;   // insert, candidate: the node (its cache slot is looked up when the queue is flushed,
    };                  //   so queueing costs no key lookup; a node the cache dropped meanwhile is skipped)
    dhtgpu_ctx* ctx() const { return cache_.context().get(); }
    /* a host Search made equal to its device row: nodes becomes the row in its order, keeping the
     * SearchNode of a node that was listed and making a new one (node->setTime(now)) for a new node */
    template <class TimePoint>
    void reconcile(SearchT& sr, const uint32_t* row, uint32_t len, bool expired, TimePoint now) {
        const auto& sl = cache_.slots().slots_;
        // a slot names a listed node when both share their owner: no lock(), no key lookup
        const auto listed = [&](uint32_t h, size_t j) {
            const NodePtr& p = sr.nodes[j].node;
            return p && h < sl.size() && !sl[h].owner_before(p) && !p.owner_before(sl[h]);
        };
        bool same = len == sr.nodes.size();   // the usual outcome: the row is the host list
        for (uint32_t r = 0; same && r < len; ++r) same = listed(row[r], r);
        if (!same) {
            std::vector<SearchNodeT> nodes;
            nodes.reserve(len);
            size_t cur = 0;   // both lists are in distance order: a kept node is found from here on
            for (uint32_t r = 0; r < len; ++r) {
                const size_t hn = sr.nodes.size();
                size_t k = cur;
                while (k < hn && !listed(row[r], k)) ++k;
                if (k == hn)
                    for (k = 0; k < cur && !listed(row[r], k); ++k) {}
                if (k < hn && listed(row[r], k)) {
                    nodes.push_back(std::move(sr.nodes[k]));
                    sr.nodes[k].node.reset();
                    if (k >= cur) cur = k + 1;
                } else if (NodePtr n = row[r] < sl.size() ? sl[row[r]].lock() : NodePtr()) {
                    nodes.push_back(SearchNodeT(n));
                    n->setTime(now);
                }
            }
            sr.nodes = std::move(nodes);
        }
        sr.expired = expired;
    }
    void ensure() {
        if (ready_) return;
        check(dhtgpu_sr_reset(ctx(), nslots_), "sr_reset");
        ready_ = true;
    }
    void flush_open(size_t b, size_t e) {
        std::vector<uint32_t> slots;
        std::vector<uint8_t> t;
        for (size_t i = b; i < e; ++i) {
            slots.push_back(log_[i].slot);
            t.insert(t.end(), log_[i].key.b, log_[i].key.b + DHTGPU_HASH_LEN);
        }
        check(dhtgpu_sr_open(ctx(), slots.data(), t.data(), (uint32_t)slots.size()), "sr_open");
    }
    void flush_insert(size_t b, size_t e) {   // grouped by slot, a slot's insertions in their order
        std::map<uint32_t, std::vector<size_t>> by;
        for (size_t i = b; i < e; ++i) by[log_[i].slot].push_back(i);
        std::vector<uint32_t> slots, handles;
        std::vector<uint64_t> off(1, 0);
        std::vector<uint8_t> ids, tok;
        for (const auto& kv : by) {
            slots.push_back(kv.first);
            for (size_t i : kv.second) {
                const uint32_t h = cache_.slots().slotOf(log_[i].node->id);
                if (h == DHTGPU_NONE) continue;
                handles.push_back(h);
                detail::put_id(ids, log_[i].node->id);
                tok.push_back(log_[i].val);
            }
            off.push_back(handles.size());
        }
        if (handles.empty()) return;
        const int rc = dhtgpu_sr_insert(ctx(), slots.data(), (uint32_t)slots.size(), off.data(), handles.data(), ids.data(),
                                        tok.data(), nullptr);
        if (rc != DHTGPU_ERANGE) check(rc, "sr_insert");
    }
    void flush_pairs(size_t b, size_t e, bool request) {   // candidate flags or request states: of equal (slot, handle) pairs the last one counts
        std::map<std::pair<uint32_t, uint32_t>, uint8_t> last;
        for (size_t i = b; i < e; ++i) {
            const uint32_t h = cache_.slots().slotOf(log_[i].node->id);
            if (h != DHTGPU_NONE) last[std::make_pair(log_[i].slot, h)] = log_[i].val;
        }
        if (last.empty()) return;
        std::vector<uint32_t> slots, handles;
        std::vector<uint8_t> val;
        for (const auto& kv : last) {
            slots.push_back(kv.first.first);
            handles.push_back(kv.first.second);
            val.push_back(kv.second);
        }
        if (request)
            check(dhtgpu_srs_set_request(ctx(), slots.data(), handles.data(), val.data(), (uint32_t)slots.size()),
                  "srs_set_request");
        else
            check(dhtgpu_sr_set_candidate(ctx(), slots.data(), handles.data(), val.data(), (uint32_t)slots.size()),
                  "sr_set_candidate");
    }
    /* the slot of the search opened for this target (DHTGPU_NONE: none) */
    template <class HashT>
    uint32_t slot_of(const HashT& id) const {
        const auto it = slot_of_target_.find(Cache::Slots::key_of(id));
        return it == slot_of_target_.end() ? DHTGPU_NONE : it->second;
    }
    /* Dht::trySearchInsert's body for one node on the host map; every (search, node) it called
     * insertNode on is queued, as noteInsert queues a reply's */
    template <class SearchMap, class TimePoint>
    bool offer_host(SearchMap& searches, const NodePtr& node, TimePoint now, std::vector<SearchT*>* touched) {
        bool inserted = false;
        const auto closest = searches.lower_bound(node->id);
        const auto visit = [&](typename SearchMap::iterator it) {   // false: the walk stops here
            SearchT& s = *it->second;
            const uint32_t slot = slot_of(it->first);
            const bool added = s.insertNode(node, now);
            if (slot != DHTGPU_NONE) noteInsert(slot, node, false);
            if (added) {
                inserted = true;
                if (touched) touched->push_back(&s);
            }
            return added || s.expired || s.done;
        };
        for (auto it = closest; it != searches.end(); ++it)
            if (!visit(it)) break;
        for (auto it = closest; it != searches.begin();) {
            --it;
            if (!visit(it)) break;
        }
        return inserted;
    }
    /* The device side of offerBatch.  Returns false -- nothing sent that changes a list -- when the
     * batch cannot go to the device: a search without a slot, a node the cache does not hold. */
    template <class SearchMap, class TimePoint>
    bool offer_device(SearchMap& searches, const NodePtr* nodes, size_t n, TimePoint now, std::vector<uint8_t>& res,
                      std::vector<SearchT*>* touched) {
        std::vector<uint32_t> slots, handles(n);
        std::vector<SearchT*> ptrs;
        std::vector<uint8_t> done, ids;
        for (auto it = searches.begin(); it != searches.end(); ++it) {
            const uint32_t slot = slot_of(it->first);
            if (slot == DHTGPU_NONE) return false;
            slots.push_back(slot);
            ptrs.push_back(&*it->second);
            done.push_back(it->second->done ? 1 : 0);
        }
        for (size_t j = 0; j < n; ++j) {
            handles[j] = cache_.slots().slotOf(nodes[j]->id);
            if (handles[j] == DHTGPU_NONE) return false;
            detail::put_id(ids, nodes[j]->id);
        }
        cache_.flush();
        flush();
        const uint32_t ns = (uint32_t)slots.size();
        if (sent_version_ != map_version_ || sent_ns_ != ns) {
            check(dhtgpu_srm_set(ctx(), slots.empty() ? nullptr : slots.data(), ns), "srm_set");
            sent_version_ = map_version_;
            sent_ns_ = ns;
        }
        if (ns) check(dhtgpu_srm_set_done(ctx(), slots.data(), done.data(), ns), "srm_set_done");
        std::vector<uint32_t> cnt(n), mask((nslots_ + 31) / 32 + 1);
        const int rc = dhtgpu_srm_offer(ctx(), handles.data(), ids.data(), (uint32_t)n, cnt.data(), mask.data(), nullptr);
        if (rc != DHTGPU_ERANGE) check(rc, "srm_offer");   // an overflowed row is still a valid list
        offered_ = true;
        for (size_t j = 0; j < n; ++j) res[j] = cnt[j] > 0;
        if (!ns) return true;
        // every mapped search: its length (a refusal cuts the list's tail and sets no bit); the
        // searches that took a node: their rows
        std::vector<uint32_t> st(ns * 4), tslots, rows, lens;
        std::vector<size_t> tidx;
        check(dhtgpu_sr_status(ctx(), slots.data(), ns, st.data()), "sr_status");
        for (uint32_t i = 0; i < ns; ++i) {
            if ((mask[slots[i] >> 5] >> (slots[i] & 31u)) & 1u) {
                tslots.push_back(slots[i]);
                tidx.push_back(i);
            } else if (st[i * 4] < ptrs[i]->nodes.size()) {
                ptrs[i]->nodes.resize(st[i * 4]);
            }
        }
        if (!tslots.empty()) {
            rows.resize(tslots.size() * DHTGPU_SR_CAP);
            lens.resize(tslots.size());
            check(dhtgpu_sr_lists(ctx(), tslots.data(), (uint32_t)tslots.size(), rows.data(), nullptr, lens.data()), "sr_lists");
            for (size_t t = 0; t < tslots.size(); ++t) {
                const size_t i = tidx[t];
                reconcile(*ptrs[i], &rows[t * DHTGPU_SR_CAP], lens[t], (st[i * 4 + 3] & 1u) != 0, now);
                if (touched) touched->push_back(ptrs[i]);
            }
        }
        return true;
    }
    Cache& cache_;
    const NodeMap& map_;
    uint32_t nslots_, next_;
    bool ready_;
    std::vector<uint32_t> free_;
    std::vector<Op> log_;
    std::map<Key, uint32_t> slot_of_target_;   // the searches' map as the device holds it: target -> slot
    std::map<uint32_t, Key> target_of_slot_;
    uint64_t map_version_, sent_version_;      // bumped by open / close; the version dhtgpu_srm_set last sent
    uint32_t sent_ns_ = 0;
    bool offered_ = false;                     // offerBatch: dhtgpu_srm_offer returned for this batch
};

/* Drop-in for NetworkEngine::bufferNodes(af, id, nodes) (src/network_engine.cpp:1003-1032)
 * over a batch: nodes[i] (candidates for targets[i], e.g. findClosestNodes results) are
 * sorted by xorCmp to targets[i], the first SEND_NODES = 8 are packed as 26 (AF_INET) /
 * 38 (AF_INET6) byte records id || address || port.  Written against the reference's
 * member names: node->id, node->getAddr().getIPv4().sin_addr/.sin_port,
 * getIPv6().sin6_addr/.sin6_port. */
template <class HashT, class NodePtr>
std::vector<std::vector<uint8_t>> bufferNodesBatch(Context& ctx, int af_inet6, const HashT* targets,
                                                   const std::vector<std::vector<NodePtr>>& nodes) {
    const uint32_t alen = af_inet6 ? 16u : 4u, rec = 20 + alen + 2;
    const size_t q = nodes.size();
    std::vector<std::vector<uint8_t>> res(q);
    if (q == 0) return res;
    size_t c = 0;
    for (const auto& v : nodes) c = v.size() > c ? v.size() : c;
    if (c > 64) throw Error(DHTGPU_EINVAL, "bufferNodes: more than 64 candidates");
    std::vector<uint8_t> ids, tail, t;
    std::vector<uint32_t> cand(q * (c ? c : 1), DHTGPU_NONE);
    uint32_t n = 0;
    for (size_t i = 0; i < q; ++i) {
        detail::put_id(t, targets[i]);
        for (size_t j = 0; j < nodes[i].size(); ++j, ++n) {
            const auto& nd = nodes[i][j];
            detail::put_id(ids, nd->id);
            const uint8_t* a;
            const uint8_t* p;
            if (af_inet6) {
                const auto& sin6 = nd->getAddr().getIPv6();
                a = reinterpret_cast<const uint8_t*>(&sin6.sin6_addr);
                p = reinterpret_cast<const uint8_t*>(&sin6.sin6_port);
            } else {
                const auto& sin = nd->getAddr().getIPv4();
                a = reinterpret_cast<const uint8_t*>(&sin.sin_addr);
                p = reinterpret_cast<const uint8_t*>(&sin.sin_port);
            }
            tail.insert(tail.end(), a, a + alen);
            tail.insert(tail.end(), p, p + 2);
            cand[i * c + j] = n;
        }
    }
    std::vector<uint8_t> out(q * 8 * rec);
    std::vector<uint32_t> len(q);
    // the candidates' own ids (the context's k-NN id set is not touched)
    check(dhtgpu_buffer_nodes_ids(ctx.get(), ids.empty() ? nullptr : ids.data(), tail.empty() ? nullptr : tail.data(), n,
                                  af_inet6 ? 6u : 4u, t.data(), (uint32_t)q, cand.data(), (uint32_t)c, out.data(),
                                  len.data()),
          "buffer_nodes");
    for (size_t i = 0; i < q; ++i) res[i].assign(out.begin() + i * 8 * rec, out.begin() + i * 8 * rec + len[i]);
    return res;
}

}  // namespace dhtgpu

#endif /* DHTGPU_HPP */
