// srmap_check.cpp -- exercises dhtgpu::ResidentSearches::offerBatch (include/dhtgpu.hpp, C++11) on mock
// Search / SearchNode / Node types of the reference's shape against Dht::trySearchInsert walked over
// the oracle's insertNode restatement.
//   (no argument)   build check: prints "built"
//   --host          no device: the below-threshold path (the reference's walk on the host map), the
//                   pairs it queues, over a cache stand-in that holds dhtgpu::CacheSlots only
//   --run           on a GPU: rounds of state changes, done flips, a closed and re-opened search and
//                   offers, with offerBatch on the device and on the host side of its threshold in turn
//   --bench NS [KEYS]  on a GPU: the timings behind dhtgpu::kMinResidentOfferBatch (see bench() below)
#include <algorithm>
#include <array>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iterator>
#include <map>
#include <memory>
#include <vector>

#include "dhtgpu.hpp"
#include "../../oracle/dht_oracle.h"
#include "mock_dht.h"

namespace mock {
typedef int time_point;
struct Node {
    InfoHash id;
    bool expired, client, removable;
    time_point time;
    uint32_t index;   // in the test's node table
    bool isExpired() const { return expired; }
    bool isClient() const { return client; }
    bool isRemovable(time_point) const { return removable; }
    void setTime(time_point t) { time = t; }
};
}  // namespace mock
#include "mock_search.h"

using mock::NodeSp;

static mock::Xorshift rng = {88172645463325252ull};
static uint32_t rnd() { return (uint32_t)rng.step(); }

// The oracle's side: every search as a row of node-table indices advanced by orc_search_insert, and
// trySearchInsert walked over the searches in target order.
struct Oracle {
    static const uint32_t cap = 256;
    std::vector<uint8_t> ids, state;   // the node table
    std::vector<uint8_t> targets, expired, flags, done;
    std::vector<uint32_t> rows, lens;
    size_t add_search(const mock::InfoHash& t) {
        targets.insert(targets.end(), t.d.begin(), t.d.end());
        expired.push_back(0);
        done.push_back(0);
        lens.push_back(0);
        rows.resize(rows.size() + cap, 0xFFFFFFFFu);
        flags.resize(flags.size() + cap, 0);
        return lens.size() - 1;
    }
    bool insert(size_t s, uint32_t node) {
        const uint64_t off[2] = {0, 1};
        uint8_t added[2] = {0, 0}, tok[2] = {0, 0};
        orc_search_insert(ids.data(), state.data(), &targets[20 * s], 1, cap, &rows[s * cap], &flags[s * cap], &lens[s],
                          &expired[s], off, &node, tok, added, 1);
        return added[0] != 0;
    }
    // order: the live searches' indices in target order
    bool offer(const std::vector<size_t>& order, const mock::InfoHash& id, uint32_t node) {
        size_t c = 0;
        while (c < order.size() && std::memcmp(&targets[20 * order[c]], id.data(), 20) < 0) ++c;
        bool inserted = false;
        for (size_t i = c; i < order.size(); ++i) {
            const size_t s = order[i];
            if (insert(s, node)) inserted = true;
            else if (!expired[s] && !done[s]) break;
        }
        for (size_t i = c; i != 0;) {
            const size_t s = order[--i];
            if (insert(s, node)) inserted = true;
            else if (!expired[s] && !done[s]) break;
        }
        return inserted;
    }
    int differs(const mock::Search& sr) const {
        const size_t s = sr.index;
        if (sr.nodes.size() != lens[s] || sr.expired != (expired[s] != 0)) return 1;
        for (size_t j = 0; j < sr.nodes.size(); ++j)
            if (sr.nodes[j].node->index != rows[s * cap + j]) return 1;
        return 0;
    }
};

struct World {
    std::vector<NodeSp> nodes;   // the node table (the owners)
    mock::NodeMap map;
    mock::SearchMap searches;
    std::map<const mock::Search*, uint32_t> slot;
    Oracle orc;
    std::vector<size_t> order() const {
        std::vector<size_t> o;
        for (const auto& kv : searches) o.push_back(kv.second->index);
        return o;
    }
    void load_state() {
        orc.state.resize(nodes.size());
        for (size_t i = 0; i < nodes.size(); ++i)
            orc.state[i] = (uint8_t)((nodes[i]->expired ? 1 : 0) | (nodes[i]->removable ? 2 : 0));
    }
};

static void build_world(World& w, int total) {
    std::vector<uint8_t> ids(20 * (size_t)total);
    orc_gen_ids(410, 0, total, ids.data());
    w.orc.ids = ids;
    for (int i = 0; i < total; ++i) {
        auto n = std::make_shared<mock::Node>();
        std::memcpy(n->id.d.data(), &ids[20 * (size_t)i], 20);
        n->expired = n->removable = n->client = false;
        n->time = 0;
        n->index = (uint32_t)i;
        w.nodes.push_back(n);
        w.map[n->id] = n;
    }
}

template <class RS>
static mock::Search* add_search(World& w, RS& rs, const mock::InfoHash& id) {
    std::shared_ptr<mock::Search> sr(new mock::Search());
    sr->id = id;
    sr->index = w.orc.add_search(id);
    w.slot[sr.get()] = rs.open(id);
    w.searches[id] = sr;
    return sr.get();
}

// The rounds, on whatever cache stands behind rs: returns mismatches.  device_rounds: bit r set = round
// r's offers run on the device side of the threshold.
template <class RS>
static int rounds(World& w, RS& rs, void (*refresh_cache)(void*), void* cache, unsigned device_rounds, bool has_device) {
    int bad = 0, flips = 0;
    for (int round = 0; round < 6; ++round) {
        const mock::time_point now = 100 + round;
        for (int i = 0; i < 5 && flips < 30; ++i, ++flips) {   // at most 30 nodes ever turn bad
            NodeSp& n = w.nodes[rnd() % w.nodes.size()];
            if (rnd() % 2) n->expired = true;
            else n->removable = true;
        }
        for (auto& kv : w.searches)   // done flips, the oracle's copy beside them
            if (rnd() % 6 == 0) w.orc.done[kv.second->index] = kv.second->done = !kv.second->done;
        if (round == 3) {   // a search dropped and a new one: the map moves
            auto it = w.searches.begin();
            std::advance(it, 5);
            rs.close(w.slot[it->second.get()]);
            w.slot.erase(it->second.get());
            w.searches.erase(it);
            mock::InfoHash id = w.nodes[77]->id;
            id.d[19] ^= 1;
            add_search(w, rs, id);
        }
        if (has_device) {
            rs.refresh(now);
            refresh_cache(cache);
        }
        w.load_state();
        rs.min_offer_batch = (device_rounds >> round) & 1u ? 1 : (size_t)-1;
        const std::vector<size_t> order = w.order();
        for (int call = 0; call < 3; ++call) {
            std::vector<NodeSp> batch;
            const size_t n = call == 0 ? 1 : (call == 1 ? 70 : 400);
            for (size_t j = 0; j < n; ++j) batch.push_back(w.nodes[rnd() % w.nodes.size()]);
            const size_t queued = rs.pending();
            std::vector<mock::Search*> touched;
            const std::vector<uint8_t> got = rs.offerBatch(w.searches, batch.data(), n, now, &touched);
            bool any = false;
            for (size_t j = 0; j < n; ++j) {
                const bool want = w.orc.offer(order, batch[j]->id, batch[j]->index);
                bad += (got[j] != 0) != want;
                any = any || want;
            }
            for (const auto& kv : w.searches) bad += w.orc.differs(*kv.second);
            if (any == touched.empty()) ++bad;
            if ((device_rounds >> round) & 1u) {
                if (rs.pending()) ++bad;                       // the device side flushes the queue
            } else if (rs.pending() <= queued) ++bad;          // the host side queues what it called insertNode on
        }
    }
    return bad;
}

static void refresh_resident(void* c) { static_cast<dhtgpu::ResidentCache<mock::NodeMap>*>(c)->refresh(); }
static void refresh_none(void*) {}

// Both sides of offerBatch's dispatch, wall clock of one call each on a batch of m nodes drawn anew
// from the cache (median of `reps` after one warm-up, the sides alternating): the device side (flush,
// done bits, dhtgpu_srm_offer, read-back and reconciliation), the host walk alone (the CPU body), and
// the host walk followed by the flush of the pairs it queued (one dhtgpu_sr_insert: the route a
// caller has without the map).  converged: lists pre-filled by a device refill of count 14 from the
// whole cache; else every search is opened again, empty, before each call (outside the clock).
static double median(std::vector<double> v) {
    std::sort(v.begin(), v.end());
    return v[v.size() / 2];
}

static void bench(dhtgpu::Context& ctx, int total, int S, bool converged, const std::vector<size_t>& ms) {
    using clk = std::chrono::steady_clock;
    World w;
    build_world(w, total);
    dhtgpu::ResidentCache<mock::NodeMap> rc(ctx);
    rc.assign(w.map);
    dhtgpu::ResidentSearches<mock::NodeMap, mock::Search> rs(rc, w.map, (uint32_t)S);
    std::vector<uint8_t> tb(20 * (size_t)S);
    orc_gen_ids(412, 0, S, tb.data());
    std::vector<mock::Search*> ptrs;
    std::vector<uint32_t> slots;
    for (int s = 0; s < S; ++s) {
        mock::InfoHash id;
        std::memcpy(id.d.data(), &tb[20 * (size_t)s], 20);
        ptrs.push_back(add_search(w, rs, id));
        slots.push_back(w.slot[ptrs.back()]);
    }
    rs.refresh(1);
    rc.refresh();
    if (converged) {
        rs.min_device_batch = 1;
        rs.refillBatch(ptrs.data(), slots.data(), ptrs.size(), 1);
    }
    const auto reopen = [&]() {
        for (auto& kv : w.searches) {
            mock::Search* sr = kv.second.get();
            sr->nodes.clear();
            sr->expired = false;
            rs.close(w.slot[sr]);
            w.slot[sr] = rs.open(sr->id);
        }
        rs.flush();
    };
    const int reps = 5;
    for (size_t m : ms) {
        std::vector<double> dev, walk, route;
        size_t taken[2] = {0, 0};
        for (int rep = 0; rep <= reps; ++rep) {
            for (int side = 0; side < 2; ++side) {
                if (!converged) reopen();
                std::vector<NodeSp> batch;
                for (size_t j = 0; j < m; ++j) batch.push_back(w.nodes[rnd() % w.nodes.size()]);
                rs.min_offer_batch = side ? (size_t)-1 : 1;
                const auto t0 = clk::now();
                const std::vector<uint8_t> got = rs.offerBatch(w.searches, batch.data(), m, 2 + rep);
                const auto t1 = clk::now();
                if (side) rs.flush();
                const auto t2 = clk::now();
                for (uint8_t g : got) taken[side] += g;
                if (!rep) continue;
                const double a = std::chrono::duration<double, std::micro>(t1 - t0).count();
                if (side) {
                    walk.push_back(a);
                    route.push_back(std::chrono::duration<double, std::micro>(t2 - t0).count());
                } else {
                    dev.push_back(a);
                }
            }
        }
        std::printf("srmap_check: offerBatch %s ns=%d m=%zu over %zu keys: device %.1f us, host walk %.1f us, "
                    "host walk + flush %.1f us (nodes taken: %zu / %zu)\n",
                    converged ? "converged" : "fresh", S, m, w.map.size(), median(dev), median(walk), median(route), taken[0],
                    taken[1]);
    }
}

int main(int argc, char** argv) {
    const bool host_only = argc >= 2 && std::strcmp(argv[1], "--host") == 0;
    if (argc >= 3 && std::strcmp(argv[1], "--bench") == 0) {   // --bench NS [KEYS]: the timings behind kMinResidentOfferBatch
        std::setvbuf(stdout, nullptr, _IOLBF, 0);
        const int S = std::atoi(argv[2]), total = argc >= 4 ? std::atoi(argv[3]) : 1 << 20;
        dhtgpu::Context ctx(0);
        bench(ctx, total, S, true, {1, 64, 1024, 16384});
        bench(ctx, total, S, false, {1, 64});
        return 0;
    }
    if (argc < 2 || (std::strcmp(argv[1], "--run") != 0 && !host_only)) { std::puts("built"); return 0; }
    std::setvbuf(stdout, nullptr, _IOLBF, 0);
    const int total = 3000, S = 40;
    std::vector<uint8_t> tb(20 * (size_t)S);
    orc_gen_ids(411, 0, S, tb.data());
    int bad = 0;
    World w;
    build_world(w, total);
    if (host_only) {
        mock::HostCache hc;
        for (const auto& n : w.nodes) hc.s.noteInsert(n->id, n);
        dhtgpu::ResidentSearches<mock::NodeMap, mock::Search, mock::HostCache> rs(hc, w.map, 64);
        for (int s = 0; s < S; ++s) {
            mock::InfoHash id;
            std::memcpy(id.d.data(), &tb[20 * (size_t)s], 20);
            add_search(w, rs, id);
        }
        bad += rounds(w, rs, refresh_none, nullptr, 0u, false);
        rs.min_offer_batch = 1;   // no device behind this cache: the offer falls back to the host walk
        const std::vector<size_t> order = w.order();
        const std::vector<uint8_t> got = rs.offerBatch(w.searches, &w.nodes[9], 1, 1);
        bad += (got[0] != 0) != w.orc.offer(order, w.nodes[9]->id, 9);
        for (const auto& kv : w.searches) bad += w.orc.differs(*kv.second);
        std::printf("srmap_check (host paths): %d mismatches\n", bad);
        return bad ? 1 : 0;
    }
    dhtgpu::Context ctx(0);
    dhtgpu::ResidentCache<mock::NodeMap> rc(ctx);
    rc.assign(w.map);
    dhtgpu::ResidentSearches<mock::NodeMap, mock::Search> rs(rc, w.map, 64);
    for (int s = 0; s < S; ++s) {
        mock::InfoHash id;
        std::memcpy(id.d.data(), &tb[20 * (size_t)s], 20);
        add_search(w, rs, id);
    }
    bad += rounds(w, rs, refresh_resident, &rc, 0x2Du, true);   // device, host, device, device, host, device
    std::printf("srmap_check (device paths): %d mismatches\n", bad);
    return bad ? 1 : 0;
}
