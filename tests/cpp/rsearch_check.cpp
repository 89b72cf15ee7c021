// rsearch_check.cpp -- exercises dhtgpu::ResidentSearches (include/dhtgpu.hpp, C++11) on mock
// Search / SearchNode / Node types of the reference's shape against the oracle's getCachedNodes and
// insertNode restatements.
//   (no argument)   build check: prints "built"
//   --host          no device: the below-threshold path (cached_nodes_host + Search::insertNode), the
//                   queue it leaves behind and the slot free list, over a cache stand-in that holds
//                   dhtgpu::CacheSlots only
//   --run [--quick] on a GPU: the same rounds -- replies, candidates, state changes, closed and
//                   re-opened searches, refills -- with refillBatch on the device and on the host
//                   side of its threshold in turn; then (without --quick) the timings behind
//                   kMinResidentRefillBatch
#include <array>
#include <chrono>
#include <cstdio>
#include <cstring>
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

// The oracle's side: every search as rows of node-table indices, advanced by orc_search_insert.
struct Oracle {
    static const uint32_t cap = 256;
    std::vector<uint8_t> ids, state;   // the node table
    std::vector<uint8_t> targets, expired, flags;
    std::vector<uint32_t> rows, lens;
    void add_search(const mock::InfoHash& t) {
        targets.insert(targets.end(), t.d.begin(), t.d.end());
        expired.push_back(0);
        lens.push_back(0);
        rows.resize(rows.size() + cap, 0xFFFFFFFFu);
        flags.resize(flags.size() + cap, 0);
    }
    void reset_search(size_t s, const mock::InfoHash& t) {
        std::memcpy(&targets[20 * s], t.data(), 20);
        expired[s] = 0;
        lens[s] = 0;
    }
    void load_state(const std::vector<NodeSp>& nodes) {
        state.resize(nodes.size());
        for (size_t i = 0; i < nodes.size(); ++i) state[i] = (uint8_t)((nodes[i]->expired ? 1 : 0) | (nodes[i]->removable ? 2 : 0));
    }
    // search s takes the nodes `ins` (token bytes tok) in order; returns the number added
    unsigned insert(size_t s, const std::vector<uint32_t>& ins, const std::vector<uint8_t>& tok) {
        const uint64_t off[2] = {0, ins.size()};
        std::vector<uint8_t> added(ins.size() + 1);
        orc_search_insert(ids.data(), state.data(), &targets[20 * s], 1, cap, &rows[s * cap], &flags[s * cap], &lens[s],
                          &expired[s], off, ins.data(), tok.data(), added.data(), 1);
        unsigned a = 0;
        for (size_t i = 0; i < ins.size(); ++i) a += added[i];
        return a;
    }
    int differs(size_t s, const mock::Search& sr) const {
        if (sr.nodes.size() != lens[s] || sr.expired != (expired[s] != 0)) return 1;
        for (size_t j = 0; j < sr.nodes.size(); ++j)
            if (sr.nodes[j].node->index != rows[s * cap + j] || sr.nodes[j].candidate != ((flags[s * cap + j] & 1) != 0)) return 1;
        return 0;
    }
};

struct World {
    std::vector<NodeSp> nodes;          // the node table (the owners)
    mock::NodeMap map;
    std::vector<std::unique_ptr<mock::Search>> searches;
    std::vector<uint32_t> slots;
    Oracle orc;
};

// Dht::refill through the oracle for every search: getCachedNodes over the map, then insertNode each
static std::vector<unsigned> oracle_refill(World& w, size_t count) {
    std::vector<uint8_t> sorted, acc;
    std::vector<uint32_t> index;
    for (const auto& kv : w.map) {
        sorted.insert(sorted.end(), kv.first.d.begin(), kv.first.d.end());
        const NodeSp n = kv.second.lock();
        acc.push_back(n && !n->isExpired() && !n->isClient());
        index.push_back(n ? n->index : 0xFFFFFFFFu);
    }
    w.orc.load_state(w.nodes);
    std::vector<unsigned> res(w.searches.size());
    for (size_t s = 0; s < w.searches.size(); ++s) {
        uint32_t pos[64];
        const uint32_t c = orc_cached_nodes(sorted.data(), w.map.size(), acc.data(), &w.orc.targets[20 * s], (uint32_t)count, pos);
        std::vector<uint32_t> ins;
        for (uint32_t r = 0; r < c; ++r) ins.push_back(index[pos[r]]);
        res[s] = w.orc.insert(s, ins, std::vector<uint8_t>(ins.size() + 1, 0));
    }
    return res;
}

// The rounds, on whatever cache stands behind rs: returns mismatches.  device_rounds: bit r set = round
// r's refill runs on the device side of the threshold.
template <class RS, class CacheT>
static int rounds(World& w, RS& rs, CacheT& slots_of, void (*refresh_cache)(void*), void* cache, unsigned device_rounds,
                  bool has_device) {
    int bad = 0;
    const size_t S = w.searches.size();
    int flips = 0;
    for (int round = 0; round < 5; ++round) {
        const mock::time_point now = 100 + round;
        // node state changes (at most 30 nodes ever turn bad), then the state upload
        for (int i = 0; i < 6 && flips < 30; ++i, ++flips) {
            NodeSp& n = w.nodes[rnd() % w.nodes.size()];
            if (rnd() % 2) n->expired = true;
            else n->removable = true;
        }
        if (has_device) {
            rs.refresh(now);
            refresh_cache(cache);
        }
        w.orc.load_state(w.nodes);
        // replies: insertNode with and without a token, on the host Search and queued
        for (size_t i = 0; i < S * 3; ++i) {
            const size_t s = rnd() % S;
            const NodeSp& n = w.nodes[rnd() % 600];
            const bool token = rnd() % 3 == 0;
            const bool a = w.searches[s]->insertNode(n, now, token);
            rs.noteInsert(w.slots[s], n, token);
            if ((w.orc.insert(s, std::vector<uint32_t>(1, n->index), std::vector<uint8_t>(1, token)) != 0) != a) ++bad;
        }
        // searchNodeGetExpired: candidate on / off for listed nodes of three fixed nodes' handles
        for (size_t i = 0; i < S / 2; ++i) {
            const size_t s = rnd() % S;
            mock::Search& sr = *w.searches[s];
            for (size_t j = 0; j < sr.nodes.size(); ++j) {
                if (sr.nodes[j].node->index >= 3) continue;
                const bool val = rnd() % 2;
                sr.nodes[j].candidate = val;
                rs.noteCandidate(w.slots[s], sr.nodes[j].node, val);
                w.orc.flags[s * Oracle::cap + j] = (uint8_t)((w.orc.flags[s * Oracle::cap + j] & ~1u) | (val ? 1u : 0u));
            }
        }
        if (round == 2) {   // searches dropped and new ones in their slots
            for (size_t s = 0; s < S; s += 7) {
                rs.noteInsert(w.slots[s], w.nodes[5], true);   // queued for a search that goes away
                rs.close(w.slots[s]);
            }
            for (size_t s = 0; s < S; s += 7) {
                std::unique_ptr<mock::Search> sr(new mock::Search());
                sr->id = w.nodes[(s * 13) % w.nodes.size()]->id;
                sr->id.d[19] ^= 1;
                const uint32_t slot = rs.open(sr->id);
                if (slots_of.slots().size() == 0 || slot >= S) ++bad;   // a freed slot, not a new one
                w.slots[s] = slot;
                w.orc.reset_search(s, sr->id);
                w.searches[s] = std::move(sr);
            }
            if (rs.freeSlots() != 0) ++bad;
        }
        rs.min_device_batch = (device_rounds >> round) & 1u ? 1 : (size_t)-1;
        std::vector<mock::Search*> ptrs;
        for (auto& sr : w.searches) ptrs.push_back(sr.get());
        const size_t queued = rs.pending();
        const std::vector<unsigned> got = rs.refillBatch(ptrs.data(), w.slots.data(), S, now);
        const std::vector<unsigned> want = oracle_refill(w, 14);
        for (size_t s = 0; s < S; ++s) bad += (got[s] != want[s]) + w.orc.differs(s, *w.searches[s]);
        if ((device_rounds >> round) & 1u) {
            if (rs.pending()) ++bad;                       // the device side flushes the queue
        } else if (rs.pending() <= queued) ++bad;          // the host side queues what it offered
    }
    return bad;
}

static void build_world(World& w, int total, int S) {
    std::vector<uint8_t> ids(20 * (size_t)total), tb(20 * (size_t)S);
    orc_gen_ids(400, 0, total, ids.data());
    orc_gen_ids(401, 0, S, tb.data());
    w.orc.ids = ids;
    for (int i = 0; i < total; ++i) {
        auto n = std::make_shared<mock::Node>();
        std::memcpy(n->id.d.data(), &ids[20 * (size_t)i], 20);
        n->expired = n->removable = false;
        n->client = (rnd() % 10) == 0;
        n->time = 0;
        n->index = (uint32_t)i;
        w.nodes.push_back(n);
        w.map[n->id] = n;
    }
    for (int i = 0; i < 8; ++i) w.nodes[10 + i]->expired = true;   // bad nodes among those that reply
    for (int s = 0; s < S; ++s) {
        std::unique_ptr<mock::Search> sr(new mock::Search());
        std::memcpy(sr->id.d.data(), &tb[20 * (size_t)s], 20);
        if (s % 5 == 0) sr->id = w.nodes[(size_t)s % w.nodes.size()]->id;   // a search for a cached key
        w.orc.add_search(sr->id);
        w.searches.push_back(std::move(sr));
    }
}

static const int kTimedKeys = 6000, kTimedSearches = 8192;   // the timing run

static void refresh_resident(void* c) { static_cast<dhtgpu::ResidentCache<mock::NodeMap>*>(c)->refresh(); }
static void refresh_none(void*) {}

int main(int argc, char** argv) {
    const bool host_only = argc >= 2 && std::strcmp(argv[1], "--host") == 0;
    if (argc < 2 || (std::strcmp(argv[1], "--run") != 0 && !host_only)) { std::puts("built"); return 0; }
    const bool quick = argc >= 3 && std::strcmp(argv[2], "--quick") == 0;
    std::setvbuf(stdout, nullptr, _IOLBF, 0);   // a line printed is a line kept
    const int total = 3000, S = 300;
    int bad = 0;
    if (host_only) {
        World w;
        build_world(w, total, S);
        mock::HostCache hc;
        for (const auto& n : w.nodes) hc.s.noteInsert(n->id, n);
        dhtgpu::ResidentSearches<mock::NodeMap, mock::Search, mock::HostCache> rs(hc, w.map, (uint32_t)S);
        for (int s = 0; s < S; ++s) w.slots.push_back(rs.open(w.searches[s]->id));
        for (int s = 0; s < S; ++s)
            if (w.slots[s] != (uint32_t)s) ++bad;
        if (rs.pending() != (size_t)S) ++bad;
        bool threw = false;   // the row of slots is used up
        try { rs.open(w.searches[0]->id); } catch (const dhtgpu::Error& e) { threw = e.code() == DHTGPU_ERANGE; }
        if (!threw) ++bad;
        bad += rounds(w, rs, hc, refresh_none, nullptr, 0u, false);
        // the free list: the last closed slot goes first
        rs.close(w.slots[4]);
        rs.close(w.slots[9]);
        if (rs.freeSlots() != 2 || rs.open(w.searches[0]->id) != w.slots[9] || rs.open(w.searches[0]->id) != w.slots[4]) ++bad;
        {   // the timing run's shape (more searches than keys), one host refill
            World t;
            build_world(t, kTimedKeys, kTimedSearches);
            mock::HostCache tc;
            for (const auto& n : t.nodes) tc.s.noteInsert(n->id, n);
            dhtgpu::ResidentSearches<mock::NodeMap, mock::Search, mock::HostCache> ts(tc, t.map, (uint32_t)kTimedSearches);
            std::vector<mock::Search*> ptrs;
            for (int s = 0; s < kTimedSearches; ++s) {
                t.slots.push_back(ts.open(t.searches[s]->id));
                ptrs.push_back(t.searches[s].get());
            }
            ts.min_device_batch = (size_t)-1;
            const std::vector<unsigned> got = ts.refillBatch(ptrs.data(), t.slots.data(), kTimedSearches, 1);
            const std::vector<unsigned> want = oracle_refill(t, 14);
            for (int s = 0; s < kTimedSearches; ++s) bad += (got[s] != want[s]) + t.orc.differs(s, *t.searches[s]);
        }
        std::printf("rsearch_check (host paths): %d mismatches\n", bad);
        return bad ? 1 : 0;
    }

    dhtgpu::Context ctx(0);
    {
        World w;
        build_world(w, total, S);
        dhtgpu::ResidentCache<mock::NodeMap> rc(ctx);
        rc.assign(w.map);
        dhtgpu::ResidentSearches<mock::NodeMap, mock::Search> rs(rc, w.map, (uint32_t)S);
        for (int s = 0; s < S; ++s) w.slots.push_back(rs.open(w.searches[s]->id));
        bad += rounds(w, rs, rc, refresh_resident, &rc, 0x1Du, true);   // device, host, device, device, device
    }
    std::printf("rsearch_check (device paths): %d mismatches\n", bad);
    if (quick || bad) return bad ? 1 : 0;

    // Both sides of the dispatch around the threshold: refresh + refillBatch on the device against
    // the host body, wall clock of one warm call each (best of five), searches whose lists are full.
    {
        using clk = std::chrono::steady_clock;
        const int big = kTimedSearches;
        World w;
        build_world(w, kTimedKeys, big);
        dhtgpu::ResidentCache<mock::NodeMap> rc(ctx);
        rc.assign(w.map);
        dhtgpu::ResidentSearches<mock::NodeMap, mock::Search> rs(rc, w.map, (uint32_t)big);
        std::vector<mock::Search*> ptrs;
        for (int s = 0; s < big; ++s) {
            w.slots.push_back(rs.open(w.searches[s]->id));
            ptrs.push_back(w.searches[s].get());
        }
        rs.min_device_batch = 1;
        rs.refresh(1);
        rs.refillBatch(ptrs.data(), w.slots.data(), big, 1);
        size_t sink = 0;
        double prev_n = 0, prev_diff = 0, cross = 0;
        for (size_t n : {64, 128, 256, 512, 1024, 2048, 4096, 8192}) {
            double us[2];
            for (int side = 0; side < 2; ++side) {
                rs.min_device_batch = side ? (size_t)-1 : 1;
                double best = 1e30;
                for (int rep = 0; rep < 6; ++rep) {
                    auto d0 = clk::now();
                    if (!side) rs.refresh(2 + rep);
                    sink += rs.refillBatch(ptrs.data(), w.slots.data(), n, 2 + rep).size();
                    const double d = std::chrono::duration<double, std::micro>(clk::now() - d0).count();
                    if (rep && d < best) best = d;
                    if (side) rs.flush();   // (what the host side queued: outside the timed call)
                }
                us[side] = best;
            }
            const double diff = us[0] - us[1];   // > 0: the host body wins
            if (!cross && prev_n && prev_diff > 0 && diff <= 0) cross = prev_n + (n - prev_n) * prev_diff / (prev_diff - diff);
            prev_n = (double)n;
            prev_diff = diff;
            std::printf("rsearch_check: refillBatch q=%zu over %zu keys: device (refresh + refill + read-back) %.1f us, host %.1f us\n",
                        n, w.map.size(), us[0], us[1]);
        }
        if (cross) std::printf("rsearch_check: crossover at %.0f searches\n", cross);
        else std::printf("rsearch_check: no crossover in the measured range (last difference %.1f us)\n", prev_diff);
        if (sink == 1) std::puts("");
    }
    return 0;
}
