// ncache_check.cpp -- exercises dhtgpu::ResidentCache (include/dhtgpu.hpp, C++11) against the mock
// map shape of adapter_check.cpp (std::map<InfoHash, weak_ptr<Node>>) and the oracle's
// getCachedNodes restatement.
//   (no argument)   build check: prints "built"
//   --host          no device: the below-threshold path (the host walk on the map it is given,
//                   expired weak_ptrs included) and ResidentCache's slot / free-list bookkeeping
//                   (dhtgpu::CacheSlots) -- insert, erase, re-insert into a freed slot
//   --run           on a GPU: both dispatch paths against the oracle through insert / erase /
//                   expiry rounds (flush() as incremental calls and as a rebuild, in turn), then
//                   the timings behind the adapter's threshold
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
struct Node {
    InfoHash id;
    bool expired, client;
    bool isExpired() const { return expired; }
    bool isClient() const { return client; }
};
typedef std::map<InfoHash, std::weak_ptr<Node>> NodeMap;
}  // namespace mock

static mock::Xorshift rng = {88172645463325252ull};
static uint32_t rnd() { return (uint32_t)rng.step(); }

typedef std::shared_ptr<mock::Node> NodeSp;

static NodeSp make_node(const uint8_t* id20) {
    auto n = std::make_shared<mock::Node>();
    std::memcpy(n->id.d.data(), id20, 20);
    n->expired = (rnd() % 4) == 0;
    n->client = (rnd() % 10) == 0;
    return n;
}

// rows of `got` against the oracle over the map as it stands; returns mismatches
static int compare(const mock::NodeMap& map, const std::vector<mock::InfoHash>& targets, size_t count,
                   const std::vector<std::vector<NodeSp>>& got) {
    std::vector<uint8_t> sorted, acc;
    for (const auto& kv : map) {
        sorted.insert(sorted.end(), kv.first.d.begin(), kv.first.d.end());
        auto n = kv.second.lock();
        acc.push_back(n && !n->isExpired() && !n->isClient());
    }
    int bad = 0;
    for (size_t i = 0; i < targets.size(); ++i) {
        uint32_t want[64];
        const uint32_t c = map.empty() ? 0 : orc_cached_nodes(sorted.data(), map.size(), acc.data(), targets[i].data(),
                                                              (uint32_t)count, want);
        if (got[i].size() != c) { ++bad; continue; }
        for (uint32_t r = 0; r < c; ++r)
            if (std::memcmp(got[i][r]->id.data(), &sorted[20 * want[r]], 20)) ++bad;
    }
    return bad;
}

int main(int argc, char** argv) {
    const bool host_only = argc >= 2 && std::strcmp(argv[1], "--host") == 0;
    if (argc < 2 || (std::strcmp(argv[1], "--run") != 0 && !host_only)) { std::puts("built"); return 0; }
    const int total = 12000, q = 400;
    std::vector<uint8_t> ids(20 * total), tb(20 * q);
    orc_gen_ids(300, 0, total, ids.data());
    orc_gen_ids(301, 0, q, tb.data());
    std::vector<mock::InfoHash> targets(q);
    for (int i = 0; i < q; ++i) std::memcpy(targets[i].d.data(), &tb[20 * i], 20);
    for (int i = 0; i < 40; ++i) std::memcpy(targets[i].d.data(), &ids[20 * (i * 11)], 20);   // equal to keys

    int bad = 0;
    if (host_only) {
        dhtgpu::CacheSlots<mock::Node> rc;   // ResidentCache's bookkeeping: no device behind it
        mock::NodeMap map;
        std::vector<NodeSp> keep;
        for (int i = 0; i < 5000; ++i) {
            keep.push_back(make_node(&ids[20 * i]));
            map[keep.back()->id] = keep.back();
            rc.noteInsert(keep.back()->id, keep.back());
        }
        if (rc.size() != 5000 || rc.slots_.size() != 5000 || rc.free_.size() != 0 || rc.pending() != 5000) ++bad;
        for (int i = 0; i < 5000; ++i)
            if (rc.slotOf(keep[i]->id) != (uint32_t)i) ++bad;
        rc.noteInsert(keep[7]->id, keep[8]);   // emplace on a present key: nothing changes
        if (rc.size() != 5000 || rc.slots_.size() != 5000 || rc.slotOf(keep[7]->id) != 7) ++bad;
        // erase: the slots go to the free list; a queued insert that is erased leaves the queue
        for (int i = 0; i < 100; ++i) {
            map.erase(keep[3 * i]->id);
            rc.noteErase(keep[3 * i]->id);
        }
        if (rc.size() != 4900 || rc.free_.size() != 100 || rc.pending() != 4900) ++bad;
        if (rc.slotOf(keep[0]->id) != DHTGPU_NONE) ++bad;
        rc.noteErase(keep[0]->id);             // absent: ignored
        if (rc.size() != 4900 || rc.free_.size() != 100) ++bad;
        // re-insert into freed slots: no new slot is allocated, the last freed slot goes first
        std::vector<NodeSp> more;
        for (int i = 0; i < 60; ++i) {
            more.push_back(make_node(&ids[20 * (5000 + i)]));
            map[more.back()->id] = more.back();
            rc.noteInsert(more.back()->id, more.back());
        }
        if (rc.slots_.size() != 5000 || rc.free_.size() != 40 || rc.size() != 4960) ++bad;
        if (rc.slotOf(more[0]->id) != 3 * 99 || rc.slotOf(more[59]->id) != 3 * 40) ++bad;
        // expiry of a weak_ptr: the host walk skips the node
        for (int i = 1; i < 5000; i += 9) keep[i].reset();
        for (size_t count : {1, 8, 14, 40}) {
            // what ResidentCache::getCachedNodesBatch runs below min_device_batch
            std::vector<std::vector<NodeSp>> got(q);
            for (int i = 0; i < q; ++i) got[i] = dhtgpu::detail::cached_nodes_host(map, targets[i], count);
            bad += compare(map, targets, count, got);
        }
        std::printf("ncache_check (host paths): %d mismatches\n", bad);
        return bad ? 1 : 0;
    }

    dhtgpu::Context ctx(0);
    dhtgpu::ResidentCache<mock::NodeMap> rc(ctx);
    mock::NodeMap map;
    std::map<mock::InfoHash, NodeSp> keep;
    for (int i = 0; i < 4000; ++i) {
        NodeSp n = make_node(&ids[20 * i]);
        keep[n->id] = n;
        map[n->id] = n;
    }
    rc.assign(map);
    int next = 4000;
    for (int round = 0; round < 6; ++round) {
        // NodeMap::getNode: new keys; clearBadNodes / getNode(id): erased keys; some erased keys
        // come back; some nodes die (their weak_ptr expires), some change state
        for (int i = 0; i < 700 && next < total; ++i, ++next) {
            NodeSp n = make_node(&ids[20 * next]);
            keep[n->id] = n;
            if (map.emplace(n->id, n).second) rc.noteInsert(n->id, n);
        }
        std::vector<mock::InfoHash> gone;
        for (const auto& kv : map)
            if (rnd() % 10 == 0) gone.push_back(kv.first);
        for (const auto& k : gone) {
            map.erase(k);
            rc.noteErase(k);
        }
        for (size_t i = 0; i < gone.size(); i += 3) {
            NodeSp n = make_node(gone[i].data());
            keep[n->id] = n;
            if (map.emplace(n->id, n).second) rc.noteInsert(n->id, n);
        }
        for (auto& kv : keep) {
            if (!kv.second) continue;
            const uint32_t r = rnd() % 20;
            if (r == 0) kv.second.reset();
            else if (r == 1) kv.second->expired = !kv.second->expired;
        }
        rc.rebuild_ratio = round % 2 ? 0.01 : 0.0;   // flush(): one erase + one insert call / a rebuild
        rc.flush();
        rc.refresh();
        if (rc.slots().size() != map.size() || rc.slots().pending()) ++bad;
        for (int dev = 0; dev < 2; ++dev) {   // the mirror, then the host walk
            rc.min_device_batch = dev ? (size_t)-1 : 1;
            for (size_t count : {1, 8, 14, 32})
                bad += compare(map, targets, count, rc.getCachedNodesBatch(map, targets.data(), q, count));
        }
    }
    // both sides of the dispatch around the threshold: refresh + getCachedNodesBatch from the mirror
    // against the host walk, wall clock of one warm call each (best of five)
    {
        using clk = std::chrono::steady_clock;
        std::vector<mock::InfoHash> big(4096);
        std::vector<uint8_t> bb(20 * big.size());
        orc_gen_ids(302, 0, big.size(), bb.data());
        for (size_t i = 0; i < big.size(); ++i) std::memcpy(big[i].d.data(), &bb[20 * i], 20);
        size_t sink = 0;
        for (size_t n : {64, 256, 512, 1024, 4096}) {
            double us[2];
            for (int side = 0; side < 2; ++side) {
                rc.min_device_batch = side ? (size_t)-1 : 1;
                double best = 1e30;
                for (int rep = 0; rep < 6; ++rep) {
                    auto d0 = clk::now();
                    if (!side) rc.refresh();
                    sink += rc.getCachedNodesBatch(map, big.data(), n, 8).size();
                    const double d = std::chrono::duration<double, std::micro>(clk::now() - d0).count();
                    if (rep && d < best) best = d;
                }
                us[side] = best;
            }
            std::printf("ncache_check: getCachedNodesBatch q=%zu over %zu keys: device (refresh + query) %.1f us, host %.1f us\n",
                        n, map.size(), us[0], us[1]);
        }
        if (sink == 1) std::puts("");
    }
    std::printf("ncache_check: %d mismatches\n", bad);
    return bad ? 1 : 0;
}
