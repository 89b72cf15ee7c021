// ncresolve_check.cpp -- exercises the keys-to-handles side of dhtgpu::ResidentCache
// (include/dhtgpu.hpp, C++11: slotsOfBatch, getNodeBatch over dhtgpu_ncr_*) against the mock map
// shape of ncache_check.cpp and a plain std::map restatement of NodeMap::getNode.
//   (no argument)   build check: prints "built"
//   --host          no device: slotsOfBatch below its threshold (CacheSlots::slotsOf), getNodeBatch's
//                   bookkeeping (CacheSlots::offer / adopt) with the library's answer restated over a
//                   std::map, free-list reuse after noteErase, an expired node made anew
//   --run           on a GPU: getNodeBatch / slotsOfBatch / noteErase rounds against std::map, the
//                   mirror exported and compared with the adapter's key map, the retry on too few handles
//   --bench [n [m ...]]   on a GPU: the timings of DESIGN.md §5p over n resident keys (default 2^20),
//                   batch sizes m (default 1, 64, 1,024, 16,384, 131,072)
#include <algorithm>
#include <array>
#include <chrono>
#include <cstdio>
#include <cstdlib>
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

typedef std::shared_ptr<mock::Node> NodeSp;
typedef dhtgpu::CacheSlots<mock::Node> Slots;

static mock::Xorshift rng = {88172645463325252ull};
static uint32_t rnd() { return (uint32_t)rng.step(); }

static mock::InfoHash hash_at(const std::vector<uint8_t>& ids, size_t i) {
    mock::InfoHash h;
    std::memcpy(h.d.data(), &ids[20 * i], 20);
    return h;
}

static NodeSp make_node(const mock::InfoHash& id, bool client) {
    auto n = std::make_shared<mock::Node>();
    n->id = id;
    n->expired = false;
    n->client = client;
    return n;
}

struct Maker {
    const std::vector<mock::InfoHash>* ids;
    std::vector<NodeSp>* keep;
    NodeSp operator()(size_t j) const {
        NodeSp n = make_node((*ids)[j], (rnd() % 8) == 0);
        keep->push_back(n);
        return n;
    }
};

// dhtgpu_ncr_get_nodes restated over a std::map: the emplace in batch order under `offer`
static size_t ref_get_nodes(std::map<mock::InfoHash, uint32_t>& dev, const std::vector<mock::InfoHash>& ids,
                            const std::vector<uint32_t>& offer, std::vector<uint32_t>& h, std::vector<uint8_t>& is_new) {
    size_t used = 0;
    h.assign(ids.size(), DHTGPU_NONE);
    is_new.assign(ids.size(), 0);
    for (size_t j = 0; j < ids.size(); ++j) {
        auto it = dev.find(ids[j]);
        if (it == dev.end()) {
            it = dev.emplace(ids[j], offer.at(used++)).first;
            is_new[j] = 1;
        }
        h[j] = it->second;
    }
    return used;
}

// the adapter's key map against the restated one; every held slot's node carries its key
static int compare_slots(const Slots& rc, const std::map<mock::InfoHash, uint32_t>& dev) {
    int bad = rc.size() != dev.size();
    for (const auto& kv : dev) {
        if (rc.slotOf(kv.first) != kv.second) { ++bad; continue; }
        const NodeSp n = rc.slots_[kv.second].lock();
        if (n && std::memcmp(n->id.data(), kv.first.data(), 20)) ++bad;
    }
    return bad;
}

static int host_checks(const std::vector<uint8_t>& ids) {
    int bad = 0;
    Slots rc;
    std::map<mock::InfoHash, uint32_t> dev;
    std::vector<NodeSp> keep;
    for (int i = 0; i < 3000; ++i) {
        keep.push_back(make_node(hash_at(ids, i), false));
        rc.noteInsert(keep.back()->id, keep.back());
        dev[keep.back()->id] = (uint32_t)i;
    }
    // slotsOfBatch below the threshold: present and absent ids, a repeat
    {
        std::vector<mock::InfoHash> probe;
        for (int i = 0; i < 400; ++i) probe.push_back(hash_at(ids, 2800 + i));
        probe.push_back(probe[0]);
        const std::vector<uint32_t> h = rc.slotsOf(probe.data(), probe.size());
        for (size_t i = 0; i < probe.size(); ++i) {
            const auto it = dev.find(probe[i]);
            if (h[i] != (it == dev.end() ? DHTGPU_NONE : it->second)) ++bad;
        }
    }
    // getNodeBatch's bookkeeping: new keys, present keys, one new key twice; no free slot yet
    std::vector<uint32_t> h;
    std::vector<uint8_t> is_new;
    {
        std::vector<mock::InfoHash> batch;
        for (int i = 0; i < 200; ++i) batch.push_back(hash_at(ids, 2900 + i));   // 100 present, 100 new
        batch.push_back(batch[150]);
        const std::vector<uint32_t> offer = rc.offer(batch.size());
        if (offer.size() != batch.size() || offer[0] != 3000 || offer.back() != 3000 + batch.size() - 1) ++bad;
        const size_t used = ref_get_nodes(dev, batch, offer, h, is_new);
        const Maker mk = {&batch, &keep};
        const std::vector<NodeSp> got = rc.adopt(batch.data(), batch.size(), h.data(), is_new.data(), used, mk);
        if (used != 100 || rc.slots_.size() != 3100 || !rc.free_.empty() || rc.pending() != 3000) ++bad;
        for (size_t j = 0; j < batch.size(); ++j)
            if (!got[j] || std::memcmp(got[j]->id.data(), batch[j].data(), 20)) ++bad;
        if (got[150] != got[200] || got[0] != keep[2900]) ++bad;
        bad += compare_slots(rc, dev);
    }
    // free-list reuse after noteErase: the last freed slot goes first, no new slot is allocated
    {
        for (int i = 0; i < 50; ++i) {
            rc.noteErase(keep[7 * i]->id);
            dev.erase(keep[7 * i]->id);
        }
        std::vector<mock::InfoHash> batch;
        for (int i = 0; i < 30; ++i) batch.push_back(hash_at(ids, 4000 + i));
        batch.push_back(keep[1]->id);   // present
        const std::vector<uint32_t> offer = rc.offer(batch.size());
        if (offer[0] != 7 * 49 || offer[29] != 7 * 20) ++bad;
        const size_t used = ref_get_nodes(dev, batch, offer, h, is_new);
        const Maker mk = {&batch, &keep};
        rc.adopt(batch.data(), batch.size(), h.data(), is_new.data(), used, mk);
        if (used != 30 || rc.slots_.size() != 3100 || rc.free_.size() != 20 || rc.free_.back() != 7 * 19) ++bad;
        if (rc.slotOf(batch[0]) != 7 * 49 || rc.slotOf(batch[29]) != 7 * 20) ++bad;
        bad += compare_slots(rc, dev);
        // more new keys than free slots: the free list, then fresh numbers
        batch.clear();
        for (int i = 0; i < 25; ++i) batch.push_back(hash_at(ids, 4100 + i));
        const std::vector<uint32_t> offer2 = rc.offer(batch.size());
        if (offer2[19] != 0 || offer2[20] != 3100 || offer2[24] != 3104) ++bad;
        const size_t used2 = ref_get_nodes(dev, batch, offer2, h, is_new);
        rc.adopt(batch.data(), batch.size(), h.data(), is_new.data(), used2, Maker{&batch, &keep});
        if (used2 != 25 || rc.slots_.size() != 3105 || !rc.free_.empty()) ++bad;
        bad += compare_slots(rc, dev);
    }
    // a present key whose node has expired: a node made anew in the same slot (:104-106)
    {
        const mock::InfoHash id = keep[2]->id;
        const uint32_t slot = rc.slotOf(id);
        keep[2].reset();
        std::vector<mock::InfoHash> batch(1, id);
        const size_t used = ref_get_nodes(dev, batch, rc.offer(1), h, is_new);
        const std::vector<NodeSp> got = rc.adopt(batch.data(), 1, h.data(), is_new.data(), used, Maker{&batch, &keep});
        if (used != 0 || is_new[0] || !got[0] || rc.slotOf(id) != slot || rc.slots_[slot].lock() != got[0]) ++bad;
    }
    std::printf("ncresolve_check (host paths): %d mismatches\n", bad);
    return bad;
}

// the mirror as exported against the adapter's key map
static int compare_mirror(dhtgpu::Context& ctx, const Slots& s) {
    uint64_t n = 0;
    dhtgpu::check(dhtgpu_nc_size(ctx.get(), &n), "nc_size");
    if (n != s.size()) return 1;
    std::vector<uint8_t> k(20 * (n ? n : 1));
    std::vector<uint32_t> h(n ? n : 1);
    dhtgpu::check(dhtgpu_nc_export(ctx.get(), k.data(), h.data()), "nc_export");
    int bad = 0;
    size_t i = 0;
    for (const auto& kh : s.slot_of_) {
        if (std::memcmp(kh.first.b, &k[20 * i], 20) || kh.second != h[i]) ++bad;
        ++i;
    }
    return bad;
}

static int run_checks(const std::vector<uint8_t>& ids, int total) {
    int bad = 0;
    dhtgpu::Context ctx(0);
    dhtgpu::ResidentCache<mock::NodeMap> rc(ctx);
    mock::NodeMap map;
    std::vector<NodeSp> keep;
    for (int i = 0; i < 4000; ++i) {
        keep.push_back(make_node(hash_at(ids, i), false));
        map[keep.back()->id] = keep.back();
    }
    rc.assign(map);
    int next = 4000;
    for (int round = 0; round < 6; ++round) {
        // a reply's records: new ids, ids already held, repeats
        std::vector<mock::InfoHash> batch;
        for (int i = 0; i < 500 && next < total; ++i, ++next) batch.push_back(hash_at(ids, next));
        for (int i = 0; i < 300; ++i) batch.push_back(hash_at(ids, rnd() % next));
        for (int i = 0; i < 40; ++i) batch.push_back(batch[rnd() % batch.size()]);
        for (size_t i = batch.size(); i > 1; --i) std::swap(batch[i - 1], batch[rnd() % i]);
        rc.max_first_offer = round == 3 ? 1 : (size_t)-1;   // round 3: ERANGE, then the retry
        size_t fresh_keys = 0;
        {
            std::map<mock::InfoHash, int> seen;
            for (const auto& k : batch)
                if (map.find(k) == map.end() && seen.emplace(k, 0).second) ++fresh_keys;
        }
        const size_t slots_before = rc.slots().slots_.size(), free_before = rc.slots().free_.size();
        const std::vector<NodeSp> got = rc.getNodeBatch(batch.data(), batch.size(), Maker{&batch, &keep});
        for (size_t j = 0; j < batch.size(); ++j) {
            if (!got[j] || std::memcmp(got[j]->id.data(), batch[j].data(), 20)) { ++bad; continue; }
            auto it = map.find(batch[j]);
            if (it == map.end()) map[batch[j]] = got[j];
            else if (it->second.lock() != got[j]) ++bad;   // the node the map already held
        }
        if (rc.slots().size() != map.size()) ++bad;
        // freed slots are taken before any new slot is allocated
        const size_t from_free = std::min(fresh_keys, free_before);
        if (rc.slots().free_.size() != free_before - from_free ||
            rc.slots().slots_.size() != slots_before + (fresh_keys - from_free)) ++bad;
        if (round > 0 && free_before == 0) ++bad;   // (the rounds do exercise the reuse)
        bad += compare_mirror(ctx, rc.slots());
        // both dispatch sides of slotsOfBatch agree, absent ids included
        std::vector<mock::InfoHash> probe(batch.begin(), batch.begin() + 200);
        for (int i = 0; i < 50; ++i) probe.push_back(hash_at(ids, total - 1 - i));
        rc.min_find_batch = 1;
        const std::vector<uint32_t> hd = rc.slotsOfBatch(probe.data(), probe.size());
        rc.min_find_batch = (size_t)-1;
        const std::vector<uint32_t> hh = rc.slotsOfBatch(probe.data(), probe.size());
        if (hd != hh) ++bad;
        for (size_t i = 0; i < probe.size(); ++i)
            if ((hh[i] == DHTGPU_NONE) != (map.find(probe[i]) == map.end())) ++bad;
        // clearBadNodes: some keys go; their slots are what the next round's new keys take
        std::vector<mock::InfoHash> gone;
        for (const auto& kv : map)
            if (rnd() % 12 == 0) gone.push_back(kv.first);
        for (const auto& k : gone) {
            map.erase(k);
            rc.noteErase(k);
        }
    }
    rc.flush();
    bad += compare_mirror(ctx, rc.slots());
    std::printf("ncresolve_check: %d mismatches\n", bad);
    return bad;
}

typedef std::chrono::steady_clock clk;
template <class F>
static double median_us(F f, int warm = 2, int reps = 9) {
    std::vector<double> t;
    for (int r = 0; r < warm + reps; ++r) {
        const double d = f();
        if (r >= warm) t.push_back(d);
    }
    std::sort(t.begin(), t.end());
    return t[t.size() / 2];
}
static double since(clk::time_point t0) { return std::chrono::duration<double, std::micro>(clk::now() - t0).count(); }

// (a) dhtgpu_ncr_find, host form, against (b) m std::map finds over the same keys
// (what CacheSlots::slotOf does); (c) dhtgpu_ncr_get_nodes against m map finds + free-list pops +
// dhtgpu_nc_insert of the new keys; (d) dhtgpu_ncr_extract against m map finds + dhtgpu_nc_erase.
// Batches: (a, b) half present, half absent; (c) half new; (d) all present.  The mirror is restored
// between timed calls (untimed).
static int bench(size_t n, const std::vector<size_t>& ms) {
    const size_t mmax = *std::max_element(ms.begin(), ms.end());
    std::vector<uint8_t> ids(20 * (n + mmax));
    orc_gen_ids(700, 0, n + mmax, ids.data());
    dhtgpu::Context ctx(0);
    std::map<Slots::Key, uint32_t> host;
    for (size_t i = 0; i < n; ++i) {
        Slots::Key k;
        std::memcpy(k.b, &ids[20 * i], 20);
        host[k] = (uint32_t)i;
    }
    dhtgpu::check(dhtgpu_nc_set(ctx.get(), ids.data(), nullptr, n), "nc_set");
    size_t sink = 0;
    for (size_t m : ms) {
        // batch j: even -> the present key at a random place, odd -> the absent key n + j
        std::vector<uint8_t> mix(20 * m), present(20 * m);
        std::vector<uint32_t> hp(m);
        for (size_t j = 0; j < m; ++j) {
            const size_t at = ((size_t)rnd() << 8 ^ rnd()) % n;
            std::memcpy(&mix[20 * j], &ids[20 * (j % 2 ? n + j : at)], 20);
        }
        const size_t start = ((size_t)rnd() << 8 ^ rnd()) % n;
        for (size_t j = 0; j < m; ++j) {
            hp[j] = (uint32_t)((start + j * 7919) % n);   // 7919 is prime to n = 2^20: distinct
            std::memcpy(&present[20 * j], &ids[20 * hp[j]], 20);
        }
        std::vector<uint32_t> h(m), fresh(m);
        std::vector<uint8_t> nw(m);
        for (size_t j = 0; j < m; ++j) fresh[j] = (uint32_t)(n + j);
        const double a = median_us([&] {
            auto t0 = clk::now();
            dhtgpu::check(dhtgpu_ncr_find(ctx.get(), mix.data(), (uint32_t)m, h.data(), nullptr), "ncr_find");
            return since(t0);
        });
        const double b = median_us([&] {
            auto t0 = clk::now();
            for (size_t j = 0; j < m; ++j) {
                Slots::Key k;
                std::memcpy(k.b, &mix[20 * j], 20);
                const auto it = host.find(k);
                h[j] = it == host.end() ? DHTGPU_NONE : it->second;
            }
            const double d = since(t0);
            sink += h[m / 2];
            return d;
        });
        // the new keys of `mix`, to take out again after each timed emplace
        std::vector<uint8_t> added;
        for (size_t j = 1; j < m; j += 2) added.insert(added.end(), &mix[20 * j], &mix[20 * j] + 20);
        auto restore_c = [&] {
            if (!added.empty())
                dhtgpu::check(dhtgpu_nc_erase(ctx.get(), added.data(), (uint32_t)(added.size() / 20), nullptr), "nc_erase");
        };
        const double c_new = median_us([&] {
            uint32_t used = 0;
            auto t0 = clk::now();
            dhtgpu::check(dhtgpu_ncr_get_nodes(ctx.get(), mix.data(), (uint32_t)m, fresh.data(), (uint32_t)m, nullptr,
                                               h.data(), nw.data(), &used), "ncr_get_nodes");
            const double d = since(t0);
            restore_c();
            return d;
        });
        const double c_old = median_us([&] {
            std::vector<uint32_t> fl(fresh.rbegin(), fresh.rend()), hs;
            std::vector<uint8_t> nk;
            auto t0 = clk::now();
            for (size_t j = 0; j < m; ++j) {
                Slots::Key k;
                std::memcpy(k.b, &mix[20 * j], 20);
                const auto it = host.find(k);
                if (it != host.end()) { h[j] = it->second; continue; }
                h[j] = fl.back();
                fl.pop_back();
                hs.push_back(h[j]);
                nk.insert(nk.end(), k.b, k.b + 20);
            }
            if (!hs.empty())
                dhtgpu::check(dhtgpu_nc_insert(ctx.get(), nk.data(), hs.data(), nullptr, (uint32_t)hs.size(), nullptr), "nc_insert");
            const double d = since(t0);
            restore_c();
            return d;
        });
        auto restore_d = [&] {
            dhtgpu::check(dhtgpu_nc_insert(ctx.get(), present.data(), hp.data(), nullptr, (uint32_t)m, nullptr), "nc_insert");
        };
        const double d_new = median_us([&] {
            auto t0 = clk::now();
            dhtgpu::check(dhtgpu_ncr_extract(ctx.get(), present.data(), (uint32_t)m, h.data()), "ncr_extract");
            const double d = since(t0);
            restore_d();
            return d;
        });
        const double d_old = median_us([&] {
            auto t0 = clk::now();
            for (size_t j = 0; j < m; ++j) {
                Slots::Key k;
                std::memcpy(k.b, &present[20 * j], 20);
                const auto it = host.find(k);
                h[j] = it == host.end() ? DHTGPU_NONE : it->second;
            }
            dhtgpu::check(dhtgpu_nc_erase(ctx.get(), present.data(), (uint32_t)m, nullptr), "nc_erase");
            const double d = since(t0);
            restore_d();
            return d;
        });
        std::printf("ncresolve_check: n=%zu m=%zu: ncr_find (host form) %.1f us, %zu std::map finds %.1f us; "
                    "ncr_get_nodes %.1f us, map finds + pops + nc_insert %.1f us; ncr_extract %.1f us, map finds + nc_erase %.1f us\n",
                    n, m, a, m, b, c_new, c_old, d_new, d_old);
        std::fflush(stdout);
    }
    if (sink == 1) std::puts("");
    return 0;
}

int main(int argc, char** argv) {
    const char* mode = argc >= 2 ? argv[1] : "";
    if (!std::strcmp(mode, "--bench")) {
        std::vector<size_t> ms;
        for (int i = 3; i < argc; ++i) ms.push_back((size_t)std::strtoull(argv[i], nullptr, 10));
        if (ms.empty()) ms = {1, 64, 1024, 16384, 131072};
        return bench(argc >= 3 ? (size_t)std::strtoull(argv[2], nullptr, 10) : (size_t)1 << 20, ms);
    }
    if (std::strcmp(mode, "--host") && std::strcmp(mode, "--run")) { std::puts("built"); return 0; }
    const int total = 12000;
    std::vector<uint8_t> ids(20 * total);
    orc_gen_ids(310, 0, total, ids.data());
    return (!std::strcmp(mode, "--host") ? host_checks(ids) : run_checks(ids, total)) ? 1 : 0;
}
