// accept_check.cpp -- exercises the accept-mask members of dhtgpu::ClosestIndex (include/dhtgpu.hpp,
// C++11) against a mock node type with isGood(now).  Build-only on CPU (tests/test_accept_cpu.py);
// with --run on a GPU it compares set_accept_good + query, update_accept and write with a host
// brute force over detail::xor_closer and exits non-zero on mismatch.
#include <algorithm>
#include <array>
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>

#include "dhtgpu.hpp"
#include "mock_dht.h"

namespace mock {
struct Node {
    InfoHash id;
    long good_until;
    bool isGood(long now) const { return now < good_until; }
};
}  // namespace mock

static mock::Xorshift rng = {0x9E3779B97F4A7C15ull};
static uint32_t rnd() { return (uint32_t)(rng.step() >> 16); }
static mock::InfoHash rnd_hash() {
    mock::InfoHash h;
    for (size_t i = 0; i < h.d.size(); ++i) h.d[i] = (uint8_t)rnd();
    return h;
}

// the k closest accepted ids of `ids` to t, ascending by xorCmp, equal ids by lower index
static std::vector<uint32_t> brute(const std::vector<mock::InfoHash>& ids, const std::vector<uint8_t>& acc,
                                   const mock::InfoHash& t, size_t k) {
    std::vector<uint32_t> v;
    for (uint32_t i = 0; i < ids.size(); ++i)
        if (acc[i]) v.push_back(i);
    const size_t m = std::min(k, v.size());
    std::partial_sort(v.begin(), v.begin() + m, v.end(), [&](uint32_t a, uint32_t b) {
        if (dhtgpu::detail::xor_closer(t.data(), ids[a].data(), ids[b].data())) return true;
        if (dhtgpu::detail::xor_closer(t.data(), ids[b].data(), ids[a].data())) return false;
        return a < b;
    });
    v.resize(m);
    return v;
}

static int compare(dhtgpu::ClosestIndex& index, const std::vector<mock::InfoHash>& ids, const std::vector<uint8_t>& acc,
                   const std::vector<mock::InfoHash>& targets, size_t k, const char* what) {
    const std::vector<std::vector<uint32_t>> got = index.query(targets.data(), targets.size(), k);
    int bad = 0;
    for (size_t i = 0; i < targets.size(); ++i)
        if (got[i] != brute(ids, acc, targets[i], k)) ++bad;
    std::printf("%s: %d of %zu rows differ\n", what, bad, targets.size());
    return bad;
}

int main(int argc, char** argv) {
    if (argc < 2 || std::strcmp(argv[1], "--run") != 0) { std::puts("built"); return 0; }
    const size_t n = 5000, q = 2000, k = 8;
    const long now = 1000;
    std::vector<std::shared_ptr<mock::Node>> nodes(n);
    std::vector<mock::InfoHash> ids(n), targets(q);
    std::vector<uint8_t> acc(n);
    for (size_t i = 0; i < n; ++i) {
        ids[i] = rnd_hash();
        if (rnd() % 16 == 0) continue;   // an empty slot: not accepted
        nodes[i] = std::make_shared<mock::Node>();
        nodes[i]->id = ids[i];
        nodes[i]->good_until = (rnd() % 10) >= 4 ? now + 1 : now;   // ~60 % good
    }
    for (size_t i = 0; i < n; ++i) acc[i] = nodes[i] && nodes[i]->isGood(now) ? 1 : 0;
    for (size_t i = 0; i < q; ++i) targets[i] = i % 4 ? rnd_hash() : ids[rnd() % n];   // a quarter are members
    int bad = 0;
    try {
        dhtgpu::Context ctx(0);
        dhtgpu::ClosestIndex index(ctx);
        index.assign(ids.data(), n);
        index.set_accept_good(nodes, now);
        bad += compare(index, ids, acc, targets, k, "set_accept_good");
        // expire 100 good nodes, revive 100 others
        std::vector<uint32_t> idx;
        std::vector<uint8_t> val;
        for (uint32_t i = 0; i < n && idx.size() < 200; ++i)
            if (nodes[i] && (idx.size() < 100) == (acc[i] != 0)) {
                idx.push_back(i);
                val.push_back(acc[i] ? 0 : 1);
            }
        for (size_t j = 0; j < idx.size(); ++j) acc[idx[j]] = val[j];
        index.update_accept(idx.data(), val.data(), idx.size());
        bad += compare(index, ids, acc, targets, k, "update_accept");
        // slot reuse: a dead node's slot gets a new id (a target, so that it shows), then is masked on
        const uint32_t slot = idx[0];
        const uint8_t on = 1;
        ids[slot] = targets[1];
        index.write(slot, &ids[slot], 1);
        bad += compare(index, ids, acc, targets, k, "write (masked off)");
        acc[slot] = 1;
        index.update_accept(&slot, &on, 1);
        bad += compare(index, ids, acc, targets, k, "write (masked on)");
        index.set_accept(acc.data(), acc.size());
        bad += compare(index, ids, acc, targets, k, "set_accept");
        index.clear_accept();
        std::fill(acc.begin(), acc.end(), 1);
        bad += compare(index, ids, acc, targets, k, "clear_accept");
    } catch (const dhtgpu::Error& e) {
        std::printf("dhtgpu error: %s\n", e.what());
        return 2;
    }
    std::printf("accept_check: %d mismatches\n", bad);
    return bad ? 1 : 0;
}
