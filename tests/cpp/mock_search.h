// mock_search.h -- Dht::Search / SearchNode of the reference's shape, the search map and the cache
// stand-in that the resident searches' checks (rsearch_check.cpp, srmap_check.cpp) run against.
// Include it after mock_dht.h and after the program's own mock::time_point and mock::Node (id,
// isExpired(), isRemovable(now), setTime(now)).
#ifndef DHTGPU_TESTS_MOCK_SEARCH_H
#define DHTGPU_TESTS_MOCK_SEARCH_H
#include <map>
#include <memory>
#include <vector>

#include "dhtgpu.hpp"
#include "mock_dht.h"

namespace mock {
typedef std::shared_ptr<Node> NodeSp;
typedef std::map<InfoHash, std::weak_ptr<Node>> NodeMap;

struct SearchNode {
    NodeSp node;
    time_point last_get_reply;
    bool candidate;
    SearchNode() : node(), last_get_reply(-1), candidate(false) {}
    SearchNode(const SearchNode&) = delete;
    SearchNode(SearchNode&&) = default;
    SearchNode& operator=(SearchNode&&) = default;
    SearchNode(const NodeSp& n) : node(n), last_get_reply(-1), candidate(false) {}
    bool isBad() const { return !node || node->isExpired() || candidate; }
};

inline int xor_cmp(const InfoHash& t, const InfoHash& a, const InfoHash& b) {
    for (int i = 0; i < 20; ++i) {
        const uint8_t x = a.d[i] ^ t.d[i], y = b.d[i] ^ t.d[i];
        if (x != y) return x < y ? -1 : 1;
    }
    return 0;
}

// Dht::Search with insertNode written after the oracle's restatement (oracle/dht_oracle.cpp, OrcSearch)
struct Search {
    static const size_t kSearchNodes = 14;
    InfoHash id;
    bool expired, done;
    std::vector<SearchNode> nodes;
    size_t index;   // in the oracle's arrays, where the program keeps one
    Search() : expired(false), done(false), index(0) {}
    size_t bad_count() const {
        size_t b = 0;
        for (const auto& sn : nodes) b += sn.isBad();
        return b;
    }
    bool insertNode(const NodeSp& snode, time_point now, bool token = false) {
        bool found = false;
        size_t n = nodes.size();
        while (n != 0) {
            --n;
            if (nodes[n].node == snode) { found = true; break; }
            if (xor_cmp(id, snode->id, nodes[n].node->id) > 0) { ++n; break; }
        }
        bool new_search_node = false;
        if (!found) {
            size_t t = nodes.size(), bad = 0;
            bool full = false;
            if (expired) {
                if (nodes.size() >= kSearchNodes) { full = true; t = kSearchNodes; }
            } else {
                bad = bad_count();
                full = nodes.size() - bad >= kSearchNodes;
                while (t - bad > kSearchNodes) {
                    --t;
                    if (nodes[t].isBad()) bad--;
                }
            }
            if (full) {
                if (t != nodes.size()) nodes.resize(t);
                if (n >= t) return false;
            }
            nodes.insert(nodes.begin() + n, SearchNode(snode));
            snode->setTime(now);
            new_search_node = true;
            if (snode->isExpired()) {
                if (!expired) bad++;
            } else if (expired) {
                bad = nodes.size() - 1;
                expired = false;
            }
            while (nodes.size() - bad > kSearchNodes) {
                if (!expired && nodes.back().isBad()) bad--;
                nodes.pop_back();
            }
        }
        if (token && n < nodes.size() && nodes[n].node == snode) {
            nodes[n].candidate = false;
            nodes[n].last_get_reply = now;
            expired = false;
        }
        if (new_search_node) {
            for (size_t e = nodes.size(); e != 0;) {
                --e;
                if (nodes[e].node->isRemovable(now)) {
                    nodes.erase(nodes.begin() + e);
                    break;
                }
            }
        }
        return new_search_node;
    }
};
typedef std::map<InfoHash, std::shared_ptr<Search>> SearchMap;

// ResidentSearches' view of a cache when no device is there: the slots only
struct HostCache {
    typedef dhtgpu::CacheSlots<Node> Slots;
    typedef Slots::NodePtr NodePtr;
    typedef Slots::Key Key;
    Slots s;
    const Slots& slots() const { return s; }
    void flush() {}
    dhtgpu::Context& context() const { throw dhtgpu::Error(DHTGPU_EDEVICE, "no device in this check"); }
};
}  // namespace mock
#endif
