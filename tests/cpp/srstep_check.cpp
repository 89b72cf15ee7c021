// srstep_check.cpp -- exercises dhtgpu::ResidentSearches::noteRequest / noteClock / stepBatch
// (include/dhtgpu.hpp, C++11) against a struct-based restatement of Dht::searchStep for the find_node
// search: the state lives in SearchNode objects that std::vector moves and destroys, as in the
// reference -- a second model, of another construction than tests/srstep_cases.py's.
//   (no argument)   build check: prints "built"
//   --host          no device: the restatement against literal cases taken from the reference, and
//                   the adapter's queue
//   --run [--quick] on a GPU: seeded traffic -- replies, expiries, offers and steps -- through the
//                   restatement and through the adapter, compared after every round
//   --bench         no device: the restatement's time per step call at 1, 1,024 and 16,384 searches
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstring>
#include <map>
#include <memory>
#include <vector>

#include "dhtgpu.hpp"
#include "mock_dht.h"

namespace mock {
typedef uint32_t time_point;   // clock ticks; 0 is time_point::min()
struct Node {
    InfoHash id;
    bool expired, client, removable;
    time_point time;
    uint32_t index;
    bool isExpired() const { return expired; }
    bool isClient() const { return client; }
    bool isRemovable(time_point) const { return removable; }
    void setTime(time_point t) { time = t; }
};
typedef std::shared_ptr<Node> NodeSp;
typedef std::map<InfoHash, std::weak_ptr<Node>> NodeMap;

static const uint32_t kNodeExpire = 600;   // Node::NODE_EXPIRE_TIME in ticks

// SearchNode with the one ANY_QUERY request of a find_node search: req 0 none, 1 pending, 2 completed
struct SearchNode {
    NodeSp node;
    time_point last_get_reply;
    bool candidate, token;
    int req;
    SearchNode() : node(), last_get_reply(0), candidate(false), token(false), req(0) {}
    SearchNode(const SearchNode&) = delete;
    SearchNode(SearchNode&&) = default;
    SearchNode& operator=(SearchNode&&) = default;
    SearchNode(const NodeSp& n) : node(n), last_get_reply(0), candidate(false), token(false), req(0) {}
    bool isBad() const { return !node || node->isExpired() || candidate; }
    bool pendingGet() const { return req == 1; }
    // src/search.h:110-113
    bool isSynced(time_point now) const {
        return !node->isExpired() && token && last_get_reply != 0 && (uint64_t)last_get_reply + kNodeExpire >= now;
    }
    // src/search.h:139-161 with getStatus = {ANY_QUERY: req} and no pagination
    bool canGet(time_point now) const {
        if (node->isExpired()) return false;
        const bool pending = req == 1, completed_sq = req == 2, pending_sq = req == 1;
        const bool stale = last_get_reply == 0 || now > (uint64_t)last_get_reply + kNodeExpire;
        return (!pending && stale) || !(completed_sq || pending_sq);
    }
};

inline int xor_cmp(const InfoHash& t, const InfoHash& a, const InfoHash& b) {
    for (int i = 0; i < 20; ++i) {
        const uint8_t x = a.d[i] ^ t.d[i], y = b.d[i] ^ t.d[i];
        if (x != y) return x < y ? -1 : 1;
    }
    return 0;
}

struct Search {
    static const size_t kSearchNodes = 14, kTargetNodes = 8, kMaxRequested = 4, kMaxBad = 25;
    InfoHash id;
    bool expired, done;
    time_point refill_time;
    std::vector<SearchNode> nodes;
    Search() : expired(false), done(false), refill_time(0) {}
    size_t bad_count() const {
        size_t b = 0;
        for (const auto& sn : nodes) b += sn.isBad();
        return b;
    }
    // src/search.h:636-722
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
            nodes[n].token = true;
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
    unsigned solicited() const {
        unsigned c = 0;
        for (const auto& n : nodes) c += !n.isBad() && n.pendingGet();
        return c;
    }
    bool isSynced(time_point now) const {
        unsigned i = 0;
        for (const auto& n : nodes) {
            if (n.isBad()) continue;
            if (!n.isSynced(now)) return false;
            if (++i == kTargetNodes) break;
        }
        return i > 0;
    }
    void setDone() {
        for (auto& n : nodes) n.req = 0;
        done = true;
    }
    // Dht::searchStep (src/dht.cpp:562-654) with no callbacks, announces or listeners; `sent` gets the
    // nodes of the find_node requests; returns the bits of dhtgpu_srs_step; *inserted = refill's count
    unsigned step(const NodeMap& cache, time_point now, size_t refill_count, std::vector<NodeSp>& sent, unsigned* inserted) {
        *inserted = 0;
        if (expired || done) return 32u | (expired ? 1u : 0u) | (done ? 4u : 0u);
        unsigned bits = 0;
        if (refill_count && (uint64_t)refill_time + kNodeExpire < now && nodes.size() - bad_count() < kSearchNodes) {
            refill_time = now;
            for (const NodeSp& n : dhtgpu::detail::cached_nodes_host(cache, id, refill_count))
                if (insertNode(n, now)) ++*inserted;
            bits |= 8u;
        }
        if (isSynced(now)) {
            setDone();
            bits |= 16u;
        }
        if (!done) {
            while (solicited() < kMaxRequested) {   // searchSendGetValues: the first node that can be asked
                SearchNode* n = nullptr;
                for (auto& sn : nodes)
                    if (sn.canGet(now)) { n = &sn; break; }
                if (!n) break;
                n->req = 1;
                sent.push_back(n->node);
            }
        }
        size_t lead = 0;
        while (lead < nodes.size() && nodes[lead].isBad()) ++lead;
        if (lead >= std::min(nodes.size(), kMaxBad)) {   // Search::expire()
            expired = true;
            nodes.clear();
            done = true;
        }
        return bits | (expired ? 1u : 0u) | (done ? 4u : 0u);
    }
};
const size_t Search::kSearchNodes, Search::kTargetNodes, Search::kMaxRequested, Search::kMaxBad;
typedef std::map<InfoHash, std::shared_ptr<Search>> SearchMap;

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

using mock::NodeSp;

static mock::Xorshift rng = {0x9E3779B97F4A7C15ull};
static uint32_t rnd() { return (uint32_t)(rng.step() >> 16); }

struct World {
    std::vector<NodeSp> nodes;
    mock::NodeMap map;
    mock::SearchMap searches;              // by target, as Dht::searches(af)
    std::vector<mock::Search*> by_slot;
};

static void build_world(World& w, int total, int S) {
    for (int i = 0; i < total; ++i) {
        auto n = std::make_shared<mock::Node>();
        for (int b = 0; b < 20; ++b) n->id.d[b] = (uint8_t)rnd();
        n->expired = n->removable = false;
        n->client = (rnd() % 10) == 0;
        n->time = 0;
        n->index = (uint32_t)i;
        w.nodes.push_back(n);
        w.map[n->id] = n;
    }
    while ((int)w.searches.size() < S) {
        auto sr = std::make_shared<mock::Search>();
        for (int b = 0; b < 20; ++b) sr->id.d[b] = (uint8_t)rnd();
        w.searches[sr->id] = sr;
    }
}

// a list of n nodes at increasing distance from an all-zero target, the first nbad of them expired, for
// the literal cases
static void literal_list(World& w, mock::Search& sr, int n, int nbad = 0) {
    sr.id.d.fill(0);
    for (int i = 0; i < n; ++i) {
        auto nd = std::make_shared<mock::Node>();
        nd->id.d.fill(0);
        nd->id.d[19] = (uint8_t)(i + 1);
        nd->removable = nd->client = false;
        nd->expired = i < nbad;
        nd->time = 0;
        nd->index = (uint32_t)w.nodes.size();
        w.nodes.push_back(nd);
        sr.insertNode(nd, 1);
    }
}

static int literal_cases() {
    int bad = 0;
    World w;
    std::vector<NodeSp> sent;
    unsigned ins;
    {   // 3 good entries, never asked: 3 requests
        mock::Search s;
        literal_list(w, s, 3);
        bad += s.step(w.map, 1000, 0, sent, &ins) != 0 || sent.size() != 3 || s.solicited() != 3;
    }
    {   // 6: the first 4
        mock::Search s;
        literal_list(w, s, 6);
        sent.clear();
        bad += s.step(w.map, 1000, 0, sent, &ins) != 0 || sent.size() != 4 || sent[3] != s.nodes[3].node || s.nodes[4].req != 0;
    }
    {   // [cand, good, cand, good, good, good, good]: entries 0-5
        mock::Search s;
        literal_list(w, s, 7);
        s.nodes[0].candidate = s.nodes[2].candidate = true;
        sent.clear();
        bad += s.step(w.map, 1000, 0, sent, &ins) != 0 || sent.size() != 6 || s.solicited() != 4 || s.nodes[6].req != 0;
    }
    for (int stale = 0; stale < 2; ++stale) {   // 8 replied at 400 (one at 399): synced and done / that one asked again
        mock::Search s;
        literal_list(w, s, 8);
        for (auto& n : s.nodes) {
            n.token = true;
            n.last_get_reply = 400;
            n.req = 2;
        }
        if (stale) s.nodes[5].last_get_reply = 399;
        sent.clear();
        const unsigned bits = s.step(w.map, 1000, 0, sent, &ins);
        if (stale) bad += bits != 0 || sent.size() != 1 || sent[0] != s.nodes[5].node;
        else bad += bits != (16u | 4u) || !sent.empty() || s.solicited() != 0 || s.nodes[0].req != 0 ||
                    s.step(w.map, 1001, 0, sent, &ins) != (32u | 4u);
    }
    {   // an empty list expires
        mock::Search s;
        sent.clear();
        bad += s.step(w.map, 1000, 0, sent, &ins) != (1u | 4u);
    }
    const int shapes[3][3] = {{26, 25, 1}, {24, 24, 1}, {30, 24, 0}};   // entries, leading bad, expires
    for (const auto& sh : shapes) {
        mock::Search s;
        literal_list(w, s, sh[0], sh[1]);
        bad += (int)s.nodes.size() != sh[0];
        sent.clear();
        const unsigned bits = s.step(w.map, 1000, 0, sent, &ins);
        bad += ((bits & 1u) != 0) != (sh[2] != 0) || (sh[2] && !s.nodes.empty());
    }
    return bad;
}

// the device's view of one search against the restatement's
template <class RS, class CacheT>
static int differs(dhtgpu_ctx* ctx, CacheT& cache, uint32_t slot, const mock::Search& sr) {
    uint32_t rows[DHTGPU_SR_CAP], len = 0, tick[DHTGPU_SR_CAP], st[4];
    uint8_t flags[DHTGPU_SR_CAP], req[DHTGPU_SR_CAP];
    dhtgpu::check(dhtgpu_sr_lists(ctx, &slot, 1, rows, flags, &len), "sr_lists");
    dhtgpu::check(dhtgpu_srs_entries(ctx, &slot, 1, req, tick), "srs_entries");
    dhtgpu::check(dhtgpu_sr_status(ctx, &slot, 1, st), "sr_status");
    if (len != sr.nodes.size() || ((st[3] & 1u) != 0) != sr.expired) return 1;
    for (size_t j = 0; j < sr.nodes.size(); ++j) {
        const mock::SearchNode& n = sr.nodes[j];
        if (rows[j] != cache.slots().slotOf(n.node->id) || (flags[j] & 1u) != (n.candidate ? 1u : 0u) ||
            ((flags[j] & 2u) != 0) != n.token || req[j] != (uint8_t)n.req || tick[j] != n.last_get_reply)
            return 1;
    }
    return 0;
}

static int traffic(dhtgpu::Context& ctx, int total, int S, int rounds) {
    typedef dhtgpu::ResidentCache<mock::NodeMap> Cache;
    typedef dhtgpu::ResidentSearches<mock::NodeMap, mock::Search> RS;
    int bad = 0;
    World w;
    build_world(w, total, S);
    Cache rc(ctx);
    rc.assign(w.map);
    RS rs(rc, w.map, (uint32_t)S);
    std::vector<uint32_t> slots;
    for (auto& kv : w.searches) {
        slots.push_back(rs.open(kv.first));
        w.by_slot.push_back(kv.second.get());
    }
    mock::time_point now = 1000;
    int flips = 0, seen = 0, victim = -1;
    for (int round = 0; round < rounds; ++round) {
        const uint32_t dts[5] = {1, 7, 50, mock::kNodeExpire, mock::kNodeExpire + 1};
        now += dts[rnd() % 5];
        for (int i = 0; i < 4 && flips < 30; ++i, ++flips) {   // at most 30 nodes ever turn bad
            NodeSp& n = w.nodes[rnd() % w.nodes.size()];
            if (rnd() % 2) n->expired = true;
            else n->removable = true;
        }
        rs.refresh(now);
        rc.refresh();
        // a step of some searches (distinct slots), with and without the refill leg
        std::vector<uint32_t> pick;
        for (int s = 0; s < S; ++s)
            if (rnd() % 3 != 0 || s == victim) pick.push_back(slots[s]);
        const uint32_t count = round % 4 == 3 ? 0u : 14u;
        const std::vector<RS::Step> got = rs.stepBatch(pick.data(), pick.size(), now, mock::kNodeExpire, count);
        rs.noteClock(now);   // (already the clock: the replies below are stamped with it)
        for (size_t i = 0; i < pick.size(); ++i) {
            mock::Search& sr = *w.by_slot[pick[i]];
            std::vector<NodeSp> want;
            unsigned ins = 0;
            const unsigned bits = sr.step(w.map, now, count, want, &ins);
            seen |= (int)bits;
            bad += (bits != (got[i].bits & ~2u)) || ins != got[i].inserted || want != got[i].send ||
                   (!sr.expired && sr.solicited() != got[i].solicited);
            // what becomes of each request: a reply with a token and a node it tells about, an expiry, nothing
            for (const NodeSp& n : want) {
                if (sr.expired) break;
                const uint32_t u = rnd() % 10;
                mock::SearchNode* sn = nullptr;
                for (auto& x : sr.nodes)
                    if (x.node == n) sn = &x;
                if (!sn) continue;
                if (u < 7) {
                    sn->req = 2;
                    rs.noteRequest(pick[i], n, 2);
                    sr.insertNode(n, now, true);
                    rs.noteInsert(pick[i], n, true);
                    const NodeSp& told = w.nodes[rnd() % w.nodes.size()];
                    sr.insertNode(told, now, false);
                    rs.noteInsert(pick[i], told, false);
                } else if (u < 9 && flips < 30) {
                    ++flips;
                    sn->req = 0;
                    sn->candidate = true;
                    rs.noteRequest(pick[i], n, 0);
                    rs.noteCandidate(pick[i], n, true);
                }
            }
        }
        // learned nodes offered to every search, on the host and on the device side of the threshold in turn
        std::vector<NodeSp> offer;
        for (int i = 0; i < 6; ++i) offer.push_back(w.nodes[rnd() % w.nodes.size()]);
        rs.min_offer_batch = round % 2 ? 1 : (size_t)-1;
        rs.offerBatch(w.searches, offer.data(), offer.size(), now);
        rs.flush();
        for (int s = 0; s < S; ++s) bad += differs<RS>(ctx.get(), rc, slots[s], *w.by_slot[slots[s]]);
        // one search loses every node of its list; the next round steps it without the refill leg: Search::expire()
        victim = -1;
        if (round % 4 == 2) {
            for (int s = 0; s < S && victim < 0; ++s) {
                mock::Search& sr = *w.by_slot[slots[s]];
                if (!sr.done && !sr.expired && !sr.nodes.empty() && sr.nodes.size() <= 16) victim = s;
            }
            if (victim >= 0)
                for (auto& sn : w.by_slot[slots[victim]]->nodes) sn.node->expired = true;
        }
    }
    if ((seen & (1 | 4 | 8 | 16 | 32)) != (1 | 4 | 8 | 16 | 32)) {
        std::printf("srstep_check: the traffic did not reach every leg (bits seen %d)\n", seen);
        ++bad;
    }
    return bad;
}

int main(int argc, char** argv) {
    const bool host_only = argc >= 2 && std::strcmp(argv[1], "--host") == 0;
    const bool bench = argc >= 2 && std::strcmp(argv[1], "--bench") == 0;
    if (argc < 2 || (std::strcmp(argv[1], "--run") != 0 && !host_only && !bench)) { std::puts("built"); return 0; }
    const bool quick = argc >= 3 && std::strcmp(argv[2], "--quick") == 0;
    std::setvbuf(stdout, nullptr, _IOLBF, 0);
    if (host_only) {
        int bad = literal_cases();
        // the adapter's queue with no device behind it: four kinds queued, a closed slot's entries leave, the clock stays
        World w;
        build_world(w, 50, 3);
        mock::HostCache hc;
        for (const auto& n : w.nodes) hc.s.noteInsert(n->id, n);
        dhtgpu::ResidentSearches<mock::NodeMap, mock::Search, mock::HostCache> rs(hc, w.map, 3);
        std::vector<uint32_t> slots;
        for (auto& kv : w.searches) slots.push_back(rs.open(kv.first));
        rs.noteClock(slots[1] ? slots[1] : 1);   // a tick that equals a slot's number
        rs.noteRequest(slots[0], w.nodes[1], 1);
        rs.noteRequest(slots[1], w.nodes[2], 2);
        rs.noteInsert(slots[0], w.nodes[1], true);
        bad += rs.pending() != 7;
        rs.close(slots[1]);   // that slot's open and request leave the queue; the clock stays
        bad += rs.pending() != 5;
        bool threw = false;   // stepBatch needs the device
        try { rs.stepBatch(slots.data(), 1, 9, mock::kNodeExpire); } catch (const dhtgpu::Error&) { threw = true; }
        bad += !threw;
        std::printf("srstep_check (host paths): %d mismatches\n", bad);
        return bad ? 1 : 0;
    }
    if (bench) {   // the CPU body: one searchStep per search and call, lists converged by earlier steps and replies
        using clk = std::chrono::steady_clock;
        const int sizes[3] = {1, 1024, 16384};
        for (int S : sizes) {
            World w;
            build_world(w, 6000, S);
            std::vector<mock::Search*> srs;
            for (auto& kv : w.searches) srs.push_back(kv.second.get());
            std::vector<NodeSp> sent;
            unsigned ins;
            mock::time_point now = 1000;
            double best = 1e30;
            size_t sink = 0;
            for (int rep = 0; rep < 7; ++rep) {
                now += 50;
                const auto t0 = clk::now();
                for (mock::Search* sr : srs) {
                    sent.clear();
                    sr->step(w.map, now, 14, sent, &ins);
                    sink += sent.size();
                    if (rep % 2 == 0)    // every other call the requests are answered, so that the next one sends again
                        for (const NodeSp& n : sent) {
                            sr->insertNode(n, now, true);
                            for (auto& x : sr->nodes)
                                if (x.node == n) x.req = 2;
                        }
                    if (sr->done && !sr->expired) sr->done = false;   // keep stepping a synced search
                }
                const double us = std::chrono::duration<double, std::micro>(clk::now() - t0).count();
                if (rep && us < best) best = us;
            }
            std::printf("srstep_check: host searchStep body, %d searches over %zu keys: %.1f us per call (%.3f us per search)%s\n",
                        S, w.map.size(), best, best / S, sink == 1 ? " " : "");
        }
        return 0;
    }
    dhtgpu::Context ctx(0);
    int bad = traffic(ctx, 600, 40, quick ? 12 : 40);
    std::printf("srstep_check (device paths): %d mismatches\n", bad);
    return bad ? 1 : 0;
}
