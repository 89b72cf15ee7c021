// rtgrow_check.cpp -- exercises the growing side of dhtgpu::ResidentTable (include/dhtgpu.hpp,
// C++11: noteNewNode / noteExpire / flush / onNewNodeBatch) against a reference-shaped mock table
// that runs RoutingTable::onNewNode / split (src/routing_table.cpp:204-262, :87-107, :176-202) and
// Dht::expireBuckets (src/dht.cpp:179-192) on the host, as the caller's own table would.
//   (no argument)   prints "built"
//   --host FILE     no device: the mock table's onNewNode / expireBuckets over the operations of
//                   FILE (tests/test_rtgrow_cpu.py writes them), its results and final table
//                   printed -- the test compares them with the Python model's
//   --run           on a GPU: the mirror follows the mock table through notes and flushes; the
//                   device paths of ResidentTable against its host paths after every few steps
#include <array>
#include <cstdio>
#include <cstring>
#include <list>
#include <memory>
#include <vector>

#include "dhtgpu.hpp"
#include "../../oracle/dht_oracle.h"
#include "mock_dht.h"

namespace mock {
struct Node {
    InfoHash id;
    SockAddr addr;
    uint32_t tag;      // the operation that brought it (the --host dump names nodes by it)
    uint8_t state;     // bit 0 good, 1 expired, 2 pending
    bool isGood(long) const { return (state & 1) != 0; }
    bool isExpired() const { return (state & 2) != 0; }
    bool isPendingMessage() const { return (state & 4) != 0; }
    const SockAddr& getAddr() const { return addr; }
};
typedef std::shared_ptr<Node> NodePtr;
}  // namespace mock
typedef mock::Bucket<mock::NodePtr> Bucket;
typedef mock::RoutingTable<mock::NodePtr> RoutingTable;

enum { kNone = 0, kKnown = 1, kPlaced = 2, kReplaced = 3, kFull = 4 };

// InfoHash::lowbit: the position of the last set bit (bit 0 the highest), -1 for the zero id
static int lowbit(const mock::InfoHash& h) {
    for (int i = 19; i >= 0; --i)
        if (h.d[i])
            for (int j = 7; j >= 0; --j)
                if (h.d[i] & (0x80 >> j)) return 8 * i + j;
    return -1;
}

struct HostTable {
    RoutingTable t;
    mock::InfoHash myid;
    bool is_client;
    typedef RoutingTable::iterator It;

    It find_bucket(const mock::InfoHash& id) {
        if (t.empty()) return t.end();
        It b = t.begin();
        for (;;) {
            It nx = std::next(b);
            if (nx == t.end() || std::memcmp(id.data(), nx->first.data(), 20) < 0) return b;
            b = nx;
        }
    }
    bool contains(It b, const mock::InfoHash& id) {
        return std::memcmp(b->first.data(), id.data(), 20) <= 0 &&
               (std::next(b) == t.end() || std::memcmp(id.data(), std::next(b)->first.data(), 20) < 0);
    }
    unsigned depth(It b) {
        const int b1 = lowbit(b->first), b2 = std::next(b) != t.end() ? lowbit(std::next(b)->first) : -1;
        return (unsigned)((b1 > b2 ? b1 : b2) + 1);
    }
    void split(It b) {
        const unsigned bit = depth(b);
        Bucket nb;
        nb.first = b->first;
        nb.first.d[bit / 8] |= (uint8_t)(0x80 >> (bit % 8));
        t.insert(std::next(b), nb);
        std::list<mock::NodePtr> nodes;
        nodes.splice(nodes.begin(), b->nodes);
        while (!nodes.empty()) {
            auto n = nodes.begin();
            It bb = find_bucket((*n)->id);
            bb->nodes.splice(bb->nodes.begin(), nodes, n);
        }
    }
    // the result code; *aux = the evicted node (REPLACED) or the ping pick (FULL), else null
    int on_new_node(const mock::NodePtr& node, mock::NodePtr* aux) {
        for (int round = 0; round < 161; ++round) {
            *aux = mock::NodePtr();
            It b = find_bucket(node->id);
            if (b == t.end()) return kNone;
            for (const auto& n : b->nodes)
                if (n == node) return kKnown;
            const bool mybucket = contains(b, myid);
            if (b->nodes.size() < 8) {
                b->nodes.emplace_front(node);
                return kPlaced;
            }
            for (auto& n : b->nodes)
                if (n->isExpired()) {
                    *aux = n;
                    n = node;
                    return kReplaced;
                }
            bool dubious = false;
            for (const auto& n : b->nodes) {
                if (n->isGood(0)) continue;
                dubious = true;
                if (!*aux && !n->isPendingMessage()) *aux = n;
            }
            const unsigned d = depth(b);
            if (!((mybucket || (is_client && d < 6)) && (!dubious || t.size() == 1)) || d >= 160) return kFull;
            split(b);
        }
        *aux = mock::NodePtr();
        return kFull;
    }
    void expire() {
        for (auto& b : t)
            b.nodes.remove_if([](const mock::NodePtr& n) { return n->isExpired(); });
    }
};

static HostTable one_bucket(const uint8_t* myid, bool client) {
    HostTable h;
    std::memcpy(h.myid.d.data(), myid, 20);
    h.is_client = client;
    Bucket b;
    b.first.d.fill(0);
    h.t.push_back(b);
    return h;
}

static mock::NodePtr make_node(const uint8_t* id, uint32_t tag, uint8_t state) {
    auto n = std::make_shared<mock::Node>();
    std::memcpy(n->id.d.data(), id, 20);
    std::memset(&n->addr, 0, sizeof n->addr);
    std::memcpy(&n->addr.v4.sin_addr, id + 3, 4);   // any bytes: the reply must carry them
    std::memcpy(&n->addr.v4.sin_port, id + 9, 2);
    n->tag = tag;
    n->state = state;
    return n;
}

// FILE: u32 client, myid[20], u32 nops, then per operation u8 kind (0 new, 1 expire, 2 state) and
// for new: id[20], u32 tag, u8 state; for state: u32 tag, u8 state
static int host_ops(const char* path) {
    FILE* f = std::fopen(path, "rb");
    if (!f) { std::perror(path); return 2; }
    uint32_t client, nops;
    uint8_t myid[20];
    if (std::fread(&client, 4, 1, f) != 1 || std::fread(myid, 20, 1, f) != 1 || std::fread(&nops, 4, 1, f) != 1) return 2;
    HostTable h = one_bucket(myid, client != 0);
    std::vector<mock::NodePtr> by_tag;
    for (uint32_t i = 0; i < nops; ++i) {
        uint8_t kind, id[20] = {0}, st;
        uint32_t tag;
        if (std::fread(&kind, 1, 1, f) != 1) return 2;
        if (kind == 1) {
            h.expire();
            std::printf("expire\n");
            continue;
        }
        if (kind == 0 && std::fread(id, 20, 1, f) != 1) return 2;
        if (std::fread(&tag, 4, 1, f) != 1 || std::fread(&st, 1, 1, f) != 1) return 2;
        if (tag >= by_tag.size()) by_tag.resize(tag + 1);
        if (kind == 2) {
            if (by_tag[tag]) by_tag[tag]->state = st;
            continue;
        }
        if (!by_tag[tag]) by_tag[tag] = make_node(id, tag, st);
        mock::NodePtr aux;
        const int r = h.on_new_node(by_tag[tag], &aux);
        std::printf("new %d %ld\n", r, aux ? (long)aux->tag : -1L);
    }
    std::fclose(f);
    for (const auto& b : h.t) {
        for (int i = 0; i < 20; ++i) std::printf("%02x", b.first.d[i]);
        for (const auto& n : b.nodes) std::printf(" %u:%u", n->tag, n->state);
        std::printf("\n");
    }
    return 0;
}

static int run() {
    typedef dhtgpu::ResidentTable<RoutingTable, long> Resident;
    int bad = 0;
    for (int client = 0; client < 2; ++client) {
        std::vector<uint8_t> myid(20), ids(20 * 3000), tg(20 * 96);
        orc_gen_ids(99, 0, 1, myid.data());
        orc_gen_ids(200 + client, 0, 3000, ids.data());
        orc_gen_ids(300, 0, 96, tg.data());
        for (int i = 0; i < 1500; ++i) std::memcpy(&ids[20 * i], myid.data(), 1 + i % 3);   // near myid: deep splits
        HostTable h = one_bucket(myid.data(), client != 0);
        mock::InfoHash my;
        std::memcpy(my.d.data(), myid.data(), 20);
        dhtgpu::Context ctx(0);
        Resident rt(ctx, my);
        rt.min_device_batch = rt.min_reply_batch = 1;
        rt.is_client = client != 0;
        if (!client) rt.max_flush_nodes = 4096;   // the device route whatever the queue holds; the client run
                                                  // keeps the default and so takes the assign fallback too
        rt.assign(h.t, 4);
        std::vector<mock::InfoHash> targets(96);
        for (int i = 0; i < 96; ++i) std::memcpy(targets[i].d.data(), &tg[20 * i], 20);
        std::vector<mock::NodePtr> all;
        for (int i = 0; i < 3000; ++i) {
            static const uint8_t states[] = {1, 1, 1, 1, 0, 4, 2, 5};
            mock::NodePtr n = make_node(&ids[20 * i], (uint32_t)i, states[(i * 7 + i / 9) % 8]), aux;
            all.push_back(n);
            h.on_new_node(n, &aux);
            rt.noteNewNode(n, 0L);
            if (i % 211 == 210) {   // some nodes expire, the sweep follows; the mirror learns the states first
                for (size_t k = i % 5; k < all.size(); k += 13)
                    if (!(all[k]->state & 1)) all[k]->state = 2;
                rt.refresh(h.t, 0L);
                h.expire();
                rt.noteExpire();
            }
            if (i % 97 != 96 && i != 2999) continue;
            rt.refresh(h.t, 0L);
            for (size_t count : {8u, 14u}) {
                const auto got = rt.findClosestNodesBatch(h.t, targets.data(), targets.size(), 0L, count);
                for (size_t q = 0; q < targets.size(); ++q) {
                    std::vector<mock::NodePtr> want;
                    dhtgpu::detail::find_closest_host(h.t, targets[q], 0L, count, want);
                    if (got[q] != want) ++bad;
                }
            }
            const auto rep = rt.replyNodesBatch(h.t, targets.data(), targets.size(), 0L);
            for (size_t q = 0; q < targets.size(); ++q)
                if (rep[q] != dhtgpu::detail::reply_nodes_host(h.t, targets[q], 0L, false)) ++bad;
        }
        size_t live = 0, held = 0;
        for (const auto& b : h.t) live += b.nodes.size();
        for (const auto& n : rt.handles()) held += n ? 1 : 0;
        if (live != held) ++bad;   // every handle names a resident node: evicted and expired ones were freed
        std::printf("rtgrow_check: client %d, %zu buckets, %zu nodes, %zu handles\n", client, h.t.size(), live, rt.handles().size());
        // stand-alone: the same nodes through onNewNodeBatch on a fresh one-bucket mirror
        HostTable h2 = one_bucket(myid.data(), client != 0);
        rt.assign(h2.t, 0);
        std::vector<mock::InfoHash> xs(3000);
        std::vector<uint32_t> hs(3000);
        for (int i = 0; i < 3000; ++i) {
            std::memcpy(xs[i].d.data(), &ids[20 * i], 20);
            hs[i] = (uint32_t)i;
        }
        const std::vector<uint8_t> res = rt.onNewNodeBatch(xs.data(), hs.data(), nullptr, nullptr, 3000);
        for (int i = 0; i < 3000; ++i) {
            mock::NodePtr aux;
            if (h2.on_new_node(make_node(&ids[20 * i], (uint32_t)i, 1), &aux) != res[i]) ++bad;
        }
    }
    std::printf("rtgrow_check: %d mismatches\n", bad);
    return bad ? 1 : 0;
}

int main(int argc, char** argv) {
    if (argc >= 3 && std::strcmp(argv[1], "--host") == 0) return host_ops(argv[2]);
    if (argc >= 2 && std::strcmp(argv[1], "--run") == 0) return run();
    std::puts("built");
    return 0;
}
