// rtable_check.cpp -- exercises dhtgpu::ResidentTable (include/dhtgpu.hpp, C++11) against
// reference-shaped mock types: adapter_check.cpp's table shape plus the node's socket address
// (getAddr().getIPv4() / getIPv6(), what bufferNodes reads).
//   (no argument)   prints "built"
//   --host          no device: the host fallback of replies and closeness tests (what batches
//                   below the device threshold run) against the oracle on a grown table
//   --tables FILE   no device: detail::find_closest_host against the oracle on the table
//                   snapshots of FILE (tests/rtable_cases.py writes them), every target at every
//                   count
//   --run           on a GPU: the device paths of ResidentTable against its host paths and the
//                   oracle, and the host cost per target of a reply (the threshold's host side)
#include <array>
#include <chrono>
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
    bool good;
    bool isGood(long) const { return good; }
    const SockAddr& getAddr() const { return addr; }
};
}  // namespace mock
typedef mock::Bucket<std::shared_ptr<mock::Node>> Bucket;
typedef mock::RoutingTable<std::shared_ptr<mock::Node>> RoutingTable;

static mock::Xorshift rng = {88172645463325252ull};
static uint32_t rnd() { return (uint32_t)rng.step(); }

// a snapshot (the arguments of orc_find_closest) as the mock table; tails (nullable): alen + 2
// bytes per node, copied into the address family's sockaddr
static RoutingTable make_table(uint32_t nb, const uint8_t* firsts, const uint32_t* off, const uint8_t* nodes,
                               const uint8_t* good, const uint8_t* tails, uint32_t alen) {
    RoutingTable table;
    for (uint32_t b = 0; b < nb; ++b) {
        Bucket bk;
        std::memcpy(bk.first.d.data(), firsts + 20 * b, 20);
        for (uint32_t i = off[b]; i < off[b + 1]; ++i) {
            auto n = std::make_shared<mock::Node>();
            std::memcpy(n->id.d.data(), nodes + 20 * i, 20);
            n->good = good[i] != 0;
            std::memset(&n->addr, 0, sizeof n->addr);
            if (tails && alen == 4) {
                std::memcpy(&n->addr.v4.sin_addr, tails + 6 * i, 4);
                std::memcpy(&n->addr.v4.sin_port, tails + 6 * i + 4, 2);
            } else if (tails) {
                std::memcpy(&n->addr.v6.sin6_addr, tails + 18 * i, 16);
                std::memcpy(&n->addr.v6.sin6_port, tails + 18 * i + 16, 2);
            }
            bk.nodes.push_back(n);
        }
        table.push_back(bk);
    }
    return table;
}

static bool read_u32(FILE* f, uint32_t* v) { return std::fread(v, 4, 1, f) == 1; }

// FILE: cases of {nb, nn, q, ncounts, counts[ncounts], firsts[nb*20], off[nb+1], nodes[nn*20], good[nn], targets[q*20]}
static int check_tables(const char* path) {
    FILE* f = std::fopen(path, "rb");
    if (!f) { std::perror(path); return 2; }
    int bad = 0, cases = 0;
    uint32_t nb;
    while (read_u32(f, &nb)) {
        uint32_t nn, q, nc;
        if (!read_u32(f, &nn) || !read_u32(f, &q) || !read_u32(f, &nc)) return 2;
        std::vector<uint32_t> counts(nc), off(nb + 1);
        std::vector<uint8_t> firsts(20 * (size_t)nb + 1), nodes(20 * (size_t)nn + 1), good(nn + 1), tg(20 * (size_t)q + 1);
        if (std::fread(counts.data(), 4, nc, f) != nc || std::fread(firsts.data(), 20, nb, f) != nb ||
            std::fread(off.data(), 4, nb + 1, f) != nb + 1 || std::fread(nodes.data(), 20, nn, f) != nn ||
            std::fread(good.data(), 1, nn, f) != nn || std::fread(tg.data(), 20, q, f) != q)
            return 2;
        const RoutingTable table = make_table(nb, firsts.data(), off.data(), nodes.data(), good.data(), nullptr, 0);
        for (uint32_t i = 0; i < q; ++i) {
            mock::InfoHash t;
            std::memcpy(t.d.data(), &tg[20 * i], 20);
            for (uint32_t count : counts) {
                uint32_t want[64];
                std::vector<std::shared_ptr<mock::Node>> got;
                dhtgpu::detail::find_closest_host(table, t, 0L, count, got);
                const uint32_t c = orc_find_closest(nb, firsts.data(), off.data(), nodes.data(), good.data(), &tg[20 * i],
                                                    count, want);
                if (got.size() != c) { ++bad; continue; }
                for (uint32_t r = 0; r < c; ++r)
                    if (std::memcmp(got[r]->id.data(), &nodes[20 * want[r]], 20)) ++bad;
            }
        }
        ++cases;
    }
    std::fclose(f);
    std::printf("rtable_check (tables): %d cases, %d mismatches\n", cases, bad);
    return bad ? 1 : 0;
}

int main(int argc, char** argv) {
    if (argc >= 3 && std::strcmp(argv[1], "--tables") == 0) return check_tables(argv[2]);
    const bool host_only = argc >= 2 && std::strcmp(argv[1], "--host") == 0;
    if (argc < 2 || (std::strcmp(argv[1], "--run") != 0 && !host_only)) { std::puts("built"); return 0; }
    // grow a table with the oracle's onNewNode restatement, then mirror it as mock types
    std::vector<uint8_t> myid(20), ids(20 * 20000);
    orc_gen_ids(99, 0, 1, myid.data());
    orc_gen_ids(100, 0, 20000, ids.data());
    orc_table* ot = orc_table_new(myid.data(), 0);
    for (int i = 0; i < 20000; ++i) orc_table_insert(ot, ids.data() + 20 * i);
    const uint32_t nb = orc_table_nbuckets(ot), nn = orc_table_nnodes(ot);
    std::vector<uint8_t> firsts(20 * nb), nodes(20 * nn), good(nn);
    std::vector<uint32_t> off(nb + 1);
    orc_table_export(ot, firsts.data(), off.data(), nodes.data());
    orc_table_free(ot);
    for (uint32_t i = 0; i < nn; ++i) good[i] = (rnd() % 10) >= 3;
    mock::InfoHash my;
    std::memcpy(my.d.data(), myid.data(), 20);
    // targets: random ones, node ids, ids next to myid (the closeness test's interesting side), myid
    const int q = 400;
    std::vector<uint8_t> tb(20 * q);
    orc_gen_ids(101, 0, q, tb.data());
    for (int i = 0; i < 40; ++i) std::memcpy(&tb[20 * (300 + i)], &nodes[20 * ((size_t)i * 7 % nn)], 20);
    for (int i = 340; i < q; ++i) {
        std::memcpy(&tb[20 * i], myid.data(), 20);
        if (i > 340) tb[20 * i + 19 - (i % 12)] ^= (uint8_t)(1u << (i % 8));
    }
    std::vector<mock::InfoHash> targets(q);
    for (int i = 0; i < q; ++i) std::memcpy(targets[i].d.data(), &tb[20 * i], 20);

    int bad = 0;
    for (uint32_t alen : {4u, 16u}) {
        std::vector<uint8_t> tails((size_t)nn * (alen + 2));
        for (auto& b : tails) b = (uint8_t)rnd();
        const RoutingTable table = make_table(nb, firsts.data(), off.data(), nodes.data(), good.data(), tails.data(), alen);
        const uint32_t pairs[2][2] = {{8, 1}, {14, 8}};
        // the oracle's answers
        std::vector<std::vector<uint8_t>> want_reply(q);
        std::vector<uint8_t> want_flag[2];
        for (int i = 0; i < q; ++i) {
            uint32_t w[32];
            uint32_t c = orc_find_closest(nb, firsts.data(), off.data(), nodes.data(), good.data(), &tb[20 * i], 8, w);
            want_reply[i].resize(8 * (22 + alen));
            want_reply[i].resize(orc_buffer_nodes(nodes.data(), tails.data(), alen, &tb[20 * i], w, c, want_reply[i].data()));
            for (int p = 0; p < 2; ++p) {
                c = orc_find_closest(nb, firsts.data(), off.data(), nodes.data(), good.data(), &tb[20 * i], pairs[p][0], w);
                want_flag[p].push_back(c >= pairs[p][1] && orc_xor_cmp(&tb[20 * i], &nodes[20 * w[c - 1]], myid.data()) < 0);
            }
        }
        for (int i = 0; i < q; ++i) {
            if (dhtgpu::detail::reply_nodes_host(table, targets[i], 0L, alen == 16) != want_reply[i]) ++bad;
            for (int p = 0; p < 2; ++p)
                if (dhtgpu::detail::closer_than_self_host(table, targets[i], 0L, pairs[p][0], pairs[p][1], myid.data()) !=
                    (want_flag[p][i] != 0))
                    ++bad;
        }
        if (host_only) continue;
        dhtgpu::Context ctx(0);
        dhtgpu::ResidentTable<RoutingTable, long> rt(ctx, my);
        rt.assign(table, alen == 4 ? 4 : 6, 1);
        rt.refresh(table, 0L);
        for (int dflt = 0; dflt < 2; ++dflt) {   // the device, then the default dispatch
            rt.min_device_batch = dflt ? dhtgpu::kMinResidentBatch : 1;
            rt.min_reply_batch = dflt ? dhtgpu::kMinResidentReplyBatch : 1;
            auto rep = rt.replyNodesBatch(table, targets.data(), q, 0L);
            auto fc = rt.findClosestNodesBatch(table, targets.data(), q, 0L, 8);
            for (int i = 0; i < q; ++i) {
                if (rep[i] != want_reply[i]) ++bad;
                std::vector<std::shared_ptr<mock::Node>> h;
                dhtgpu::detail::find_closest_host(table, targets[i], 0L, 8, h);
                if (fc[i] != h) ++bad;
            }
            for (int p = 0; p < 2; ++p)
                if (rt.closerThanSelfBatch(table, targets.data(), q, 0L, pairs[p][0], pairs[p][1]) != want_flag[p]) ++bad;
        }
        if (alen == 4) {   // the host side of the dispatch threshold
            using clk = std::chrono::steady_clock;
            const int reps = 100000;
            size_t sink = 0;
            auto t0 = clk::now();
            for (int i = 0; i < reps; ++i) sink += dhtgpu::detail::reply_nodes_host(table, targets[i % 300], 0L, false).size();
            auto t1 = clk::now();
            std::printf("rtable_check: host reply (findClosestNodes + pack) %.3f us per target over %u buckets / %u nodes [sink %zu]\n",
                        std::chrono::duration<double, std::micro>(t1 - t0).count() / reps, nb, nn, sink);
            // both sides of the dispatch around the threshold: refresh + replyNodesBatch from the mirror
            // against the host walk, wall clock of one warm call each
            std::vector<mock::InfoHash> big(4096);
            std::vector<uint8_t> bb(20 * big.size());
            orc_gen_ids(202, 0, big.size(), bb.data());
            for (size_t i = 0; i < big.size(); ++i) std::memcpy(big[i].d.data(), &bb[20 * i], 20);
            for (size_t n : {64, 256, 512, 1024, 4096}) {
                double us[2];
                for (int side = 0; side < 2; ++side) {
                    rt.min_reply_batch = side ? (size_t)-1 : 1;
                    double best = 1e30;
                    for (int rep = 0; rep < 6; ++rep) {
                        auto d0 = clk::now();
                        if (!side) rt.refresh(table, 0L);
                        sink += rt.replyNodesBatch(table, big.data(), n, 0L).size();
                        const double d = std::chrono::duration<double, std::micro>(clk::now() - d0).count();
                        if (rep && d < best) best = d;
                    }
                    us[side] = best;
                }
                std::printf("rtable_check: replyNodesBatch q=%zu device (refresh + reply) %.1f us, host %.1f us\n", n, us[0], us[1]);
                for (int side = 0; side < 2; ++side) {
                    rt.min_device_batch = side ? (size_t)-1 : 1;
                    double best = 1e30;
                    for (int rep = 0; rep < 6; ++rep) {
                        auto d0 = clk::now();
                        if (!side) rt.refresh(table, 0L);
                        sink += rt.findClosestNodesBatch(table, big.data(), n, 0L, 8).size();
                        const double d = std::chrono::duration<double, std::micro>(clk::now() - d0).count();
                        if (rep && d < best) best = d;
                    }
                    us[side] = best;
                }
                std::printf("rtable_check: findClosestNodesBatch q=%zu device (refresh + query) %.1f us, host %.1f us\n", n, us[0], us[1]);
            }
            rt.min_device_batch = dhtgpu::kMinResidentBatch;
            rt.min_reply_batch = dhtgpu::kMinResidentReplyBatch;
        }
    }
    std::printf("rtable_check%s: %d mismatches\n", host_only ? " (host paths)" : "", bad);
    return bad ? 1 : 0;
}
