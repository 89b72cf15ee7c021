// mock_dht.h -- the reference-shaped types the adapter checks share (same member names as
// dht::InfoHash / dht::SockAddr / dht::Bucket / dht::RoutingTable) and their random generator.
// mock::Node is not here: each program declares its own, because the members a node type has (or
// lacks) are what that program tests -- detail::node_state picks its overload by them.
#ifndef DHTGPU_TESTS_MOCK_DHT_H
#define DHTGPU_TESTS_MOCK_DHT_H
#include <netinet/in.h>

#include <array>
#include <cstdint>
#include <cstring>
#include <list>

namespace mock {
struct InfoHash {
    std::array<uint8_t, 20> d;
    const uint8_t* data() const { return d.data(); }
    bool operator<(const InfoHash& o) const { return std::memcmp(d.data(), o.d.data(), 20) < 0; }
};

// what bufferNodes reads of a node: getAddr().getIPv4() / getIPv6()
struct SockAddr {
    sockaddr_in v4;
    sockaddr_in6 v6;
    const sockaddr_in& getIPv4() const { return v4; }
    const sockaddr_in6& getIPv6() const { return v6; }
};

template <class NodePtr>
struct Bucket {
    InfoHash first;
    std::list<NodePtr> nodes;
};
template <class NodePtr>
using RoutingTable = std::list<Bucket<NodePtr>>;

// xorshift64 with its state in the open: a program keeps its own seed and its own way of drawing
// 32 bits from step()
struct Xorshift {
    uint64_t state;
    uint64_t step() {
        state ^= state << 13;
        state ^= state >> 7;
        state ^= state << 17;
        return state;
    }
};
}  // namespace mock
#endif
