// rg_route.h -- the AllowedIPs table of cryptokey routing (rustyguard-tun/src/lib.rs: peer_net, an
// Ipv4LCTrieMap<PeerId> whose root value is a sentinel peer), written once for the host and the device: the
// table layout, its builder (host) and the lookup (host and device, one text).  The device half runs in
// rg_route.hip, one lane per packet; the host half is rg_route_table_words / _build / _lookup of
// include/rg_aead.h and is tested on a CPU under sanitizers (tests/route_host/driver.cpp).
//
// Layout: a fixed-stride 16-8-8 multibit trie in uint32_t words, built by controlled prefix expansion with
// leaf pushing.
//   words [0, 65536)                       the root: one entry per value of the address's top 16 bits
//   words [65536 + 256 b, 65536 + 256 b + 256)   child block b = 0, 1, ...: one entry per value of the next 8 bits
// A block of the second level (bits 15..8) hangs off a root entry, a block of the third level (bits 7..0) off
// a second-level entry.  An entry is one word:
//   0x00000000 .. 0x7FFFFFFF   leaf: the peer id itself
//   0xFFFFFFFF                 leaf: no peer (RG_PEER_NONE itself)
//   0x80000000 | b             pointer to child block b, b < 0x7FFFFFFF
// so a leaf word is the lookup's result as it stands, and a lookup is at most three dependent loads.  Every
// entry a longer prefix does not cover carries the longest shorter match (leaf pushing): no backtracking.
//
// The builder inserts the prefixes by ascending length, rows of one length in array order.  A prefix then only
// ever meets leaves in the range it expands to (a pointer there would need a longer prefix, which comes
// later), the same (network, length) given twice ends with the last row's peer, and the block numbers depend on
// the rows alone: the table is a function of the prefix array, byte for byte.  Blocks are numbered as they
// are first needed.  Size: 65536 + 256 * (distinct /16 networks among the prefixes longer than 16 + distinct
// /24 networks among those longer than 24) words, which rg_route_table_words computes without building.
//
// The lookup trusts no word: a child index is formed in 64 bits and compared with table_words before it is
// used, and a pointer met on the third level ends the walk; both give RG_PEER_NONE.  A corrupt table can
// misroute, it cannot make a lane read outside the table.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "rg_aead.h"

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define RG_ROUTE_HD __host__ __device__
#else
#define RG_ROUTE_HD
#endif

#include <algorithm>
#include <vector>

namespace rg {
namespace route {

constexpr uint32_t kRootWords = 65536;  // 16-bit stride
constexpr uint32_t kBlockWords = 256;   // 8-bit strides
constexpr uint32_t kPointer = 0x80000000u;
constexpr uint32_t kMaxPeer = 0x7FFFFFFFu;

RG_ROUTE_HD static inline bool is_pointer(uint32_t e) { return e >= kPointer && e != RG_PEER_NONE; }

// First word of the block a pointer names, in 64 bits (b < 2^31: 65536 + 256 b < 2^40).
RG_ROUTE_HD static inline uint64_t block_base(uint32_t e) {
    return (uint64_t)kRootWords + (uint64_t)(e & kMaxPeer) * kBlockWords;
}

// Longest-prefix match of `a` (the address as a big-endian number: a.b.c.d -> a << 24 | b << 16 | c << 8 | d).
// table_words >= kRootWords is the caller's to check.
RG_ROUTE_HD static inline uint32_t lookup(const uint32_t *table, uint64_t table_words, uint32_t a) {
    uint32_t e = table[a >> 16];
    if (!is_pointer(e)) return e;
    uint64_t at = block_base(e) + ((a >> 8) & 255u);
    if (at >= table_words) return RG_PEER_NONE;
    e = table[at];
    if (!is_pointer(e)) return e;
    at = block_base(e) + (a & 255u);
    if (at >= table_words) return RG_PEER_NONE;
    e = table[at];
    return is_pointer(e) ? RG_PEER_NONE : e;
}

RG_ROUTE_HD static inline uint32_t addr_be(const uint8_t addr[4]) {
    return (uint32_t)addr[0] << 24 | (uint32_t)addr[1] << 16 | (uint32_t)addr[2] << 8 | addr[3];
}

// The IPv4 acceptance rule of both directions on the packet's first four bytes as a
// little-endian word w0 and its length L: L >= 20, version 4, 20 <= 4 IHL <= total_length <= L.  Returns
// total_length, or 0 when the packet is not acceptable.
RG_ROUTE_HD static inline uint32_t ipv4_total_length(uint32_t w0, uint32_t L) {
    if (L < 20u) return 0u;
    const uint32_t version = (w0 >> 4) & 15u, hdr = (w0 & 15u) * 4u;
    const uint32_t total = ((w0 >> 16) & 255u) << 8 | (w0 >> 24);
    if (version != 4u || hdr < 20u || hdr > total || total > L) return 0u;
    return total;
}

// ------------------------------------------------------------------ builder (host)
static inline uint32_t network(const rg_route_prefix &p) {
    const uint32_t mask = p.prefix_len ? 0xFFFFFFFFu << (32u - p.prefix_len) : 0u;
    return addr_be(p.addr) & mask;
}

static inline bool rows_valid(const rg_route_prefix *p, uint32_t np) {
    if (np && !p) return false;
    for (uint32_t i = 0; i < np; ++i)
        if (p[i].prefix_len > 32u || p[i].peer > kMaxPeer) return false;
    return true;
}

static inline size_t distinct(std::vector<uint32_t> &v) {
    std::sort(v.begin(), v.end());
    return (size_t)(std::unique(v.begin(), v.end()) - v.begin());
}

// exact size in words; 0 if a row is invalid
static inline size_t table_words(const rg_route_prefix *p, uint32_t np) {
    if (!rows_valid(p, np)) return 0;
    std::vector<uint32_t> mid, low; // the /16 networks that get a second-level block, the /24 a third-level one
    for (uint32_t i = 0; i < np; ++i) {
        if (p[i].prefix_len > 16u) mid.push_back(network(p[i]) >> 16);
        if (p[i].prefix_len > 24u) low.push_back(network(p[i]) >> 8);
    }
    return (size_t)kRootWords + (size_t)kBlockWords * (distinct(mid) + distinct(low));
}

// The entry's child block; a leaf is first replaced by a new block that carries its value in every entry.
static inline uint32_t *descend(uint32_t *table, uint32_t &entry, uint32_t &nblocks) {
    if (!is_pointer(entry)) {
        uint32_t *blk = table + block_base(nblocks);
        std::fill(blk, blk + kBlockWords, entry);
        entry = kPointer | nblocks++;
    }
    return table + block_base(entry);
}

static inline int table_build(const rg_route_prefix *p, uint32_t np, uint32_t *table, size_t cap_words) {
    if (!table || !rows_valid(p, np)) return RG_EINVAL;
    const size_t need = table_words(p, np);
    if (cap_words < need) return RG_EFULL; // nothing written
    std::fill(table, table + kRootWords, (uint32_t)RG_PEER_NONE);
    uint32_t nblocks = 0;
    for (uint32_t len = 0; len <= 32u; ++len) {
        for (uint32_t i = 0; i < np; ++i) {
            if (p[i].prefix_len != len) continue;
            const uint32_t net = network(p[i]);
            uint32_t *level = table, at = net >> 16, bits = 16;
            if (len > 16u) {
                level = descend(table, table[at], nblocks);
                at = (net >> 8) & 255u;
                bits = 24;
            }
            if (len > 24u) {
                level = descend(table, level[at], nblocks);
                at = net & 255u;
                bits = 32;
            }
            std::fill(level + at, level + at + (1u << (bits - len)), p[i].peer);
        }
    }
    return (size_t)kRootWords + (size_t)kBlockWords * nblocks == need ? RG_OK : RG_EINVAL; // cannot differ
}

} // namespace route
} // namespace rg
