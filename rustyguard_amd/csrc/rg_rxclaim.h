// rg_rxclaim.h -- how a kernel enters (id, row) into an rg_rx_entry table that rx_find (rg_internal.h) reads:
// the claim loop of the receiver-table rebuild (rg_session.hip) and of the pending-table rebuild
// (rg_pending.hip).  Device code only.
#pragma once
#include "rg_internal.h"

namespace rg {

constexpr unsigned long long kRxEmpty = ~0ull; // a free entry: receiver and key_idx all ones

// One lane per live row, behind a fill of the whole table with kRxEmpty: the row takes the first free entry from
// its id's home slot with a 64-bit atomicCAS.  cap is a power of two; the probe is bounded by it and masked, so no
// index leaves the table.  Which of two colliding rows gets the earlier entry depends on arrival; what rx_find
// answers does not.
__device__ __forceinline__ void rx_claim(unsigned long long *table, uint32_t cap, uint32_t id, uint32_t row) {
    const unsigned long long mine = (unsigned long long)id | ((unsigned long long)row << 32);
    uint32_t s = rx_slot(id, cap) & (cap - 1);
    for (uint32_t probe = 0; probe < cap; ++probe, s = (s + 1) & (cap - 1))
        if (atomicCAS(&table[s], kRxEmpty, mine) == kRxEmpty) return;
}

} // namespace rg
