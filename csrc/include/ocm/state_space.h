// The remote half of a pair as an optimizer kernel takes it (the moments' pair of AdamArgs, the
// accumulators' of AdamAccArgs and AccNormArgs, the table's of AdamRowsArgs): one struct, one
// launch-time check, and the address arithmetic in a form the host can replay
// (csrc/tools/ocm_adam_plan_tests.cpp). Calls nothing of HIP.
#pragma once
#include <cstdint>

#include "ocm/list.h"
#include "ocm/xfer.h"

namespace ocm {

struct StateSpace {
    char *ext[kXferMaxExtents];      // extent bases
    uint32_t n_ext;
    uint32_t unit_shift;             // log2(stripe unit) when n_ext > 1
    uint32_t host;                   // 1: the space is all in the pinned host tier (PCIe-bound launch shape)
    uint32_t host_span;              // (set by the launcher) bytes of the host extent the kernel may touch
};
static_assert(sizeof(StateSpace) == kXferMaxExtents * sizeof(char *) + 16, "StateSpace layout");

// What every launcher asks of a space: no 16-byte vector crosses a stripe unit, and 1 << unit_shift
// is defined. The library makes the shift from a 64-bit unit (log2_exact): it is never above 63.
inline bool state_space_ok(const StateSpace &s) {
    return s.n_ext >= 1 && s.n_ext <= (uint32_t)kXferMaxExtents && (s.n_ext == 1 || (s.unit_shift >= 4 && s.unit_shift < 64));
}

// Where byte x of a space lies: stripe unit u = x >> unit_shift lives on extent u % n_ext at
// (u / n_ext) << unit_shift. A 16-byte vector at a 16-byte aligned x never crosses a unit
// (units are powers of two >= 16).
struct StatePlace {
    uint32_t index;                  // of the extent
    uint64_t off;                    // bytes from its base
};

// Up to 2^32 units (64 GiB of state at a 16-byte unit): stripe over 3/5/6/7 peers, where 64-bit
// division is a ~100-instruction software routine on gfx950 and 32-bit a handful.
OCM_LIST_HD inline StatePlace state_place32(uint32_t n_ext, uint32_t unit_shift, uint64_t x) {
    const uint64_t mask = (1ull << unit_shift) - 1;
    const uint32_t u32 = (uint32_t)(x >> unit_shift), q = u32 / n_ext;
    return StatePlace{u32 - q * n_ext, ((uint64_t)q << unit_shift) | (x & mask)};
}
OCM_LIST_HD inline StatePlace state_place64(uint32_t n_ext, uint32_t unit_shift, uint64_t x) {
    const uint64_t u = x >> unit_shift, mask = (1ull << unit_shift) - 1;
    return StatePlace{(uint32_t)(u % n_ext), ((u / n_ext) << unit_shift) | (x & mask)};
}
OCM_LIST_HD inline bool state_units_fit32(uint32_t unit_shift, uint64_t x) { return (x >> unit_shift) <= 0xFFFFFFFFull; }

OCM_LIST_HD inline StatePlace state_place(uint32_t n_ext, uint32_t unit_shift, uint64_t x) {
    if (n_ext == 1) return StatePlace{0, x};
    return state_units_fit32(unit_shift, x) ? state_place32(n_ext, unit_shift, x) : state_place64(n_ext, unit_shift, x);
}

}  // namespace ocm
