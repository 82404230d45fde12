// Host-side helpers shared by the transfer launchers. Hidden: the libraries that
// link these units export nothing new.
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstdlib>

#include "ocm/xfer.h"

namespace ocm::kernels {

__attribute__((visibility("hidden"))) inline int env_int(const char *k, int dflt) {
    const char *v = std::getenv(k);
    return (v && *v) ? std::atoi(v) : dflt;
}

// Compute units of the current device, asked once (256 when it cannot be asked).
__attribute__((visibility("hidden"))) inline int num_cus() {
    static int cus = 0;
    if (cus) return cus;
    int dev = 0, n = 0;
    if (hipGetDevice(&dev) == hipSuccess && hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && n > 0)
        cus = n;
    else
        cus = 256;
    return cus;
}

// Whether a descriptor list with something to do can be launched (every kind alike):
// INLINE ops travel in the kernel arguments, a longer list needs its device copy and
// wave table. UNIT16: the kernel maps 16-byte vectors through the extents one by one,
// so a vector must fit a stripe unit.
template <bool UNIT16, class Op, int INLINE>
inline bool list_args_valid(const ListArgs<Op, INLINE> &a) {
    if (a.n_ext < 1 || a.n_ext > (uint32_t)kXferMaxExtents || a.grid == 0) return false;
    if (UNIT16 && a.n_ext > 1 && a.unit_shift < 4) return false;
    return a.n_ops <= (uint32_t)INLINE || (a.ops && a.wave_op);
}

// Whether the tiles of a list of rows are cut so that a tile is at most one stripe unit
// (two spans a tile at the most).
template <class Op, int INLINE>
inline bool list_tile_fits_unit(const ListArgs<Op, INLINE> &a) {
    return a.tile_shift <= 63 && (a.n_ext <= 1 || a.tile_shift <= a.unit_shift);
}

}  // namespace ocm::kernels
