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

// Whether a descriptor list with something to do can be launched (batch, converting,
// strided and accumulate lists alike): `inline_cap` ops travel in the kernel arguments,
// a longer list needs its device copy and wave table. UNIT16: the kernel maps 16-byte
// vectors through the extents one by one, so a vector must fit a stripe unit.
// NO_ABS_LIN: the kernel reads op.lin_off as an offset only.
template <bool UNIT16, bool NO_ABS_LIN, class Args>
inline bool list_args_valid(const Args &a, int inline_cap) {
    if (a.n_ext < 1 || a.n_ext > (uint32_t)kXferMaxExtents || a.grid == 0) return false;
    if (UNIT16 && a.n_ext > 1 && a.unit_shift < 4) return false;
    if constexpr (NO_ABS_LIN)
        if (a.abs_lin) return false;
    return a.n_ops <= (uint32_t)inline_cap || (a.ops && a.wave_op);
}

}  // namespace ocm::kernels
