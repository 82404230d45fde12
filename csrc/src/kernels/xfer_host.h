// Host-side helpers shared by the transfer launchers. Hidden: the libraries that
// link these units export nothing new.
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstdlib>

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

}  // namespace ocm::kernels
