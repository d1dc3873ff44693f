// Host side of a kernel launch ("Table-driven kernels", host side): the status of a launch, the dynamic-LDS grant of a
// kernel instantiation, the dropout conversion and the argument check of a bag table.  What a forward and its backward, or the
// single-bag and the batched entry of one kernel, must agree on is written here once.  Host code only.
#pragma once
#include "vlsa_common.h"

namespace vlsa {

// VLSA_OK unless a launch (or an attribute call) since the last look left an error behind.
inline int launch_status() { return hipGetLastError() == hipSuccess ? VLSA_OK : VLSA_ELAUNCH; }

// hipFuncSetAttribute(MaxDynamicSharedMemorySize) is per device: the bytes one kernel instantiation has been granted on each device
// of this process (normally one process drives one GPU, but a host may also walk over several).  covers() is false on the first use
// per device, whatever the byte count, and again whenever a launch asks for more than an earlier one did (the text tower's products
// size their LDS by K); an unknown device asks every time.
struct LdsGrant {
    int granted[64];
    LdsGrant() { for (int& g : granted) g = -1; }
    bool covers(int bytes) {
        int d = 0;
        if (hipGetDevice(&d) != hipSuccess || d < 0 || d >= 64) return false;
        if (granted[d] >= bytes) return true;
        granted[d] = bytes;
        return false;
    }
};

// Launch Kernel with lds_bytes of dynamic LDS, raising the instantiation's limit first where it has not been raised that far on this
// device.  The attribute and the launch name the same instantiation by construction: there is no list of kernels to keep by hand.
template <auto Kernel>
inline LdsGrant& lds_grant() {
    static LdsGrant grant;
    return grant;
}
template <auto Kernel, typename... Args>
inline void launch_lds(dim3 grid, dim3 block, size_t lds_bytes, hipStream_t stream, Args... args) {
    if (!lds_grant<Kernel>().covers((int)lds_bytes))
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(Kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
    hipLaunchKernelGGL(Kernel, grid, block, lds_bytes, stream, args...);
}

// Dropout with probability p as the kernels take it (dropout_bits, vlsa_common.h): a unit is kept iff its 32 mask bits are >= thr
// and then scaled by `scale`.  thr = p * 2^32 rounded down and clamped to 1 (a p > 0 never switches dropout off), scale = 1 / (1 - p);
// p <= 0: off (thr 0, scale 1).  False for a p that is no probability below 1: the caller returns VLSA_EINVAL.  A forward and its
// backward recompute the same mask from these two numbers, so both take them from here.
struct DropSpec {
    unsigned int thr = 0u;
    float scale = 1.f;
};
inline bool drop_spec(float p, DropSpec* out) {
    *out = DropSpec{};
    if (p <= 0.f) return true;
    if (!(p < 1.f)) return false;
    out->thr = (unsigned int)((double)p * 4294967296.0);
    if (out->thr == 0u) out->thr = 1u;
    out->scale = 1.f / (1.f - p);
    return true;
}

// The part of a table-driven entry point's argument check that every route shares (bag_table.h): a device table of B <= 64 bag
// descriptors and a start table [B + 1] whose last entry n_table (tiles, parts, blocks) gives every bag at least one.
inline bool bag_table_ok(const void* bag_desc, int B, const void* table, long long n_table) {
    return bag_desc && table && B >= 1 && B <= 64 && n_table >= B;
}

}  // namespace vlsa
