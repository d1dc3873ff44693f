// Row operations of the survival loss kernels (surv_objectives.hip): a sample per 16-LANE ROW, a bin per lane, through DPP.
#pragma once
#include "vlsa_common.h"

namespace vlsa {

#define VLSA_DPP(v, ctrl) __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), ctrl, 0xf, 0xf, true))
// (row16_sum: vlsa_common.h)
__device__ __forceinline__ float row16_max(float v) {
    v = fmaxf(v, VLSA_DPP(v, 0x128)); v = fmaxf(v, VLSA_DPP(v, 0x124)); v = fmaxf(v, VLSA_DPP(v, 0x122)); v = fmaxf(v, VLSA_DPP(v, 0x121));
    return v;
}
// Cumulative sums IN BIN ORDER, as torch.cumsum and its backward add them: c_k = (((v_0 + v_1) + v_2) + ...) + v_k, fifteen dependent
// shifted adds (after step s lane k holds the left-to-right sum of v_{k-s} .. v_k).  The order matters: the reference clamps
// 1 - CIF[t] at eps, and whether a censored sample in the last bin lands on the clamp -- zero gradient or c / sv ~ 1e7 -- is decided by the
// last ulp of that cumsum (a log-step scan moved a 40-step training run off the CPU twin's loss curve by 0.3 % at step 6).
__device__ __forceinline__ float row16_prefix(float v) {      // inclusive, over the lanes <= this one (row_shr:1, zeros shift in)
    float c = v;
#pragma unroll
    for (int s = 0; s < 15; ++s) c = VLSA_DPP(c, 0x111) + v;
    return c;
}
__device__ __forceinline__ float row16_suffix(float v) {      // inclusive, over the lanes >= this one, added from the right (row_shl:1)
    float c = v;
#pragma unroll
    for (int s = 0; s < 15; ++s) c = VLSA_DPP(c, 0x101) + v;
    return c;
}
// Cumulative products IN BIN ORDER, as torch.cumprod multiplies them: c_k = (((v_0 v_1) v_2) ...) v_k.  Ones shift in at the row's left end
// (bound_ctrl off: a lane without a source keeps `old` = 1.0f), so lane 0 holds 1 * v_0 = v_0 exactly.
__device__ __forceinline__ float row16_prefix_prod(float v) {
    float c = v;
#pragma unroll
    for (int s = 0; s < 15; ++s)
        c = __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(1.f), __float_as_int(c), 0x111, 0xf, 0xf, false)) * v;
    return c;
}
#undef VLSA_DPP

}  // namespace vlsa
