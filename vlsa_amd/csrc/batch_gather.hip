// Device-side batch gather of the training step (vlsa_amd/train_step.py: TrainStep.step_next): the B bags an optimizer step sees are
// picked ON THE DEVICE from a resident set -- descriptor rows and labels copied into slots at fixed addresses, a cursor word moved on --
// so that a captured step (whose launches have the slots' addresses baked in) serves every batch a reshuffling sampler draws
// (reference: DataLoader(shuffle=True), runner/base_handler.py:241).  One launch of one wave, no host data: capturable.
#include "vlsa_common.h"
#include "launch.h"

namespace vlsa {

constexpr int kGatherThreads = 64;      // one thread per slot: B <= vlsa_batch_max_bags() = 64

// The streaming kernels trust a descriptor row (a wrong pointer or N is a device fault there), so nothing is written before all B
// picks are known to be good: the barrier that combines the checks also orders every thread's read of the cursor before its update.
__global__ __launch_bounds__(kGatherThreads) void k_batch_gather(const int64_t* __restrict__ src_desc, const int64_t* __restrict__ t_all,
                                                                 const float* __restrict__ e_all, int64_t M,
                                                                 const int64_t* __restrict__ order, int64_t L, int B, int64_t* cursor,
                                                                 int64_t* __restrict__ slot_desc, int64_t* __restrict__ t_slot,
                                                                 float* __restrict__ e_slot, int* __restrict__ status) {
    const int j = threadIdx.x;
    const int64_t c = *cursor;
    const bool in_order = c >= 0 && c <= L - (int64_t)B;        // (c + B <= L without the sum: a wild cursor cannot wrap)
    int64_t src = 0;
    bool bad = false;
    if (in_order && j < B) {
        src = order[c + j];
        bad = src < 0 || src >= M;
    }
    const int any_bad = __syncthreads_or(bad ? 1 : 0);
    if (!in_order || any_bad) {          // slots, labels and cursor stay as they are: the slots still hold the previous valid batch
        if (j == 0) *status = in_order ? VLSA_GATHER_BAD_INDEX : VLSA_GATHER_BAD_CURSOR;
        return;
    }
    if (j < B) {
        slot_desc[3 * j + 0] = src_desc[3 * src + 0];
        slot_desc[3 * j + 1] = src_desc[3 * src + 1];
        slot_desc[3 * j + 2] = src_desc[3 * src + 2];
        t_slot[j] = t_all[src];
        e_slot[j] = e_all[src];
    }
    if (j == 0) *cursor = c + B;
}

}  // namespace vlsa

using namespace vlsa;

extern "C" int vlsa_batch_gather(const void* src_desc, const int64_t* t_all, const float* e_all, int64_t M, const int64_t* order,
                                 int64_t L, int B, int64_t* cursor, void* slot_desc, int64_t* t_slot, float* e_slot, int* status,
                                 void* stream) {
    if (!src_desc || !t_all || !e_all || !order || !cursor || !slot_desc || !t_slot || !e_slot || !status) return VLSA_EINVAL;
    if (M < 1 || L < 0 || B < 1 || B > kGatherThreads) return VLSA_EINVAL;
    static_assert(sizeof(vlsa_bag_desc) == 3 * sizeof(int64_t), "a descriptor row is three 64-bit words");
    hipLaunchKernelGGL(k_batch_gather, dim3(1), dim3(kGatherThreads), 0, (hipStream_t)stream, (const int64_t*)src_desc, t_all, e_all, M,
                       order, L, B, cursor, (int64_t*)slot_desc, t_slot, e_slot, status);
    return launch_status();
}
