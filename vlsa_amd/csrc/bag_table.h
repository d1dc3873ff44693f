// What the table-driven kernels share ("Table-driven kernels"): a launch over a table of B <= 64 bags whose workgroups
// find their bag in a [B + 1] start table, the MFMA wrappers, the row-split count of the weight-gradient products and the format of
// the ReLU-decision mask.  The streaming kernels keep their table in LDS (vlfan_stream.h) and do not come through here.
#pragma once
#include "vlsa_common.h"

namespace vlsa {

// ---- which bag owns block / tile / row i -----------------------------------------------------------------------------------------
// start: B <= 64 starts, start[0] = 0, strictly increasing (int32 tile_start / part_start [B + 1], or the int64 row offsets [B]).
// Returns the b with start[b] <= i < start[b + 1]: one vector load of the table and a popcount of the ballot, no dependent scalar
// search.  -1 when i < start[0]; B - 1 when i >= start[B] (the entry start[B] itself is never read).  The popcount of a ballot is
// wave-uniform by construction and the compiler keeps it in SGPRs (the descriptor loads behind it are scalar loads); a readfirstlane
// on top adds nothing but a convergent call that moved the register allocation of k_scores_tile_p (docs/LAB_NOTEBOOK.md).
// PRECONDITION: i is wave-uniform and every lane < B of the calling wave is active -- the call sits at the top of a kernel or under
// block-uniform control flow of a kernel whose blocks are whole waves.
__device__ __forceinline__ int bag_of(const int* start, int B, int i) {
    const int ts = (int)(threadIdx.x & 63) < B ? start[threadIdx.x & 63] : 0x7fffffff;
    return __builtin_popcountll(__builtin_amdgcn_ballot_w64(ts <= i)) - 1;
}
__device__ __forceinline__ int bag_of(const long long* start, int B, long long i) {
    const long long ts = (int)(threadIdx.x & 63) < B ? start[threadIdx.x & 63] : 0x7fffffffffffffffll;
    return __builtin_popcountll(__builtin_amdgcn_ballot_w64(ts <= i)) - 1;
}

// the bag of i, i's index within the bag and the bag's count of blocks / tiles (start [B + 1]).  b stays inside 0 .. B - 1 whatever
// the table holds (a start[0] > i gives bag 0, as the scan this replaced did): no descriptor is read from outside the table.
struct BagSpan { int b, idx, count; };
__device__ __forceinline__ BagSpan bag_span(const int* start, int B, int i) {
    const int b = max(bag_of(start, B, i), 0), s = start[b];
    return BagSpan{b, i - s, start[b + 1] - s};
}

// ---- MFMA wrappers -----------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ f32x4 mfma_bf16(bf16x8 a, bf16x8 b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0); }
__device__ __forceinline__ f32x4 mfma_f32(float a, float b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }

// row splits of a weight-gradient product over n_tiles row tiles (k_cp_backward, k_rm_wgrad): four tiles per split, at most 64
// partials for the fixed-order reduce
inline int splits_of(int n_tiles) {
    const int r = (n_tiles + 3) / 4;
    return r < 1 ? 1 : (r > 64 ? 64 : r);
}

// ---- the ReLU-decision mask -------------------------------------------------------------------------------------------------------
// 256 bits per row as eight 32-bit words, [sum N_b][8] at the launch's packed row index: bit (u & 31) of word (u >> 5) is set iff the
// pre-activation of hidden unit u was > 0.  The writers hold unit 64 w + 16 hg + i16 of row 4 gq + e (of a 16-row tile) in accumulator
// [hg][e] of lane (gq, i16) of wave w, take bal[hg] = ballot(acc[hg][e] > 0) and let lanes i16 = 0, 1 of every 16-lane group write
// word 2 w + i16 of the group's row: relu_mask_word.  A reader takes single bits (relu_mask_bit) or the words of its hidden slice
// (bwd_load of cluster_pool.hip).
__device__ __forceinline__ unsigned int relu_mask_word(const unsigned long long (&bal)[4], int i16, int gq) {
    const unsigned long long lo = i16 ? bal[2] : bal[0], hi = i16 ? bal[3] : bal[1];
    return (unsigned int)((lo >> (16 * gq)) & 0xffffull) | ((unsigned int)((hi >> (16 * gq)) & 0xffffull) << 16);
}
__device__ __forceinline__ bool relu_mask_bit(const unsigned int* row_words, int unit) { return (row_words[unit >> 5] >> (unit & 31)) & 1u; }

}  // namespace vlsa
