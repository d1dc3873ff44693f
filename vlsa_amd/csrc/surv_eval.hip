// Scoring a split on the device: what NLLSurv_Evaluator (eval/evaluator_surv.py:45-235, a backend other than SurvivalEVAL) computes
// on the host from the [M, K] predictions of a pass over train / val / test -- the risk Harrell's C ranks the patients by
// (eval/cindex.py:36-43), the pair counts of the vendored scikit-survival concordance_index_censored (eval/cindex.py:86-150) and the
// loss metrics (SurvIFMLE / SurvMLE with the evaluator's alpha and with alpha = 0, loss/loss_surv.py:104-169; the handler's SurvIFMLE
// and SurvEMD as "ext" losses, eval/evaluator_surv.py:198-235) -- in two launches: k_surv_eval_rows (per sample, float64 throughout)
// and k_concordance_pairs (every pair, integer counts).  Forward only.
#include "vlsa_common.h"
#include "launch.h"

namespace vlsa {

// ---- per-sample work: one thread per sample, ONE workgroup walking the samples in chunks of blockDim.x, so that every sum has one
// fixed order (thread-local over the chunks, then the lanes of a wave, then the waves) and two runs give the same bits.  The sample's
// converted prediction (K doubles) lives in LDS, [k][thread]: as a dynamically indexed private array it would sit in scratch memory
// (see k_surv_terms).  The launch sizes the workgroup so that K * blockDim.x doubles fit kEvalLdsDoubles.
constexpr int kEvalLdsDoubles = 7680;       // 60 KB
constexpr int kEvalMaxThreads = 256;
constexpr int kEvalSums = 6;                // result[0 .. 5]
struct EvalVec {
    double* p;
    int stride;
    __device__ __forceinline__ double& operator[](int k) const { return p[k * stride]; }
};
// torch's clamp(min = eps): a NaN stays a NaN (fmax would drop it)
__device__ __forceinline__ double clamp_min(double v, double eps) { return v < eps ? eps : v; }
__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

__global__ __launch_bounds__(kEvalMaxThreads) void k_surv_eval_rows(
    const float* __restrict__ x, int converted, int hazard, const int64_t* __restrict__ t_, const float* __restrict__ e_, int M, int K,
    double alpha, double eps, const float* __restrict__ ls_ptr, double ls_value, int ls_is_log, int ext_mask, double ext_alpha,
    double ext_eps, int p, int raw_distance, double w_ifmle, double w_emd, double* __restrict__ est_out, double* __restrict__ time_out,
    float* __restrict__ surv, double* __restrict__ result) {
    __shared__ double vec[kEvalLdsDoubles];
    __shared__ double red[kEvalMaxThreads / 64][kEvalSums];
    const int T = blockDim.x, tid = threadIdx.x;
    // the pair counters of k_concordance_pairs, which the stream orders behind this kernel: no memset node in between
    if (tid >= VLSA_EVAL_CONCORDANT && tid < VLSA_EVAL_RESULT_WORDS) reinterpret_cast<unsigned long long*>(result)[tid] = 0ull;
    double ls = 0.0;
    if (ext_mask & 2) {
        ls = ls_ptr != nullptr ? (double)ls_ptr[0] : ls_value;
        if (ls_is_log) ls = exp(ls);
    }
    double acc[kEvalSums] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    const EvalVec y{vec + tid, T};
    for (int i = tid; i < M; i += T) {
        const float* xi = x + (size_t)i * K;
        const long long t_raw = t_[i];
        const int t = t_raw < 0 ? 0 : (t_raw >= K ? K - 1 : (int)t_raw);
        const double e = (double)e_[i], c = 1.0 - e;
        // ---- the handler's output converter (utils/func.py:43-46: softmax / sigmoid), or the given values
        if (converted) {
            for (int k = 0; k < K; ++k) y[k] = (double)xi[k];
        } else if (hazard) {
            for (int k = 0; k < K; ++k) y[k] = 1.0 / (1.0 + exp(-(double)xi[k]));
        } else {
            double mx = (double)xi[0], s = 0.0;
            for (int k = 1; k < K; ++k) { const double v = (double)xi[k]; mx = (v > mx || v != v) ? v : mx; }
            for (int k = 0; k < K; ++k) { const double v = exp((double)xi[k] - mx); y[k] = v; s += v; }
            for (int k = 0; k < K; ++k) y[k] /= s;
        }
        // ---- survival curve, risk (eval/cindex.py:36-43: UNCLAMPED), and the curve's values the likelihood reads
        double est = 0.0, s_at = 0.0, s_before = 1.0;      // S_padded[t + 1] and S_padded[t] of SurvMLE; 1 - CIF[t] of SurvIFMLE
        {
            double run = hazard ? 1.0 : 0.0;
            for (int k = 0; k < K; ++k) {
                double S;
                if (hazard) { run *= 1.0 - y[k]; S = run; } else { run += y[k]; S = 1.0 - run; }
                est -= S;
                if (k == t) s_at = S;
                if (k == t - 1) s_before = S;
                if (surv != nullptr) surv[(size_t)i * K + k] = S < 0.0 ? 0.f : (float)S;      // evaluator_surv.py:110-116
            }
        }
        est_out[i] = est;
        time_out[i] = (double)t_raw;
        const double a = y[t];
        // ---- the type's MLE: loss/loss_surv.py:113-122 (hazard) / 153-161 (incidence)
        double unc, cen = -c * log(clamp_min(s_at, eps));
        if (hazard) unc = -(1.0 - c) * (log(clamp_min(s_before, eps)) + log(clamp_min(a, eps)));
        else unc = -(1.0 - c) * log(clamp_min(a, eps));
        acc[0] += (1.0 - alpha) * (cen + unc) + alpha * unc;
        acc[1] += (1.0 - 0.0) * (cen + unc) + 0.0 * unc;    // loss_mle_org: the same expression at alpha = 0 (an infinite unc gives the reference's NaN)
        acc[4] += e != 0.0 ? 1.0 : 0.0;
        acc[5] += (est - est == 0.0) ? 0.0 : 1.0;          // inf - inf and NaN - NaN are NaN
        // ---- ext losses of the handler (incidence only): SurvIFMLE with its own alpha / eps, SurvEMD as in k_surv_terms
        if (ext_mask & 1) {
            const double u = -(1.0 - c) * log(clamp_min(a, ext_eps)), z = -c * log(clamp_min(s_at, ext_eps));
            acc[2] += (1.0 - ext_alpha) * (z + u) + ext_alpha * u;
        }
        if (ext_mask & 2) {
            const int ei = (int)e_[i];                       // e.long() of the reference
            const double nc = (double)(1 - ei), ne = (double)ei;
            double mp = -INFINITY, mt = -INFINITY;
            for (int k = 0; k < K; ++k) {
                const double tg = (k == t ? 1.0 : 0.0) + (k > t ? nc : 0.0);              // convert_survival_label
                const double pd = nc * ((1.0 - tg) * y[k] + tg * ls) + ne * y[k], td = (2.0 * tg - 1.0) * ls;
                mp = (pd > mp || pd != pd) ? pd : mp;
                mt = (td > mt || td != td) ? td : mt;
            }
            double sp = 0.0, st = 0.0;
            for (int k = 0; k < K; ++k) {
                const double tg = (k == t ? 1.0 : 0.0) + (k > t ? nc : 0.0);
                const double pd = nc * ((1.0 - tg) * y[k] + tg * ls) + ne * y[k];
                const double pe = exp(pd - mp);
                y[k] = pe;                                   // the incidence is not read again
                sp += pe;
                st += exp((2.0 * tg - 1.0) * ls - mt);
            }
            double cp = 0.0, ct = 0.0, S = 0.0;
            for (int k = 0; k < K; ++k) {
                const double tg = (k == t ? 1.0 : 0.0) + (k > t ? nc : 0.0);
                cp += y[k] / sp;
                ct += exp((2.0 * tg - 1.0) * ls - mt) / st;
                const double d = cp - ct;
                S += (p == 1) ? fabs(d) : d * d;
            }
            acc[3] += (p == 2 && !raw_distance) ? sqrt(S) : S;
        }
    }
    // ---- lanes, then waves, in index order
    const int wave = tid >> 6, n_waves = T >> 6;
#pragma unroll
    for (int q = 0; q < kEvalSums; ++q) {
        const double s = wave_sum_f64(acc[q]);
        if ((tid & 63) == 0) red[wave][q] = s;
    }
    __syncthreads();
    if (tid < kEvalSums) {
        double s = red[0][tid];
        for (int w = 1; w < n_waves; ++w) s += red[w][tid];
        if (tid == VLSA_EVAL_SUM_IFMLE) s *= w_ifmle;
        if (tid == VLSA_EVAL_SUM_EMD) s *= w_emd;
        result[tid] = s;
    }
    if (tid == VLSA_EVAL_M) result[tid] = (double)M;
    if (tid == VLSA_EVAL_M + 1) result[tid] = 0.0;
}

// ---- every pair: the counts of eval/cindex.py:86-150.  Sample i (one per thread, a workgroup owns 256 of them) with an event is
// compared with every j of the workgroup's j-range, which streams through LDS in tiles of 256 (all lanes read the same address: a
// broadcast).  j is comparable to i when time_j > time_i, or time_j == time_i with j censored (which also rules out j == i).  Counts
// are integers: any order of adding them gives the same result.
constexpr int kPairTile = 256;
__global__ __launch_bounds__(kPairTile) void k_concordance_pairs(const double* __restrict__ time, const float* __restrict__ e,
                                                                 const double* __restrict__ est, int M, double tied_tol, int tiles_per_block,
                                                                 unsigned long long* __restrict__ counters) {
    __shared__ double s_time[kPairTile], s_est[kPairTile];
    __shared__ int s_cen[kPairTile];
    __shared__ unsigned int s_red[kPairTile / 64][5];
    const int tid = threadIdx.x, i = blockIdx.x * kPairTile + tid;
    const bool act = i < M && e[i] != 0.f;
    const double ti = act ? time[i] : 0.0, si = act ? est[i] : 0.0;
    unsigned int con = 0, tied_risk = 0, tied_time = 0, comparable = 0;
    const int n_tiles = (M + kPairTile - 1) / kPairTile, tile0 = blockIdx.y * tiles_per_block;
    const int tile1 = tile0 + tiles_per_block < n_tiles ? tile0 + tiles_per_block : n_tiles;
    for (int tile = tile0; tile < tile1; ++tile) {
        const int j0 = tile * kPairTile, j = j0 + tid;
        if (j < M) { s_time[tid] = time[j]; s_est[tid] = est[j]; s_cen[tid] = e[j] == 0.f ? 1 : 0; }
        __syncthreads();
        const int jn = M - j0 < kPairTile ? M - j0 : kPairTile;
        if (act) {
            for (int jj = 0; jj < jn; ++jj) {
                const double tj = s_time[jj], sj = s_est[jj];
                const bool same = tj == ti && s_cen[jj] != 0;
                const bool comp = tj > ti || same;
                const bool tie = fabs(sj - si) <= tied_tol;
                comparable += comp ? 1u : 0u;
                tied_time += same ? 1u : 0u;
                tied_risk += (comp && tie) ? 1u : 0u;
                con += (comp && !tie && sj < si) ? 1u : 0u;
            }
        }
        __syncthreads();
    }
    unsigned int v[5] = {con, comparable - con - tied_risk, tied_risk, tied_time, comparable};     // the order of VLSA_EVAL_CONCORDANT ..
#pragma unroll
    for (int q = 0; q < 5; ++q) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) v[q] += __shfl_xor(v[q], o);
        if ((tid & 63) == 0) s_red[tid >> 6][q] = v[q];
    }
    __syncthreads();
    if (tid < 5) {
        const unsigned long long s = (unsigned long long)s_red[0][tid] + s_red[1][tid] + s_red[2][tid] + s_red[3][tid];
        if (s != 0ull) atomicAdd(&counters[tid], s);
    }
}

}  // namespace vlsa

using namespace vlsa;

extern "C" int vlsa_surv_eval_rows(const float* x, int x_kind, int pred_type, const int64_t* t, const float* e, int M, int K, double alpha,
                                   double eps, const float* logit_scale, double logit_scale_value, int ls_is_log, int ext_mask,
                                   double ext_alpha, double ext_eps, int p, int raw_distance, double w_ifmle, double w_emd, double* est,
                                   double* time, float* surv, double* result, void* stream) {
    if (!x || !t || !e || !est || !time || !result || M < 1 || K < 1 || K > VLSA_MAX_K) return VLSA_EINVAL;
    if ((x_kind != VLSA_EVAL_RAW && x_kind != VLSA_EVAL_CONVERTED) || (pred_type != VLSA_EVAL_INCIDENCE && pred_type != VLSA_EVAL_HAZARD) ||
        (ext_mask & ~3) != 0)
        return VLSA_EINVAL;
    if (M > VLSA_EVAL_MAX_M) return VLSA_EUNSUPPORTED;
    if (ext_mask != 0 && pred_type != VLSA_EVAL_INCIDENCE) return VLSA_EUNSUPPORTED;
    if ((ext_mask & 2) != 0 && p != 1 && p != 2) return VLSA_EUNSUPPORTED;
    int threads = kEvalLdsDoubles / K / 64 * 64;           // K doubles per thread in kEvalLdsDoubles: 256 threads up to K = 30, 64 at K = 64
    threads = threads > kEvalMaxThreads ? kEvalMaxThreads : threads;
    hipLaunchKernelGGL(k_surv_eval_rows, dim3(1), dim3(threads), 0, (hipStream_t)stream, x, x_kind == VLSA_EVAL_CONVERTED ? 1 : 0,
                       pred_type == VLSA_EVAL_HAZARD ? 1 : 0, t, e, M, K, alpha, eps, logit_scale, logit_scale_value, ls_is_log, ext_mask,
                       ext_alpha, ext_eps, p, raw_distance, w_ifmle, w_emd, est, time, surv, result);
    return launch_status();
}

extern "C" int vlsa_concordance_pairs(const double* time, const float* e, const double* est, int M, double tied_tol, uint64_t* counters,
                                      int zero_first, void* stream) {
    if (!time || !e || !est || !counters || M < 1) return VLSA_EINVAL;
    if (M > VLSA_EVAL_MAX_M) return VLSA_EUNSUPPORTED;
    if (zero_first && hipMemsetAsync(counters, 0, 5 * sizeof(uint64_t), (hipStream_t)stream) != hipSuccess) return VLSA_ELAUNCH;
    // 2-D grid over (i-tile, j-range): at most 32 j-ranges, so that M ~ 1000 already gives 4 x 4 workgroups and M = 65 536 adds
    // 256 x 32 x 5 integers
    const int n_tiles = (M + kPairTile - 1) / kPairTile;
    const int tiles_per_block = (n_tiles + 31) / 32, gy = (n_tiles + tiles_per_block - 1) / tiles_per_block;
    hipLaunchKernelGGL(k_concordance_pairs, dim3(n_tiles, gy), dim3(kPairTile), 0, (hipStream_t)stream, time, e, est, M, tied_tol,
                       tiles_per_block, reinterpret_cast<unsigned long long*>(counters));
    return launch_status();
}
