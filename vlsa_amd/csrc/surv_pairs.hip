// The continuous survival heads' objective on the device: what calc_objective_loss computes on a [B, 1] prediction under
// loss_type SurvPLE (loss/loss_surv.py:172-209) or recon_loss / rank_loss / MSE_loss (loss/loss_surv.py:11-86) -- value, every term's
// value and d objective / d pred in ONE launch.  The reference builds SurvPLE's risk matrix with a Python double loop and rank_loss
// with three [B, B] matrices; here every pair is an LDS broadcast read.
//
// SurvPLE in two passes over the pairs (theta = min(pred, 10), shifted by the batch's largest theta so that no exp overflows):
//   D_i = sum_{j: T_j >= T_i} exp theta_j              (pass 1; ties included, as the reference's R matrix has them)
//   H_k = sum_{i: e_i = 1, T_i <= T_k} 1 / D_i         (pass 2; Breslow's cumulative baseline hazard at T_k)
//   value = -(1/B) sum_i e_i (theta_i - log D_i),      d value / d theta_k = -(1/B) (e_k - exp theta_k * H_k)
// rank_loss rides on pass 1: sample i adds its pairs (i, j) as the earlier event AND the pairs (j, i) as the later sample, so that it owns
// its whole gradient.  recon_loss and MSE_loss are per sample.
//
// Below the objective: the same two passes for a whole split, float64 throughout (vlsa_cox_risk_sets, vlsa_cox_cum_hazard, vlsa_cox_finish:
// CoxSurv_Evaluator's loss and Breslow baseline, eval/evaluator_surv.py:238-378, eval/utils_coxph.py:178-280) and RegSurv_Evaluator's sums
// (vlsa_reg_eval, eval/evaluator_surv.py:381-466).
//
// The objective is one workgroup; sample i belongs to thread i % blockDim.x.  Every sum has one fixed order (j ascending; then the
// thread's samples, the lanes of a wave, the waves): no atomics, two runs give the same bits.  exp, log and every sum are float64 -- exp
// once per sample, not once per pair -- so what the fp32 outputs lose is their own rounding.
#include "vlsa_common.h"
#include "launch.h"

namespace vlsa {

constexpr int kPairObjThreads = 1024;       // the largest workgroup; a smaller batch takes its size rounded up to whole waves
constexpr int kPairObjOwned = 4;            // samples per thread at most: kPairObjOwned * kPairObjThreads = kPairObjMaxB
constexpr int kPairObjMaxB = 4096;
constexpr int kPairObjLdsPerSample = 32;    // bytes: time, exp theta, e / D as doubles, pred and e as floats
static_assert(kPairObjOwned * kPairObjThreads == kPairObjMaxB, "every sample needs an owner");
static_assert(kPairObjMaxB * kPairObjLdsPerSample <= 160 * 1024 - 1024, "the batch and the reduction scratch share the 160 KB of LDS");

struct PairObjArgs {
    const float* pred;
    const void* time;
    const float* e;
    int B, time_f64;
    double w_ple, w_rank, w_recon, w_mse, rank_gamma, recon_alpha, recon_gamma;
    int rank_l2, recon_l2, mse_censored;
    float* objective;
    float* grad;
};

__device__ __forceinline__ double pair_wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
// the sum over the workgroup, handed to every thread: lanes, then the waves in index order
__device__ __forceinline__ double pair_block_sum(double v, double* red, int tid, int n_waves) {
    v = pair_wave_sum(v);
    __syncthreads();
    if ((tid & 63) == 0) red[tid >> 6] = v;
    __syncthreads();
    double s = red[0];
    for (int w = 1; w < n_waves; ++w) s += red[w];
    return s;
}
__device__ __forceinline__ double pair_block_max(double v, double* red, int tid, int n_waves) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { const double u = __shfl_xor(v, o); v = u > v ? u : v; }
    __syncthreads();
    if ((tid & 63) == 0) red[tid >> 6] = v;
    __syncthreads();
    double s = red[0];
    for (int w = 1; w < n_waves; ++w) s = red[w] > s ? red[w] : s;
    return s;
}

__global__ __launch_bounds__(kPairObjThreads) void k_surv_pair_objective(const PairObjArgs a) {
    extern __shared__ __align__(16) unsigned char pair_lds[];
    __shared__ double red[kPairObjThreads / 64];
    const int B = a.B, T = blockDim.x, tid = threadIdx.x, n_waves = T >> 6;
    double* s_time = reinterpret_cast<double*>(pair_lds);
    double* s_exp = s_time + B;          // exp(theta_j - max theta)
    double* s_inv = s_exp + B;           // e_j / D_j
    float* s_pred = reinterpret_cast<float*>(s_inv + B);
    float* s_e = s_pred + B;
    const bool ple = a.w_ple != 0.0, rank = a.w_rank != 0.0;

    // ---- the batch into LDS; the largest theta
    double mx = -INFINITY;
    for (int i = tid; i < B; i += T) {
        const float p = a.pred[i];
        const double th = p > 10.f ? 10.0 : (double)p;
        mx = th > mx ? th : mx;
        s_pred[i] = p;
        s_e[i] = a.e[i];
        s_time[i] = a.time_f64 ? static_cast<const double*>(a.time)[i] : (double)static_cast<const float*>(a.time)[i];
    }
    mx = pair_block_max(mx, red, tid, n_waves);
    for (int i = tid; i < B; i += T) {
        const float p = s_pred[i];
        s_exp[i] = exp((p > 10.f ? 10.0 : (double)p) - mx);
    }
    __syncthreads();

    // ---- pass 1: the risk-set sums, and every rank pair from both of its ends
    double v_ple = 0.0, v_rank = 0.0, v_recon = 0.0, v_mse = 0.0, n_pairs = 0.0;       // (a count below 2^53 is exact in a double)
    double rank_g[kPairObjOwned];
#pragma unroll
    for (int s = 0; s < kPairObjOwned; ++s) {
        rank_g[s] = 0.0;
        const int i = tid + s * T;
        if (i >= B) continue;
        const double ti = s_time[i], pi = (double)s_pred[i], ei = (double)s_e[i];
        if (ple) {
            double D = 0.0;
            for (int j = 0; j < B; ++j) D += s_time[j] >= ti ? s_exp[j] : 0.0;
            const double th = (pi > 10.0 ? 10.0 : pi) - mx;
            v_ple += ei != 0.0 ? ei * (th - log(D)) : 0.0;
            s_inv[i] = ei != 0.0 ? ei / D : 0.0;
        }
        if (rank) {
            // (i, j) with e_i == 1 and t_i < t_j costs relu(gamma + p_i - p_j)^norm; its derivative is +f' for p_i and -f' for p_j
            const bool ev_i = ei == 1.0;
            double num = 0.0, g = 0.0;
            unsigned int cnt = 0;
            for (int j = 0; j < B; ++j) {
                const double tj = s_time[j], pj = (double)s_pred[j];
                const bool first = ev_i && ti < tj, second = s_e[j] == 1.f && tj < ti;
                const double x = a.rank_gamma + pi - pj, y = a.rank_gamma + pj - pi;
                const double rx = x > 0.0 ? x : 0.0, ry = y > 0.0 ? y : 0.0;
                double fx, dx, dy;
                if (a.rank_l2) { fx = rx * rx; dx = 2.0 * rx; dy = 2.0 * ry; }
                else { fx = rx; dx = x > 0.0 ? 1.0 : 0.0; dy = y > 0.0 ? 1.0 : 0.0; }
                num += first ? fx : 0.0;
                g += (first ? dx : 0.0) - (second ? dy : 0.0);
                cnt += first ? 1u : 0u;
            }
            v_rank += num;
            n_pairs += (double)cnt;
            rank_g[s] = g;
        }
    }
    if (rank) n_pairs = pair_block_sum(n_pairs, red, tid, n_waves);
    __syncthreads();       // s_inv is complete

    // ---- pass 2: the cumulative hazard at every sample's time; the gradient
    const double inv_B = 1.0 / (double)B;
#pragma unroll
    for (int s = 0; s < kPairObjOwned; ++s) {
        const int i = tid + s * T;
        if (i >= B) continue;
        const double ti = s_time[i], pi = (double)s_pred[i], ei = (double)s_e[i];
        double g = 0.0;
        if (ple) {
            double H = 0.0;
            for (int j = 0; j < B; ++j) H += s_time[j] <= ti ? s_inv[j] : 0.0;
            if (!(pi > 10.0)) g += a.w_ple * (-inv_B) * (ei - s_exp[i] * H);       // d theta / d pred: 1 up to the cap, 0 above
        }
        if (rank && n_pairs > 0.0) g += a.w_rank * rank_g[s] / n_pairs;
        const double d = pi - ti;
        if (a.w_recon != 0.0) {
            // recon_loss: (1 - alpha) (obs + cen) + alpha obs; torch's abs and relu have derivative 0 at 0
            const double x = a.recon_gamma - d, ad = d < 0.0 ? -d : d, sg = d > 0.0 ? 1.0 : (d < 0.0 ? -1.0 : 0.0);
            double obs = ei * ad, cen = (1.0 - ei) * (x > 0.0 ? x : 0.0);
            double d_obs = ei * sg, d_cen = x > 0.0 ? -(1.0 - ei) : 0.0;
            if (a.recon_l2) { d_obs *= 2.0 * obs; d_cen *= 2.0 * cen; obs *= obs; cen *= cen; }
            v_recon += (1.0 - a.recon_alpha) * (obs + cen) + a.recon_alpha * obs;
            g += a.w_recon * inv_B * ((1.0 - a.recon_alpha) * (d_obs + d_cen) + a.recon_alpha * d_obs);
        }
        if (a.w_mse != 0.0) {
            const double w = ei + (a.mse_censored ? 1.0 - ei : 0.0);
            v_mse += w * d * d;
            g += a.w_mse * inv_B * 2.0 * w * d;
        }
        if (a.grad != nullptr) a.grad[i] = (float)g;
    }

    // ---- the values: 0 - sum keeps a batch without an event at +0
    v_ple = 0.0 - pair_block_sum(v_ple, red, tid, n_waves) * inv_B;
    v_rank = pair_block_sum(v_rank, red, tid, n_waves);
    v_rank = n_pairs > 0.0 ? v_rank / n_pairs : 0.0;
    v_recon = pair_block_sum(v_recon, red, tid, n_waves) * inv_B;
    v_mse = pair_block_sum(v_mse, red, tid, n_waves) * inv_B;
    if (tid == 0) {
        double total = 0.0;       // a term without a weight is neither computed nor added
        if (ple) total += a.w_ple * v_ple;
        if (rank) total += a.w_rank * v_rank;
        if (a.w_recon != 0.0) total += a.w_recon * v_recon;
        if (a.w_mse != 0.0) total += a.w_mse * v_mse;
        a.objective[VLSA_PAIR_OBJ_TOTAL] = (float)total;
        a.objective[VLSA_PAIR_OBJ_PLE] = (float)v_ple;
        a.objective[VLSA_PAIR_OBJ_RANK] = (float)v_rank;
        a.objective[VLSA_PAIR_OBJ_RECON] = (float)v_recon;
        a.objective[VLSA_PAIR_OBJ_MSE] = (float)v_mse;
        a.objective[VLSA_PAIR_OBJ_PAIRS] = (float)n_pairs;
    }
}

// ---- a split (up to VLSA_EVAL_MAX_M samples): the same two passes as launches of their own, everything float64.  Sample i (one per
// thread, a workgroup owns kSplitTile of them) meets every j, which streams through LDS in tiles of kSplitTile -- all lanes read the same
// address: a broadcast --, as k_concordance_pairs does.  What a tile needs of sample j (exp theta_j, e_j / D_j) is computed where the
// tile is loaded, once per sample and workgroup, never per pair.  Each output has one owner who adds in ascending j: no atomics, the
// same bits from run to run.
constexpr int kSplitTile = 256;

__global__ __launch_bounds__(kSplitTile) void k_cox_risk_sets(const float* __restrict__ theta, const double* __restrict__ time, int M, double cap,
                                                              double* __restrict__ D) {
    __shared__ double s_time[kSplitTile], s_exp[kSplitTile];
    const int tid = threadIdx.x, i = blockIdx.x * kSplitTile + tid;
    const bool act = i < M;
    const double ti = act ? time[i] : 0.0;
    double acc = 0.0;
    for (int j0 = 0; j0 < M; j0 += kSplitTile) {
        const int j = j0 + tid;
        if (j < M) {
            const double th = (double)theta[j];
            s_time[tid] = time[j];
            s_exp[tid] = exp(th > cap ? cap : th);
        }
        __syncthreads();
        const int jn = M - j0 < kSplitTile ? M - j0 : kSplitTile;
        if (act)
            for (int jj = 0; jj < jn; ++jj) acc += s_time[jj] >= ti ? s_exp[jj] : 0.0;
        __syncthreads();
    }
    if (act) D[i] = acc;
}

__global__ __launch_bounds__(kSplitTile) void k_cox_cum_hazard(const double* __restrict__ time, const float* __restrict__ e,
                                                               const double* __restrict__ D, int M, const double* __restrict__ query, int Q,
                                                               double* __restrict__ H) {
    __shared__ double s_time[kSplitTile], s_inv[kSplitTile];
    const int tid = threadIdx.x, q = blockIdx.x * kSplitTile + tid;
    const bool act = q < Q;
    const double u = act ? query[q] : 0.0;
    double acc = 0.0;
    for (int j0 = 0; j0 < M; j0 += kSplitTile) {
        const int j = j0 + tid;
        if (j < M) {
            const double ej = (double)e[j];
            s_time[tid] = time[j];
            s_inv[tid] = ej != 0.0 ? ej / D[j] : 0.0;
        }
        __syncthreads();
        const int jn = M - j0 < kSplitTile ? M - j0 : kSplitTile;
        if (act)
            for (int jj = 0; jj < jn; ++jj) acc += s_time[jj] <= u ? s_inv[jj] : 0.0;
        __syncthreads();
    }
    if (act) H[q] = acc;
}

// sums over a split by ONE workgroup: thread-local over the samples tid, tid + 256, .., then the lanes, then the waves
template <int N>
__device__ __forceinline__ void split_reduce(double (&acc)[N], double (*red)[N], int tid) {
#pragma unroll
    for (int q = 0; q < N; ++q) {
        const double s = pair_wave_sum(acc[q]);
        if ((tid & 63) == 0) red[tid >> 6][q] = s;
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < N; ++q) {
        double s = red[0][q];
        for (int w = 1; w < kSplitTile / 64; ++w) s += red[w][q];
        acc[q] = s;
    }
}

__global__ __launch_bounds__(kSplitTile) void k_cox_finish(const float* __restrict__ theta, const float* __restrict__ e,
                                                           const double* __restrict__ D, int M, double cap, double* __restrict__ result) {
    __shared__ double red[kSplitTile / 64][3];
    const int tid = threadIdx.x;
    // the pair counters of k_concordance_pairs, which the stream orders behind this kernel, and the words nothing is written to
    if (tid > VLSA_CEVAL_M && tid < VLSA_CEVAL_RESULT_WORDS) reinterpret_cast<unsigned long long*>(result)[tid] = 0ull;
    double acc[3] = {0.0, 0.0, 0.0};
    for (int i = tid; i < M; i += kSplitTile) {
        const double p = (double)theta[i], th = p > cap ? cap : p, ei = (double)e[i];
        acc[0] += ei != 0.0 ? ei * (th - log(D[i])) : 0.0;
        acc[1] += ei != 0.0 ? 1.0 : 0.0;
        acc[2] += (p - p == 0.0) ? 0.0 : 1.0;          // inf - inf and NaN - NaN are NaN
    }
    split_reduce<3>(acc, red, tid);
    if (tid == 0) {
        result[VLSA_CEVAL_SUM_PLE] = acc[0];
        result[VLSA_CEVAL_EVENTS] = acc[1];
        result[VLSA_CEVAL_NONFINITE] = acc[2];
        result[VLSA_CEVAL_M] = (double)M;
    }
}

// RegSurv_Evaluator's pair work: sample i's share of rank_loss -- numerator and pair count of its pairs (i, j) as the earlier event -- and,
// where asked, its whole unnormalised gradient (the pairs (j, i) subtracted: k_surv_pair_objective's bookkeeping)
__global__ __launch_bounds__(kSplitTile) void k_reg_pairs(const float* __restrict__ pred, const double* __restrict__ time, const float* __restrict__ e,
                                                          int M, double gamma, int l2, double* __restrict__ partial, double* __restrict__ grad) {
    __shared__ double s_time[kSplitTile], s_pred[kSplitTile];
    __shared__ int s_ev[kSplitTile];
    const int tid = threadIdx.x, i = blockIdx.x * kSplitTile + tid;
    const bool act = i < M;
    const double ti = act ? time[i] : 0.0, pi = act ? (double)pred[i] : 0.0;
    const bool ev_i = act && e[i] == 1.f;
    double num = 0.0, g = 0.0;
    unsigned int cnt = 0;
    for (int j0 = 0; j0 < M; j0 += kSplitTile) {
        const int j = j0 + tid;
        if (j < M) { s_time[tid] = time[j]; s_pred[tid] = (double)pred[j]; s_ev[tid] = e[j] == 1.f ? 1 : 0; }
        __syncthreads();
        const int jn = M - j0 < kSplitTile ? M - j0 : kSplitTile;
        if (act) {
            for (int jj = 0; jj < jn; ++jj) {
                const double tj = s_time[jj], pj = s_pred[jj];
                const bool first = ev_i && ti < tj, second = s_ev[jj] != 0 && tj < ti;
                const double x = gamma + pi - pj, y = gamma + pj - pi;
                const double rx = x > 0.0 ? x : 0.0, ry = y > 0.0 ? y : 0.0;
                double fx, dx, dy;
                if (l2) { fx = rx * rx; dx = 2.0 * rx; dy = 2.0 * ry; }
                else { fx = rx; dx = x > 0.0 ? 1.0 : 0.0; dy = y > 0.0 ? 1.0 : 0.0; }
                num += first ? fx : 0.0;
                g += (first ? dx : 0.0) - (second ? dy : 0.0);
                cnt += first ? 1u : 0u;
            }
        }
        __syncthreads();
    }
    if (act) {
        partial[i] = num;
        partial[M + i] = (double)cnt;
        if (grad != nullptr) grad[i] = g;
    }
}

constexpr int kRegSums = 12;
__global__ __launch_bounds__(kSplitTile) void k_reg_finish(const float* __restrict__ pred, const double* __restrict__ time, const float* __restrict__ e,
                                                           int M, double alpha, double gamma, int l2, double end_time,
                                                           const double* __restrict__ partial, double* __restrict__ result) {
    __shared__ double red[kSplitTile / 64][kRegSums];
    const int tid = threadIdx.x;
    if (tid >= VLSA_REVAL_CONCORDANT && tid < VLSA_REVAL_CONCORDANT + 5) reinterpret_cast<unsigned long long*>(result)[tid] = 0ull;
    double acc[kRegSums];
#pragma unroll
    for (int q = 0; q < kRegSums; ++q) acc[q] = 0.0;
    for (int i = tid; i < M; i += kSplitTile) {
        const double p = (double)pred[i], t = time[i], ei = (double)e[i], d = p - t;
        acc[0] += partial[i];
        acc[1] += partial[M + i];
        // recon_loss (loss/loss_surv.py:11-31) at the evaluator's alpha, and at alpha = 0
        const double x = gamma - d;
        double obs = ei * (d < 0.0 ? -d : d), cen = (1.0 - ei) * (x > 0.0 ? x : 0.0);
        if (l2) { obs *= obs; cen *= cen; }
        acc[2] += (1.0 - alpha) * (obs + cen) + alpha * obs;
        acc[3] += obs + cen;
        // eval/evaluator_surv.py:436-458: diff = t - y_hat for the two RAE, y_hat - t for the two NRE
        const double td = t - p;
        if (ei == 1.0) {
            acc[4] += (td < 0.0 ? -td : td) / end_time;
            acc[6] += d / end_time;
            acc[8] += 1.0;
        }
        if (ei == 0.0) {
            acc[5] += (td > 0.0 ? td : 0.0) / end_time;
            acc[7] += -((-d) > 0.0 ? -d : 0.0) / end_time;
            acc[9] += 1.0;
        }
        acc[10] += (p - p == 0.0) ? 0.0 : 1.0;
        acc[11] += ei != 0.0 ? 1.0 : 0.0;
    }
    split_reduce<kRegSums>(acc, red, tid);
    if (tid == 0) {
        result[VLSA_REVAL_RANK_NUM] = acc[0];
        result[VLSA_REVAL_RANK_PAIRS] = acc[1];
        result[VLSA_REVAL_RECON] = acc[2];
        result[VLSA_REVAL_RECON_ORG] = acc[3];
        result[VLSA_REVAL_EVT_RAE] = acc[4];
        result[VLSA_REVAL_NOEVT_RAE] = acc[5];
        result[VLSA_REVAL_EVT_NRE] = acc[6];
        result[VLSA_REVAL_NOEVT_NRE] = acc[7];
        result[VLSA_REVAL_N_EVT] = acc[8];
        result[VLSA_REVAL_N_NOEVT] = acc[9];
        result[VLSA_REVAL_NONFINITE] = acc[10];
        result[VLSA_REVAL_EVENTS] = acc[11];
        result[VLSA_REVAL_M] = (double)M;
    }
}

}  // namespace vlsa

using namespace vlsa;

static int split_size(int M) { return M < 1 ? VLSA_EINVAL : (M > VLSA_EVAL_MAX_M ? VLSA_EUNSUPPORTED : VLSA_OK); }

extern "C" int vlsa_cox_risk_sets(const float* theta, const double* time, const float* e, int M, double cap, double* D, void* stream) {
    if (!theta || !time || !e || !D || cap != cap) return VLSA_EINVAL;
    if (const int rc = split_size(M)) return rc;
    hipLaunchKernelGGL(k_cox_risk_sets, dim3((M + kSplitTile - 1) / kSplitTile), dim3(kSplitTile), 0, (hipStream_t)stream, theta, time, M, cap, D);
    return launch_status();
}

extern "C" int vlsa_cox_cum_hazard(const double* time, const float* e, const double* D, int M, const double* query, int Q, double* H,
                                   void* stream) {
    if (!time || !e || !D || !query || !H || Q < 1) return VLSA_EINVAL;
    if (const int rc = split_size(M)) return rc;
    if (Q > VLSA_EVAL_MAX_M) return VLSA_EUNSUPPORTED;
    hipLaunchKernelGGL(k_cox_cum_hazard, dim3((Q + kSplitTile - 1) / kSplitTile), dim3(kSplitTile), 0, (hipStream_t)stream, time, e, D, M, query, Q,
                       H);
    return launch_status();
}

extern "C" int vlsa_cox_finish(const float* theta, const float* e, const double* D, int M, double cap, double* result, void* stream) {
    if (!theta || !e || !D || !result || cap != cap) return VLSA_EINVAL;
    if (const int rc = split_size(M)) return rc;
    hipLaunchKernelGGL(k_cox_finish, dim3(1), dim3(kSplitTile), 0, (hipStream_t)stream, theta, e, D, M, cap, result);
    return launch_status();
}

extern "C" int vlsa_reg_eval(const float* pred, const double* time, const float* e, int M, double rank_gamma, int rank_norm,
                             double recon_alpha, double recon_gamma, int recon_norm, double end_time, double* partial, double* rank_grad,
                             double* result, void* stream) {
    if (!pred || !time || !e || !partial || !result) return VLSA_EINVAL;
    if ((rank_norm != VLSA_PAIR_NORM_L1 && rank_norm != VLSA_PAIR_NORM_L2) || (recon_norm != VLSA_PAIR_NORM_L1 && recon_norm != VLSA_PAIR_NORM_L2))
        return VLSA_EINVAL;
    if (const int rc = split_size(M)) return rc;
    hipLaunchKernelGGL(k_reg_pairs, dim3((M + kSplitTile - 1) / kSplitTile), dim3(kSplitTile), 0, (hipStream_t)stream, pred, time, e, M, rank_gamma,
                       rank_norm == VLSA_PAIR_NORM_L2 ? 1 : 0, partial, rank_grad);
    hipLaunchKernelGGL(k_reg_finish, dim3(1), dim3(kSplitTile), 0, (hipStream_t)stream, pred, time, e, M, recon_alpha, recon_gamma,
                       recon_norm == VLSA_PAIR_NORM_L2 ? 1 : 0, end_time, (const double*)partial, result);
    return launch_status();
}

extern "C" int vlsa_surv_pair_objective(const float* pred, const void* time, int time_dtype, const float* e, int B, double w_ple,
                                        double w_rank, double w_recon, double w_mse, double rank_gamma, int rank_norm, double recon_alpha,
                                        double recon_gamma, int recon_norm, int mse_include_censored, float* objective, float* grad,
                                        void* stream) {
    if (!pred || !time || !e || !objective || B < 1) return VLSA_EINVAL;
    if (time_dtype != VLSA_PAIR_TIME_F32 && time_dtype != VLSA_PAIR_TIME_F64) return VLSA_EINVAL;
    if ((rank_norm != VLSA_PAIR_NORM_L1 && rank_norm != VLSA_PAIR_NORM_L2) || (recon_norm != VLSA_PAIR_NORM_L1 && recon_norm != VLSA_PAIR_NORM_L2))
        return VLSA_EINVAL;
    if (B > kPairObjMaxB) return VLSA_EUNSUPPORTED;
    const PairObjArgs a{pred, time, e, B, time_dtype == VLSA_PAIR_TIME_F64 ? 1 : 0, w_ple, w_rank, w_recon, w_mse, rank_gamma, recon_alpha,
                        recon_gamma, rank_norm == VLSA_PAIR_NORM_L2 ? 1 : 0, recon_norm == VLSA_PAIR_NORM_L2 ? 1 : 0,
                        mse_include_censored ? 1 : 0, objective, grad};
    int threads = (B + 63) / 64 * 64;
    threads = threads > kPairObjThreads ? kPairObjThreads : threads;
    launch_lds<k_surv_pair_objective>(dim3(1), dim3(threads), (size_t)B * kPairObjLdsPerSample, (hipStream_t)stream, a);
    return launch_status();
}
