// On-device loss tail of the training step: the handler's objectives on the [B, K] bag predictions
// (runner/vlsa_handler.py:33-41, 241-258; loss/utils.py:52-76), forward AND gradient in one launch, from the raw logits (the handler's
// converter fused in) or from converted values.  The INCIDENCE family -- SurvIFMLE (loss/loss_surv.py:127-169) behind the softmax -- and
// the HAZARD family -- SurvMLE (loss/loss_surv.py:89-124) behind the sigmoid --, each with SurvEMD (loss/loss_surv_ext.py:43-109,
// cdf_loss 13-38) on the converted values, and SurvT2I (loss/loss_surv_ext.py:126-195), a masked softmax over the SAMPLES of the batch
// for each time bin.  The reference spends ~40 elementwise launches and a Python loop over the batch (convert_survival_label) on this.
// One kernel pair serves every entry point: a 16-lane row per sample up to 16 bins, a sample per thread with LDS vectors up to 64;
// cumulative products and sums in bin order (see row16_prefix); every reduction in a fixed order: two runs give the same bits.
#include "vlsa_common.h"
#include "launch.h"
#include "surv_rows16.h"

namespace vlsa {

struct SurvTermArgs {
    const float* x; const int64_t* t; const float* e; int B, K;
    int conv, family;                    // VLSA_CONV_*, VLSA_SURV_*
    const float* ls; int ls_is_log;
    float alpha, eps; int p, raw;
    float w_main, w_emd, w_t2i; int t2i_kl, t2i_mean;
    float *out_main, *out_emd, *grad, *objective;
};

// ---- SurvT2I: one softmax per bin over the samples that take part in it
// A sample takes part in bin k when it is an event, or censored with t > k (sel_ind: a censored sample is dropped wherever its converted
// label is 1); the positives are the events with t == k.  A bin without a positive is skipped (one without a participant has none).
struct T2iCol { float mx, inv_s, tp, tn; };            // max and 1 / sum exp over the participants; the target of a positive / another participant.  inv_s == 0: skipped
template <int NT> struct T2iScratch { double s[3][NT]; float mx[NT]; int np[NT], nn[NT]; };

__device__ __forceinline__ int clamp_bin(int64_t t, int K) { const int v = (int)t; return v < 0 ? 0 : (v >= K ? K - 1 : v); }

// Column gcol by the nrg threads {rg = 0 .. nrg - 1} that share lcol (slot of a thread: rg * ncb + lcol == threadIdx.x): thread rg walks the
// samples rg, rg + nrg, ...; maxima and counts are exact in any order, the three sums are added in double, per thread in sample order and
// then over rg = 0, 1, ... by the thread rg == 0.  Leaves cols[lcol] and val[lcol] (the bin's loss) in LDS; ends with a barrier.
template <int NT>
__device__ __forceinline__ void t2i_column(const float* __restrict__ x, const int64_t* __restrict__ t_, const float* __restrict__ e_, int B, int K,
                                           int gcol, int lcol, int ncb, int rg, int nrg, float ls, int kl, T2iScratch<NT>& sc, T2iCol* cols,
                                           double* val) {
    const int tid = threadIdx.x;
    const bool live = gcol < K;
    float mx = -INFINITY;
    int np = 0, nn = 0;
    if (live)
        for (int b = rg; b < B; b += nrg) {
            const int t = clamp_bin(t_[b], K);
            const bool ev = (int)e_[b] != 0;
            if (ev || t > gcol) {
                mx = fmaxf(mx, x[(size_t)b * K + gcol]);
                if (ev && t == gcol) ++np; else ++nn;
            }
        }
    sc.mx[tid] = mx; sc.np[tid] = np; sc.nn[tid] = nn;
    __syncthreads();
    mx = -INFINITY; np = 0; nn = 0;
    for (int r = 0; r < nrg; ++r) { const int s = r * ncb + lcol; mx = fmaxf(mx, sc.mx[s]); np += sc.np[s]; nn += sc.nn[s]; }
    const bool counted = live && np > 0;
    double s0 = 0., s1 = 0., s2 = 0.;
    if (counted)
        for (int b = rg; b < B; b += nrg) {
            const int t = clamp_bin(t_[b], K);
            const bool ev = (int)e_[b] != 0;
            if (ev || t > gcol) {
                const float d = x[(size_t)b * K + gcol] - mx;
                s0 += (double)expf(d);
                if (ev && t == gcol) s1 += (double)d; else s2 += (double)d;
            }
        }
    sc.s[0][tid] = s0; sc.s[1][tid] = s1; sc.s[2][tid] = s2;
    __syncthreads();
    if (rg == 0) {
        T2iCol c{0.f, 0.f, 0.f, 0.f};
        double v = 0.;
        if (counted) {
            double S = 0., sp = 0., sn = 0.;
            for (int r = 0; r < nrg; ++r) { const int s = r * ncb + lcol; S += sc.s[0][s]; sp += sc.s[1][s]; sn += sc.s[2][s]; }
            const double logS = log(S), dnp = (double)np, dnn = (double)nn;
            double tp, tn = 0.;
            if (!kl) {              // SupConLoss: -mean over the positives of the log-softmax
                tp = 1. / dnp;
                v = logS - sp / dnp;
            } else {                // KLDivLoss('sum') against softmax((2 target - 1) ls): two values, a positive's and another participant's
                const double q = exp(-2. * (double)ls), Z = dnp + dnn * q;
                tp = 1. / Z;
                tn = q / Z;
                v = dnp * tp * log(tp) + (tn > 0. ? dnn * tn * log(tn) : 0.) - tp * (sp - dnp * logS) - tn * (sn - dnn * logS);
            }
            c = T2iCol{mx, (float)(1. / S), (float)tp, (float)tn};
        }
        cols[lcol] = c;
        val[lcol] = v;
    }
    __syncthreads();
}

// d T2I / d x[b, k] of a sample with label (ev, t), before the weight and the 1 / (counted bins) of 'mean'
__device__ __forceinline__ float t2i_grad(float xv, bool ev, int t, int k, const T2iCol& c) {
    if (c.inv_s == 0.f || !(ev || t > k)) return 0.f;
    return expf(xv - c.mx) * c.inv_s - ((ev && t == k) ? c.tp : c.tn);
}

// value (sum over the counted bins in bin order, or their mean) and the factor of the gradient
__device__ __forceinline__ void t2i_total(const T2iCol* cols, const double* val, int K, int mean, float weight, double& value, float& coef) {
    int nc = 0;
    double v = 0.;
    for (int k = 0; k < K; ++k)
        if (cols[k].inv_s != 0.f) { ++nc; v += val[k]; }
    const bool div = mean && nc > 0;
    value = div ? v / (double)nc : v;
    coef = div ? weight / (float)nc : weight;
}

// ---- 17 .. 64 bins: one sample per thread (the first kTermThreads threads of the block), the K-vectors in LDS [vector][k][thread].
// (As dynamically indexed private arrays the K-vectors sat in scratch memory and the launch took 18.6 us for 32 samples x 12 bins, round 4:
// profiles/r04_step_kernel_stats.csv.  Same serial order per sample as then: the results are bit-identical.)
// objective == null: a block of kTermThreads per 32 samples, per-sample values and the unscaled gradient rows.
// objective != null (round 6): ONE block of kTermBlock threads; its first 32 walk the batch in chunks of 32 samples and also write the scalar
// objective[0] = mean_i (w_main main_i + w_emd emd_i) (+ w_t2i T2I) -- the handler's calc_objective_loss for 'mean'-reduced losses -- and
// `grad` comes out scaled by 1 / B (the gradient of that mean): the five elementwise / reduction launches behind the per-sample values
// were 25 us of a 1.7 ms optimizer step.  ls_is_log: `ls` points at the RAW (log) logit scale parameter and is exponentiated here (saves
// the step's `logit_scale.exp()` launch).  All kTermBlock threads take the SurvT2I columns (a bin per thread, kTermBlock / 64 sample groups).
// (Round 6, tried and removed: the same arithmetic with the per-sample vectors in registers and every bin loop unrolled to 16 -- 14.1 us
//  against 12.5 us for the LDS loops below inside the training step: one wave running ~20 KB of straight-line code once is bound by
//  instruction fetch, not by the LDS round trips.  Parking the sample's K inputs in LDS with one batch of loads first: no change either,
//  12.7 -> 13.5 us on another box -- the time is the ~500 dependent LDS accesses of the bin loops.)
constexpr int kTermThreads = 32, kTermBlock = 256, kTermCols = 64;
struct TermVec {
    float* p;
    __device__ __forceinline__ float& operator[](int k) const { return p[k * kTermThreads]; }
};
template <bool T2I>
__global__ __launch_bounds__(kTermBlock) void k_surv_terms(const SurvTermArgs a) {
    __shared__ float sm[4][VLSA_MAX_K][kTermThreads];
    __shared__ T2iScratch<kTermBlock> sc;
    __shared__ T2iCol cols[kTermCols];
    __shared__ double colval[kTermCols];
    const int tid = threadIdx.x, B = a.B, K = a.K;
    constexpr bool t2i = T2I;
    const bool obj = a.objective != nullptr;
    const bool need_emd = a.w_emd != 0.f || a.out_emd != nullptr;
    float ls = 0.f;
    if (need_emd || t2i) ls = a.ls_is_log ? expf(a.ls[0]) : a.ls[0];
    double t2i_value = 0.;
    float t2i_coef = 0.f;
    if constexpr (t2i) {
        t2i_column<kTermBlock>(a.x, a.t, a.e, B, K, tid % kTermCols, tid % kTermCols, kTermCols, tid / kTermCols, kTermBlock / kTermCols, ls, a.t2i_kl,
                               sc, cols, colval);
        t2i_total(cols, colval, K, a.t2i_mean, a.w_t2i, t2i_value, t2i_coef);
    }
    if (tid >= kTermThreads) return;                    // (no barrier below this line)
    float obj_acc = 0.f;
    const int n_chunks = obj ? (B + kTermThreads - 1) / kTermThreads : 1;
    const float gscale = obj ? 1.f / (float)B : 1.f;
    const float alpha = a.alpha, eps = a.eps, w_main = a.w_main, w_emd = a.w_emd;
    const int p = a.p;
    for (int chunk = 0; chunk < n_chunks; ++chunk) {
        const int i = (obj ? chunk : (int)blockIdx.x) * kTermThreads + tid;
        if (i >= B) continue;
        const TermVec y{&sm[0][0][tid]}, q{&sm[1][0][tid]}, pd{&sm[2][0][tid]}, td{&sm[3][0][tid]};
        const float* xi = a.x + (size_t)i * K;
        const int t = clamp_bin(a.t[i], K);
        const float e = a.e[i], c = 1.f - e;
        const int ei = (int)e;  // e.long() of the reference
        // ---- the converter (utils/func.py:43-46) or the given values.  1 - h is formed as sigmoid(-x): 1 - sigmoid(x) loses it to rounding
        if (a.conv == VLSA_CONV_SOFTMAX) {
            float mx = -INFINITY, s = 0.f;
            for (int k = 0; k < K; ++k) mx = fmaxf(mx, xi[k]);
            for (int k = 0; k < K; ++k) { y[k] = expf(xi[k] - mx); s += y[k]; }
            for (int k = 0; k < K; ++k) y[k] /= s;
        } else if (a.conv == VLSA_CONV_SIGMOID) {
            for (int k = 0; k < K; ++k) { y[k] = 1.f / (1.f + expf(-xi[k])); q[k] = 1.f / (1.f + expf(xi[k])); }
        } else {
            for (int k = 0; k < K; ++k) { y[k] = xi[k]; q[k] = 1.f - xi[k]; }
        }
        // ---- the likelihood term: value and three coefficients of its gradient -- cA at bin t, cLE on the bins <= t, cLT on the bins < t
        float l_main, cA = 0.f, cLE = 0.f, cLT = 0.f;
        const float av = y[t];
        if (a.family == VLSA_SURV_IFMLE) {
            float cif = 0.f;
            for (int k = 0; k <= t; ++k) cif += y[k];
            const float sv = 1.f - cif;
            const float unc = -(1.f - c) * logf(fmaxf(av, eps));
            const float cen = -c * logf(fmaxf(sv, eps));
            l_main = (1.f - alpha) * (cen + unc) + alpha * unc;
            if (av >= eps) cA = w_main * (-(1.f - c) / av);             // the clamp passes the gradient at >= eps
            if (sv >= eps) cLE = w_main * (1.f - alpha) * c / sv;
        } else {                                                        // SurvMLE: S_padded = [1, cumprod(1 - h)]
            float st = 1.f;
            for (int k = 0; k < t; ++k) st *= q[k];
            const float st1 = st * q[t];
            const float unc = -(1.f - c) * (logf(fmaxf(st, eps)) + logf(fmaxf(av, eps)));
            const float cen = -c * logf(fmaxf(st1, eps));
            l_main = (1.f - alpha) * (cen + unc) + alpha * unc;
            // d -log S_padded[t] / d x_k = h_k (k < t), d -log h_t / d x_t = -sigmoid(-x_t); d . / d h_k = 1 / (1 - h_k), -1 / h_t
            if (st >= eps) cLT = w_main * (1.f - c);
            if (av >= eps) cA = -w_main * (1.f - c);
            if (st1 >= eps) cLE = w_main * (1.f - alpha) * c;
        }

        // ---- SurvEMD on y
        float l_emd = 0.f, emd_outer = 0.f, emd_dot = 0.f;
        if (need_emd) {
            float mp = -INFINITY, mt = -INFINITY;
            for (int k = 0; k < K; ++k) {
                const float tg = (k == t ? 1.f : 0.f) + (k > t ? (float)(1 - ei) : 0.f);   // convert_survival_label
                td[k] = (2.f * tg - 1.f) * ls;
                pd[k] = (float)(1 - ei) * ((1.f - tg) * y[k] + tg * ls) + (float)ei * y[k];
                mp = fmaxf(mp, pd[k]);
                mt = fmaxf(mt, td[k]);
            }
            float sp = 0.f, st = 0.f;
            for (int k = 0; k < K; ++k) { pd[k] = expf(pd[k] - mp); sp += pd[k]; td[k] = expf(td[k] - mt); st += td[k]; }
            float cp = 0.f, ct = 0.f, S = 0.f;
            for (int k = 0; k < K; ++k) {
                pd[k] /= sp;
                cp += pd[k];
                ct += td[k] / st;
                const float d = cp - ct;
                td[k] = d;                                   // td now holds the cdf difference
                S += (p == 1) ? fabsf(d) : d * d;
            }
            const bool root = (p == 2 && !a.raw);
            l_emd = root ? sqrtf(S) : S;
            if (w_emd != 0.f) {
                emd_outer = w_emd * (root ? (S > 0.f ? 0.5f / sqrtf(S) : 0.f) : 1.f);
                float r = 0.f;
                for (int k = K - 1; k >= 0; --k) {          // r_j = d dist / d pd_j = suffix sum of d S / d d_k
                    const float d = td[k];
                    r += (p == 1) ? (d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f)) : 2.f * d;
                    td[k] = r;
                    emd_dot += pd[k] * r;
                }
            }
        }

        if (a.out_main != nullptr) a.out_main[i] = l_main;
        if (a.out_emd != nullptr) a.out_emd[i] = l_emd;
        obj_acc += w_main * l_main + w_emd * l_emd;
        if (a.grad != nullptr) {
            float* gi = a.grad + (size_t)i * K;
            float ydot = 0.f;
            for (int k = 0; k < K; ++k) {                   // pd[k] <- the gradient at bin k: in x for the sigmoid converter, else in y
                float ge = 0.f;
                if (w_emd != 0.f) {
                    const float tg = (k == t ? 1.f : 0.f) + (k > t ? (float)(1 - ei) : 0.f);
                    ge = emd_outer * pd[k] * (td[k] - emd_dot) * ((float)(1 - ei) * (1.f - tg) + (float)ei);
                }
                const float cf = (k < t ? cLT : 0.f) + (k <= t ? cLE : 0.f);
                float g;
                if (a.family == VLSA_SURV_IFMLE) g = cf + (k == t ? cA : 0.f) + ge;
                else if (a.conv == VLSA_CONV_SIGMOID) g = cf * y[k] + (k == t ? cA * q[k] : 0.f) + ge * (y[k] * q[k]);
                else g = (cf != 0.f ? cf / q[k] : 0.f) + ((k == t && cA != 0.f) ? cA / av : 0.f) + ge;
                pd[k] = g;
                ydot += y[k] * g;
            }
            for (int k = 0; k < K; ++k) {
                float g = pd[k];
                if (a.conv == VLSA_CONV_SOFTMAX) g = y[k] * (g - ydot);      // softmax backward to the raw logits
                g *= gscale;
                // (an explicit fma onto the ROUNDED g * gscale, as the kernel computed it while SurvT2I was a run-time branch: left to the
                //  compiler, the product g * gscale is the one that gets fused into the sum -- another last bit)
                if constexpr (t2i) g = fmaf(t2i_coef, t2i_grad(xi[k], ei != 0, t, k, cols[k]), g);
                gi[k] = g;
            }
        }
    }
    if (obj) {
        float s = obj_acc;      // fixed-order sum over the 32 lanes (lanes without a sample hold 0)
#pragma unroll
        for (int o = 16; o > 0; o >>= 1) s += __shfl_xor(s, o, 32);
        if (tid == 0) a.objective[0] = s / (float)B + (float)((double)a.w_t2i * t2i_value);
    }
}

// ---- K <= 16 bins (the reference's 4 .. 12): a sample per 16-LANE ROW, a bin per lane -- every loop over the bins above becomes a row
// operation through DPP (sum / max by row rotations, the cumulative sums and products by shifted adds and multiplies), 32 samples per
// 512-thread workgroup and pass.  Same formulas; the cumulative sums keep the bin order (see row16_prefix), plain sums run in tree order.
// Inside the training step, SurvIFMLE + SurvEMD: 12.7 -> 4.7 us = the floor of a launch (the loops above are ~500 dependent LDS accesses
// on one wave; measured on k_surv_loss_rows16, the kernel this one took over: back to back the same work is 3.55 us here against 3.44 us
// there, profiles/r22_surv_terms_fold_ab.txt).  (row16_sum: vlsa_common.h; row16_max, row16_prefix, row16_suffix, row16_prefix_prod: surv_rows16.h)
// The SurvT2I columns: bin = lane of the row, 32 sample groups.
constexpr int kTermWide = 512, kTermWideSamples = kTermWide / 16;
template <bool T2I>
__global__ __launch_bounds__(kTermWide) void k_surv_terms_rows16(const SurvTermArgs a) {
    __shared__ float sval[kTermWideSamples];
    __shared__ T2iScratch<kTermWide> sc;
    __shared__ T2iCol cols[16];
    __shared__ double colval[16];
    const int tid = threadIdx.x, k = tid & 15, sub = tid >> 4, B = a.B, K = a.K;
    constexpr bool t2i = T2I;
    const bool obj = a.objective != nullptr, kk = k < K;
    const bool need_emd = a.w_emd != 0.f || a.out_emd != nullptr;
    const int n_chunks = obj ? (B + kTermWideSamples - 1) / kTermWideSamples : 1;
    const float gscale = obj ? 1.f / (float)B : 1.f;
    const float alpha = a.alpha, eps = a.eps, w_main = a.w_main, w_emd = a.w_emd;
    const int p = a.p;
    float ls = 0.f;
    if (need_emd || t2i) ls = a.ls_is_log ? expf(a.ls[0]) : a.ls[0];
    double t2i_value = 0.;
    float t2i_coef = 0.f;
    T2iCol col{0.f, 0.f, 0.f, 0.f};
    if constexpr (t2i) {
        t2i_column<kTermWide>(a.x, a.t, a.e, B, K, k, k, 16, sub, kTermWideSamples, ls, a.t2i_kl, sc, cols, colval);
        t2i_total(cols, colval, K, a.t2i_mean, a.w_t2i, t2i_value, t2i_coef);
        if (kk) col = cols[k];
    }
    float obj_acc = 0.f;                      // threads 0 .. 31: the samples chunk * 32 + tid
    for (int chunk = 0; chunk < n_chunks; ++chunk) {
        const int i = (obj ? chunk : (int)blockIdx.x) * kTermWideSamples + sub;
        const bool valid = i < B;             // (rows without a sample run on zeros: every lane takes part in the row operations)
        const float xv = (valid && kk) ? a.x[(size_t)i * K + k] : 0.f;
        const int t = valid ? clamp_bin(a.t[i], K) : 0;
        const float e = valid ? a.e[i] : 0.f, c = 1.f - e;
        const int ei = (int)e;
        float y, q = 1.f;                     // (lanes past the last bin: y = 0, 1 - y = 1)
        if (a.conv == VLSA_CONV_SOFTMAX) {
            const float mx = row16_max(kk ? xv : -INFINITY);
            const float ex = kk ? expf(xv - mx) : 0.f;
            y = ex / row16_sum(ex);
        } else if (a.conv == VLSA_CONV_SIGMOID) {
            y = kk ? 1.f / (1.f + expf(-xv)) : 0.f;
            q = kk ? 1.f / (1.f + expf(xv)) : 1.f;
        } else {
            y = kk ? xv : 0.f;
            q = kk ? 1.f - xv : 1.f;
        }
        // (row operations are evaluated by EVERY lane, outside any lane-dependent condition)
        const float av = row16_sum(k == t ? y : 0.f);
        float l_main, cA = 0.f, cLE = 0.f, cLT = 0.f;
        if (a.family == VLSA_SURV_IFMLE) {
            const float cum = row16_prefix(y);
            const float sv = 1.f - row16_sum(k == t ? cum : 0.f);
            const float unc = -(1.f - c) * logf(fmaxf(av, eps));
            const float cen = -c * logf(fmaxf(sv, eps));
            l_main = (1.f - alpha) * (cen + unc) + alpha * unc;
            if (av >= eps) cA = w_main * (-(1.f - c) / av);
            if (sv >= eps) cLE = w_main * (1.f - alpha) * c / sv;
        } else {
            const float cum = row16_prefix_prod(q);                       // cumprod(1 - h) in bin order
            const float st1 = row16_sum(k == t ? cum : 0.f);
            const float stp = row16_sum(k == t - 1 ? cum : 0.f);
            const float st = t == 0 ? 1.f : stp;                          // S_padded[t]
            const float unc = -(1.f - c) * (logf(fmaxf(st, eps)) + logf(fmaxf(av, eps)));
            const float cen = -c * logf(fmaxf(st1, eps));
            l_main = (1.f - alpha) * (cen + unc) + alpha * unc;
            if (st >= eps) cLT = w_main * (1.f - c);
            if (av >= eps) cA = -w_main * (1.f - c);
            if (st1 >= eps) cLE = w_main * (1.f - alpha) * c;
        }
        float l_emd = 0.f, ge = 0.f;
        if (need_emd) {
            const float tg = (k == t ? 1.f : 0.f) + (k > t ? (float)(1 - ei) : 0.f);       // convert_survival_label
            const float tdv = kk ? (2.f * tg - 1.f) * ls : -INFINITY;
            const float pdv = kk ? (float)(1 - ei) * ((1.f - tg) * y + tg * ls) + (float)ei * y : -INFINITY;
            const float dpv = (float)(1 - ei) * (1.f - tg) + (float)ei;
            const float mp = row16_max(pdv), mt = row16_max(tdv);
            const float pe = kk ? expf(pdv - mp) : 0.f, te = kk ? expf(tdv - mt) : 0.f;
            const float pn = pe / row16_sum(pe), tn = te / row16_sum(te);
            const float cp = row16_prefix(pn), ct = row16_prefix(tn);
            const float d = kk ? cp - ct : 0.f;
            const float S = row16_sum((p == 1) ? fabsf(d) : d * d);
            const bool root = (p == 2 && !a.raw);
            l_emd = root ? sqrtf(S) : S;
            if (w_emd != 0.f) {
                const float outer = root ? (S > 0.f ? 0.5f / sqrtf(S) : 0.f) : 1.f;
                const float r = row16_suffix((p == 1) ? (d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f)) : 2.f * d);
                const float dot = row16_sum(pn * r);
                ge = w_emd * outer * pn * (r - dot) * dpv;
            }
        }
        if (valid && k == 0) {
            if (a.out_main != nullptr) a.out_main[i] = l_main;
            if (a.out_emd != nullptr) a.out_emd[i] = l_emd;
        }
        if (a.grad != nullptr) {
            const float cf = (k < t ? cLT : 0.f) + (k <= t ? cLE : 0.f);
            float g;
            if (a.family == VLSA_SURV_IFMLE) g = cf + (k == t ? cA : 0.f) + ge;
            else if (a.conv == VLSA_CONV_SIGMOID) g = cf * y + (k == t ? cA * q : 0.f) + ge * (y * q);
            else g = (cf != 0.f ? cf / q : 0.f) + ((k == t && cA != 0.f) ? cA / av : 0.f) + ge;
            const float ydot = row16_sum(y * g);
            if (a.conv == VLSA_CONV_SOFTMAX) g = y * (g - ydot);          // softmax backward to the raw logits
            g *= gscale;
            if constexpr (t2i) { if (kk) g += t2i_coef * t2i_grad(xv, ei != 0, t, k, col); }
            if (valid && kk) a.grad[(size_t)i * K + k] = g;
        }
        if (obj) {
            if (k == 0) sval[sub] = valid ? w_main * l_main + w_emd * l_emd : 0.f;
            __syncthreads();
            if (tid < kTermWideSamples) obj_acc += sval[tid];
            __syncthreads();
        }
    }
    if (obj && tid < 32) {
        float s = obj_acc;
#pragma unroll
        for (int o = 16; o > 0; o >>= 1) s += __shfl_xor(s, o, 32);
        if (tid == 0) a.objective[0] = s / (float)B + (float)((double)a.w_t2i * t2i_value);
    }
}

// ---- SurvT2I alone, any batch the evaluator takes: a workgroup per bin leaves the column's numbers in `work`, then a launch over the
// elements writes the gradient and (its first thread) the value.
constexpr int kT2iThreads = 256;
__global__ __launch_bounds__(kT2iThreads) void k_t2i_columns(const float* __restrict__ x, const int64_t* __restrict__ t_, const float* __restrict__ e_,
                                                             int B, int K, const float* __restrict__ ls_, int ls_is_log, int kl, double* __restrict__ work) {
    __shared__ T2iScratch<kT2iThreads> sc;
    __shared__ T2iCol cols[1];
    __shared__ double colval[1];
    const float ls = ls_is_log ? expf(ls_[0]) : ls_[0];
    t2i_column<kT2iThreads>(x, t_, e_, B, K, (int)blockIdx.x, 0, 1, (int)threadIdx.x, kT2iThreads, ls, kl, sc, cols, colval);
    if (threadIdx.x == 0) {
        double* w = work + (size_t)blockIdx.x * VLSA_T2I_WORK_PER_BIN;
        w[0] = cols[0].mx; w[1] = cols[0].inv_s; w[2] = cols[0].tp; w[3] = cols[0].tn; w[4] = colval[0];
    }
}
__global__ __launch_bounds__(kT2iThreads) void k_t2i_finish(const float* __restrict__ x, const int64_t* __restrict__ t_, const float* __restrict__ e_,
                                                            int B, int K, int mean, float weight, const double* __restrict__ work,
                                                            float* __restrict__ value, float* __restrict__ grad) {
    __shared__ T2iCol cols[VLSA_MAX_K];
    __shared__ double colval[VLSA_MAX_K];
    if ((int)threadIdx.x < K) {
        const double* w = work + (size_t)threadIdx.x * VLSA_T2I_WORK_PER_BIN;
        cols[threadIdx.x] = T2iCol{(float)w[0], (float)w[1], (float)w[2], (float)w[3]};
        colval[threadIdx.x] = w[4];
    }
    __syncthreads();
    double v;
    float coef;
    t2i_total(cols, colval, K, mean, weight, v, coef);
    if (blockIdx.x == 0 && threadIdx.x == 0 && value != nullptr) value[0] = (float)((double)weight * v);
    if (grad == nullptr) return;
    const size_t n = (size_t)B * K, idx = (size_t)blockIdx.x * kT2iThreads + threadIdx.x;
    if (idx >= n) return;
    const int b = (int)(idx / K), k = (int)(idx % K);
    grad[idx] = coef * t2i_grad(x[idx], (int)e_[b] != 0, clamp_bin(t_[b], K), k, cols[k]);
}

}  // namespace vlsa

using namespace vlsa;

constexpr int kOneBlockMaxB = 4096;       // one block walks the batch

static int check_terms(const float* x, const int64_t* t, const float* e, int B, int K, int conv, int family, const float* ls, float w_emd,
                       bool want_emd, int p) {
    if (!x || !t || !e || B < 1 || K < 1 || K > VLSA_MAX_K) return VLSA_EINVAL;
    if (conv != VLSA_CONV_NONE && conv != VLSA_CONV_SOFTMAX && conv != VLSA_CONV_SIGMOID) return VLSA_EINVAL;
    if (family != VLSA_SURV_IFMLE && family != VLSA_SURV_MLE) return VLSA_EINVAL;
    if ((w_emd != 0.f || want_emd) && !ls) return VLSA_EINVAL;
    // the handler's rule (runner/vlsa_handler.py:33-41): incidences come from the softmax, hazards from the sigmoid
    if ((conv == VLSA_CONV_SOFTMAX && family == VLSA_SURV_MLE) || (conv == VLSA_CONV_SIGMOID && family == VLSA_SURV_IFMLE)) return VLSA_EUNSUPPORTED;
    if (p != 1 && p != 2) return VLSA_EUNSUPPORTED;
    return VLSA_OK;
}

// The dispatch of every entry point below.  a.objective == null: a block per 32 samples; else the ONE block that walks the batch.
// SurvT2I is a compile-time parameter of both kernels: the instantiation without it carries neither the column scratch nor its registers,
// and above 16 bins it is launched without the threads that would only walk the columns.
static int launch_terms(const SurvTermArgs& a, void* stream) {
    const bool obj = a.objective != nullptr, t2i = obj && a.w_t2i != 0.f;
    if (a.K <= 16)
        hipLaunchKernelGGL(t2i ? k_surv_terms_rows16<true> : k_surv_terms_rows16<false>,
                           dim3(obj ? 1 : (a.B + kTermWideSamples - 1) / kTermWideSamples), dim3(kTermWide), 0, (hipStream_t)stream, a);
    else
        hipLaunchKernelGGL(t2i ? k_surv_terms<true> : k_surv_terms<false>, dim3(obj ? 1 : (a.B + kTermThreads - 1) / kTermThreads),
                           dim3(t2i ? kTermBlock : kTermThreads), 0, (hipStream_t)stream, a);
    return launch_status();
}

extern "C" int vlsa_surv_terms(const float* x, const int64_t* t, const float* e, int B, int K, int converter, int family,
                               const float* logit_scale_exp, float alpha, float eps, int p, int raw_distance, float w_main, float w_emd,
                               float* out_main, float* out_emd, float* grad, void* stream) {
    const int rc = check_terms(x, t, e, B, K, converter, family, logit_scale_exp, w_emd, out_emd != nullptr, p);
    if (rc != VLSA_OK) return rc;
    return launch_terms(SurvTermArgs{x, t, e, B, K, converter, family, logit_scale_exp, 0, alpha, eps, p, raw_distance, w_main, w_emd, 0.f, 0, 0,
                                     out_main, out_emd, grad, nullptr}, stream);
}

extern "C" int vlsa_surv_objective_terms(const float* x, const int64_t* t, const float* e, int B, int K, int converter, int family,
                                         const float* logit_scale, int ls_is_log, float alpha, float eps, int p, int raw_distance,
                                         float w_main, float w_emd, float w_t2i, int t2i_loss, int t2i_reduction, float* objective,
                                         float* grad, void* stream) {
    const int rc = check_terms(x, t, e, B, K, converter, family, logit_scale, w_emd, false, p);
    if (rc != VLSA_OK) return rc;
    if (!objective || B > kOneBlockMaxB) return VLSA_EINVAL;
    if (w_t2i != 0.f) {
        if (converter == VLSA_CONV_NONE || !logit_scale) return VLSA_EINVAL;       // SurvT2I reads the raw logits
        if ((t2i_loss != VLSA_T2I_CL && t2i_loss != VLSA_T2I_KL) || (t2i_reduction != VLSA_T2I_SUM && t2i_reduction != VLSA_T2I_MEAN))
            return VLSA_EUNSUPPORTED;
    }
    return launch_terms(SurvTermArgs{x, t, e, B, K, converter, family, logit_scale, ls_is_log, alpha, eps, p, raw_distance, w_main, w_emd, w_t2i,
                                     t2i_loss == VLSA_T2I_KL, t2i_reduction == VLSA_T2I_MEAN, nullptr, nullptr, grad, objective}, stream);
}

// ---- the incidence family under its first names: SurvIFMLE + SurvEMD from the raw logits (from_logits != 0: the softmax converter) or
// from incidences.  vlsa_surv_loss is vlsa_surv_terms, vlsa_surv_objective is vlsa_surv_objective_terms without SurvT2I.
extern "C" int vlsa_surv_loss(const float* x, const int64_t* t, const float* e, int B, int K, int from_logits,
                              const float* logit_scale_exp, float alpha, float eps, int p, int raw_distance, float w_ifmle,
                              float w_emd, float* out_ifmle, float* out_emd, float* grad, void* stream) {
    return vlsa_surv_terms(x, t, e, B, K, from_logits ? VLSA_CONV_SOFTMAX : VLSA_CONV_NONE, VLSA_SURV_IFMLE, logit_scale_exp, alpha, eps, p,
                           raw_distance, w_ifmle, w_emd, out_ifmle, out_emd, grad, stream);
}

// logit_scale: the EXPONENTIATED scale (ls_is_log == 0, the reference's `net.get_logit_scale()`) or the raw parameter (ls_is_log != 0).
extern "C" int vlsa_surv_objective(const float* x, const int64_t* t, const float* e, int B, int K, int from_logits, const float* logit_scale,
                                   int ls_is_log, float alpha, float eps, int p, int raw_distance, float w_ifmle, float w_emd,
                                   float* objective, float* grad, void* stream) {
    if (!objective || B > kOneBlockMaxB) return VLSA_EINVAL;                       // (ahead of the check of p, as this entry always had it)
    return vlsa_surv_objective_terms(x, t, e, B, K, from_logits ? VLSA_CONV_SOFTMAX : VLSA_CONV_NONE, VLSA_SURV_IFMLE, logit_scale, ls_is_log,
                                     alpha, eps, p, raw_distance, w_ifmle, w_emd, 0.f, VLSA_T2I_CL, VLSA_T2I_MEAN, objective, grad, stream);
}

extern "C" int vlsa_surv_t2i(const float* x, const int64_t* t, const float* e, int B, int K, const float* logit_scale, int ls_is_log,
                             int t2i_loss, int t2i_reduction, float weight, double* work, float* value, float* grad, void* stream) {
    if (!x || !t || !e || !logit_scale || !work || (!value && !grad) || B < 1 || K < 1 || K > VLSA_MAX_K) return VLSA_EINVAL;
    if (B > VLSA_EVAL_MAX_M) return VLSA_EUNSUPPORTED;
    if ((t2i_loss != VLSA_T2I_CL && t2i_loss != VLSA_T2I_KL) || (t2i_reduction != VLSA_T2I_SUM && t2i_reduction != VLSA_T2I_MEAN))
        return VLSA_EUNSUPPORTED;
    hipLaunchKernelGGL(k_t2i_columns, dim3(K), dim3(kT2iThreads), 0, (hipStream_t)stream, x, t, e, B, K, logit_scale, ls_is_log,
                       (int)(t2i_loss == VLSA_T2I_KL), work);
    const size_t n = grad ? (size_t)B * K : 1;
    hipLaunchKernelGGL(k_t2i_finish, dim3((unsigned)((n + kT2iThreads - 1) / kT2iThreads)), dim3(kT2iThreads), 0, (hipStream_t)stream, x, t, e, B, K,
                       (int)(t2i_reduction == VLSA_T2I_MEAN), weight, (const double*)work, value, grad);
    return launch_status();
}
