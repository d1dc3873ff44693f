// DSMIL (Li et al., CVPR 2021; model/deepmil.py:638-721) over a table of bags, forward and backward, gfx950.
//
// The reference forms Q = q(X) and V = v(X) for all N rows (two [N,512] x [512,256] products per bag).  Only C <= 16 rows of Q are
// ever used as queries, and V enters through A^T V alone, so the module collapses to two streaming passes over the bag with C query
// rows (fp32 FMA throughout -- no split-bf16 products: an argmax whose runner-up is 3e-4 away must not flip):
//   pass 1  c[n,k] = x_n . Wc[k] (+ bc[k]), never stored: per bag and class the maximum and its row index.  EQUAL maxima resolve to
//           the LOWEST row index; the reference's torch.sort leaves ties open, so ties are not comparable against it.
//   rows    x* = x_{m_k}, qmax_k = Wq x* + bq, u_k = Wq^T qmax_k / sqrt(H)            (B * C small blocks)
//   pass 2  online softmax over n of x_n . u_k (the bq . qmax_k term is constant over n), z_k = sum_n A[n,k] drop(x_n)
//   head    B_k = Wv z_k + bv, logits = 0.5 (fcc(B) + cmax)
// Backward (parameters only): dz_j = Wv^T dB_j, ds[n,j] = A[n,j] (drop(x_n) . dz_j - z_j . dz_j), du_j = sum_n ds[n,j] x_n in one more
// streaming pass that recomputes A from the kept (m, l) and regenerates the masks; then the parameter gradients on C rows per bag,
// summed over the bags in bag order by one launch (bit-reproducible run to run).
//
// A bag of N rows is cut into vlsa_dsmil_parts(N) partial records -- a function of N alone, so a bag's result does not depend on the
// batch it travels in (a batch of B bags equals B single calls bit for bit).  Part g of a bag with G parts takes the row tiles
// g, g + G, ... of that bag.  A workgroup finds its bag and part with bag_span (bag_table.h; DESIGN.md, "Table-driven kernels").
//
// Lane layout of the dot products: 16 lanes share a row, lane j holds the four 8-feature chunks (k * 16 + j), k = 0..3; the C
// partial sums of a row are reduced over the 16 lanes by an exchange that halves the value count per step (15 shuffles for 16
// classes) and leaves class (j * CP / 16) in lane j.  The weighted sums run as a register-tiled [CP x rows] x [rows x 512] product
// out of an LDS copy of the row tile.
#include "bag_table.h"
#include "launch.h"

namespace {
using namespace vlsa;

constexpr int kD = 512, kH = 256, kMaxC = 16, kThreads = 256;
// rows per 16-lane group in the score-only kernels (tiles of 16 x this many rows): as many as the registers hold without spilling
constexpr int rows_per_group(int cp) { return cp <= 4 ? 4 : 2; }
constexpr int kTileB = 32;        // rows per tile of the kernels that keep the tile in LDS (2 rows per group)
constexpr float kInvSqrtH = 0.0625f;
constexpr int kPartRows = 512, kMaxParts = 64;     // rows per partial record of a bag, records per bag


__device__ __forceinline__ void load8(const float* p, float* o) {
    const float4 a = reinterpret_cast<const float4*>(p)[0], b = reinterpret_cast<const float4*>(p)[1];
    o[0] = a.x; o[1] = a.y; o[2] = a.z; o[3] = a.w; o[4] = b.x; o[5] = b.y; o[6] = b.z; o[7] = b.w;
}
__device__ __forceinline__ void load8(const __bf16* p, float* o) {
    const bf16x8 v = *reinterpret_cast<const bf16x8*>(p);
#pragma unroll
    for (int e = 0; e < 8; ++e) o[e] = (float)v[e];
}
__device__ __forceinline__ void store8(float* p, const float* o) {
    reinterpret_cast<float4*>(p)[0] = make_float4(o[0], o[1], o[2], o[3]);
    reinterpret_cast<float4*>(p)[1] = make_float4(o[4], o[5], o[6], o[7]);
}
__device__ __forceinline__ void store8(__bf16* p, const float* o) {      // (exact: the values came from bf16)
    bf16x8 v;
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = (__bf16)o[e];
    *reinterpret_cast<bf16x8*>(p) = v;
}

// R rows of a 16-lane group into registers: x[r][k * 8 + e] = feature (k * 16 + j) * 8 + e of row min(row0 + r, N - 1)
template <typename T, int R>
__device__ __forceinline__ void load_rows(const T* X, long long ldx, long long N, long long row0, int j, float (&x)[R][32]) {
#pragma unroll
    for (int r = 0; r < R; ++r) {
        long long row = row0 + r;
        if (row > N - 1) row = N - 1;
        const T* p = X + row * ldx + j * 8;
#pragma unroll
        for (int k = 0; k < 4; ++k) load8(p + k * 128, &x[r][k * 8]);
    }
}

// acc[r][c] = this lane's share of x_r . W[c] (W: LDS [CP][512] fp32)
template <int CP, int R>
__device__ __forceinline__ void dots(const float (&x)[R][32], const float* W, int j, float (&acc)[R][CP]) {
#pragma unroll
    for (int c = 0; c < CP; ++c) {
        float a[R];
#pragma unroll
        for (int r = 0; r < R; ++r) a[r] = 0.f;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            float w[8];
            load8(W + c * kD + (k * 16 + j) * 8, w);
#pragma unroll
            for (int e = 0; e < 8; ++e)
#pragma unroll
                for (int r = 0; r < R; ++r) a[r] = fmaf(x[r][k * 8 + e], w[e], a[r]);
        }
#pragma unroll
        for (int r = 0; r < R; ++r) acc[r][c] = a[r];
    }
}

// Sum of v[c] over the 16 lanes of a group; lane j returns class j / (16 / CP) (every lane of a class holds the same bits).
template <int CP>
__device__ __forceinline__ float reduce16(float (&v)[CP], int j) {
    int mask = 8;
#pragma unroll
    for (int n = CP; n > 1; n >>= 1, mask >>= 1) {
        const bool up = (j & mask) != 0;
#pragma unroll
        for (int i = 0; i < n / 2; ++i) {
            const float send = up ? v[i] : v[i + n / 2];
            const float keep = up ? v[i + n / 2] : v[i];
            v[i] = keep + __shfl_xor(send, mask);
        }
    }
    for (; mask > 0; mask >>= 1) v[0] += __shfl_xor(v[0], mask);
    return v[0];
}

__device__ __forceinline__ void fill_queries(float* W, const float* src, int C, int CP, float scale) {
    for (int i = threadIdx.x; i < CP * kD; i += kThreads) W[i] = (i < C * kD) ? src[i] * scale : 0.f;
}

// ---- pass 1: per part and class the largest instance score and its row -----------------------------------------------------------
template <typename T, int CP>
__global__ __launch_bounds__(kThreads) void k_dsmil_scores(const vlsa_bag_desc* bags, int B, int C, const int* part_start, const float* Wc,
                                                           float* pmax, int* pidx) {
    __shared__ float W[CP * kD];
    __shared__ float rv[16][CP];
    __shared__ int ri[16][CP];
    const BagSpan part = bag_span(part_start, B, blockIdx.x);
    const int b = part.b, g = part.idx, G = part.count;
    fill_queries(W, Wc, C, CP, 1.f);
    __syncthreads();
    const T* X = static_cast<const T*>(bags[b].X);
    const long long N = bags[b].N, ldx = bags[b].ldx;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, grp = lane >> 4, j = lane & 15;
    constexpr int kRep = 16 / CP;
    float best = -INFINITY;
    int bidx = 0x7fffffff;
    constexpr int R = rows_per_group(CP), kTile = 16 * R;
    const long long ntiles = (N + kTile - 1) / kTile;
    for (long long t = g; t < ntiles; t += G) {
        asm volatile("" ::: "memory");        // the LDS query reads stay inside the loop (hoisted, they would fill the register file)
        const long long row0 = t * kTile + wave * 4 * R + grp * R;
        float x[R][32], acc[R][CP];
        load_rows<T, R>(X, ldx, N, row0, j, x);
        dots<CP, R>(x, W, j, acc);
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const float v = reduce16<CP>(acc[r], j);
            if (row0 + r < N && v > best) {      // rows ascend within a lane: the first of equal scores stays
                best = v;
                bidx = (int)(row0 + r);
            }
        }
    }
    if (j % kRep == 0) {
        rv[wave * 4 + grp][j / kRep] = best;
        ri[wave * 4 + grp][j / kRep] = bidx;
    }
    __syncthreads();
    if (threadIdx.x < CP) {
        float v = rv[0][threadIdx.x];
        int i = ri[0][threadIdx.x];
        for (int s = 1; s < 16; ++s) {
            const float v2 = rv[s][threadIdx.x];
            const int i2 = ri[s][threadIdx.x];
            if (v2 > v || (v2 == v && i2 < i)) {
                v = v2;
                i = i2;
            }
        }
        pmax[(size_t)blockIdx.x * kMaxC + threadIdx.x] = v;
        pidx[(size_t)blockIdx.x * kMaxC + threadIdx.x] = i;
    }
}

// ---- critical rows: one block per (bag, class) -----------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(kThreads) void k_dsmil_critical(const vlsa_bag_desc* bags, int C, const int* part_start, const float* pmax,
                                                             const int* pidx, const float* bc, const float* Wq, const float* bq,
                                                             int* crit, float* cmax, float* xcrit, float* qmax, float* u) {
    __shared__ float sv[kThreads];
    __shared__ int si[kThreads];
    __shared__ float xs[kD];
    __shared__ float qs[kH];
    const int b = blockIdx.x / C, k = blockIdx.x % C, t = threadIdx.x;
    const int p0 = part_start[b], G = part_start[b + 1] - p0;
    float v = -INFINITY;
    int idx = 0x7fffffff;
    for (int i = t; i < G; i += kThreads) {
        const float v2 = pmax[(size_t)(p0 + i) * kMaxC + k];
        const int i2 = pidx[(size_t)(p0 + i) * kMaxC + k];
        if (v2 > v || (v2 == v && i2 < idx)) {
            v = v2;
            idx = i2;
        }
    }
    sv[t] = v;
    si[t] = idx;
    __syncthreads();
    for (int s = kThreads / 2; s > 0; s >>= 1) {
        if (t < s) {
            const float v2 = sv[t + s];
            const int i2 = si[t + s];
            if (v2 > sv[t] || (v2 == sv[t] && i2 < si[t])) {
                sv[t] = v2;
                si[t] = i2;
            }
        }
        __syncthreads();
    }
    const long long N = bags[b].N;
    long long m = si[0];
    const bool have = N > 0 && m >= 0 && m < N;          // (an empty bag, or scores that are all NaN: zero rows, nothing read)
    if (!have) m = 0;
    if (t == 0) {
        crit[b * kMaxC + k] = (int)m;
        cmax[b * kMaxC + k] = have ? sv[0] + bc[k] : 0.f;
    }
    const T* row = static_cast<const T*>(bags[b].X) + m * bags[b].ldx;
    const size_t o512 = ((size_t)b * C + k) * kD, o256 = ((size_t)b * C + k) * kH;
    for (int f = t; f < kD; f += kThreads) {
        const float xv = have ? load_as_float(row + f) : 0.f;
        xs[f] = xv;
        xcrit[o512 + f] = xv;
    }
    __syncthreads();
    const int lane = t & 63, wave = t >> 6;
    float xr[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) xr[e] = xs[lane * 8 + e];
    for (int h = wave * 64; h < wave * 64 + 64; ++h) {
        float w[8];
        load8(Wq + (size_t)h * kD + lane * 8, w);
        float a = 0.f;
#pragma unroll
        for (int e = 0; e < 8; ++e) a = fmaf(w[e], xr[e], a);
        a = wave_sum(a) + bq[h];
        if (lane == 0) {
            qs[h] = a;
            qmax[o256 + h] = a;
        }
    }
    __syncthreads();
    for (int d = t; d < kD; d += kThreads) {
        float a = 0.f;
        for (int h = 0; h < kH; ++h) a = fmaf(Wq[(size_t)h * kD + d], qs[h], a);
        u[o512 + d] = a * kInvSqrtH;
    }
}

// ---- the streaming kernels that keep a 32-row tile in LDS -------------------------------------------------------------------------
template <typename T> struct TileRow { static constexpr int kLd = kD + 16 / (int)sizeof(T); };     // 16 bytes of padding per row

template <typename T, int CP, bool BWD>
constexpr int tile_lds_bytes() {
    return (BWD ? 2 : 1) * CP * kD * 4 + kTileB * TileRow<T>::kLd * (int)sizeof(T) + kTileB * CP * 4 + 4 * kMaxC * 4;
}

// acc[c][e] += sum over this thread's 16 rows of S[r][c] * x[r][ft * 4 + e]; DROP: x masked with the bag's dropout bits
template <typename T, int CP, bool DROP>
__device__ __forceinline__ void weighted_rows(const T* xt, const float* S, int half, int ft, long long tile_row0, unsigned int seed,
                                              unsigned int thr, float keep_scale, float (&acc)[CP][4]) {
    constexpr int ld = TileRow<T>::kLd;
    for (int r = half * 16; r < half * 16 + 16; ++r) {
        float xv[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) xv[e] = (float)xt[r * ld + ft * 4 + e];
        if (DROP) {
            const unsigned int row = (unsigned int)(tile_row0 + r);
#pragma unroll
            for (int e = 0; e < 4; ++e) xv[e] = dropout_bits(seed, row, (unsigned int)(ft * 4 + e)) >= thr ? xv[e] * keep_scale : 0.f;
        }
#pragma unroll
        for (int c = 0; c < CP; ++c) {
            const float p = S[r * CP + c];
#pragma unroll
            for (int e = 0; e < 4; ++e) acc[c][e] = fmaf(p, xv[e], acc[c][e]);
        }
    }
}

// the two row halves of the block summed and written: out[c][512] for c < C
template <int CP>
__device__ __forceinline__ void write_weighted(float* scratch, const float (&acc)[CP][4], int half, int ft, int C, float* out) {
    __syncthreads();
    if (half == 1) {
#pragma unroll
        for (int c = 0; c < CP; ++c)
#pragma unroll
            for (int e = 0; e < 4; ++e) scratch[c * kD + ft * 4 + e] = acc[c][e];
    }
    __syncthreads();
    if (half == 0) {
#pragma unroll
        for (int c = 0; c < CP; ++c)
            if (c < C) {
                float4 o;
                o.x = acc[c][0] + scratch[c * kD + ft * 4 + 0];
                o.y = acc[c][1] + scratch[c * kD + ft * 4 + 1];
                o.z = acc[c][2] + scratch[c * kD + ft * 4 + 2];
                o.w = acc[c][3] + scratch[c * kD + ft * 4 + 3];
                *reinterpret_cast<float4*>(out + c * kD + ft * 4) = o;
            }
    }
}

// pass 2: per part (m, l, sum_n exp2(s - m) drop(x_n)) with the C rows of u as queries
template <typename T, int CP, bool DROP>
__global__ __launch_bounds__(kThreads) void k_dsmil_aggregate(const vlsa_bag_desc* bags, int B, int C, const int* part_start, const float* u,
                                                              unsigned int drop_thr, float drop_scale, const long long* seed_word,
                                                              float* pm, float* pl, float* pacc) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    constexpr int ld = TileRow<T>::kLd;
    float* U = reinterpret_cast<float*>(lds);
    T* xt = reinterpret_cast<T*>(U + CP * kD);
    float* S = reinterpret_cast<float*>(xt + kTileB * ld);
    float* Mrun = S + kTileB * CP;
    float* Scale = Mrun + kMaxC;
    const BagSpan part = bag_span(part_start, B, blockIdx.x);
    const int b = part.b, g = part.idx, G = part.count;
    fill_queries(U, u + (size_t)b * C * kD, C, CP, kLog2e);
    if (threadIdx.x < kMaxC) Mrun[threadIdx.x] = -INFINITY;
    __syncthreads();
    const T* X = static_cast<const T*>(bags[b].X);
    const long long N = bags[b].N, ldx = bags[b].ldx;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, grp = lane >> 4, j = lane & 15;
    const int half = threadIdx.x >> 7, ft = threadIdx.x & 127;
    constexpr int kRep = 16 / CP;
    unsigned int seed = 0, thr = 0;
    float keep_scale = 1.f;
    if (DROP) {
        seed = bag_drop_seed((unsigned int)(*seed_word), b);
        thr = drop_thr;           // (drop_spec, launch.h: the backward recomputes the forward's mask from the same two numbers)
        keep_scale = drop_scale;
    }
    float acc[CP][4];
#pragma unroll
    for (int c = 0; c < CP; ++c)
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[c][e] = 0.f;
    float lrun = 0.f;
    const long long ntiles = (N + kTileB - 1) / kTileB;
    for (long long t = g; t < ntiles; t += G) {
        const int rl = wave * 8 + grp * 2;
        const long long row0 = t * kTileB + rl;
        {
            float x[2][32], sc[2][CP];
            load_rows<T, 2>(X, ldx, N, row0, j, x);
#pragma unroll
            for (int r = 0; r < 2; ++r)
#pragma unroll
                for (int k = 0; k < 4; ++k) store8(xt + (rl + r) * ld + (k * 16 + j) * 8, &x[r][k * 8]);
            dots<CP, 2>(x, U, j, sc);
#pragma unroll
            for (int r = 0; r < 2; ++r) {
                const float v = reduce16<CP>(sc[r], j);
                if (j % kRep == 0) S[(rl + r) * CP + j / kRep] = (row0 + r < N) ? v : -INFINITY;
            }
        }
        __syncthreads();
        if (wave == 0) {                       // running maximum per class and the factor the sums kept so far shrink by
            const int c = lane % CP;
            float mx = -INFINITY;
            for (int r = lane / CP; r < kTileB; r += 64 / CP) mx = fmaxf(mx, S[r * CP + c]);
#pragma unroll
            for (int o = CP; o < 64; o <<= 1) mx = fmaxf(mx, __shfl_xor(mx, o));
            if (lane < CP) {
                const float m_old = Mrun[lane], m_new = fmaxf(m_old, mx);
                Scale[lane] = (m_old == -INFINITY) ? 0.f : fast_exp2(m_old - m_new);
                Mrun[lane] = m_new;
            }
        }
        __syncthreads();
        for (int i = threadIdx.x; i < kTileB * CP; i += kThreads) S[i] = fast_exp2(S[i] - Mrun[i % CP]);
        __syncthreads();
#pragma unroll
        for (int c = 0; c < CP; ++c) {
            const float s = Scale[c];
#pragma unroll
            for (int e = 0; e < 4; ++e) acc[c][e] *= s;
        }
        weighted_rows<T, CP, DROP>(xt, S, half, ft, t * kTileB, seed, thr, keep_scale, acc);
        if (threadIdx.x < CP) {
            float sum = 0.f;
            for (int r = 0; r < kTileB; ++r) sum += S[r * CP + threadIdx.x];
            lrun = lrun * Scale[threadIdx.x] + sum;
        }
        __syncthreads();
    }
    if (threadIdx.x < kMaxC) {
        pm[(size_t)blockIdx.x * kMaxC + threadIdx.x] = threadIdx.x < CP ? Mrun[threadIdx.x] : -INFINITY;
        pl[(size_t)blockIdx.x * kMaxC + threadIdx.x] = threadIdx.x < CP ? lrun : 0.f;
    }
    write_weighted<CP>(U, acc, half, ft, C, pacc + (size_t)blockIdx.x * C * kD);
}

// ---- head: merge the parts, B = Wv z + bv, fcc, + cmax, * 0.5: one block per bag -------------------------------------------------------
__global__ __launch_bounds__(kThreads) void k_dsmil_head(int C, const int* part_start, const float* pm, const float* pl,
                                                         const float* pacc, const float* Wv, const float* bv, const float* Wf,
                                                         const float* bf, const float* cmax, float* m2, float* l, float* z, float* bm,
                                                         float* logits) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    float* zs = reinterpret_cast<float*>(lds);          // [C][512]
    float* bs = zs + C * kD;                            // [C][256]
    float* red = bs + C * kH;                           // [4]
    const int b = blockIdx.x, t = threadIdx.x;
    const int p0 = part_start[b], G = part_start[b + 1] - p0;
    for (int c = 0; c < C; ++c) {
        float M = -INFINITY;
        for (int g = 0; g < G; ++g) M = fmaxf(M, pm[(size_t)(p0 + g) * kMaxC + c]);
        float ls = 0.f, a0 = 0.f, a1 = 0.f;
        for (int g = 0; g < G; ++g) {
            const float pmg = pm[(size_t)(p0 + g) * kMaxC + c];
            const float w = (pmg == -INFINITY) ? 0.f : fast_exp2(pmg - M);
            ls = fmaf(w, pl[(size_t)(p0 + g) * kMaxC + c], ls);
            const float* pa = pacc + ((size_t)(p0 + g) * C + c) * kD;
            a0 = fmaf(w, pa[t], a0);
            a1 = fmaf(w, pa[t + kThreads], a1);
        }
        const float inv = ls > 0.f ? 1.f / ls : 0.f;
        zs[c * kD + t] = a0 * inv;
        zs[c * kD + t + kThreads] = a1 * inv;
        z[((size_t)b * C + c) * kD + t] = a0 * inv;
        z[((size_t)b * C + c) * kD + t + kThreads] = a1 * inv;
        if (t == 0) {
            m2[b * kMaxC + c] = M;
            l[b * kMaxC + c] = ls;
        }
    }
    __syncthreads();
    const int lane = t & 63, wave = t >> 6;
    for (int h = wave * 64; h < wave * 64 + 64; ++h) {
        float w[8];
        load8(Wv + (size_t)h * kD + lane * 8, w);
        const float bias = bv[h];
        for (int c = 0; c < C; ++c) {
            float a = 0.f;
#pragma unroll
            for (int e = 0; e < 8; ++e) a = fmaf(w[e], zs[c * kD + lane * 8 + e], a);
            a = wave_sum(a) + bias;
            if (lane == 0) {
                bs[c * kH + h] = a;
                bm[((size_t)b * C + c) * kH + h] = a;
            }
        }
    }
    __syncthreads();
    for (int k = 0; k < C; ++k) {
        float a = 0.f;
        for (int jc = 0; jc < C; ++jc) a = fmaf(Wf[((size_t)k * C + jc) * kH + t], bs[jc * kH + t], a);
        a = block_sum_256(a, red);
        if (t == 0) logits[b * C + k] = 0.5f * (a + bf[k] + cmax[b * kMaxC + k]);
    }
}

// ---- attention output: mean_k A[n,k], recomputed from the kept (m, l) --------------------------------------------------------------
template <typename T, int CP>
__global__ __launch_bounds__(kThreads) void k_dsmil_attn(const vlsa_bag_desc* bags, int B, int C, const int* part_start, const float* u,
                                                         const float* m2, const float* l, float* attn, const long long* a_off) {
    __shared__ float U[CP * kD];
    const BagSpan part = bag_span(part_start, B, blockIdx.x);
    const int b = part.b, g = part.idx, G = part.count;
    fill_queries(U, u + (size_t)b * C * kD, C, CP, kLog2e);
    __syncthreads();
    const T* X = static_cast<const T*>(bags[b].X);
    const long long N = bags[b].N, ldx = bags[b].ldx;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, grp = lane >> 4, j = lane & 15;
    constexpr int kRep = 16 / CP;
    const int cls = j / kRep;
    const float mc = cls < C ? m2[b * kMaxC + cls] : 0.f;
    const float wc = cls < C ? 1.f / (l[b * kMaxC + cls] * (float)(kRep * C)) : 0.f;
    float* out = attn + a_off[b];
    constexpr int R = rows_per_group(CP), kTile = 16 * R;
    const long long ntiles = (N + kTile - 1) / kTile;
    for (long long t = g; t < ntiles; t += G) {
        asm volatile("" ::: "memory");        // the LDS query reads stay inside the loop (hoisted, they would fill the register file)
        const long long row0 = t * kTile + wave * 4 * R + grp * R;
        float x[R][32], acc[R][CP];
        load_rows<T, R>(X, ldx, N, row0, j, x);
        dots<CP, R>(x, U, j, acc);
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const float s = reduce16<CP>(acc[r], j);
            float p = cls < C ? fast_exp2(s - mc) * wc : 0.f;
#pragma unroll
            for (int o = 8; o > 0; o >>= 1) p += __shfl_xor(p, o);
            if (j == 0 && row0 + r < N) out[row0 + r] = p;
        }
    }
}

// ---- backward -------------------------------------------------------------------------------------------------------------------
// one block per (bag, class j): dB_j = 0.5 sum_k g_k Wf[k][j], dz_j = Wv^T dB_j, z_j . dz_j
__global__ __launch_bounds__(kThreads) void k_dsmil_bwd_prep(int C, const float* Wv, const float* Wf, const float* dlogits,
                                                             const float* z, float* dB, float* dz, float* zdz) {
    __shared__ float dbs[kH];
    __shared__ float red[4];
    const int b = blockIdx.x / C, jc = blockIdx.x % C, t = threadIdx.x;
    const size_t o512 = ((size_t)b * C + jc) * kD, o256 = ((size_t)b * C + jc) * kH;
    float a = 0.f;
    for (int k = 0; k < C; ++k) a = fmaf(dlogits[b * C + k], Wf[((size_t)k * C + jc) * kH + t], a);
    a *= 0.5f;
    dbs[t] = a;
    dB[o256 + t] = a;
    __syncthreads();
    float dot = 0.f;
    for (int d = t; d < kD; d += kThreads) {
        float s = 0.f;
        for (int h = 0; h < kH; ++h) s = fmaf(Wv[(size_t)h * kD + d], dbs[h], s);
        dz[o512 + d] = s;
        dot = fmaf(s, z[o512 + d], dot);
    }
    dot = block_sum_256(dot, red);
    if (t == 0) zdz[b * kMaxC + jc] = dot;
}

// the streaming pass of the backward: per part sum_n ds[n,j] x_n with ds[n,j] = A[n,j] (drop(x_n) . dz_j - z_j . dz_j)
template <typename T, int CP, bool DROP>
__global__ __launch_bounds__(kThreads) void k_dsmil_bwd_stream(const vlsa_bag_desc* bags, int B, int C, const int* part_start, const float* u,
                                                               const float* dz, const float* zdz, const float* m2, const float* l,
                                                               unsigned int drop_thr, float drop_scale, const long long* seed_word,
                                                               float* pdu) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    constexpr int ld = TileRow<T>::kLd;
    float* U = reinterpret_cast<float*>(lds);
    float* DZ = U + CP * kD;
    T* xt = reinterpret_cast<T*>(DZ + CP * kD);
    float* S = reinterpret_cast<float*>(xt + kTileB * ld);
    const BagSpan part = bag_span(part_start, B, blockIdx.x);
    const int b = part.b, g = part.idx, G = part.count;
    fill_queries(U, u + (size_t)b * C * kD, C, CP, kLog2e);
    fill_queries(DZ, dz + (size_t)b * C * kD, C, CP, 1.f);
    __syncthreads();
    const T* X = static_cast<const T*>(bags[b].X);
    const long long N = bags[b].N, ldx = bags[b].ldx;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, grp = lane >> 4, j = lane & 15;
    const int half = threadIdx.x >> 7, ft = threadIdx.x & 127;
    constexpr int kRep = 16 / CP;
    const int cls = j / kRep;
    const bool live = cls < C;
    const float mc = live ? m2[b * kMaxC + cls] : 0.f;
    const float il = live ? 1.f / l[b * kMaxC + cls] : 0.f;
    const float zd = live ? zdz[b * kMaxC + cls] : 0.f;
    unsigned int seed = 0, thr = 0;
    float keep_scale = 1.f;
    if (DROP) {
        seed = bag_drop_seed((unsigned int)(*seed_word), b);
        thr = drop_thr;           // (drop_spec, launch.h: the backward recomputes the forward's mask from the same two numbers)
        keep_scale = drop_scale;
    }
    float acc[CP][4];
#pragma unroll
    for (int c = 0; c < CP; ++c)
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[c][e] = 0.f;
    const long long ntiles = (N + kTileB - 1) / kTileB;
    for (long long t = g; t < ntiles; t += G) {
        const int rl = wave * 8 + grp * 2;
        const long long row0 = t * kTileB + rl;
        {
            float x[2][32], sc[2][CP], td[2][CP];
            load_rows<T, 2>(X, ldx, N, row0, j, x);
#pragma unroll
            for (int r = 0; r < 2; ++r)
#pragma unroll
                for (int k = 0; k < 4; ++k) store8(xt + (rl + r) * ld + (k * 16 + j) * 8, &x[r][k * 8]);
            dots<CP, 2>(x, U, j, sc);
            if (DROP) {
#pragma unroll
                for (int r = 0; r < 2; ++r)
#pragma unroll
                    for (int k = 0; k < 4; ++k)
#pragma unroll
                        for (int e = 0; e < 8; ++e)
                            x[r][k * 8 + e] = dropout_bits(seed, (unsigned int)(row0 + r), (unsigned int)((k * 16 + j) * 8 + e)) >= thr
                                                  ? x[r][k * 8 + e] * keep_scale : 0.f;
            }
            dots<CP, 2>(x, DZ, j, td);
#pragma unroll
            for (int r = 0; r < 2; ++r) {
                const float s = reduce16<CP>(sc[r], j), tq = reduce16<CP>(td[r], j);
                const float ds = (live && row0 + r < N) ? fast_exp2(s - mc) * il * (tq - zd) : 0.f;
                if (j % kRep == 0) S[(rl + r) * CP + cls] = ds;
            }
        }
        __syncthreads();
        weighted_rows<T, CP, false>(xt, S, half, ft, t * kTileB, 0u, 0u, 1.f, acc);
        __syncthreads();
    }
    write_weighted<CP>(U, acc, half, ft, C, pdu + (size_t)blockIdx.x * C * kD);
}

// one block per (bag, class j): du_j = sum over the parts, dqmax_j = Wq du_j / sqrt(H)
__global__ __launch_bounds__(kThreads) void k_dsmil_bwd_merge(int C, const int* part_start, const float* pdu, const float* Wq,
                                                              float* du, float* dqm) {
    __shared__ float ds[kD];
    const int b = blockIdx.x / C, jc = blockIdx.x % C, t = threadIdx.x;
    const int p0 = part_start[b], G = part_start[b + 1] - p0;
    const size_t o512 = ((size_t)b * C + jc) * kD, o256 = ((size_t)b * C + jc) * kH;
    float a0 = 0.f, a1 = 0.f;
    for (int g = 0; g < G; ++g) {
        const float* p = pdu + ((size_t)(p0 + g) * C + jc) * kD;
        a0 += p[t];
        a1 += p[t + kThreads];
    }
    ds[t] = a0;
    ds[t + kThreads] = a1;
    du[o512 + t] = a0;
    du[o512 + t + kThreads] = a1;
    __syncthreads();
    const int lane = t & 63, wave = t >> 6;
    float dr[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) dr[e] = ds[lane * 8 + e];
    for (int h = wave * 64; h < wave * 64 + 64; ++h) {
        float w[8];
        load8(Wq + (size_t)h * kD + lane * 8, w);
        float a = 0.f;
#pragma unroll
        for (int e = 0; e < 8; ++e) a = fmaf(w[e], dr[e], a);
        a = wave_sum(a);
        if (lane == 0) dqm[o256 + h] = a * kInvSqrtH;
    }
}

// the parameter gradients, summed over the bags in bag order.  Blocks 0..511: 256 entries each of dWq and dWv; block 512: dbq, dbv;
// blocks 513 + k: row k of dWc, dbc[k], dbf[k], dWf[k].
__global__ __launch_bounds__(kThreads) void k_dsmil_bwd_params(int B, int C, const float* dlogits, const float* xcrit,
                                                               const float* qmax, const float* z, const float* bm, const float* dB,
                                                               const float* du, const float* dqm, float* dWc, float* dbc, float* dWq,
                                                               float* dbq, float* dWv, float* dbv, float* dWf, float* dbf) {
    const int t = threadIdx.x, blk = blockIdx.x, rows = B * C;
    if (blk < 512) {
        const int h = blk >> 1, d = (blk & 1) * kThreads + t;
        float aq = 0.f, av = 0.f;
        for (int r = 0; r < rows; ++r) {
            const size_t o512 = (size_t)r * kD + d, o256 = (size_t)r * kH + h;
            aq = fmaf(qmax[o256] * kInvSqrtH, du[o512], aq);
            aq = fmaf(dqm[o256], xcrit[o512], aq);
            av = fmaf(dB[o256], z[o512], av);
        }
        dWq[(size_t)h * kD + d] = aq;
        dWv[(size_t)h * kD + d] = av;
    } else if (blk == 512) {
        float aq = 0.f, av = 0.f;
        for (int r = 0; r < rows; ++r) {
            aq += dqm[(size_t)r * kH + t];
            av += dB[(size_t)r * kH + t];
        }
        dbq[t] = aq;
        dbv[t] = av;
    } else {
        const int k = blk - 513;
        float a0 = 0.f, a1 = 0.f, gs = 0.f;
        for (int b = 0; b < B; ++b) {
            const float gk = 0.5f * dlogits[b * C + k];
            const float* xr = xcrit + ((size_t)b * C + k) * kD;
            a0 = fmaf(gk, xr[t], a0);
            a1 = fmaf(gk, xr[t + kThreads], a1);
            gs += gk;
        }
        dWc[(size_t)k * kD + t] = a0;
        dWc[(size_t)k * kD + t + kThreads] = a1;
        if (t == 0) {
            dbc[k] = gs;
            dbf[k] = gs;
        }
        for (int jc = 0; jc < C; ++jc) {
            float a = 0.f;
            for (int b = 0; b < B; ++b) a = fmaf(0.5f * dlogits[b * C + k], bm[((size_t)b * C + jc) * kH + t], a);
            dWf[((size_t)k * C + jc) * kH + t] = a;
        }
    }
}

// ---- host side -------------------------------------------------------------------------------------------------------------------
struct StateLayout {
    size_t crit, cmax, m2, l, xcrit, qmax, u, z, bm, total;
    StateLayout(int B, int C) {
        crit = 0;
        cmax = crit + (size_t)B * kMaxC;
        m2 = cmax + (size_t)B * kMaxC;
        l = m2 + (size_t)B * kMaxC;
        xcrit = l + (size_t)B * kMaxC;
        qmax = xcrit + (size_t)B * C * kD;
        u = qmax + (size_t)B * C * kH;
        z = u + (size_t)B * C * kD;
        bm = z + (size_t)B * C * kD;
        total = bm + (size_t)B * C * kH;
    }
};

struct WsLayout {      // in floats
    size_t pmax, pidx, pm, pl, pacc, dB, dz, zdz, du, dqm, total;
    WsLayout(int n_parts, int C) {
        const size_t np = (size_t)n_parts, bc = (size_t)64 * C;
        pmax = 0;
        pidx = pmax + np * kMaxC;
        pm = pidx + np * kMaxC;
        pl = pm + np * kMaxC;
        pacc = pl + np * kMaxC;           // the backward's per-part du records share it
        dB = pacc + np * C * kD;
        dz = dB + bc * kH;
        zdz = dz + bc * kD;
        du = zdz + (size_t)64 * kMaxC;
        dqm = du + bc * kD;
        total = dqm + bc * kH;
    }
};

int check_common(const void* bag_desc, int B, int x_dtype, int D, int H, int C, const int* part_start, int n_parts, float drop_p,
                 const int64_t* seed_word, DropSpec* drop) {
    if (!bag_table_ok(bag_desc, B, part_start, n_parts) || C < 1 || !(drop_p >= 0.f) || !drop_spec(drop_p, drop)) return VLSA_EINVAL;
    if (drop_p > 0.f && !seed_word) return VLSA_EINVAL;
    if (D != kD || H != kH || C > kMaxC || (x_dtype != VLSA_DT_F32 && x_dtype != VLSA_DT_BF16)) return VLSA_EUNSUPPORTED;
    return VLSA_OK;
}

// launch KERNEL<T, CP, ...> for the row type and the class count padded to 4 / 8 / 16
#define DSMIL_BY_CP(MACRO)        \
    if (C <= 4) MACRO(4);         \
    else if (C <= 8) MACRO(8);    \
    else MACRO(16)

}  // namespace

extern "C" int vlsa_dsmil_part_rows(void) { return kPartRows; }

extern "C" int vlsa_dsmil_parts(int64_t N) {
    const int64_t g = (N + kPartRows - 1) / kPartRows;
    return (int)(g < 1 ? 1 : (g > kMaxParts ? kMaxParts : g));
}

extern "C" size_t vlsa_dsmil_workspace_bytes(int n_parts, int C) {
    if (n_parts < 1 || C < 1 || C > kMaxC) return 0;
    return WsLayout(n_parts, C).total * sizeof(float);
}

extern "C" size_t vlsa_dsmil_state_floats(int B, int C, int64_t* offsets9) {
    if (B < 1 || C < 1 || C > kMaxC) return 0;
    const StateLayout s(B, C);
    if (offsets9) {
        const size_t o[9] = {s.crit, s.cmax, s.m2, s.l, s.xcrit, s.qmax, s.u, s.z, s.bm};
        for (int i = 0; i < 9; ++i) offsets9[i] = (int64_t)o[i];
    }
    return s.total;
}

extern "C" int vlsa_dsmil_forward_batch(const void* bag_desc, int B, int x_dtype, int D, int H, int C, const int* part_start,
                                        int n_parts, const float* Wc, const float* bc, const float* Wq, const float* bq,
                                        const float* Wv, const float* bv, const float* Wf, const float* bf, float drop_p,
                                        const int64_t* seed_word, void* ws, float* state, float* logits, float* attn,
                                        const int64_t* a_off, void* stream) {
    DropSpec ds;
    const int rc = check_common(bag_desc, B, x_dtype, D, H, C, part_start, n_parts, drop_p, seed_word, &ds);
    if (rc != VLSA_OK) return rc;
    if (!Wc || !bc || !Wq || !bq || !Wv || !bv || !Wf || !bf || !ws || !state || !logits || (attn && !a_off)) return VLSA_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    const vlsa_bag_desc* bags = static_cast<const vlsa_bag_desc*>(bag_desc);
    const WsLayout w(n_parts, C);
    const StateLayout s(B, C);
    float* wsf = static_cast<float*>(ws);
    float *pmax = wsf + w.pmax, *pm = wsf + w.pm, *pl = wsf + w.pl, *pacc = wsf + w.pacc;
    int* pidx = reinterpret_cast<int*>(wsf + w.pidx);
    int* crit = reinterpret_cast<int*>(state + s.crit);
    float *cmax = state + s.cmax, *m2 = state + s.m2, *l = state + s.l, *xcrit = state + s.xcrit, *qmax = state + s.qmax;
    float *u = state + s.u, *z = state + s.z, *bm = state + s.bm;
    const long long* seed = reinterpret_cast<const long long*>(seed_word);
    const long long* aoff = reinterpret_cast<const long long*>(a_off);
    const bool f32 = x_dtype == VLSA_DT_F32, drop = ds.thr != 0u;

#define DSMIL_SCORES(CP_)                                                                                                          \
    do {                                                                                                                           \
        if (f32) hipLaunchKernelGGL((k_dsmil_scores<float, CP_>), dim3(n_parts), dim3(kThreads), 0, st, bags, B, C, part_start, Wc, \
                                    pmax, pidx);                                                                                   \
        else hipLaunchKernelGGL((k_dsmil_scores<__bf16, CP_>), dim3(n_parts), dim3(kThreads), 0, st, bags, B, C, part_start, Wc,    \
                                pmax, pidx);                                                                                       \
    } while (0)
    DSMIL_BY_CP(DSMIL_SCORES);
#undef DSMIL_SCORES
    if (f32) hipLaunchKernelGGL(k_dsmil_critical<float>, dim3(B * C), dim3(kThreads), 0, st, bags, C, part_start, pmax, pidx, bc, Wq, bq,
                                crit, cmax, xcrit, qmax, u);
    else hipLaunchKernelGGL(k_dsmil_critical<__bf16>, dim3(B * C), dim3(kThreads), 0, st, bags, C, part_start, pmax, pidx, bc, Wq, bq,
                            crit, cmax, xcrit, qmax, u);

#define DSMIL_AGG_ONE(T_, CP_, DROP_)                                                                                              \
    do {                                                                                                                           \
        launch_lds<k_dsmil_aggregate<T_, CP_, DROP_>>(dim3(n_parts), dim3(kThreads), tile_lds_bytes<T_, CP_, false>(), st, bags, B, C, \
                                                      part_start, u, ds.thr, ds.scale, seed, pm, pl, pacc);                        \
    } while (0)
#define DSMIL_AGG(CP_)                                  \
    do {                                                \
        if (f32 && drop) DSMIL_AGG_ONE(float, CP_, true);        \
        else if (f32) DSMIL_AGG_ONE(float, CP_, false);          \
        else if (drop) DSMIL_AGG_ONE(__bf16, CP_, true);         \
        else DSMIL_AGG_ONE(__bf16, CP_, false);                  \
    } while (0)
    DSMIL_BY_CP(DSMIL_AGG);
#undef DSMIL_AGG
#undef DSMIL_AGG_ONE

    hipLaunchKernelGGL(k_dsmil_head, dim3(B), dim3(kThreads), (size_t)(C * (kD + kH) + 4) * sizeof(float), st, C, part_start, pm, pl,
                       pacc, Wv, bv, Wf, bf, cmax, m2, l, z, bm, logits);
    if (attn) {
#define DSMIL_ATTN(CP_)                                                                                                            \
    do {                                                                                                                           \
        if (f32) hipLaunchKernelGGL((k_dsmil_attn<float, CP_>), dim3(n_parts), dim3(kThreads), 0, st, bags, B, C, part_start, u, m2, \
                                    l, attn, aoff);                                                                                \
        else hipLaunchKernelGGL((k_dsmil_attn<__bf16, CP_>), dim3(n_parts), dim3(kThreads), 0, st, bags, B, C, part_start, u, m2, l, \
                                attn, aoff);                                                                                       \
    } while (0)
        DSMIL_BY_CP(DSMIL_ATTN);
#undef DSMIL_ATTN
    }
    return launch_status();
}

extern "C" int vlsa_dsmil_backward_batch(const void* bag_desc, int B, int x_dtype, int D, int H, int C, const int* part_start,
                                         int n_parts, const float* Wq, const float* Wv, const float* Wf, const float* dlogits,
                                         float drop_p, const int64_t* seed_word, const float* state, void* ws, float* dWc, float* dbc,
                                         float* dWq, float* dbq, float* dWv, float* dbv, float* dWf, float* dbf, void* stream) {
    DropSpec ds;
    const int rc = check_common(bag_desc, B, x_dtype, D, H, C, part_start, n_parts, drop_p, seed_word, &ds);
    if (rc != VLSA_OK) return rc;
    if (!Wq || !Wv || !Wf || !dlogits || !state || !ws || !dWc || !dbc || !dWq || !dbq || !dWv || !dbv || !dWf || !dbf) return VLSA_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    const vlsa_bag_desc* bags = static_cast<const vlsa_bag_desc*>(bag_desc);
    const WsLayout w(n_parts, C);
    const StateLayout s(B, C);
    float* wsf = static_cast<float*>(ws);
    float *pdu = wsf + w.pacc, *dB = wsf + w.dB, *dz = wsf + w.dz, *zdz = wsf + w.zdz, *du = wsf + w.du, *dqm = wsf + w.dqm;
    const float *m2 = state + s.m2, *l = state + s.l, *xcrit = state + s.xcrit, *qmax = state + s.qmax, *u = state + s.u;
    const float *z = state + s.z, *bm = state + s.bm;
    const long long* seed = reinterpret_cast<const long long*>(seed_word);
    const bool f32 = x_dtype == VLSA_DT_F32, drop = ds.thr != 0u;

    hipLaunchKernelGGL(k_dsmil_bwd_prep, dim3(B * C), dim3(kThreads), 0, st, C, Wv, Wf, dlogits, z, dB, dz, zdz);
#define DSMIL_BWD_ONE(T_, CP_, DROP_)                                                                                              \
    do {                                                                                                                           \
        launch_lds<k_dsmil_bwd_stream<T_, CP_, DROP_>>(dim3(n_parts), dim3(kThreads), tile_lds_bytes<T_, CP_, true>(), st, bags, B, C, \
                                                       part_start, u, dz, zdz, m2, l, ds.thr, ds.scale, seed, pdu);                \
    } while (0)
#define DSMIL_BWD(CP_)                                  \
    do {                                                \
        if (f32 && drop) DSMIL_BWD_ONE(float, CP_, true);        \
        else if (f32) DSMIL_BWD_ONE(float, CP_, false);          \
        else if (drop) DSMIL_BWD_ONE(__bf16, CP_, true);         \
        else DSMIL_BWD_ONE(__bf16, CP_, false);                  \
    } while (0)
    DSMIL_BY_CP(DSMIL_BWD);
#undef DSMIL_BWD
#undef DSMIL_BWD_ONE
    hipLaunchKernelGGL(k_dsmil_bwd_merge, dim3(B * C), dim3(kThreads), 0, st, C, part_start, pdu, Wq, du, dqm);
    hipLaunchKernelGGL(k_dsmil_bwd_params, dim3(513 + C), dim3(kThreads), 0, st, B, C, dlogits, xcrit, qmax, z, bm, dB, du, dqm, dWc,
                       dbc, dWq, dbq, dWv, dbv, dWf, dbf);
    return launch_status();
}
