// ILRA (Xiang et al., ICLR 2023; model/deepmil.py:409-535) over a table of bags, forward and backward, gfx950.  With topk = 1 the model
// is two N-sized operations per block, everything else is [1, 256]-sized and stays on the host side of the ABI:
//   pooling   Z[b][p] = sum_n softmax_n(E[p] . x_n) x_n      P <= 16 effective queries E shared by all bags (no row norms, no scale)
//   row map   u = Wq x + b~[b],  t = Wo u + bo,  o = u + relu(t),  xhat = o * silu(Wg x + bg)          [N, D] -> [N, 256]
// Row sources: bag rows through the descriptor table (bf16 or fp32, D = 512), or the packed fp32 [sum N_b, 256] output of a previous
// row map (`xp`, D = 256; the table then supplies the bag sizes only).  bf16 rows are widened to fp32 when a tile is staged in LDS
// (exact); every product is the fp32-input MFMA (16x16x4: an exact fp32 FMA chain per output), so the ReLU decisions differ from
// float64 only within fp32 rounding of t.
//
// Everything is cut along tables that are functions of the bag sizes alone -- tiles of kTile rows that never straddle a bag, and
// vlsa_ilra_pool_parts(N) partial records per bag -- so a bag's result is bit-equal alone and in a batch.  All sums across workgroups
// go through partial records added in a fixed order: no float atomics, bit-reproducible run to run.
//
// Pooling forward: part g of G walks the tiles g, g + G, ... with an online softmax (running maximum, sum and Z[16][D] in registers;
// wave w owns the features w D/4 ..); the scores of a tile are a K-split over the four waves, added in wave order.  k_ip_merge folds a
// bag's parts in part order and keeps the maximum and the sum for the backward.
// Pooling backward: a_p(n) recomputed from the kept maximum and sum, c_p(n) = a_p(n) (g_p . x_n - g_p . z_p), both dot products through
// the same MFMA chain; dE = sum c x (partials per
// part, added in part order over all bags) and, for packed rows, dX_n = sum_p a_p(n) g_p + c_p(n) e_p.
// Row map forward: per tile u and the gate pre-activation share the staged rows; u goes through LDS for the 256 -> 256 product; the
// ReLU decisions t > 0 leave in the shared mask format (bag_table.h; DESIGN.md, "Table-driven kernels", also for the bag lookup).
// Row map backward: recomputes u, t and the gate from the rows, READS the mask, stages u, du, ds, dt ([sum N_b, 256] fp32 each) in the
// workspace, forms du = do + Wo^T dt (and dX = Wq^T du + Wg^T ds for packed rows) in the same kernel, then three [256, n] x [n, D]
// products (k_rm_wgrad: row splits in registers, partials added in split order) and the column sums per bag.
#include "bag_table.h"
#include "launch.h"

namespace {
using namespace vlsa;

constexpr int kH = 256, kThreads = 256, kMaxP = 16;
constexpr int kTile = 32;          // rows per tile of the row map and the weight-gradient products
constexpr int kPoolTile = 16;      // rows per tile of the pooling kernels
constexpr int kPoolRowsPerPart = 256, kMaxParts = 64;
constexpr int kChunk = 128;        // features per staged chunk of the row map
constexpr int kXld = kChunk + 4;   // floats per LDS row of a chunk
constexpr int kUld = kH + 4;       // floats per LDS row of a [32][256] tile read as an A operand
constexpr int kGld = kH + 16;      // ... read as a B operand (row stride = 16 banks)
constexpr int kWld = kChunk + 16;
constexpr int kSegs = 8;

// rows row0 .. row0 + rows - 1, features c0 .. c0 + CH - 1 as fp32 into xs (ld floats per row); rows past the bag's end are zeros
template <typename T>
__device__ __forceinline__ void stage_tile(float_ma* xs, int ld, const T* X, long long ldx, long long row0, long long N, int c0, int CH,
                                           int rows, int tid) {
    const int upr = CH / 4;
    for (int u = tid; u < rows * upr; u += kThreads) {
        const int r = u / upr, cu = u % upr;
        f32x4 v = f32x4{0.f, 0.f, 0.f, 0.f};
        if (row0 + r < N) {
            const T* p = X + (row0 + r) * ldx + c0 + 4 * cu;
            if constexpr (sizeof(T) == 2) {
                const uint2 q = *reinterpret_cast<const uint2*>(p);
                v[0] = __uint_as_float(q.x << 16);
                v[1] = __uint_as_float(q.x & 0xffff0000u);
                v[2] = __uint_as_float(q.y << 16);
                v[3] = __uint_as_float(q.y & 0xffff0000u);
            } else {
                v = *reinterpret_cast<const f32x4*>(p);
            }
        }
        *reinterpret_cast<f32x4_ma*>(xs + r * ld + 4 * cu) = v;
    }
}

// acc[rt][hg][e] (row 16 rt + 4 gq + e, unit 64 w + 16 hg + i16) += sum_k A[row][k] W[unit][k], k < K: A in LDS (lda floats per row), W in
// memory (ldw floats per row, the pointer already at the first of the K columns).  Blocks of 16 k as four K = 4 steps.
__device__ __forceinline__ void lin_acc(f32x4 (&acc)[2][4], const float_ma* A, int lda, const float* __restrict__ W, int ldw, int K, int w,
                                        int gq, int i16) {
#pragma unroll 2
    for (int kb = 0; kb < K / 16; ++kb) {
        f32x4 bw[4];
#pragma unroll
        for (int hg = 0; hg < 4; ++hg) bw[hg] = *reinterpret_cast<const f32x4*>(W + (size_t)(64 * w + 16 * hg + i16) * ldw + kb * 16 + 4 * gq);
#pragma unroll
        for (int rt = 0; rt < 2; ++rt) {
            const f32x4 a = *reinterpret_cast<const f32x4_ma*>(A + (rt * 16 + i16) * lda + kb * 16 + 4 * gq);
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int hg = 0; hg < 4; ++hg) acc[rt][hg] = mfma_f32(a[j], bw[hg][j], acc[rt][hg]);
        }
    }
}

__device__ __forceinline__ void tile_to_lds(float_ma* us, const f32x4 (&acc)[2][4], int w, int gq, int i16) {
#pragma unroll
    for (int rt = 0; rt < 2; ++rt)
#pragma unroll
        for (int hg = 0; hg < 4; ++hg)
#pragma unroll
            for (int e = 0; e < 4; ++e) us[(rt * 16 + 4 * gq + e) * kUld + 64 * w + 16 * hg + i16] = acc[rt][hg][e];
}

struct RowSrc {
    const void* X;
    long long N, ldx, roff;
};
template <int D>
__device__ __forceinline__ RowSrc row_src(const vlsa_bag_desc* bags, const long long* row_off, const void* xp, int b) {
    RowSrc s;
    s.N = bags[b].N;
    s.roff = row_off[b];
    if (xp != nullptr) {
        s.X = static_cast<const float*>(xp) + s.roff * D;
        s.ldx = D;
    } else {
        s.X = bags[b].X;
        s.ldx = bags[b].ldx;
    }
    return s;
}

// ---- pooling -----------------------------------------------------------------------------------------------------------------------
// partial scores of the staged tile against Q (rows p < P of a [P][D] matrix), this wave's quarter of the features:
// sp[(w * 16 + row) * 16 + p]
template <int D>
__device__ __forceinline__ void tile_scores(float_ma* sp, const float_ma* xs, const float* __restrict__ Q, int P, int w, int gq, int i16) {
    constexpr int kLd = D + 4, kQ = D / 4;
    f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll 4
    for (int kb = 0; kb < kQ / 16; ++kb) {
        const int k0 = w * kQ + kb * 16 + 4 * gq;
        const f32x4 a = *reinterpret_cast<const f32x4_ma*>(xs + i16 * kLd + k0);
        f32x4 q = f32x4{0.f, 0.f, 0.f, 0.f};
        if (i16 < P) q = *reinterpret_cast<const f32x4*>(Q + (size_t)i16 * D + k0);
#pragma unroll
        for (int j = 0; j < 4; ++j) acc = mfma_f32(a[j], q[j], acc);
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) sp[(w * 16 + 4 * gq + e) * 16 + i16] = acc[e];
}
__device__ __forceinline__ float score_of(const float_ma* sp, int row, int p) {
    return ((sp[(0 * 16 + row) * 16 + p] + sp[(1 * 16 + row) * 16 + p]) + sp[(2 * 16 + row) * 16 + p]) + sp[(3 * 16 + row) * 16 + p];
}

template <typename T, int D>
__global__ __launch_bounds__(kThreads) void k_ip_forward(const vlsa_bag_desc* __restrict__ bags, int B, int P, const int* __restrict__ part_start,
                                                         const long long* __restrict__ row_off, const void* __restrict__ xp,
                                                         const float* __restrict__ E, float* __restrict__ pm, float* __restrict__ pl,
                                                         float* __restrict__ pZ) {
    constexpr int kLd = D + 4, kFg = D / 64;
    __shared__ __attribute__((aligned(16))) float xs_[kPoolTile * kLd];
    __shared__ __attribute__((aligned(16))) float sp_[4 * 16 * 16];
    float_ma* xs = xs_;
    float_ma* sp = sp_;
    const BagSpan part = bag_span(part_start, B, blockIdx.x);
    const int b = part.b, g = part.idx, G = part.count;
    const RowSrc src = row_src<D>(bags, row_off, xp, b);
    const T* X = static_cast<const T*>(src.X);
    const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6), gq = lane >> 4, i16 = lane & 15;
    f32x4 z[kFg];
#pragma unroll
    for (int fg = 0; fg < kFg; ++fg) z[fg] = f32x4{0.f, 0.f, 0.f, 0.f};
    float m_run = -INFINITY, l_run = 0.f;          // of query i16
    const long long ntiles = (src.N + kPoolTile - 1) / kPoolTile;
    for (long long t = g; t < ntiles; t += G) {
        const long long row0 = t * kPoolTile;
        __syncthreads();                           // the previous tile's LDS reads are done
        stage_tile<T>(xs, kLd, X, src.ldx, row0, src.N, 0, D, kPoolTile, tid);
        __syncthreads();
        tile_scores<D>(sp, xs, E, P, w, gq, i16);
        __syncthreads();
        float s[16], m_new = m_run;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            s[r] = score_of(sp, r, i16);
            if (row0 + r < src.N) m_new = fmaxf(m_new, s[r]);
        }
        const float scale = expf(m_run - m_new);   // 0 on the first tile
        float lsum = 0.f, a4[4];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const float a = (row0 + r < src.N) ? expf(s[r] - m_new) : 0.f;
            lsum += a;
            if ((r & 3) == gq) a4[r >> 2] = a;     // row 4 step + gq
        }
        l_run = l_run * scale + lsum;
        m_run = m_new;
        float sc[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) sc[e] = __shfl(scale, 4 * gq + e);
#pragma unroll
        for (int fg = 0; fg < kFg; ++fg)
#pragma unroll
            for (int e = 0; e < 4; ++e) z[fg][e] *= sc[e];
#pragma unroll
        for (int step = 0; step < 4; ++step)
#pragma unroll
            for (int fg = 0; fg < kFg; ++fg)
                z[fg] = mfma_f32(a4[step], xs[(4 * step + gq) * kLd + w * (D / 4) + 16 * fg + i16], z[fg]);
    }
    // z[fg][e] = query 4 gq + e, feature w D/4 + 16 fg + i16
    if (tid < 16) {
        pm[(size_t)blockIdx.x * 16 + tid] = m_run;
        pl[(size_t)blockIdx.x * 16 + tid] = l_run;
    }
#pragma unroll
    for (int fg = 0; fg < kFg; ++fg)
#pragma unroll
        for (int e = 0; e < 4; ++e) pZ[((size_t)blockIdx.x * 16 + 4 * gq + e) * D + w * (D / 4) + 16 * fg + i16] = z[fg][e];
}

// grid (B, P): a bag's parts in part order
__global__ __launch_bounds__(kThreads) void k_ip_merge(int D, const int* __restrict__ part_start, const float* __restrict__ pm,
                                                       const float* __restrict__ pl, const float* __restrict__ pZ, int P, float* __restrict__ Z,
                                                       float* __restrict__ m, float* __restrict__ l) {
    const int b = blockIdx.x, p = blockIdx.y, t = threadIdx.x;
    const int p0 = part_start[b], G = part_start[b + 1] - p0;
    float M = -INFINITY;
    for (int g = 0; g < G; ++g) M = fmaxf(M, pm[(size_t)(p0 + g) * 16 + p]);
    float L = 0.f;
    for (int g = 0; g < G; ++g) L += pl[(size_t)(p0 + g) * 16 + p] * expf(pm[(size_t)(p0 + g) * 16 + p] - M);
    for (int f = t; f < D; f += kThreads) {
        float a = 0.f;
        for (int g = 0; g < G; ++g) a += pZ[((size_t)(p0 + g) * 16 + p) * D + f] * expf(pm[(size_t)(p0 + g) * 16 + p] - M);
        Z[((size_t)b * P + p) * D + f] = a / L;
    }
    if (t == 0) {
        m[b * 16 + p] = M;
        l[b * 16 + p] = L;
    }
}

template <typename T, int D, bool DX>
__global__ __launch_bounds__(kThreads) void k_ip_backward(const vlsa_bag_desc* __restrict__ bags, int B, int P, const int* __restrict__ part_start,
                                                          const long long* __restrict__ row_off, const void* __restrict__ xp,
                                                          const float* __restrict__ E, const float* __restrict__ dZ, const float* __restrict__ Z,
                                                          const float* __restrict__ m, const float* __restrict__ l, float* __restrict__ pdE,
                                                          float* __restrict__ dX) {
    constexpr int kLd = D + 4, kFg = D / 64;
    __shared__ __attribute__((aligned(16))) float xs_[kPoolTile * kLd];
    __shared__ __attribute__((aligned(16))) float sp_[4 * 16 * 16];
    __shared__ __attribute__((aligned(16))) float gp_[4 * 16 * 16];
    __shared__ __attribute__((aligned(16))) float at_[16 * 20];
    __shared__ __attribute__((aligned(16))) float ct_[16 * 20];
    float_ma* xs = xs_;
    float_ma* sp = sp_;
    float_ma* gp = gp_;
    float_ma* at = at_;
    float_ma* ct = ct_;
    const BagSpan part = bag_span(part_start, B, blockIdx.x);
    const int b = part.b, g = part.idx, G = part.count;
    const RowSrc src = row_src<D>(bags, row_off, xp, b);
    const T* X = static_cast<const T*>(src.X);
    const float* Gb = dZ + (size_t)b * P * D;
    const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6), gq = lane >> 4, i16 = lane & 15;
    const bool pv = i16 < P;
    const float mp = pv ? m[b * 16 + i16] : 0.f, rl = pv ? 1.f / l[b * 16 + i16] : 0.f;
    // g_p . z_p through the SAME chain as g_p . x_n (z as a tile of P rows): where the softmax is one-hot -- a bag of one row -- z is that
    // row bit for bit and g . x - g . z an exact zero, as the reference's autograd gives; a dot product formed elsewhere leaves its
    // rounding difference (1e-7 of sum |g_i x_i|) in dE
    stage_tile<float>(xs, kLd, Z + (size_t)b * P * D, D, 0, P, 0, D, kPoolTile, tid);
    __syncthreads();
    tile_scores<D>(gp, xs, Gb, P, w, gq, i16);
    __syncthreads();
    const float gzp = pv ? score_of(gp, i16, i16) : 0.f;
    f32x4 de[kFg];
#pragma unroll
    for (int fg = 0; fg < kFg; ++fg) de[fg] = f32x4{0.f, 0.f, 0.f, 0.f};
    const long long ntiles = (src.N + kPoolTile - 1) / kPoolTile;
    for (long long t = g; t < ntiles; t += G) {
        const long long row0 = t * kPoolTile;
        __syncthreads();
        stage_tile<T>(xs, kLd, X, src.ldx, row0, src.N, 0, D, kPoolTile, tid);
        __syncthreads();
        tile_scores<D>(sp, xs, E, P, w, gq, i16);
        tile_scores<D>(gp, xs, Gb, P, w, gq, i16);
        __syncthreads();
        float c4[4];
#pragma unroll
        for (int step = 0; step < 4; ++step) {
            const int r = 4 * step + gq;
            const float a = (pv && row0 + r < src.N) ? expf(score_of(sp, r, i16) - mp) * rl : 0.f;
            c4[step] = a * (score_of(gp, r, i16) - gzp);
            if (DX && w == 0) {
                at[r * 20 + i16] = a;
                ct[r * 20 + i16] = c4[step];
            }
        }
#pragma unroll
        for (int step = 0; step < 4; ++step)
#pragma unroll
            for (int fg = 0; fg < kFg; ++fg)
                de[fg] = mfma_f32(c4[step], xs[(4 * step + gq) * kLd + w * (D / 4) + 16 * fg + i16], de[fg]);
        if constexpr (DX) {
            __syncthreads();
            f32x4 dx[kFg];
#pragma unroll
            for (int fg = 0; fg < kFg; ++fg) dx[fg] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int step = 0; step < 4; ++step) {
                const int p = 4 * step + gq;
                const float av = at[i16 * 20 + p], cv = ct[i16 * 20 + p];
#pragma unroll
                for (int fg = 0; fg < kFg; ++fg) {
                    const int f = w * (D / 4) + 16 * fg + i16;
                    const float gv = p < P ? Gb[(size_t)p * D + f] : 0.f, ev = p < P ? E[(size_t)p * D + f] : 0.f;
                    dx[fg] = mfma_f32(av, gv, dx[fg]);
                    dx[fg] = mfma_f32(cv, ev, dx[fg]);
                }
            }
#pragma unroll
            for (int fg = 0; fg < kFg; ++fg)
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (row0 + 4 * gq + e < src.N) dX[(size_t)(src.roff + row0 + 4 * gq + e) * D + w * (D / 4) + 16 * fg + i16] = dx[fg][e];
        }
    }
#pragma unroll
    for (int fg = 0; fg < kFg; ++fg)
#pragma unroll
        for (int e = 0; e < 4; ++e) pdE[((size_t)blockIdx.x * 16 + 4 * gq + e) * D + w * (D / 4) + 16 * fg + i16] = de[fg][e];
}

// dE[p][f] = the parts of all bags in part order
__global__ __launch_bounds__(kThreads) void k_ip_reduce(int D, int P, int n_parts, const float* __restrict__ pdE, float* __restrict__ dE) {
    const int i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= P * D) return;
    const int p = i / D, f = i % D;
    float a = 0.f;
    for (int g = 0; g < n_parts; ++g) a += pdE[((size_t)g * 16 + p) * D + f];
    dE[i] = a;
}

// ---- row map -----------------------------------------------------------------------------------------------------------------------
// u (started at b~[b]) and the gate pre-activation s (started at bg) of the tile's 32 rows
template <typename T, int D>
__device__ __forceinline__ void rm_u_s(f32x4 (&u)[2][4], f32x4 (&s)[2][4], float_ma* xs, const RowSrc& src, long long row0,
                                       const float* __restrict__ Wq, const float* __restrict__ btil, const float* __restrict__ Wg,
                                       const float* __restrict__ bg, int tid, int w, int gq, int i16) {
    const T* X = static_cast<const T*>(src.X);
#pragma unroll
    for (int hg = 0; hg < 4; ++hg) {
        const float b0 = btil[64 * w + 16 * hg + i16], b1 = bg[64 * w + 16 * hg + i16];
#pragma unroll
        for (int rt = 0; rt < 2; ++rt) {
            u[rt][hg] = f32x4{b0, b0, b0, b0};
            s[rt][hg] = f32x4{b1, b1, b1, b1};
        }
    }
#pragma unroll 1
    for (int c = 0; c < D / kChunk; ++c) {
        __syncthreads();
        stage_tile<T>(xs, kXld, X, src.ldx, row0, src.N, c * kChunk, kChunk, kTile, tid);
        __syncthreads();
        lin_acc(u, xs, kXld, Wq + c * kChunk, D, kChunk, w, gq, i16);
        lin_acc(s, xs, kXld, Wg + c * kChunk, D, kChunk, w, gq, i16);
    }
}

__device__ __forceinline__ void bias_init(f32x4 (&t)[2][4], const float* __restrict__ bias, int w, int i16) {
#pragma unroll
    for (int hg = 0; hg < 4; ++hg) {
        const float b0 = bias[64 * w + 16 * hg + i16];
#pragma unroll
        for (int rt = 0; rt < 2; ++rt) t[rt][hg] = f32x4{b0, b0, b0, b0};
    }
}

template <typename T, int D>
__global__ __launch_bounds__(kThreads) void k_rm_forward(const vlsa_bag_desc* __restrict__ bags, int B, const int* __restrict__ tile_start,
                                                         const long long* __restrict__ row_off, const void* __restrict__ xp,
                                                         const float* __restrict__ Wq, const float* __restrict__ btil,
                                                         const float* __restrict__ Wo, const float* __restrict__ bo,
                                                         const float* __restrict__ Wg, const float* __restrict__ bg, float* __restrict__ out,
                                                         unsigned int* __restrict__ mask) {
    __shared__ __attribute__((aligned(16))) float xs_[kTile * kXld];
    __shared__ __attribute__((aligned(16))) float us_[kTile * kUld];
    __shared__ unsigned int mt[kTile * 8];
    float_ma* xs = xs_;
    float_ma* us = us_;
    const BagSpan tile = bag_span(tile_start, B, blockIdx.x);
    const int b = tile.b;
    const RowSrc src = row_src<D>(bags, row_off, xp, b);
    const long long row0 = (long long)tile.idx * kTile;
    const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6), gq = lane >> 4, i16 = lane & 15;
    f32x4 u[2][4], s[2][4], t[2][4];
    rm_u_s<T, D>(u, s, xs, src, row0, Wq, btil + (size_t)b * kH, Wg, bg, tid, w, gq, i16);
    tile_to_lds(us, u, w, gq, i16);
    __syncthreads();
    bias_init(t, bo, w, i16);
    lin_acc(t, us, kUld, Wo, kH, kH, w, gq, i16);
#pragma unroll
    for (int rt = 0; rt < 2; ++rt)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int row = rt * 16 + 4 * gq + e;
            unsigned long long bal[4];
#pragma unroll
            for (int hg = 0; hg < 4; ++hg) bal[hg] = __builtin_amdgcn_ballot_w64(t[rt][hg][e] > 0.f);
            if (i16 < 2) mt[row * 8 + 2 * w + i16] = relu_mask_word(bal, i16, gq);
            if (row0 + row < src.N) {
#pragma unroll
                for (int hg = 0; hg < 4; ++hg) {
                    const float tv = t[rt][hg][e], sv = s[rt][hg][e];
                    const float o = u[rt][hg][e] + (tv > 0.f ? tv : 0.f);
                    out[(size_t)(src.roff + row0 + row) * kH + 64 * w + 16 * hg + i16] = o * (sv / (1.f + expf(-sv)));
                }
            }
        }
    if (mask != nullptr) {
        __syncthreads();
        const int r = tid >> 3;
        if (row0 + r < src.N) mask[(size_t)(src.roff + row0 + r) * 8 + (tid & 7)] = mt[tid];
    }
}

// ws: u, du, ds, dt as [total][256] fp32 each
template <typename T, int D, bool DX>
__global__ __launch_bounds__(kThreads) void k_rm_backward(const vlsa_bag_desc* __restrict__ bags, int B, const int* __restrict__ tile_start,
                                                          const long long* __restrict__ row_off, const void* __restrict__ xp, long long total,
                                                          const float* __restrict__ Wq, const float* __restrict__ btil,
                                                          const float* __restrict__ Wo, const float* __restrict__ bo,
                                                          const float* __restrict__ Wg, const float* __restrict__ bg,
                                                          const float* __restrict__ WoT, const float* __restrict__ WqT,
                                                          const float* __restrict__ WgT, const unsigned int* __restrict__ mask,
                                                          const float* __restrict__ dOut, float* __restrict__ ws, float* __restrict__ dX) {
    __shared__ __attribute__((aligned(16))) float xs_[kTile * kXld];
    __shared__ __attribute__((aligned(16))) float us_[kTile * kUld];
    float_ma* xs = xs_;
    float_ma* us = us_;
    const BagSpan tile = bag_span(tile_start, B, blockIdx.x);
    const int b = tile.b;
    const RowSrc src = row_src<D>(bags, row_off, xp, b);
    const long long row0 = (long long)tile.idx * kTile;
    const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6), gq = lane >> 4, i16 = lane & 15;
    float* wu = ws;
    float* wdu = ws + (size_t)total * kH;
    float* wds = ws + (size_t)total * kH * 2;
    float* wdt = ws + (size_t)total * kH * 3;
    f32x4 u[2][4], s[2][4], t[2][4];
    rm_u_s<T, D>(u, s, xs, src, row0, Wq, btil + (size_t)b * kH, Wg, bg, tid, w, gq, i16);
    tile_to_lds(us, u, w, gq, i16);
    __syncthreads();
    bias_init(t, bo, w, i16);
    lin_acc(t, us, kUld, Wo, kH, kH, w, gq, i16);
    // u <- do, s <- ds, t <- dt; rows past the bag's end: zeros, nothing stored
#pragma unroll
    for (int rt = 0; rt < 2; ++rt)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int row = rt * 16 + 4 * gq + e;
            const bool ok = row0 + row < src.N;
            const size_t grow = ok ? (size_t)(src.roff + row0 + row) : 0;
#pragma unroll
            for (int hg = 0; hg < 4; ++hg) {
                const int unit = 64 * w + 16 * hg + i16;
                float dov = 0.f, dsv = 0.f, dtv = 0.f;
                if (ok) {
                    const float g = dOut[grow * kH + unit];
                    const bool bit = relu_mask_bit(mask + grow * 8, unit);
                    const float uv = u[rt][hg][e], sv = s[rt][hg][e];
                    const float o = uv + (bit ? t[rt][hg][e] : 0.f);
                    const float sig = 1.f / (1.f + expf(-sv));
                    dov = g * (sv * sig);
                    dsv = g * o * (sig * (1.f + sv * (1.f - sig)));
                    dtv = bit ? dov : 0.f;
                    wu[grow * kH + unit] = uv;
                    wds[grow * kH + unit] = dsv;
                    wdt[grow * kH + unit] = dtv;
                }
                u[rt][hg][e] = dov;
                s[rt][hg][e] = dsv;
                t[rt][hg][e] = dtv;
            }
        }
    __syncthreads();                              // the reads of u in LDS are done
    tile_to_lds(us, t, w, gq, i16);
    __syncthreads();
    lin_acc(u, us, kUld, WoT, kH, kH, w, gq, i16);       // du = do + Wo^T dt
#pragma unroll
    for (int rt = 0; rt < 2; ++rt)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int row = rt * 16 + 4 * gq + e;
            if (row0 + row < src.N)
#pragma unroll
                for (int hg = 0; hg < 4; ++hg) wdu[(size_t)(src.roff + row0 + row) * kH + 64 * w + 16 * hg + i16] = u[rt][hg][e];
        }
    if constexpr (DX) {                           // D == 256: dX = Wq^T du + Wg^T ds, the output "units" are the 256 features
        __syncthreads();
        tile_to_lds(us, u, w, gq, i16);
        __syncthreads();
#pragma unroll
        for (int rt = 0; rt < 2; ++rt)
#pragma unroll
            for (int hg = 0; hg < 4; ++hg) t[rt][hg] = f32x4{0.f, 0.f, 0.f, 0.f};
        lin_acc(t, us, kUld, WqT, kH, kH, w, gq, i16);
        __syncthreads();
        tile_to_lds(us, s, w, gq, i16);
        __syncthreads();
        lin_acc(t, us, kUld, WgT, kH, kH, w, gq, i16);
#pragma unroll
        for (int rt = 0; rt < 2; ++rt)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int row = rt * 16 + 4 * gq + e;
                if (row0 + row < src.N)
#pragma unroll
                    for (int hg = 0; hg < 4; ++hg) dX[(size_t)(src.roff + row0 + row) * D + 64 * w + 16 * hg + i16] = t[rt][hg][e];
            }
    }
}

// pdW[split][256][D] = sum over the split's tiles of G^T X: grid (R, D / 128); G packed [total][256] fp32
template <typename T, int D>
__global__ __launch_bounds__(kThreads) void k_rm_wgrad(const vlsa_bag_desc* __restrict__ bags, int B, const int* __restrict__ tile_start,
                                                       int n_tiles, const long long* __restrict__ row_off, const void* __restrict__ xp,
                                                       const float* __restrict__ G, float* __restrict__ pdW) {
    __shared__ __attribute__((aligned(16))) float gs_[kTile * kGld];
    __shared__ __attribute__((aligned(16))) float xs_[kTile * kWld];
    float_ma* gs = gs_;
    float_ma* xs = xs_;
    const int R = gridDim.x, split = blockIdx.x, f0 = blockIdx.y * kChunk;
    const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6), gq = lane >> 4, i16 = lane & 15;
    f32x4 acc[4][8];
#pragma unroll
    for (int hg = 0; hg < 4; ++hg)
#pragma unroll
        for (int fg = 0; fg < 8; ++fg) acc[hg][fg] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int t = split; t < n_tiles; t += R) {
        const BagSpan tile = bag_span(tile_start, B, t);       // (t is block-uniform, the loop bound too)
        const RowSrc src = row_src<D>(bags, row_off, xp, tile.b);
        const long long row0 = (long long)tile.idx * kTile;
        __syncthreads();
        stage_tile<float>(gs, kGld, G + (size_t)src.roff * kH, kH, row0, src.N, 0, kH, kTile, tid);
        stage_tile<T>(xs, kWld, static_cast<const T*>(src.X), src.ldx, row0, src.N, f0, kChunk, kTile, tid);
        __syncthreads();
#pragma unroll 2
        for (int step = 0; step < kTile / 4; ++step) {
            const int r = 4 * step + gq;
            float a[4], x[8];
#pragma unroll
            for (int hg = 0; hg < 4; ++hg) a[hg] = gs[r * kGld + 64 * w + 16 * hg + i16];
#pragma unroll
            for (int fg = 0; fg < 8; ++fg) x[fg] = xs[r * kWld + 16 * fg + i16];
#pragma unroll
            for (int hg = 0; hg < 4; ++hg)
#pragma unroll
                for (int fg = 0; fg < 8; ++fg) acc[hg][fg] = mfma_f32(a[hg], x[fg], acc[hg][fg]);
        }
    }
    // acc[hg][fg][e] = dW[64 w + 16 hg + 4 gq + e][f0 + 16 fg + i16]
    float* o = pdW + (size_t)split * kH * D;
#pragma unroll
    for (int hg = 0; hg < 4; ++hg)
#pragma unroll
        for (int e = 0; e < 4; ++e)
#pragma unroll
            for (int fg = 0; fg < 8; ++fg) o[(size_t)(64 * w + 16 * hg + 4 * gq + e) * D + f0 + 16 * fg + i16] = acc[hg][fg][e];
}

__global__ __launch_bounds__(kThreads) void k_rm_reduce(int R, int n, const float* __restrict__ pdW, float* __restrict__ dW) {
    const size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x;
    float a = 0.f;
    for (int r = 0; r < R; ++r) a += pdW[(size_t)r * n + i];
    dW[i] = a;
}

// grid (B, 3, kSegs): column sums of du, ds, dt over segment seg of bag b's rows -> pcs[((b * 3 + m) * kSegs + seg) * 256 + unit]
__global__ __launch_bounds__(kThreads) void k_rm_colsum(const vlsa_bag_desc* __restrict__ bags, const long long* __restrict__ row_off, long long total,
                                                        const float* __restrict__ ws, float* __restrict__ pcs) {
    const int b = blockIdx.x, mtx = blockIdx.y, seg = blockIdx.z, t = threadIdx.x;
    const long long N = bags[b].N, r0 = N * seg / kSegs, r1 = N * (seg + 1) / kSegs;
    const float* M = ws + (size_t)total * kH * (mtx + 1) + (size_t)row_off[b] * kH;
    float a = 0.f;
    for (long long r = r0; r < r1; ++r) a += M[(size_t)r * kH + t];
    pcs[((size_t)(b * 3 + mtx) * kSegs + seg) * kH + t] = a;
}
// blocks 0 .. B - 1: db~[b] (du); block B: dbg (ds) and dbo (dt) over the bags in bag order
__global__ __launch_bounds__(kThreads) void k_rm_colfold(int B, const float* __restrict__ pcs, float* __restrict__ dbtil, float* __restrict__ dbo,
                                                         float* __restrict__ dbg) {
    const int t = threadIdx.x;
    if ((int)blockIdx.x < B) {
        float a = 0.f;
        for (int seg = 0; seg < kSegs; ++seg) a += pcs[((size_t)(blockIdx.x * 3 + 0) * kSegs + seg) * kH + t];
        dbtil[(size_t)blockIdx.x * kH + t] = a;
        return;
    }
    float g = 0.f, o = 0.f;
    for (int b = 0; b < B; ++b)
        for (int seg = 0; seg < kSegs; ++seg) {
            g += pcs[((size_t)(b * 3 + 1) * kSegs + seg) * kH + t];
            o += pcs[((size_t)(b * 3 + 2) * kSegs + seg) * kH + t];
        }
    dbg[t] = g;
    dbo[t] = o;
}

// 0: bf16 bag rows, 1: fp32 bag rows (D = 512); 2: packed fp32 rows (D = 256); < 0: the error
int source_of(const void* bag_desc, int B, int x_dtype, int D, const void* xp, const int* table, int n_table, const void* row_off) {
    if (!bag_table_ok(bag_desc, B, table, n_table) || !row_off) return VLSA_EINVAL;
    if (x_dtype != VLSA_DT_F32 && x_dtype != VLSA_DT_BF16) return VLSA_EUNSUPPORTED;
    if (xp == nullptr) return D == 512 ? (x_dtype == VLSA_DT_BF16 ? 0 : 1) : VLSA_EUNSUPPORTED;
    return (D == 256 && x_dtype == VLSA_DT_F32) ? 2 : VLSA_EUNSUPPORTED;
}

size_t pool_ws_bytes(int n_parts, int D) { return (size_t)n_parts * (32 + (size_t)16 * D) * 4; }

}  // namespace

extern "C" int vlsa_ilra_tile_rows(void) { return kTile; }

extern "C" int vlsa_ilra_pool_part_rows(void) { return kPoolRowsPerPart; }

extern "C" int vlsa_ilra_pool_parts(int64_t N) {
    const int64_t g = (N + kPoolRowsPerPart - 1) / kPoolRowsPerPart;
    return (int)(g < 1 ? 1 : (g > kMaxParts ? kMaxParts : g));
}

extern "C" size_t vlsa_ilra_pool_workspace_bytes(int n_parts, int D) {
    if (n_parts < 1 || (D != 512 && D != 256)) return 0;
    return pool_ws_bytes(n_parts, D);
}

extern "C" size_t vlsa_ilra_rowmap_backward_workspace_bytes(int64_t total_rows, int n_tiles, int B, int D) {
    if (total_rows < 1 || n_tiles < 1 || B < 1 || B > 64 || (D != 512 && D != 256)) return 0;
    return ((size_t)total_rows * kH * 4 + (size_t)splits_of(n_tiles) * kH * D + (size_t)B * 3 * kSegs * kH) * 4;
}

extern "C" int vlsa_ilra_pool_forward_batch(const void* bag_desc, int B, int x_dtype, int D, int P, const int* part_start, int n_parts,
                                            const int64_t* row_off, const void* xp, const float* E, void* ws, float* Z, float* m, float* l,
                                            void* stream) {
    const int src = source_of(bag_desc, B, x_dtype, D, xp, part_start, n_parts, row_off);
    if (src < 0) return src;
    if (P < 1 || !E || !ws || !Z || !m || !l) return VLSA_EINVAL;
    if (P > kMaxP) return VLSA_EUNSUPPORTED;
    hipStream_t st = (hipStream_t)stream;
    const vlsa_bag_desc* bags = static_cast<const vlsa_bag_desc*>(bag_desc);
    const long long* roff = reinterpret_cast<const long long*>(row_off);
    float* pm = static_cast<float*>(ws);
    float* pl = pm + (size_t)n_parts * 16;
    float* pZ = pl + (size_t)n_parts * 16;
    if (src == 0)
        hipLaunchKernelGGL((k_ip_forward<__bf16, 512>), dim3(n_parts), dim3(kThreads), 0, st, bags, B, P, part_start, roff, xp, E, pm, pl, pZ);
    else if (src == 1)
        hipLaunchKernelGGL((k_ip_forward<float, 512>), dim3(n_parts), dim3(kThreads), 0, st, bags, B, P, part_start, roff, xp, E, pm, pl, pZ);
    else
        hipLaunchKernelGGL((k_ip_forward<float, 256>), dim3(n_parts), dim3(kThreads), 0, st, bags, B, P, part_start, roff, xp, E, pm, pl, pZ);
    hipLaunchKernelGGL(k_ip_merge, dim3(B, P), dim3(kThreads), 0, st, D, part_start, pm, pl, pZ, P, Z, m, l);
    return launch_status();
}

extern "C" int vlsa_ilra_pool_backward_batch(const void* bag_desc, int B, int x_dtype, int D, int P, const int* part_start, int n_parts,
                                             const int64_t* row_off, const void* xp, const float* E, const float* dZ, const float* Z,
                                             const float* m, const float* l, void* ws, float* dE, float* dX, void* stream) {
    const int src = source_of(bag_desc, B, x_dtype, D, xp, part_start, n_parts, row_off);
    if (src < 0) return src;
    if (P < 1 || !E || !dZ || !Z || !m || !l || !ws || !dE) return VLSA_EINVAL;
    if (P > kMaxP) return VLSA_EUNSUPPORTED;
    if (dX != nullptr && src != 2) return VLSA_EINVAL;          // bag rows never receive a gradient
    hipStream_t st = (hipStream_t)stream;
    const vlsa_bag_desc* bags = static_cast<const vlsa_bag_desc*>(bag_desc);
    const long long* roff = reinterpret_cast<const long long*>(row_off);
    float* pdE = static_cast<float*>(ws);
    if (src == 0)
        hipLaunchKernelGGL((k_ip_backward<__bf16, 512, false>), dim3(n_parts), dim3(kThreads), 0, st, bags, B, P, part_start, roff, xp, E, dZ, Z,
                           m, l, pdE, dX);
    else if (src == 1)
        hipLaunchKernelGGL((k_ip_backward<float, 512, false>), dim3(n_parts), dim3(kThreads), 0, st, bags, B, P, part_start, roff, xp, E, dZ, Z, m,
                           l, pdE, dX);
    else if (dX == nullptr)
        hipLaunchKernelGGL((k_ip_backward<float, 256, false>), dim3(n_parts), dim3(kThreads), 0, st, bags, B, P, part_start, roff, xp, E, dZ, Z, m,
                           l, pdE, dX);
    else
        hipLaunchKernelGGL((k_ip_backward<float, 256, true>), dim3(n_parts), dim3(kThreads), 0, st, bags, B, P, part_start, roff, xp, E, dZ, Z, m,
                           l, pdE, dX);
    hipLaunchKernelGGL(k_ip_reduce, dim3((P * D + kThreads - 1) / kThreads), dim3(kThreads), 0, st, D, P, n_parts, pdE, dE);
    return launch_status();
}

extern "C" int vlsa_ilra_rowmap_forward_batch(const void* bag_desc, int B, int x_dtype, int D, int H, const int* tile_start, int n_tiles,
                                              const int64_t* row_off, const void* xp, const float* Wq, const float* btil, const float* Wo,
                                              const float* bo, const float* Wg, const float* bg, float* out, uint32_t* mask, void* stream) {
    const int src = source_of(bag_desc, B, x_dtype, D, xp, tile_start, n_tiles, row_off);
    if (src < 0) return src;
    if (H != kH) return VLSA_EUNSUPPORTED;
    if (!Wq || !btil || !Wo || !bo || !Wg || !bg || !out) return VLSA_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    const vlsa_bag_desc* bags = static_cast<const vlsa_bag_desc*>(bag_desc);
    const long long* roff = reinterpret_cast<const long long*>(row_off);
    if (src == 0)
        hipLaunchKernelGGL((k_rm_forward<__bf16, 512>), dim3(n_tiles), dim3(kThreads), 0, st, bags, B, tile_start, roff, xp, Wq, btil, Wo, bo, Wg,
                           bg, out, mask);
    else if (src == 1)
        hipLaunchKernelGGL((k_rm_forward<float, 512>), dim3(n_tiles), dim3(kThreads), 0, st, bags, B, tile_start, roff, xp, Wq, btil, Wo, bo, Wg,
                           bg, out, mask);
    else
        hipLaunchKernelGGL((k_rm_forward<float, 256>), dim3(n_tiles), dim3(kThreads), 0, st, bags, B, tile_start, roff, xp, Wq, btil, Wo, bo, Wg,
                           bg, out, mask);
    return launch_status();
}

namespace {
template <typename T, int D>
void launch_wgrads(hipStream_t st, const vlsa_bag_desc* bags, int B, const int* tile_start, int n_tiles, const long long* roff, const void* xp,
                   long long total, float* ws, float* pdW, float* dWq, float* dWg, float* dWo) {
    const int R = splits_of(n_tiles);
    const float* wu = ws;
    const float* wdu = ws + (size_t)total * kH;
    const float* wds = ws + (size_t)total * kH * 2;
    const float* wdt = ws + (size_t)total * kH * 3;
    hipLaunchKernelGGL((k_rm_wgrad<T, D>), dim3(R, D / kChunk), dim3(kThreads), 0, st, bags, B, tile_start, n_tiles, roff, xp, wdu, pdW);
    hipLaunchKernelGGL(k_rm_reduce, dim3(kH * D / kThreads), dim3(kThreads), 0, st, R, kH * D, pdW, dWq);
    hipLaunchKernelGGL((k_rm_wgrad<T, D>), dim3(R, D / kChunk), dim3(kThreads), 0, st, bags, B, tile_start, n_tiles, roff, xp, wds, pdW);
    hipLaunchKernelGGL(k_rm_reduce, dim3(kH * D / kThreads), dim3(kThreads), 0, st, R, kH * D, pdW, dWg);
    hipLaunchKernelGGL((k_rm_wgrad<float, 256>), dim3(R, kH / kChunk), dim3(kThreads), 0, st, bags, B, tile_start, n_tiles, roff,
                       static_cast<const void*>(wu), wdt, pdW);
    hipLaunchKernelGGL(k_rm_reduce, dim3(kH * kH / kThreads), dim3(kThreads), 0, st, R, kH * kH, pdW, dWo);
}
}  // namespace

extern "C" int vlsa_ilra_rowmap_backward_batch(const void* bag_desc, int B, int x_dtype, int D, int H, const int* tile_start, int n_tiles,
                                               const int64_t* row_off, const void* xp, int64_t total_rows, const float* Wq, const float* btil,
                                               const float* Wo, const float* bo, const float* Wg, const float* bg, const float* WoT,
                                               const float* WqT, const float* WgT, const uint32_t* mask, const float* dOut, void* ws,
                                               float* dWq, float* dbtil, float* dWo, float* dbo, float* dWg, float* dbg, float* dX,
                                               void* stream) {
    const int src = source_of(bag_desc, B, x_dtype, D, xp, tile_start, n_tiles, row_off);
    if (src < 0) return src;
    if (H != kH) return VLSA_EUNSUPPORTED;
    if (total_rows < 1 || !Wq || !btil || !Wo || !bo || !Wg || !bg || !WoT || !mask || !dOut || !ws || !dWq || !dbtil || !dWo || !dbo || !dWg ||
        !dbg)
        return VLSA_EINVAL;
    if (dX != nullptr && (src != 2 || !WqT || !WgT)) return VLSA_EINVAL;          // bag rows never receive a gradient
    hipStream_t st = (hipStream_t)stream;
    const vlsa_bag_desc* bags = static_cast<const vlsa_bag_desc*>(bag_desc);
    const long long* roff = reinterpret_cast<const long long*>(row_off);
    const long long total = total_rows;
    float* w = static_cast<float*>(ws);
    float* pdW = w + (size_t)total * kH * 4;
    float* pcs = pdW + (size_t)splits_of(n_tiles) * kH * D;
#define VLSA_RM_BWD(T, DD, DXX)                                                                                                             \
    hipLaunchKernelGGL((k_rm_backward<T, DD, DXX>), dim3(n_tiles), dim3(kThreads), 0, st, bags, B, tile_start, roff, xp, total, Wq, btil, Wo, bo, \
                       Wg, bg, WoT, WqT, WgT, mask, dOut, w, dX)
    if (src == 0) {
        VLSA_RM_BWD(__bf16, 512, false);
        launch_wgrads<__bf16, 512>(st, bags, B, tile_start, n_tiles, roff, xp, total, w, pdW, dWq, dWg, dWo);
    } else if (src == 1) {
        VLSA_RM_BWD(float, 512, false);
        launch_wgrads<float, 512>(st, bags, B, tile_start, n_tiles, roff, xp, total, w, pdW, dWq, dWg, dWo);
    } else {
        if (dX != nullptr) {
            VLSA_RM_BWD(float, 256, true);
        } else {
            VLSA_RM_BWD(float, 256, false);
        }
        launch_wgrads<float, 256>(st, bags, B, tile_start, n_tiles, roff, xp, total, w, pdW, dWq, dWg, dWo);
    }
#undef VLSA_RM_BWD
    hipLaunchKernelGGL(k_rm_colsum, dim3(B, 3, kSegs), dim3(kThreads), 0, st, bags, roff, total, w, pcs);
    hipLaunchKernelGGL(k_rm_colfold, dim3(B + 1), dim3(kThreads), 0, st, B, pcs, dbtil, dbo, dbg);
    return launch_status();
}
