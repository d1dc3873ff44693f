// DeepAttnMISL's cluster layer (Yao et al., MedIA 2020; model/deepmil.py:565-577) over a table of bags, forward and backward, gfx950:
//     pre_n = Wp x_n + bp,  h_n = relu(pre_n),  hc_k = mean over {n: c_n = k} of h_n        (Wp [256, 512], c_n the row's cluster id)
// The reference runs num_clusters boolean gathers, a 1x1 convolution each and an adaptive pool.  Here: ONE streaming kernel whose
// h never leaves registers, a merge of the per-workgroup records, and for the backward one [256, N] x [N, 512] product.
//
// Forward.  A bag of N rows is cut into vlsa_cluster_pool_parts(N) partial records -- a function of N alone, so a bag's hc is bit-equal
// alone and in a batch; part g of G takes the 64-row tiles g, g + G, ...  A workgroup is four waves, wave w owns the hidden units
// 64 w .. 64 w + 63 of all 64 rows of the tile: 4 row tiles x 4 unit groups of 16x16 accumulators, started at the bias.  The tile's rows
// come through LDS in four chunks of 128 features.
//   * bf16 rows are consumed exactly; the weights are a THREE-term bf16 split (residual 2^-24 of an entry) in MFMA fragment order,
//     packed by k_cp_prep into the workspace: 3 x mfma_f32_16x16x32_bf16 per fragment pair, fp32 accumulation.  Two terms (2^-17) put
//     the worst pre of a 2 798-row bag 9e-7 off, too close to the 1e-6 band inside which the ReLU mask is allowed to differ.
//   * fp32 rows take the fp32-input MFMA (16x16x4, an exact fp32 FMA chain) on the fp32 weights as they are.
// Epilogue: the ReLU decisions leave as wave ballots in the shared mask format (bag_table.h) and the per-cluster sums are one
// more fp32 MFMA per accumulator register with the 0/1 matrix [cluster k][row] as the A operand: exact fp32 adds in a fixed order,
// 16 running registers per lane for the whole part, no LDS, no atomics.  (Bag lookup, mask and MFMA wrappers: DESIGN.md, "Table-driven
// kernels".)  Ids outside [0, Kc) belong to no cluster; an empty cluster's
// row of hc is zero.  k_cp_merge adds a bag's parts in part order and divides by the count.  A row of no cluster enters the sums as
// an exact 0 whatever it holds; a non-finite value in a row that HAS a cluster reaches all clusters of its tile (0 x Inf in the 0/1 MFMA),
// and the backward multiplies every row of a tile, clustered or not, by its (possibly zero) dpre: the rows must be finite.
//
// Backward (Wp and bp only; the rows get no gradient).  dS_{b,k} = dhc_{b,k} / cnt_{b,k}; dpre_n = mask_n * dS_{b(n), c_n} with the mask
// READ from the forward's bits; dWp = sum_n dpre_n x_n^T.  The launch's rows are cut into 32-row tiles that never straddle a bag; the
// grid is (row split r of R, hidden slice s of 4).  A workgroup keeps its [64, 512] block of dWp in registers (wave w: features
// 128 w .. 128 w + 127), walks the tiles r, r + R, ... and per tile stages X TRANSPOSED in LDS (the reduction runs over the rows, so the
// MFMA wants 8 rows of one feature per lane), builds the A fragments (dpre as a two-term bf16 split, 2^-17: the gradients are held
// to 1e-4) once per workgroup and issues 2 (bf16 rows) or 3 (fp32 rows as hi + lo: hi hi, hi lo, lo hi) MFMAs per fragment pair.
// The R <= 64 partials ([256, 512] + [256] floats each: at most 32.1 MiB) are added in split order by k_cp_reduce: bit-reproducible.
#include "bag_table.h"
#include "launch.h"

namespace {
using namespace vlsa;

constexpr int kD = 512, kH = 256, kMaxK = 16, kThreads = 256;
constexpr int kTileF = 64;         // rows per forward tile
constexpr int kChunk = 128;        // features per staged chunk of the forward
constexpr int kMaxParts = 128;     // partial records per bag
constexpr int kTileB = 32;         // rows per backward tile (one MFMA K step)
constexpr size_t kWpackBytes = (size_t)16 * 16 * 3 * 1024;
constexpr int kDsLd = 80;          // floats per cluster row of the backward's dS table in LDS

// wpack[((hg * 16 + ks) * 3 + term) * 1024 + lane * 16 + 2 e] = term of Wp[16 hg + (lane & 15)][32 ks + 8 (lane >> 4) + e]; grid 768 x 64
__global__ __launch_bounds__(64) void k_cp_prep(const float* __restrict__ Wp, unsigned char* __restrict__ wpack) {
    const int blk = blockIdx.x, lane = threadIdx.x;
    const int term = blk % 3, ks = (blk / 3) % 16, hg = blk / 48;
    const int h = 16 * hg + (lane & 15), k0 = 32 * ks + 8 * (lane >> 4);
    bf16x8 o;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const float x = Wp[(size_t)h * kD + k0 + e];
        const __bf16 hi = (__bf16)x;
        const float r1 = x - (float)hi;
        const __bf16 mid = (__bf16)r1;
        const __bf16 lo = (__bf16)(r1 - (float)mid);
        o[e] = term == 0 ? hi : term == 1 ? mid : lo;
    }
    *reinterpret_cast<bf16x8*>(wpack + (size_t)blk * 1024 + lane * 16) = o;
}

template <typename T> struct FwdTile {
    static constexpr int kLd = kChunk * (int)sizeof(T) + 16;       // bytes per LDS row: 16 bytes of padding
    static constexpr int kUnits = kChunk * (int)sizeof(T) / 16;    // 16-byte units per row of a chunk
    static constexpr int kLoads = kTileF * kUnits / kThreads;      // per thread
};

template <typename T>
__global__ __launch_bounds__(kThreads) void k_cp_forward(const vlsa_bag_desc* __restrict__ bags, int B, int Kc, const int* __restrict__ part_start,
                                                         const long long* __restrict__ row_off, const int* __restrict__ ids,
                                                         const float* __restrict__ Wp, const float* __restrict__ bp,
                                                         const unsigned char* __restrict__ wpack, float* __restrict__ pS,
                                                         int* __restrict__ pcnt, unsigned int* __restrict__ mask) {
    using F = FwdTile<T>;
    constexpr bool BF = sizeof(T) == 2;
    __shared__ __attribute__((aligned(16))) unsigned char xs[kTileF * F::kLd];
    __shared__ __attribute__((aligned(16))) int cids[kTileF];
    __shared__ unsigned int mt[kTileF * 8];
    const BagSpan part = bag_span(part_start, B, blockIdx.x);
    const int b = part.b, g = part.idx, G = part.count;
    const T* X = static_cast<const T*>(bags[b].X);
    const long long N = bags[b].N, ldx = bags[b].ldx, roff = row_off[b];
    const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6), gq = lane >> 4, i16 = lane & 15;
    float bias[4];
#pragma unroll
    for (int hg = 0; hg < 4; ++hg) bias[hg] = bp[64 * w + 16 * hg + i16];
    f32x4 S[4];
#pragma unroll
    for (int hg = 0; hg < 4; ++hg) S[hg] = f32x4{0.f, 0.f, 0.f, 0.f};
    int cnt = 0;
    const long long ntiles = (N + kTileF - 1) / kTileF;
    for (long long t = g; t < ntiles; t += G) {
        const long long row0 = t * kTileF;
        f32x4 acc[4][4];
#pragma unroll
        for (int rt = 0; rt < 4; ++rt)
#pragma unroll
            for (int hg = 0; hg < 4; ++hg) acc[rt][hg] = f32x4{bias[hg], bias[hg], bias[hg], bias[hg]};
#pragma unroll 1
        for (int c = 0; c < kD / kChunk; ++c) {
            // the chunk's rows, clamped to the bag's last row (valid memory; such rows join no cluster and store no mask)
            u32x4 v[F::kLoads];
#pragma unroll
            for (int i = 0; i < F::kLoads; ++i) {
                const int u = i * kThreads + tid, r = u / F::kUnits, cu = u % F::kUnits;
                long long row = row0 + r;
                if (row > N - 1) row = N - 1;
                v[i] = *reinterpret_cast<const u32x4*>(reinterpret_cast<const unsigned char*>(X + row * ldx + c * kChunk) + cu * 16);
            }
            __syncthreads();                     // the previous chunk's (and tile's) LDS reads are done
            if (c == 0 && tid < kTileF) {
                int id = -1;
                if (row0 + tid < N) {
                    id = ids[roff + row0 + tid];
                    if (id < 0 || id >= Kc) id = -1;
                }
                cids[tid] = id;
            }
#pragma unroll
            for (int i = 0; i < F::kLoads; ++i) {
                const int u = i * kThreads + tid, r = u / F::kUnits, cu = u % F::kUnits;
                *reinterpret_cast<u32x4_ma*>(xs + r * F::kLd + cu * 16) = v[i];
            }
            __syncthreads();
            if constexpr (BF) {
#pragma unroll
                for (int ksl = 0; ksl < 4; ++ksl) {
                    const int ks = c * 4 + ksl;
                    bf16x8 bw[4][3];
#pragma unroll
                    for (int hg = 0; hg < 4; ++hg)
#pragma unroll
                        for (int term = 0; term < 3; ++term)
                            bw[hg][term] = *reinterpret_cast<const bf16x8*>(wpack + (size_t)(((4 * w + hg) * 16 + ks) * 3 + term) * 1024 + lane * 16);
#pragma unroll
                    for (int rt = 0; rt < 4; ++rt) {
                        const bf16x8 a = *reinterpret_cast<const bf16x8_ma*>(xs + (rt * 16 + i16) * F::kLd + (ksl * 32 + 8 * gq) * 2);
#pragma unroll
                        for (int term = 2; term >= 0; --term)
#pragma unroll
                            for (int hg = 0; hg < 4; ++hg) acc[rt][hg] = mfma_bf16(a, bw[hg][term], acc[rt][hg]);
                    }
                }
            } else {
                // blocks of 16 features as four K = 4 steps; step j takes feature 4 (lane >> 4) + j of the block on both operands
#pragma unroll 2
                for (int kb = 0; kb < kChunk / 16; ++kb) {
                    f32x4 bw[4];
#pragma unroll
                    for (int hg = 0; hg < 4; ++hg)
                        bw[hg] = *reinterpret_cast<const f32x4*>(Wp + (size_t)(64 * w + 16 * hg + i16) * kD + c * kChunk + kb * 16 + 4 * gq);
#pragma unroll
                    for (int rt = 0; rt < 4; ++rt) {
                        const f32x4 a = *reinterpret_cast<const f32x4_ma*>(xs + (rt * 16 + i16) * F::kLd + (kb * 16 + 4 * gq) * 4);
#pragma unroll
                        for (int j = 0; j < 4; ++j)
#pragma unroll
                            for (int hg = 0; hg < 4; ++hg) acc[rt][hg] = mfma_f32(a[j], bw[hg][j], acc[rt][hg]);
                    }
                }
            }
        }
        // acc[rt][hg][e] = pre of row rt * 16 + 4 gq + e, unit 64 w + 16 hg + i16
#pragma unroll
        for (int rt = 0; rt < 4; ++rt) {
            const i32x4 cv = *reinterpret_cast<const i32x4*>(&cids[rt * 16 + 4 * gq]);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                unsigned long long bal[4];
#pragma unroll
                for (int hg = 0; hg < 4; ++hg) bal[hg] = __builtin_amdgcn_ballot_w64(acc[rt][hg][e] > 0.f);
                if (mask != nullptr && i16 < 2) mt[(rt * 16 + 4 * gq + e) * 8 + 2 * w + i16] = relu_mask_word(bal, i16, gq);
                const float sel = cv[e] == i16 ? 1.f : 0.f;
                const bool in = cv[e] >= 0;             // a row of no cluster enters as 0, so that an Inf or NaN in it stays out of the sums
#pragma unroll
                for (int hg = 0; hg < 4; ++hg) {
                    const float pre = acc[rt][hg][e];
                    S[hg] = mfma_f32(sel, (in && pre > 0.f) ? pre : 0.f, S[hg]);
                }
            }
        }
        if (tid < kMaxK)
            for (int r = 0; r < kTileF; ++r) cnt += cids[r] == tid ? 1 : 0;
        if (mask != nullptr) {
            __syncthreads();
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const int idx = i * kThreads + tid, r = idx >> 3;
                if (row0 + r < N) mask[(size_t)(roff + row0 + r) * 8 + (idx & 7)] = mt[idx];
            }
        }
    }
    // S[hg][e] = sum of cluster 4 gq + e, unit 64 w + 16 hg + i16
#pragma unroll
    for (int e = 0; e < 4; ++e)
        if (4 * gq + e < Kc)
#pragma unroll
            for (int hg = 0; hg < 4; ++hg) pS[((size_t)blockIdx.x * Kc + 4 * gq + e) * kH + 64 * w + 16 * hg + i16] = S[hg][e];
    if (tid < kMaxK) pcnt[(size_t)blockIdx.x * kMaxK + tid] = cnt;
}

// one block per (bag, cluster): the parts in part order, then the mean
__global__ __launch_bounds__(kThreads) void k_cp_merge(int Kc, const int* __restrict__ part_start, const float* __restrict__ pS,
                                                       const int* __restrict__ pcnt, float* __restrict__ hc, int* __restrict__ cnt) {
    const int b = blockIdx.x / Kc, k = blockIdx.x % Kc, t = threadIdx.x;
    const int p0 = part_start[b], G = part_start[b + 1] - p0;
    float a = 0.f;
    int n = 0;
    for (int g = 0; g < G; ++g) {
        a += pS[((size_t)(p0 + g) * Kc + k) * kH + t];
        n += pcnt[(size_t)(p0 + g) * kMaxK + k];
    }
    hc[((size_t)b * Kc + k) * kH + t] = n > 0 ? a / (float)n : 0.f;
    if (t == 0) cnt[b * Kc + k] = n;
}

// ---- backward ----------------------------------------------------------------------------------------------------------------------
// 16-byte unit of feature F, row block s (rows 8 s .. 8 s + 7) in the transposed tile image: 64 bytes per feature, the unit index XORed
// so that the 64 lanes of a fragment read spread over all 16 unit positions of the banks
__device__ __forceinline__ int t_off(int F, int s) { return (F * 4 + (s ^ ((F >> 2) & 3))) * 16; }

template <typename T> struct BwdTile {
    static constexpr int kImages = sizeof(T) == 2 ? 1 : 2;             // fp32 rows: hi and lo
    static constexpr int kImageBytes = kD * kTileB * 2;                // 32 KiB
    static constexpr int kAfr = kImages * kImageBytes;                 // A fragments: [4 unit groups][hi, lo][64 lanes x 16 B]
    static constexpr int kDs = kAfr + 4 * 2 * 1024;                    // dS table [16][kDsLd] floats
    static constexpr int kCid = kDs + kMaxK * kDsLd * 4;               // [32] ints
    static constexpr int kMw = kCid + kTileB * 4;                      // [32][2] mask words of the slice
    static constexpr int kBytes = kMw + kTileB * 2 * 4;
};

// the thread's share of a tile in registers: feature pair tid of the rows 8 i + j (raw bits), the tile's ids and mask words
template <typename T> struct BwdRegs {
    unsigned int x[4][8 * (int)sizeof(T) / 2];
    int cid;
    unsigned int mw;
};

template <typename T>
__device__ __forceinline__ void bwd_load(BwdRegs<T>& r, const vlsa_bag_desc* bags, int B, const int* tile_start, const long long* row_off,
                                         const int* ids, const unsigned int* mask, int Kc, int slice, int t, int tid) {
    const BagSpan tile = bag_span(tile_start, B, t);       // (t and the branches around the calls are block-uniform)
    const int b = tile.b;
    const T* X = static_cast<const T*>(bags[b].X);
    const long long N = bags[b].N, ldx = bags[b].ldx, roff = row_off[b], row0 = (long long)tile.idx * kTileB;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            long long row = row0 + 8 * i + j;
            if (row > N - 1) row = N - 1;
            const T* p = X + row * ldx + 2 * tid;
            if constexpr (sizeof(T) == 2) {
                r.x[i][j] = *reinterpret_cast<const unsigned int*>(p);
            } else {
                const uint2 v = *reinterpret_cast<const uint2*>(p);
                r.x[i][2 * j] = v.x;
                r.x[i][2 * j + 1] = v.y;
            }
        }
    r.cid = -1;
    r.mw = 0u;
    if (tid < kTileB && row0 + tid < N) {
        const int id = ids[roff + row0 + tid];
        r.cid = (id < 0 || id >= Kc) ? -1 : id;
    }
    // the two mask words (bag_table.h) of this hidden slice of 64 units
    if (tid < 2 * kTileB && row0 + (tid >> 1) < N) r.mw = mask[(size_t)(roff + row0 + (tid >> 1)) * 8 + 2 * slice + (tid & 1)];
}

__device__ __forceinline__ unsigned int bf16_bits(float f) { return (unsigned int)__builtin_bit_cast(unsigned short, (__bf16)f); }

template <typename T>
__device__ __forceinline__ void bwd_publish(const BwdRegs<T>& r, unsigned char* lds, int tid) {
    using L = BwdTile<T>;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        u32x4 o0, o1;          // features 2 tid and 2 tid + 1, rows 8 i .. 8 i + 7
        if constexpr (sizeof(T) == 2) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                o0[q] = (r.x[i][2 * q] & 0xffffu) | (r.x[i][2 * q + 1] << 16);
                o1[q] = (r.x[i][2 * q] >> 16) | (r.x[i][2 * q + 1] & 0xffff0000u);
            }
            *reinterpret_cast<u32x4_ma*>(lds + t_off(2 * tid, i)) = o0;
            *reinterpret_cast<u32x4_ma*>(lds + t_off(2 * tid + 1, i)) = o1;
        } else {
            u32x4 l0, l1;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                unsigned int hi[2][2], lo[2][2];          // [row 2 q + a][feature f]
#pragma unroll
                for (int a = 0; a < 2; ++a)
#pragma unroll
                    for (int f = 0; f < 2; ++f) {
                        const float v = __uint_as_float(r.x[i][2 * (2 * q + a) + f]);
                        const __bf16 h = (__bf16)v;
                        hi[a][f] = bf16_bits((float)h);
                        lo[a][f] = bf16_bits(v - (float)h);
                    }
                o0[q] = hi[0][0] | (hi[1][0] << 16);
                o1[q] = hi[0][1] | (hi[1][1] << 16);
                l0[q] = lo[0][0] | (lo[1][0] << 16);
                l1[q] = lo[0][1] | (lo[1][1] << 16);
            }
            *reinterpret_cast<u32x4_ma*>(lds + t_off(2 * tid, i)) = o0;
            *reinterpret_cast<u32x4_ma*>(lds + t_off(2 * tid + 1, i)) = o1;
            *reinterpret_cast<u32x4_ma*>(lds + L::kImageBytes + t_off(2 * tid, i)) = l0;
            *reinterpret_cast<u32x4_ma*>(lds + L::kImageBytes + t_off(2 * tid + 1, i)) = l1;
        }
    }
    if (tid < kTileB) reinterpret_cast<int_ma*>(lds + L::kCid)[tid] = r.cid;
    if (tid < 2 * kTileB) reinterpret_cast<unsigned int __attribute__((may_alias))*>(lds + L::kMw)[tid] = r.mw;
}

// grid (R, 4): row split blockIdx.x of R, hidden slice blockIdx.y
template <typename T>
__global__ __launch_bounds__(kThreads) void k_cp_backward(const vlsa_bag_desc* __restrict__ bags, int B, int Kc, const int* __restrict__ tile_start,
                                                          int n_tiles, const long long* __restrict__ row_off, const int* __restrict__ ids,
                                                          const unsigned int* __restrict__ mask, const float* __restrict__ dhc,
                                                          const int* __restrict__ cnt, float* __restrict__ pdW, float* __restrict__ pdb) {
    using L = BwdTile<T>;
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    const int R = gridDim.x, split = blockIdx.x, slice = blockIdx.y;
    const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6), gq = lane >> 4, i16 = lane & 15;
    float_ma* dSs = reinterpret_cast<float_ma*>(lds + L::kDs);
    const int_ma* cids = reinterpret_cast<const int_ma*>(lds + L::kCid);
    const unsigned int __attribute__((may_alias))* mws = reinterpret_cast<const unsigned int __attribute__((may_alias))*>(lds + L::kMw);
    f32x4 acc[4][8];
#pragma unroll
    for (int hg = 0; hg < 4; ++hg)
#pragma unroll
        for (int fg = 0; fg < 8; ++fg) acc[hg][fg] = f32x4{0.f, 0.f, 0.f, 0.f};
    float dbsum = 0.f;
    int table_bag = -1;
    BwdRegs<T> regs;
    if (split < n_tiles) bwd_load<T>(regs, bags, B, tile_start, row_off, ids, mask, Kc, slice, split, tid);
    for (int t = split; t < n_tiles; t += R) {
        const int b = bag_span(tile_start, B, t).b;
        bwd_publish<T>(regs, lds, tid);
        if (b != table_bag) {            // dS of this bag and slice: dhc / cnt, zero for an empty cluster
            for (int i = tid; i < kMaxK * 64; i += kThreads) {
                const int k = i >> 6, hl = i & 63;
                float v = 0.f;
                if (k < Kc) {
                    const int n = cnt[b * Kc + k];
                    if (n > 0) v = dhc[((size_t)b * Kc + k) * kH + 64 * slice + hl] / (float)n;
                }
                dSs[k * kDsLd + hl] = v;
            }
            table_bag = b;
        }
        __syncthreads();
        if (t + R < n_tiles) bwd_load<T>(regs, bags, B, tile_start, row_off, ids, mask, Kc, slice, t + R, tid);      // in flight under the MFMAs
        {   // wave w builds the A fragments of unit group w: dpre of unit 64 slice + 16 w + i16, rows 8 gq + j
            bf16x8 hi, lo;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int row = 8 * gq + j, cid = cids[row];
                const unsigned int bit = (mws[row * 2 + (w >> 1)] >> (16 * (w & 1) + i16)) & 1u;
                const float ds = dSs[(cid < 0 ? 0 : cid) * kDsLd + 16 * w + i16];
                const float v = (cid >= 0 && bit) ? ds : 0.f;
                dbsum += v;
                hi[j] = (__bf16)v;
                lo[j] = (__bf16)(v - (float)hi[j]);
            }
            *reinterpret_cast<bf16x8_ma*>(lds + L::kAfr + (w * 2 + 0) * 1024 + lane * 16) = hi;
            *reinterpret_cast<bf16x8_ma*>(lds + L::kAfr + (w * 2 + 1) * 1024 + lane * 16) = lo;
        }
        __syncthreads();
        bf16x8 af[4][2];
#pragma unroll
        for (int hg = 0; hg < 4; ++hg)
#pragma unroll
            for (int term = 0; term < 2; ++term) af[hg][term] = *reinterpret_cast<const bf16x8_ma*>(lds + L::kAfr + (hg * 2 + term) * 1024 + lane * 16);
#pragma unroll
        for (int fg = 0; fg < 8; ++fg) {
            const int F = 128 * w + 16 * fg + i16;
            const bf16x8 xh = *reinterpret_cast<const bf16x8_ma*>(lds + t_off(F, gq));
#pragma unroll
            for (int hg = 0; hg < 4; ++hg) acc[hg][fg] = mfma_bf16(af[hg][1], xh, acc[hg][fg]);
            if constexpr (L::kImages == 2) {
                const bf16x8 xl = *reinterpret_cast<const bf16x8_ma*>(lds + L::kImageBytes + t_off(F, gq));
#pragma unroll
                for (int hg = 0; hg < 4; ++hg) acc[hg][fg] = mfma_bf16(af[hg][0], xl, acc[hg][fg]);
            }
#pragma unroll
            for (int hg = 0; hg < 4; ++hg) acc[hg][fg] = mfma_bf16(af[hg][0], xh, acc[hg][fg]);
        }
        __syncthreads();                 // the tile's LDS reads are done before the next one is published
    }
    // acc[hg][fg][e] = dWp[64 slice + 16 hg + 4 gq + e][128 w + 16 fg + i16]
    float* out = pdW + (size_t)split * kH * kD;
#pragma unroll
    for (int hg = 0; hg < 4; ++hg)
#pragma unroll
        for (int e = 0; e < 4; ++e)
#pragma unroll
            for (int fg = 0; fg < 8; ++fg) out[(size_t)(64 * slice + 16 * hg + 4 * gq + e) * kD + 128 * w + 16 * fg + i16] = acc[hg][fg][e];
    dbsum += __shfl_xor(dbsum, 16);
    dbsum += __shfl_xor(dbsum, 32);
    if (gq == 0) pdb[(size_t)split * kH + 64 * slice + 16 * w + i16] = dbsum;
}

// blocks 0..511: 256 entries of dWp each; block 512: dbp.  The splits in split order.
__global__ __launch_bounds__(kThreads) void k_cp_reduce(int R, const float* __restrict__ pdW, const float* __restrict__ pdb, float* __restrict__ dWp,
                                                        float* __restrict__ dbp) {
    const int t = threadIdx.x;
    float a = 0.f;
    if (blockIdx.x < 512) {
        const size_t i = (size_t)blockIdx.x * kThreads + t;
        for (int r = 0; r < R; ++r) a += pdW[(size_t)r * kH * kD + i];
        dWp[i] = a;
    } else {
        for (int r = 0; r < R; ++r) a += pdb[(size_t)r * kH + t];
        dbp[t] = a;
    }
}

int check_common(const void* bag_desc, int B, int x_dtype, int D, int H, int Kc, const int* table, int n_table) {
    if (!bag_table_ok(bag_desc, B, table, n_table) || Kc < 1) return VLSA_EINVAL;
    if (D != kD || H != kH || Kc > kMaxK || (x_dtype != VLSA_DT_F32 && x_dtype != VLSA_DT_BF16)) return VLSA_EUNSUPPORTED;
    return VLSA_OK;
}

}  // namespace

extern "C" int vlsa_cluster_pool_tile_rows(void) { return kTileF; }

extern "C" int vlsa_cluster_pool_parts(int64_t N) {
    const int64_t g = (N + kTileF - 1) / kTileF;
    return (int)(g < 1 ? 1 : (g > kMaxParts ? kMaxParts : g));
}

extern "C" size_t vlsa_cluster_pool_workspace_bytes(int n_parts, int Kc) {
    if (n_parts < 1 || Kc < 1 || Kc > kMaxK) return 0;
    return kWpackBytes + (size_t)n_parts * ((size_t)Kc * kH + kMaxK) * 4;
}

extern "C" int vlsa_cluster_pool_backward_tile_rows(void) { return kTileB; }

extern "C" size_t vlsa_cluster_pool_backward_workspace_bytes(int n_tiles) {
    if (n_tiles < 1) return 0;
    return (size_t)splits_of(n_tiles) * ((size_t)kH * kD + kH) * 4;
}

extern "C" int vlsa_cluster_pool_forward_batch(const void* bag_desc, int B, int x_dtype, int D, int H, int Kc, const int* part_start,
                                               int n_parts, const int64_t* row_off, const int* ids, const float* Wp, const float* bp,
                                               void* ws, float* hc, int* cnt, uint32_t* mask, void* stream) {
    const int rc = check_common(bag_desc, B, x_dtype, D, H, Kc, part_start, n_parts);
    if (rc != VLSA_OK) return rc;
    if (!row_off || !ids || !Wp || !bp || !ws || !hc || !cnt) return VLSA_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    const vlsa_bag_desc* bags = static_cast<const vlsa_bag_desc*>(bag_desc);
    unsigned char* wpack = static_cast<unsigned char*>(ws);
    float* pS = reinterpret_cast<float*>(wpack + kWpackBytes);
    int* pcnt = reinterpret_cast<int*>(pS + (size_t)n_parts * Kc * kH);
    const long long* roff = reinterpret_cast<const long long*>(row_off);
    if (x_dtype == VLSA_DT_BF16) {
        hipLaunchKernelGGL(k_cp_prep, dim3(16 * 16 * 3), dim3(64), 0, st, Wp, wpack);
        hipLaunchKernelGGL(k_cp_forward<__bf16>, dim3(n_parts), dim3(kThreads), 0, st, bags, B, Kc, part_start, roff, ids, Wp, bp, wpack, pS,
                           pcnt, mask);
    } else {
        hipLaunchKernelGGL(k_cp_forward<float>, dim3(n_parts), dim3(kThreads), 0, st, bags, B, Kc, part_start, roff, ids, Wp, bp, wpack, pS,
                           pcnt, mask);
    }
    hipLaunchKernelGGL(k_cp_merge, dim3(B * Kc), dim3(kThreads), 0, st, Kc, part_start, pS, pcnt, hc, cnt);
    return launch_status();
}

extern "C" int vlsa_cluster_pool_backward_batch(const void* bag_desc, int B, int x_dtype, int D, int H, int Kc, const int* tile_start,
                                                int n_tiles, const int64_t* row_off, const int* ids, const uint32_t* mask, const float* dhc,
                                                const int* cnt, void* ws, float* dWp, float* dbp, void* stream) {
    const int rc = check_common(bag_desc, B, x_dtype, D, H, Kc, tile_start, n_tiles);
    if (rc != VLSA_OK) return rc;
    if (!row_off || !ids || !mask || !dhc || !cnt || !ws || !dWp || !dbp) return VLSA_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    const vlsa_bag_desc* bags = static_cast<const vlsa_bag_desc*>(bag_desc);
    const int R = splits_of(n_tiles);
    float* pdW = static_cast<float*>(ws);
    float* pdb = pdW + (size_t)R * kH * kD;
    const long long* roff = reinterpret_cast<const long long*>(row_off);
    if (x_dtype == VLSA_DT_BF16) {
        launch_lds<k_cp_backward<__bf16>>(dim3(R, 4), dim3(kThreads), BwdTile<__bf16>::kBytes, st, bags, B, Kc, tile_start, n_tiles, roff,
                                          ids, mask, dhc, cnt, pdW, pdb);
    } else {
        launch_lds<k_cp_backward<float>>(dim3(R, 4), dim3(kThreads), BwdTile<float>::kBytes, st, bags, B, Kc, tile_start, n_tiles, roff, ids,
                                         mask, dhc, cnt, pdW, pdb);
    }
    hipLaunchKernelGGL(k_cp_reduce, dim3(513), dim3(kThreads), 0, st, R, pdW, pdb, dWp, dbp);
    return launch_status();
}
