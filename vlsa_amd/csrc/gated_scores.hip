// Attention scores of the ABMIL-style pooling modules over ALL N patches of a bag:
//     Gated_Attention_Pooling (model/layers.py:85-122):  a_n = w2 . (tanh(Wa x_n + ba) * sigmoid(Wg x_n + bg)) + c
//     Attention_Pooling       (model/layers.py:125-153): a_n = w2 .  tanh(Wa x_n + ba)                       + c
// with Wa, Wg in [256, 512].  This is the one MFMA-bound piece of the path (2 x 512 x 256 FLOP per patch and branch);
// the reference (and the first version here) runs it as two library GEMMs that write [N, 256] fp32 hidden activations to
// memory and re-read them.  Here: ONE kernel, hidden activations never leave registers.
//
//   * workgroup = 256 rows x HALF of the hidden units (128 of each branch), 8 waves; wave w owns 16 hidden units of BOTH
//     branches, so the gate product is wave-local: 16 row tiles x 2 branches = 128 accumulator registers per lane.  The two
//     workgroups of a row tile add their partial scores into a zeroed a[] (two addends: order-independent).
//   * K loop in 16 steps of 32: the wave's weight fragments of a step (bf16 hi + lo split of the fp32 weights, pre-scaled by
//     the exp2 factors and packed in fragment order by k_prepare_gated_weights: 4 KB, contiguous, L2 resident) are loaded
//     straight into a register ring three steps ahead; the thread's 32 B of the step's X chunk (256 rows x 64 B) are loaded
//     two steps ahead into registers and published to a double-buffered LDS tile (16-B chunks XOR-swizzled for the
//     non-contiguous ds_read_b128 lane groups: 0 bank conflicts).  One barrier per step.  Plain loads only: the compiler
//     counts vmcnt exactly (a variant with LDS-DMA for X and register loads for W showed that the two kinds do NOT retire in
//     one common order).
//   * X is bf16 and consumed exactly; weights are 2-term bf16 splits (rel. 2^-17); fp32 accumulation: 64 MFMAs
//     (16x16x32 bf16) per step and wave, hi and lo terms interleaved so that back-to-back MFMAs never share an accumulator.
//   * epilogue: accumulators start at the bias; tanh * sigmoid as (1 - u) / ((1 + u)(1 + v)) with two v_exp_f32 and one
//     v_rcp_f32 per value; dot with w2 over the wave's 16 hidden units by four DPP row rotations; cross-wave sum through LDS.
//   * the ungated module (half the accumulators) runs as FOUR-wave workgroups of 128 rows x 128 hidden units, wave w owning two
//     groups of 16 hidden units (template HG = 2): an A fragment feeds four MFMAs instead of two, 152 registers let three such
//     workgroups share a CU out of step with each other (gs_tiling() below has the measurements and what the gated module did
//     with the same shapes).
//   * bags that fit one round of the 256 CUs use smaller tiles (rows per tile = smallest multiple of 16 that still fits one
//     round: a 2 798-patch bag runs on 176 CUs instead of 22); larger bags use the static 256-row variant.
// Roofline: MFMA-bound: 2 terms x 2 branches x 2 x 512 x 256 = 1.05 MFLOP per patch -> 52 GFLOP per 50k bag = 21 us at
// 2.5 PFLOP/s dense bf16.  Round 3 (four-wave shapes, gs_tiling() below): gated 57 us per 50k bag, 383 us at 400k = 21.9 %
// algorithmic; ungated 32 / 188 us = 22.1 %.  Rounds 1-2 (8 waves x 256 rows): 62 us per 50k bag and 389 us at N = 400k =
// 1.08 PFLOP/s executed = 43 % of the dense peak (a register-only probe with this accumulator / operand pattern reaches
// 2.0 PFLOP/s at 2 waves per SIMD, tools/probes/mfma_rate.hip).  What was measured on the way (tools/kbench_gated.py, and the
// timing-only ablations listed at gs_tiling() below): of the 435 us at 400k patches the X loads cost 92 (343 without them), the
// weight loads 36, the activations 34 (they were ~25 % of a tile with IEEE divisions and ds_bpermute shuffles), the barrier 25,
// the A-fragment reads 7; LDS-DMA ring vs register ring vs deeper prefetch: equal.
//
// Round 5: large bf16 bags (gs_tile_use() below: gated from 18 432 rows on, ungated 18 432 .. 65 536) and ALL scores + pooling launches
// of bf16 bags / batches take k_scores_tile_p
// (gated_scores_tile.hip: both operands through LDS-DMA, persistent 256 x 256 tiles); this file keeps the fragment-order kernels for
// everything else (fp32 bags, the ungated module's plain scores, small bags) and the C entry points, which dispatch.
#include <cstdlib>

#include "vlsa_common.h"
#include "gated_scores.h"
#include "launch.h"

// Timing-only ablations of k_gated_scores (results are WRONG with any bit set; tools/attic/gs_ablate.sh builds one library per bit):
// 1 = no A-fragment reads from LDS, 2 = no weight loads, 4 = no X loads / publication, 8 = no per-step barrier,
// 16 = no activations in the epilogue, 32 = no MFMAs, 64 = no X loads (stale registers are published), 128 = X loaded, not published.
// (Two more existed while X came through flat loads: X rows from the first 4 MB of the bag only, and a step's chunk read as one
// contiguous block; their results are in the notes at gs_tiling().)
#ifndef VLSA_GS_ABL
#define VLSA_GS_ABL 0
#endif

namespace vlsa {

namespace gs {
constexpr int kRows = 256;                        // patch rows per workgroup tile
constexpr int kXBuf = kRows * 64;                 // one K step of the tile: 256 rows x 32 bf16 = 16 KiB
constexpr int kXOff = 0;
constexpr int kScrOff = kXOff + 2 * kXBuf;        // 32 KiB
constexpr int kLds = kScrOff + 8 * kRows * 4;     // + 8 KiB
// fp32 bags: every step's chunk is published as TWO bf16 images (hi, lo = the 2-term split of the fp32 values): 4 buffers
constexpr int kScrOff32 = kXOff + 4 * kXBuf;      // 64 KiB
constexpr int kLds32 = kScrOff32 + 8 * kRows * 4;
}  // namespace gs

// packed[(((half * 8 + w) * 16 + ks) * NF + f) * 1024 + lane * 16 + 2 e] =
//     term(f & 1) of W_br[128 half + 16 w + (lane & 15)][32 ks + 8 (lane >> 4) + e],   f = br * 2 + term,  NF = 4 (gated) / 2.
// grid = 2 * 8 * 16 * NF workgroups of 64 threads.
__global__ __launch_bounds__(64) void k_prepare_gated_weights(const float* __restrict__ Wa, const float* __restrict__ ba,
                                                               const float* __restrict__ Wg, const float* __restrict__ bg,
                                                               const float* __restrict__ w2, const float* __restrict__ c,
                                                               int gated, unsigned char* __restrict__ prep) {
    const GatedPrepLayout L(gated);
    const int NF = gated ? 4 : 2;
    const int blk = blockIdx.x, lane = threadIdx.x;
    const int f = blk % NF, ks = (blk / NF) % gs::kSteps, hw = blk / (NF * gs::kSteps);  // hw = half * 8 + w
    const int term = f & 1, br = f >> 1;
    const float* W = br ? Wg : Wa;
    const int h = 16 * hw + (lane & 15), k0 = 32 * ks + 8 * (lane >> 4);
    bf16x8 o;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        // branch a is pre-scaled by -2 log2(e), branch g by -log2(e): the accumulators then ARE the v_exp_f32 arguments of
        // u = e^{-2x} and v = e^{-y} (see gate_act)
        const float x = W[(size_t)h * gs::kD + k0 + e] * (br ? -kLog2e : -2.f * kLog2e);
        const __bf16 hi = (__bf16)x;
        o[e] = term ? (__bf16)(x - (float)hi) : hi;
    }
    *reinterpret_cast<bf16x8*>(prep + L.wpack + (size_t)blk * 1024 + lane * 16) = o;
    if (blk == 0) {
        float* pba = reinterpret_cast<float*>(prep + L.ba);
        float* pbg = reinterpret_cast<float*>(prep + L.bg);
        float* pw2 = reinterpret_cast<float*>(prep + L.w2);
        for (int i = lane; i < gs::kHid; i += 64) {
            pba[i] = (ba ? ba[i] : 0.f) * (-2.f * kLog2e);
            pbg[i] = ((gated && bg) ? bg[i] : 0.f) * (-kLog2e);
            pw2[i] = w2[i];
        }
        if (lane == 0) reinterpret_cast<float*>(prep + L.c)[0] = c ? c[0] : 0.f;
    }
}

__device__ __forceinline__ f32x4 gs_mfma(bf16x8 a, bf16x8 b, f32x4 c, int, int, int) {
#if VLSA_GS_ABL & 32
    asm volatile("" ::"v"(a), "v"(b));     // operands still have to arrive in registers
    return c;
#else
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
#endif
}
// XF32: fp32 bags (the reference's own feature format, dataset/PatchWSI.py:205-215).  The thread splits its 16 fp32 values of a
// step into bf16 hi + lo on the fly and publishes both images; per accumulator the step then issues X_hi W_hi + X_hi W_lo +
// X_lo W_hi (the lo x lo term is 2^-16 relative and dropped): 1.5x the MFMA work of a bf16 bag, no [N, 256] activations in
// memory, no library GEMM.  (XF32 always takes the two-deep weight ring: 256-register budget.)
// RT = row tiles of 16 patches per workgroup (16; 8 for gated fp32 bags: 64 instead of 128 accumulator registers leave room for
// the fp32 staging registers -- with 16 the kernel spilled).  HG = groups of 16 hidden units per wave: the workgroup has 8 / HG
// waves (HG = 2, RT = 8: the four-wave shape of the ungated module).
// Several bags per launch (the DeepMIL encoder over a batch of slides, runner/vlsa_handler.py:315-345): bags != null, row tile
// t of the launch belongs to the bag b with tile_start[b] <= t < tile_start[b + 1]; its scores go to a_out + a_off[b].
template <bool GATED, bool FULL, bool XF32, int RT = 16, int HG = 1, int NW = 8 / HG>
__global__ __launch_bounds__(64 * NW, 2) void k_gated_scores(const void* __restrict__ Xv, long long N, long long ldx,
                                                       const unsigned char* __restrict__ prep, float* __restrict__ a_out,
                                                       int rows_per_tile, const GsBatch bt) {
    using namespace gs;
    constexpr bool DEEP = FULL && !XF32 && HG == 1;   // four-deep weight ring
    constexpr int AQ = 4 / HG;            // row tiles per group of A fragments (MFMAs on one accumulator stay 4 NB apart)
    // NW waves per workgroup, a wave owns HG groups of 16 hidden units (of both branches): the workgroup covers 16 HG NW of the 256
    // hidden units -- one half (two workgroups per row tile) or all of them (ONE: the X rows are then loaded by one CU only)
    // fp32 bags on a four-wave shape: 128-row images of 8 KB, four of them + the scratch in the 40 KB of the bf16 layout
    constexpr bool XSMALL = XF32 && NW == 4 && RT <= 8;
    constexpr int XIS = XSMALL ? RT * 1024 : kXBuf;       // bytes between the LDS images of a step
    constexpr int HALVES = 16 / (HG * NW);
    static_assert(HALVES == 1 || HALVES == 2, "workgroup covers half or all of the hidden units");
    constexpr int NF = GATED ? 4 : 2;     // weight fragments per step and wave: (branch) x (hi, lo)
    constexpr int NB = GATED ? 2 : 1;     // branches
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int g = lane >> 4, i16 = lane & 15;
    // The two hidden halves of a row tile read the same X rows: blocks b and b + 8 (same XCD under the round-robin dispatch, its L2
    // then serves the second read -- with b, b + 1 they sat on two XCDs and X came out of HBM twice, which, not the MFMA pipe,
    // was what bounded the kernel: without the X loads 400k patches took 115 instead of 208 us).  Speed only: any placement is correct.
    const int bid = blockIdx.x, nfull = (int)(gridDim.x >> 4) << 4;
    const int half = HALVES == 1 ? 0 : bid < nfull ? (bid >> 3) & 1 : bid & 1;
    // rows_per_tile (a multiple of 16, <= 256) is chosen by the host so that the launch is a whole number of full rounds of
    // the 256 CUs: a 50k-patch bag runs as 2 x 241 tiles of 208 rows instead of 2 x 196 tiles of 256 (1.5 rounds rounded up)
    // FULL: 256-row tiles, everything static (large bags); otherwise the row-tile count is a run-time, wave-uniform value
    const int nrt = FULL ? RT : (rows_per_tile >> 4);
    int tile = HALVES == 1 ? bid : bid < nfull ? ((bid >> 4) << 3) + (bid & 7) : bid >> 1;
    unsigned int drop_seed = bt.drop_seed;
    if (bt.bags != nullptr) {
        const int b = bag_of(bt.tile_start, bt.B, tile);
        if (GATED && bt.seed_word != nullptr) drop_seed = bag_drop_seed((unsigned int)*bt.seed_word, b);
        const vlsa_bag_desc bag = bt.bags[b];
        Xv = bag.X;
        N = bag.N;
        ldx = bag.ldx;
        a_out += bt.a_off[b];
        tile -= bt.tile_start[b];
    }
    const long long row0 = (long long)tile * rows_per_tile;
    const int nrows = (int)((N - row0) < rows_per_tile ? (N - row0) : rows_per_tile);
    const GatedPrepLayout L(GATED ? 1 : 0);
    const unsigned int rid0 = bt.row_base + (unsigned int)row0;   // row index inside this bag's score array (dropout counter)

    // plain (compiler-tracked) loads only: weight fragments one step ahead (double-buffered registers; a 4-deep ring measured
    // no faster: the loop is not load-bound), the thread's 32 B of the X chunk two steps ahead in registers and from there
    // into the shared LDS tile of its step
    const unsigned char* wp = prep + L.wpack + (size_t)(half * 8 + HG * w) * kSteps * NF * 1024 + lane * 16;
    // 16-B chunks (8 values) of a step's X chunk per thread (a row has 4); fp32 bags: two, one on the 64-row four-wave shape
    constexpr int XCH = XF32 ? ((NW == 4 && RT == 4) ? 1 : 2) : (RT / NW) > 1 ? (RT / NW) : 1;
    // QUADX (the ungated module's bf16 bags): four lanes share the 64 contiguous bytes of a row (chunk tid & 3), the thread's chunk j
    // sits XRS rows further down -- 16 rows x 64 B per load instruction instead of 32 rows x 2 x 16 B (199 vs 207 us at 400k
    // patches).  Otherwise (fp32 bags; the gated module, whose 256-register budget the second row pointer broke: 64 spilled
    // registers, 671 vs 409 us): 4 / XCH lanes per row, XCH contiguous chunks each.
    constexpr bool QUADX = !XF32 && !GATED;
    constexpr int XRS = QUADX ? 16 * NW : 0, XCS = QUADX ? 0 : 1;      // row / chunk step between the thread's chunks
    const int xr = QUADX ? tid >> 2 : tid / (4 / XCH), xc = QUADX ? tid & 3 : (tid % (4 / XCH)) * XCH;
    // X comes through BUFFER loads whose descriptor ends behind the tile's last row: lanes of rows past the end of the bag get zeros
    // without a memory request and WITHOUT a branch.  A load under `if (row < nrows)` sits in its own basic block; the compiler's
    // s_waitcnt bookkeeping then counts it as "maybe not issued", and every wait for an OLDER load (the weights of this step, the X
    // chunk to publish) also drained the X loads issued a moment before: vmcnt(1) / vmcnt(0) at the end of every step instead of
    // vmcnt(7) / vmcnt(6) -- the ring depths were fiction.  (Clamping the row instead made all 512 threads of a 16-row tile load.)
    // Where it pays is where PEEL (below) does; the gated static and fp32 kernels measured 2-5 % slower with buffer loads, the
    // ungated module's small bags (run-time tile heights of 16-48 rows) 0.7-1.5 us per bag: those keep flat loads under the row
    // predicate.
    constexpr bool XBUF = GATED ? (XF32 ? (NW == 4 && FULL) : (!FULL || NW == 4)) : FULL;
    const bool xok = xr < nrows;
    const __bf16* xsrc = (XBUF || XF32) ? nullptr : static_cast<const __bf16*>(Xv) + (row0 + xr) * ldx + xc * 8;          // + 32 ks; QUADX: + j XRS ldx
    const float* xsrc32 = (!XBUF && XF32) ? static_cast<const float*>(Xv) + (row0 + xr) * ldx + xc * 8 : nullptr;
    constexpr int XESZ = XF32 ? 4 : 2;
    const unsigned long long xbase = reinterpret_cast<unsigned long long>(Xv) + (unsigned long long)row0 * ldx * XESZ;
    const __amdgpu_buffer_rsrc_t xrs = __builtin_amdgcn_make_buffer_rsrc(
        reinterpret_cast<void*>((static_cast<unsigned long long>((unsigned)__builtin_amdgcn_readfirstlane((int)(xbase >> 32))) << 32) |
                                (unsigned)__builtin_amdgcn_readfirstlane((int)xbase)),
        0, __builtin_amdgcn_readfirstlane((int)(((long long)(nrows - 1) * ldx + kD) * XESZ)), 0x00020000);
    const int xvoff = (int)((long long)xr * ldx + xc * 8) * XESZ;                    // + 64 (128: fp32) per K step
    const int xrs_step = __builtin_amdgcn_readfirstlane((int)((long long)XRS * ldx * XESZ));   // QUADX: the thread's second row
    // 16-B chunk c of row r is stored at position c ^ f(r), f(r) = (-(r >> 2)) & 3: ds_read_b128 is serviced in the lane groups
    // {0-3, 12-15, 20-27}, {4-11, 16-19, 28-31}, ... (MI355X_MICROARCH.md, LDS), and with this f the 16 lanes of every
    // group hit 16 different 4-bank sets
    const int fx = (0 - (xr >> 2)) & 3;
    const int x_dst0 = xr * 64 + ((xc ^ fx) << 4), x_dst1 = xr * 64 + (((xc + 1) ^ fx) << 4);   // chunk j: xr * 64 + (((xc + j) ^ fx) << 4)
    const int a_off = i16 * 64 + ((g ^ ((0 - (i16 >> 2)) & 3)) << 4);    // A fragment of row tile rt: + rt * 1024
    // the thread's 16 values of a step: two 16-byte bf16 chunks c0, c1 (bf16 bags), or four float4 (fp32 bags)
    struct XPair { bf16x8 c[XF32 ? 1 : XCH]; f32x4 f[XF32 ? 2 * XCH : 1]; };
    auto load_x = [&](int ks) -> XPair {
        XPair r = {};
        if constexpr (!XBUF) {
            if constexpr (QUADX) {
#pragma unroll
                for (int j = 0; j < XCH; ++j)
                    if (xr + j * XRS < nrows) r.c[j] = *reinterpret_cast<const bf16x8*>(xsrc + (long long)j * XRS * ldx + 32 * ks);
            } else if (xok) {
                if constexpr (XF32) {
#pragma unroll
                    for (int q = 0; q < 2 * XCH; ++q) r.f[q] = *reinterpret_cast<const f32x4*>(xsrc32 + 32 * ks + 4 * q);
                } else {
#pragma unroll
                    for (int j = 0; j < XCH; ++j) r.c[j] = *reinterpret_cast<const bf16x8*>(xsrc + 32 * ks + 8 * j);
                }
            }
        } else if constexpr (XF32) {
#pragma unroll
            for (int q = 0; q < 2 * XCH; ++q)
                r.f[q] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(xrs, xvoff, 128 * ks + 16 * q, 0));
        } else if (!(VLSA_GS_ABL & (4 | 64))) {
#pragma unroll
            for (int j = 0; j < XCH; ++j)
                r.c[j] = __builtin_bit_cast(bf16x8, __builtin_amdgcn_raw_buffer_load_b128(xrs, xvoff + (QUADX ? j * xrs_step : 0), 64 * ks + (QUADX ? 0 : 16 * j), 0));   // (the range check sees the VGPR offset: the row goes there)
        }
        return r;
    };
    auto load_b = [&](int ks, bf16x8 (&dst)[HG * NF]) {
        if ((VLSA_GS_ABL & 2) && ks > 1) return;
#pragma unroll
        for (int hg = 0; hg < HG; ++hg)
#pragma unroll
            for (int f = 0; f < NF; ++f)
                dst[hg * NF + f] = *reinterpret_cast<const bf16x8*>(wp + (size_t)((hg * kSteps + ks) * NF + f) * 1024);
    };

    // accumulators start at the (pre-scaled) bias of the lane's hidden unit
    const int h0 = 128 * half + 16 * HG * w + i16;   // hidden unit of group hg: h0 + 16 hg
    float w2v[HG];
    f32x4 acc[RT][HG][NB];
#pragma unroll
    for (int hg = 0; hg < HG; ++hg) {
        const float bav = reinterpret_cast<const float*>(prep + L.ba)[h0 + 16 * hg];
        const float bgv = GATED ? reinterpret_cast<const float*>(prep + L.bg)[h0 + 16 * hg] : 0.f;
        w2v[hg] = reinterpret_cast<const float*>(prep + L.w2)[h0 + 16 * hg];
#pragma unroll
        for (int rt = 0; rt < RT; ++rt)
#pragma unroll
            for (int b = 0; b < NB; ++b) {
                const float bb = b == 0 ? bav : bgv;
                acc[rt][hg][b] = f32x4{bb, bb, bb, bb};
            }
    }

    bf16x8 B0[HG * NF], B1[HG * NF], B2[DEEP ? NF : 1], B3[DEEP ? NF : 1];   // FULL: 4-deep ring, weights three steps ahead; else B0 / B1, one step ahead
    XPair X0, X1;
    X0 = load_x(0);
    load_b(0, B0);
    X1 = load_x(1);
    if constexpr (DEEP) {
        load_b(1, B1);
        load_b(2, B2);
    }

    bf16x8 abl_a[AQ] = {};
    // one K step: publish this step's X share, barrier, start the loads of later steps, 16 A reads, 64 (32) MFMAs
    // `body` (a literal): this is a step of the loop body, where every later step exists -- its loads are unconditional.  The last
    // four steps are a second copy with literal step numbers, so that no load of the loop sits behind a branch (see xrc above).
    auto step = [&](int s, const bool body, bf16x8 (&cur)[HG * NF], bf16x8 (&nxt)[HG * NF], XPair& xcur) {
        unsigned char* xb = smem + kXOff + (s & 1) * (XF32 ? 2 : 1) * XIS;     // fp32 bags: hi image, lo image behind it
        if constexpr (XF32) {
#pragma unroll
            for (int j = 0; j < XCH; ++j) {
                bf16x8 h, l;
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    const float v = xcur.f[2 * j + (e >> 2)][e & 3];
                    const __bf16 a = (__bf16)v;
                    h[e] = a;
                    l[e] = (__bf16)(v - (float)a);
                }
                *reinterpret_cast<bf16x8_ma*>(xb + (j ? x_dst1 : x_dst0)) = h;
                *reinterpret_cast<bf16x8_ma*>(xb + XIS + (j ? x_dst1 : x_dst0)) = l;
            }
        } else if (!(VLSA_GS_ABL & (4 | 128)) || s < 2) {
#pragma unroll
            for (int j = 0; j < XCH; ++j) *reinterpret_cast<bf16x8_ma*>(xb + (xr + j * XRS) * 64 + (((xc + j * XCS) ^ fx) << 4)) = xcur.c[j];
        } else if (VLSA_GS_ABL & 128) {
#pragma unroll
            for (int j = 0; j < XCH; ++j) asm volatile("" ::"v"(xcur.c[j]));
        }
        if (!(VLSA_GS_ABL & 8) || s < 2) __syncthreads();                     // X(s) published by every wave; everyone is done reading buffer (s + 1) & 1
        if (body || s + (DEEP ? 3 : 1) < kSteps) load_b(s + (DEEP ? 3 : 1), nxt);
        if (body || s + 2 < kSteps) xcur = load_x(s + 2);
        if constexpr (!GATED && FULL) __builtin_amdgcn_sched_barrier(0);   // the loads stay HERE, in front of the step's MFMAs (the scheduler sank them to its end)
#pragma unroll
        for (int q = 0; q < RT / AQ; ++q) {
            if (AQ * q >= nrt) break;         // uniform
            bf16x8 A[AQ], AL[XF32 ? AQ : 1];
#pragma unroll
            for (int r4 = 0; r4 < AQ; ++r4) {
                if ((VLSA_GS_ABL & 1) && (s > 0 || q > 0)) { A[r4] = abl_a[r4]; continue; }
                A[r4] = *reinterpret_cast<const bf16x8_ma*>(xb + (AQ * q + r4) * 1024 + a_off);
                if (VLSA_GS_ABL & 1) abl_a[r4] = A[r4];
                if constexpr (XF32) AL[r4] = *reinterpret_cast<const bf16x8_ma*>(xb + XIS + (AQ * q + r4) * 1024 + a_off);
            }
            if (AQ * q + AQ <= nrt) {
                // hi terms of the 4 NB accumulators of this group, then the lo terms: MFMAs on one accumulator are 4 NB apart
#pragma unroll
                for (int term = 0; term < 2; ++term)
#pragma unroll
                    for (int hg = 0; hg < HG; ++hg)
#pragma unroll
                        for (int r4 = 0; r4 < AQ; ++r4)
#pragma unroll
                            for (int b = 0; b < NB; ++b)
                                acc[AQ * q + r4][hg][b] = gs_mfma(A[r4], cur[hg * NF + 2 * b + term], acc[AQ * q + r4][hg][b], 0, 0, 0);
                if constexpr (XF32) {
#pragma unroll
                    for (int hg = 0; hg < HG; ++hg)
#pragma unroll
                        for (int r4 = 0; r4 < AQ; ++r4)
#pragma unroll
                            for (int b = 0; b < NB; ++b)
                                acc[AQ * q + r4][hg][b] = gs_mfma(AL[r4], cur[hg * NF + 2 * b], acc[AQ * q + r4][hg][b], 0, 0, 0);
                }
            } else {                          // the last, partly filled group of row tiles
#pragma unroll
                for (int r4 = 0; r4 < AQ - 1; ++r4)
                    if (AQ * q + r4 < nrt) {
#pragma unroll
                        for (int hg = 0; hg < HG; ++hg)
#pragma unroll
                        for (int b = 0; b < NB; ++b) {
                            acc[AQ * q + r4][hg][b] = gs_mfma(A[r4], cur[hg * NF + 2 * b], acc[AQ * q + r4][hg][b], 0, 0, 0);
                            acc[AQ * q + r4][hg][b] = gs_mfma(A[r4], cur[hg * NF + 2 * b + 1], acc[AQ * q + r4][hg][b], 0, 0, 0);
                            if constexpr (XF32)
                                acc[AQ * q + r4][hg][b] = gs_mfma(AL[r4], cur[hg * NF + 2 * b], acc[AQ * q + r4][hg][b], 0, 0, 0);
                        }
                    }
            }
        }
    };
    // Where buffer loads + the second copy pay (same box, tools/kbench_gated_ab.py, profiles/r03_kbench_gated_ab2.txt): the ungated
    // static kernels (bf16 400k patches 205 -> 192 us; fp32 50k 69.6 -> 61) and the gated run-time-height kernel (bf16 20k 31.8 ->
    // 29.3, 50k 70.8 -> 67.6 through its remainder launch).  Not: the gated static kernel (256 registers: the copy made it spill,
    // 460 vs 432 us at 400k), the ungated run-time-height kernel (bags below one round: + 0.7-1.5 us per bag), the gated fp32
    // kernels (+ 1-5 %) -- those keep flat loads and the one loop with uniform branches around the last steps' loads.
    constexpr bool PEEL = XBUF;
#pragma unroll 1
    for (int s = 0; s < (PEEL ? kSteps - 4 : kSteps); s += 4) {
        if constexpr (DEEP) {
            step(s, PEEL, B0, B3, X0);
            step(s + 1, PEEL, B1, B0, X1);
            step(s + 2, PEEL, B2, B1, X0);
            step(s + 3, PEEL, B3, B2, X1);
        } else {
            step(s, PEEL, B0, B1, X0);
            step(s + 1, PEEL, B1, B0, X1);
            step(s + 2, PEEL, B0, B1, X0);
            step(s + 3, PEEL, B1, B0, X1);
        }
    }
    if constexpr (!PEEL) {
    } else if constexpr (DEEP) {
        step(kSteps - 4, false, B0, B3, X0);
        step(kSteps - 3, false, B1, B0, X1);
        step(kSteps - 2, false, B2, B1, X0);
        step(kSteps - 1, false, B3, B2, X1);
    } else {
        step(kSteps - 4, false, B0, B1, X0);
        step(kSteps - 3, false, B1, B0, X1);
        step(kSteps - 2, false, B0, B1, X0);
        step(kSteps - 1, false, B1, B0, X1);
    }

    // ---- epilogue: activations, gate, w2, sum over this wave's 16 hidden units, then over the 8 waves, then (atomically) over
    // the two workgroups that share the row tile
    float_ma* scr = reinterpret_cast<float_ma*>(smem + ((XF32 && !XSMALL) ? kScrOff32 : kScrOff));
#pragma unroll
    for (int rt = 0; rt < RT; ++rt)
        if (rt < nrt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            float ew = 0.f;
#pragma unroll
            for (int hg = 0; hg < HG; ++hg) {
                float e = (VLSA_GS_ABL & 16) ? acc[rt][hg][0][r] + acc[rt][hg][NB - 1][r]
                          : GATED ? gate_act(acc[rt][hg][0][r], acc[rt][hg][NB - 1][r]) : tanh_act(acc[rt][hg][0][r]);
                if (GATED && bt.drop_thr != 0u) {      // uniform: training-mode dropout on both branches
                    const unsigned int row = rid0 + 16 * rt + 4 * g + r, h = (unsigned int)(h0 + 16 * hg);
                    const bool ka = dropout_bits(drop_seed, row, h) >= bt.drop_thr;
                    const bool kg = dropout_bits(drop_seed, row, h + 256u) >= bt.drop_thr;
                    e = (ka && kg) ? e * bt.drop_scale * bt.drop_scale : 0.f;
                }
                ew += e * w2v[hg];
            }
            const float v = row16_sum(ew);
            if (i16 == 0) scr[w * kRows + 16 * rt + 4 * g + r] = v;
        }
    __syncthreads();
    if (tid < kRows && tid < nrows) {
        float sum = half == 0 ? reinterpret_cast<const float*>(prep + L.c)[0] : 0.f;
#pragma unroll
        for (int ww = 0; ww < NW; ++ww) sum += scr[ww * kRows + tid];
        atomicAdd(a_out + row0 + tid, sum);     // two addends per element on a zeroed array: order-independent
    }
}


// (Round 4's whole-row variant k_gated_scores_rows -- 128 x 128 tiles, X staged as whole rows in LDS -- measured no faster than
// k_gated_scores (profiles/r04_kbench_gated_rows.txt) and left the library in round 6: docs/LAB_NOTEBOOK.md, `git log -S k_gated_scores_rows`.)
}  // namespace vlsa

using namespace vlsa;

extern "C" size_t vlsa_gated_prep_bytes(int gated) { return GatedPrepLayout(gated ? 1 : 0).total; }

extern "C" int vlsa_prepare_gated_weights(const float* Wa, const float* ba, const float* Wg, const float* bg, const float* w2,
                                          const float* c, int dim_in, int dim_hid, int gated, void* prep, void* stream) {
    if (!Wa || !w2 || !prep || (gated && !Wg)) return VLSA_EINVAL;
    if (dim_in != gs::kD || dim_hid != gs::kHid) return VLSA_EUNSUPPORTED;
    const int NF = gated ? 4 : 2;
    hipLaunchKernelGGL(k_prepare_gated_weights, dim3(gs::kHalves * 8 * gs::kSteps * NF), dim3(64), 0, (hipStream_t)stream, Wa, ba, Wg, bg, w2, c,
                       gated ? 1 : 0, static_cast<unsigned char*>(prep));
    if (launch_status() != VLSA_OK) return VLSA_ELAUNCH;
    return gs_tile_prepare(Wa, Wg, gated, static_cast<unsigned char*>(prep), (hipStream_t)stream);
}

// Which plain score launches of bf16 bags take k_scores_tile_p (gated_scores_tile.hip).  Size sweep, both kernels on one box, 16 bags in
// rotation (profiles/r05_gs_sweep.txt; us, tile kernel / fragment-order kernel):
//   gated:   12k 21.0 / 18.8, 16 384: 23.3 / 20.9, 20k 25.8 / 28.0, 28k 32.0 / 37.5, 32 768: 34.6 / 40.0, 40k 45.8 / 45.4, 50k 52.3 / 57.9,
//            70k 71 / 74.5, 100k 97 / 105, 200k 177 / 196, 400k 343.5 / 383.5                                  -> from 18 432 rows on;
//   ungated: 16 384: 16.6 / 16.4, 20k 17.7 / 20.4, 28k 22.3 / 24.2, 32 768: 23.8 / 22.5, 40k 26.5 / 28.4, 50k 29.9 / 33.0, 60k 33.0 / 37.5,
//            70k 44.3 / 41.7, 100k 53.2 / 55.5, 200k 101.6 / 99.6, 400k 191 / 189  -> 18 432 .. 65 536 rows (one round of its 256 walkers).
// VLSA_GS_TILE = <rows>: from that many rows on, both modules; 0: never.
static long long gs_tile_env() {
    static const long long env = [] { const char* e = VLSA_ENV("VLSA_GS_TILE"); return e ? atoll(e) : -1ll; }();
    return env;
}
static bool gs_tile_use(bool gated, long long N) {
    const long long env = gs_tile_env();
    if (env == 0) return false;
    if (env > 0) return N >= env;
    return gated ? N >= 18432 : (N >= 18432 && N <= 65536);
}
// rows of a batch (or a bag) from which scores + pooling in ONE launch of that kernel beat two launches: every size, both modules
// -- below ~16k rows the two-launch route is bound by its host work and its launches, not by either kernel (one 2 798-patch bag: 29.6 vs
// 40.6 us gated, 20.4 vs 35.3 ungated; a batch of 4: 47 vs 51 / 36 vs 51 us per call; profiles/r05_kbench_pool_small.txt).
// VLSA_GS_TILE = <rows> also moves this threshold (0: never).
static long long gs_tile_min_rows_pooled() {
    const long long env = gs_tile_env();
    return env == 0 ? (1ll << 62) : env > 0 ? env : 1;
}

static bool gs_round64() {
    static const bool on = [] { const char* e = VLSA_ENV("VLSA_GS_R64"); return e && atoi(e) == 1; }();   // (A/B hook; off: +-2 us either way, tools/gs_rows.py)
    return on;
}

// Workgroup shape per (bag dtype, module): rows of the largest tile, row tiles in one round of the 256 CUs, workgroups per row
// tile (hidden halves) and whether a four-wave kernel serves it.
//   * gated, bf16:   four waves x 64 rows (below; VLSA_GS_G4=0: 256 rows x 128 hidden units of both branches, 8 waves, one
//     workgroup per CU -- the shape of rounds 1-2);
//   * gated, fp32:   four waves x 64 rows as for bf16 (VLSA_GS_F4=0: 8 waves x 128 rows);
//   * ungated, bf16: FOUR waves, 128 rows.  Shape 1: 128 hidden units per workgroup, 32 per wave (HG = 2): every A fragment read
//     from LDS feeds four MFMAs instead of two, 150 registers -> three independent workgroups per CU whose prologues / epilogues
//     overlap the others' K loops: 400k patches 251 -> 199 us, 20k: 21.4 -> 19.5 (same box, tools/kbench_gated_ab.py).  Shape 2: all
//     256 hidden units, 64 per wave (HG = 4), two workgroups per CU, X loaded by ONE workgroup: one round holds 65 536 rows instead
//     of 49 152 -- faster only for bags of 32k..64k rows (50k: 32.3 vs 36.6 us, 65 536: 38.4 vs 41.0; 70k: 50 vs 43), which is
//     where it is used.  For the gated module 128 x 128 four-wave tiles need 256 registers (473 vs 430 us at 400k), a 256 x 128 tile at
//     one wave per SIMD and 512 registers 584; 64-row tiles lost at 182 registers (447 vs 418) and won once they fit three per CU.
// What bounds the loop -- timing-only ablations (VLSA_GS_ABL, tools/attic/gs_ablate.sh), compared in SHADER CYCLES (GRBM_GUI_ACTIVE,
// tools/attic/pmc_gs_variants.sh): wall time misleads here, the clock follows the data (zeroed X operands: 2.33 instead of 1.96 GHz).
// Ungated shape 1, 400k patches: 375k cycles per XCD, of which the MFMAs need 200k (53 % busy).  Without the MFMAs the rest of the
// loop still takes 347k: the kernel is bound by its vector-memory path, not by the matrix pipe.  On that MFMA-less loop: no X loads
// 156k, no weight loads 265k, no A-fragment reads 346k, no activations 344k, no barrier 392k -- per round of three workgroups' steps
// (1 536 MFMA cycles per SIMD) the 24 KB of X cost ~1 470 cycles (16 B/clk/CU: the per-CU miss path) and the 48 KB of weights ~630
// (L2 hits at the L1's 64 B/clk).  What did NOT change it: X four steps ahead (207 vs 207 us), weights AND X four steps ahead at two
// workgroups per CU (228 vs 227), double-buffered A fragments (211 vs 213), the publication pinned behind the MFMAs (198 vs 198),
// full 128-byte lines per row and step pair with half the barriers (399k vs 377k cycles), DRAM-page-friendly addresses (403k vs
// 394k); non-temporal X loads cost 17 % (the second half of every line comes from the L2).  What is left is the byte budget: a
// 128-row x 128-unit workgroup tile needs 8 KB of X and 16 KB of weights per 512 MFMA cycles and wave.
struct GsTiling { int max_rows, round_tiles; bool four_waves; int halves; };
static GsTiling gs_tiling(bool f32, bool gated, int64_t n_hint) {
    static const int shape = [] { const char* e = VLSA_ENV("VLSA_GS_HG2"); return e ? atoi(e) : -1; }();   // (A/B hook: 0 / 1 / 2)
    if (!f32 && !gated && shape != 0) {
        const bool all_hidden = shape == 2 || (shape < 0 && n_hint > 32768 && n_hint <= 65536);
        if (all_hidden) return {128, 512, true, 1};
        return {128, 256, true, 2};
    }
    static const bool g4 = [] { const char* e = VLSA_ENV("VLSA_GS_G4"); return !(e && atoi(e) == 0); }();   // (A/B hook)
    // gated, bf16: four waves x 64 rows x 128 hidden units of both branches (HG = 2): 154 registers -> three workgroups per CU, as
    // for the ungated module (it took the leaner buffer loads to get under 168 registers; with 182 the shape lost, 447 vs 418 us).
    // 400k patches 429 -> 379 us, 50k 63.8 -> 56.8, 24 576 33.4 -> 30.0 (same box).  A workgroup streams its 512 KB of weights
    // whatever its tile height, so small bags keep 64-row tiles too (10k patches: 17.1 us with 64 rows, 21.4 with 32); the
    // "round" reported to the batch caller is 64 tiles for that reason.
    if (!f32 && gated && g4) return {64, 64, true, 2};
    // fp32 bags: the same two shapes (LDS images of RT KB; 164 registers): ungated 50k patches 62.4 -> 52.0 us, gated 105.7 -> 81.5
    static const bool f4 = [] { const char* e = VLSA_ENV("VLSA_GS_F4"); return !(e && atoi(e) == 0); }();   // (A/B hook)
    if (f32 && !gated && f4) return {128, 256, true, 2};
    if (f32 && gated && f4) return {64, 64, true, 2};
    return {(f32 && gated) ? 128 : gs::kRows, 128, false, 2};
}

// Rows per tile of the persistent LDS-DMA kernel (gated_scores_tile.hip) and the total number of rows from which a batched launch
// should use it -- 0 / 0 where it does not apply (fp32 bags).
extern "C" int vlsa_gated_scores_big_tile(int x_dtype, int gated, int* rows, int64_t* min_total_rows) {
    if ((x_dtype != VLSA_DT_BF16 && x_dtype != VLSA_DT_F32) || !rows || !min_total_rows) return VLSA_EINVAL;
    // (this answer steers the batched / pooled routes: both modules; plain score launches: gs_tile_use)
    const long long mn = gs_tile_min_rows_pooled();
    const bool on = x_dtype == VLSA_DT_BF16 && mn < (1ll << 61);       // (VLSA_GS_TILE=0 switches the kernel off)
    *rows = on ? 256 : 0;
    *min_total_rows = on ? mn : 0;
    return VLSA_OK;
}

// vlsa_gated_scores_batch's caller sizes its tile table with this: rows of the largest tile and row tiles per round.
extern "C" int vlsa_gated_scores_tiling(int x_dtype, int gated, int* max_rows, int* round_tiles) {
    if ((x_dtype != VLSA_DT_BF16 && x_dtype != VLSA_DT_F32) || !max_rows || !round_tiles) return VLSA_EINVAL;
    const GsTiling tl = gs_tiling(x_dtype == VLSA_DT_F32, gated != 0, 0);
    *max_rows = tl.max_rows;
    *round_tiles = tl.round_tiles;
    return VLSA_OK;
}

// The one place that maps (tiling, bag dtype, module, whole tiles) to an instantiation of k_gated_scores and launches it: the single-bag
// segments and the batched launch differ in the arguments they built (X / N / ldx or a bag table in `bt`), not in the kernel.
// tiles = row tiles x tl.halves.  full: rows_per_tile is the shape's max_rows (the kernel's static tile height), otherwise the kernel
// takes the height at run time.  LDS: the images of the four-wave shapes fit gs::kLds for either dtype, the 8-wave fp32 shapes need
// gs::kLds32.  (The arms stand in the order the kernels have always been instantiated in, which is their order in the code object.)
struct GsCall {
    unsigned int tiles;
    hipStream_t st;
    const void* X;
    long long N, ldx;
    const unsigned char* prep;
    float* a;
    int rows_per_tile;
    GsBatch bt;
};
template <bool GATED, bool FULL, bool XF32, int RT, int HG, int NW>
static void gs_go(const GsCall& c) {
    launch_lds<k_gated_scores<GATED, FULL, XF32, RT, HG, NW>>(dim3(c.tiles), dim3(64 * NW), XF32 && NW == 8 ? gs::kLds32 : gs::kLds, c.st, c.X,
                                                               c.N, c.ldx, c.prep, c.a, c.rows_per_tile, c.bt);
}
static void gs_launch(const GsTiling& tl, bool f32, bool gated, bool full, const GsCall& c) {
#define VLSA_GS(G, X32, RT, HG, NW) do { if (full) gs_go<G, true, X32, RT, HG, NW>(c); else gs_go<G, false, X32, RT, HG, NW>(c); } while (0)
    if (!tl.four_waves) {       // the 8-wave shapes of rounds 1-2: behind the VLSA_GS_G4 / VLSA_GS_F4 / VLSA_GS_HG2 hooks (-DVLSA_EXPERIMENT) only
        if (!f32) { if (gated) VLSA_GS(true, false, 16, 1, 8); else VLSA_GS(false, false, 16, 1, 8); }
        else      { if (gated) VLSA_GS(true, true, 8, 1, 8); else VLSA_GS(false, true, 16, 1, 8); }
    } else if (f32) {
        if (gated) VLSA_GS(true, true, 4, 2, 4); else VLSA_GS(false, true, 8, 2, 4);
    } else if (gated) {
        VLSA_GS(true, false, 4, 2, 4);
    } else if (tl.halves == 1) {
        gs_go<false, false, false, 8, 4, 4>(c);      // all 256 hidden units per workgroup: run-time tile height only
    } else {
        VLSA_GS(false, false, 8, 2, 4);
    }
#undef VLSA_GS
}

static int gated_scores_impl(const void* X, int x_dtype, int64_t N, int64_t ldx, int D, const void* prep, int gated, float* a,
                             float drop_p, unsigned int seed, void* stream) {
    if (!X || !prep || !a || N < 1 || ldx < D) return VLSA_EINVAL;
    if (D != gs::kD || (x_dtype != VLSA_DT_BF16 && x_dtype != VLSA_DT_F32)) return VLSA_EUNSUPPORTED;
    const bool f32 = x_dtype == VLSA_DT_F32;
    const long long esz = f32 ? 4 : 2;
    if ((reinterpret_cast<uintptr_t>(X) & 15) || ((ldx * esz) % 16) || ldx * esz * gs::kRows >= (1ll << 31)) return VLSA_EINVAL;
    // Rows per tile.  One round of the 256 CUs covers 2 halves x 128 tiles.  A bag that fits one round (N <= 128 tiles of the
    // largest height) uses the smallest multiple of 16 rows that still fits it (a 2 798-patch bag runs as 2 x 88 tiles of 32
    // rows instead of 2 x 11 of 256).  A larger bag is covered by TWO launches: whole rounds of the static 256-row kernel
    // (every CU busy, every tile full), then the remainder as one more single-round launch with its own, smaller tile height --
    // instead of a last round in which 256-row tiles occupy a fraction of the CUs for a full tile time (50k patches: 1.53
    // rounds were paid as 2).
    const GsTiling tl = gs_tiling(f32, gated != 0, N);
    const int max_rows = tl.max_rows, round_tiles = tl.round_tiles;
    hipStream_t st = (hipStream_t)stream;
    const unsigned char* pp = static_cast<const unsigned char*>(prep);
    GsBatch dropb{nullptr, nullptr, nullptr, 0, 0u, 0u, 1.f, 0u};
    if (gated && drop_p > 0.f) {
        DropSpec ds;
        if (!drop_spec(drop_p, &ds)) return VLSA_EINVAL;
        dropb.drop_thr = ds.thr;
        dropb.drop_seed = seed;
        dropb.drop_scale = ds.scale;
    }
    // round 5: large bf16 bags take the LDS-DMA tile kernel (gated_scores_tile.hip)
    if (!f32 && gs_tile_use(gated != 0, (long long)N) && 256ll * ldx * 2 < (1ll << 31)) {
        // the ungated module's tiles are whole (one workgroup per row tile stores its scores): nothing to zero
        if (gated && hipMemsetAsync(a, 0, (size_t)N * sizeof(float), st) != hipSuccess) return VLSA_ELAUNCH;
        return gs_tile_launch(X, (long long)N, (long long)ldx, pp, gated, a, 0, 0, dropb, nullptr, nullptr, st);
    }
    if (hipMemsetAsync(a, 0, (size_t)N * sizeof(float), st) != hipSuccess) return VLSA_ELAUNCH;
    const int64_t round_rows = round_tiles * (int64_t)max_rows;
    static const bool split = [] { const char* e = VLSA_ENV("VLSA_GS_SPLIT"); return !(e && atoi(e) == 0); }();   // (A/B hook)
    int64_t seg_rows[2] = {N, 0};
    // (four-wave workgroups: three fit a CU and run out of step with each other, a partly filled last round costs little and a
    // second launch more -- 50k patches: 37.8 us as one launch of 128-row tiles, 41.5 split; tools/gs_rows_sweep.py)
    if (split && !tl.four_waves && N > round_rows && N % round_rows != 0) {
        seg_rows[0] = N / round_rows * round_rows;
        seg_rows[1] = N - seg_rows[0];
    }
    int64_t off = 0;
    for (int sgi = 0; sgi < 2 && seg_rows[sgi] > 0; ++sgi) {
        const int64_t n = seg_rows[sgi];
        int rows_per_tile = max_rows;
        if (gated && tl.four_waves) {
            rows_per_tile = n > 4096 ? 64 : n > 1024 ? 32 : 16;
        } else if (n <= round_rows) {
            rows_per_tile = (int)(((n + round_tiles - 1) / round_tiles + 15) / 16 * 16);
            // (optional: whole groups of four 16-row tiles above 64 rows -- helps 30k / 60k patches, hurts 10k / 20k / 50k)
            if (rows_per_tile > 64 && gs_round64()) rows_per_tile = (rows_per_tile + 63) / 64 * 64;
            if (rows_per_tile > max_rows) rows_per_tile = max_rows;
        }
        if (const char* e = VLSA_ENV("VLSA_GS_ROWS")) {          // experiment hook (tools/gs_rows.py): force the tile height
            const int v = atoi(e);
            if (v >= 16 && v <= max_rows && v % 16 == 0) rows_per_tile = v;
        }
        const bool full = rows_per_tile == max_rows;
        const unsigned int tiles = (unsigned int)((n + rows_per_tile - 1) / rows_per_tile) * tl.halves;  // (row tile, hidden half)
        const void* Xs = static_cast<const unsigned char*>(X) + off * ldx * esz;
        float* as = a + off;
        dropb.row_base = (unsigned int)off;
        gs_launch(tl, f32, gated != 0, full, GsCall{tiles, st, Xs, (long long)n, (long long)ldx, pp, as, rows_per_tile, dropb});
        off += n;
    }
    return launch_status();
}

extern "C" int vlsa_gated_scores(const void* X, int x_dtype, int64_t N, int64_t ldx, int D, const void* prep, int gated, float* a,
                                 void* stream) {
    return gated_scores_impl(X, x_dtype, N, ldx, D, prep, gated, a, 0.f, 0u, stream);
}

// Training-mode forward of Gated_Attention_Pooling's scores: dropout with probability drop_p behind tanh and behind sigmoid
// (model/layers.py:94,99), masks from the counter-based generator dropout_bits(seed, row, unit) that vlsa_attn_scores_backward
// re-evaluates.  drop_p = 0 (or gated = 0: Attention_Pooling has no dropout) is vlsa_gated_scores.
extern "C" int vlsa_gated_scores_train(const void* X, int x_dtype, int64_t N, int64_t ldx, int D, const void* prep, int gated, float* a,
                                       float drop_p, unsigned int seed, void* stream) {
    return gated_scores_impl(X, x_dtype, N, ldx, D, prep, gated, a, drop_p, seed, stream);
}

// B bags in ONE launch.  bag_desc: device table of vlsa_bag_desc {X, N, ldx}; tile_start [B + 1] (device, int32): first row tile
// of every bag for tiles of `rows_per_tile` rows (a multiple of 16, <= 256; <= 128 for gated fp32 bags), n_tiles = tile_start[B];
// a: one buffer holding all bags' scores, bag b at a + a_off[b] (device, int64), a_floats = its length (zeroed here).
static int gated_scores_batch_impl(const void* bag_desc, int B, int x_dtype, int D, const void* prep, int gated,
                                   const int* tile_start, int n_tiles, int rows_per_tile, float* a, const int64_t* a_off,
                                   int64_t a_floats, float drop_p, const int64_t* seed_word, void* stream) {
    if (!bag_table_ok(bag_desc, B, tile_start, n_tiles) || !prep || !a || !a_off || a_floats < 1) return VLSA_EINVAL;
    if (D != gs::kD || (x_dtype != VLSA_DT_BF16 && x_dtype != VLSA_DT_F32)) return VLSA_EUNSUPPORTED;
    GsBatch bt{static_cast<const vlsa_bag_desc*>(bag_desc), tile_start, reinterpret_cast<const long long*>(a_off), B, 0u, 0u, 1.f, 0u, nullptr};
    if (gated && drop_p > 0.f) {     // the seed comes from the device word
        DropSpec ds;
        if (!drop_spec(drop_p, &ds) || !seed_word) return VLSA_EINVAL;
        bt.drop_thr = ds.thr;
        bt.drop_scale = ds.scale;
        bt.seed_word = reinterpret_cast<const long long*>(seed_word);
    }
    const bool f32 = x_dtype == VLSA_DT_F32;
    const GsTiling tl = gs_tiling(f32, gated != 0, 0);
    const int max_rows = tl.max_rows;
    if (!f32 && rows_per_tile > max_rows && rows_per_tile <= 256 && (rows_per_tile % 32) == 0) {
        // tiles higher than the fragment-order kernel's: the persistent LDS-DMA kernel (vlsa_gated_scores_big_tile)
        hipStream_t st = (hipStream_t)stream;
        if (gated && hipMemsetAsync(a, 0, (size_t)a_floats * sizeof(float), st) != hipSuccess) return VLSA_ELAUNCH;
        return gs_tile_launch(nullptr, 0ll, 0ll, static_cast<const unsigned char*>(prep), gated, a, n_tiles, rows_per_tile, bt, nullptr, nullptr, st);
    }
    if (rows_per_tile < 16 || rows_per_tile > max_rows || (rows_per_tile % 16)) return VLSA_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(a, 0, (size_t)a_floats * sizeof(float), st) != hipSuccess) return VLSA_ELAUNCH;
    gs_launch(tl, f32, gated != 0, rows_per_tile == max_rows,
              GsCall{(unsigned int)n_tiles * tl.halves, st, nullptr, 0ll, 0ll, static_cast<const unsigned char*>(prep), a, rows_per_tile, bt});
    return launch_status();
}

extern "C" int vlsa_gated_scores_batch(const void* bag_desc, int B, int x_dtype, int D, const void* prep, int gated,
                                       const int* tile_start, int n_tiles, int rows_per_tile, float* a, const int64_t* a_off,
                                       int64_t a_floats, void* stream) {
    return gated_scores_batch_impl(bag_desc, B, x_dtype, D, prep, gated, tile_start, n_tiles, rows_per_tile, a, a_off, a_floats, 0.f,
                                   nullptr, stream);
}

// Training-mode forward of vlsa_gated_scores_batch: the gated module's dropout (probability drop_p behind tanh and behind sigmoid,
// the dropout_bits masks of vlsa_gated_scores_train) with the seed READ FROM THE DEVICE WORD seed_word (int64, low 32 bits): an
// in-stream op that advances the word between steps is recorded by a captured graph, a by-value seed would be baked into it.  Bag b
// of the batch draws its masks under bag_drop_seed(seed, b) (bag 0: the seed itself).  drop_p = 0 or gated = 0: the inference
// launch (seed_word may then be NULL).
extern "C" int vlsa_gated_scores_batch_train(const void* bag_desc, int B, int x_dtype, int D, const void* prep, int gated,
                                             const int* tile_start, int n_tiles, int rows_per_tile, float* a, const int64_t* a_off,
                                             int64_t a_floats, float drop_p, const int64_t* seed_word, void* stream) {
    if (drop_p < 0.f) return VLSA_EINVAL;
    return gated_scores_batch_impl(bag_desc, B, x_dtype, D, prep, gated, tile_start, n_tiles, rows_per_tile, a, a_off, a_floats, drop_p,
                                   seed_word, stream);
}

// Scores AND attention pooling of a batch of bf16 bags in ONE launch of the persistent LDS-DMA kernel (+ the per-bag fold of its
// per-tile partials).  Arguments as vlsa_gated_scores_batch with rows_per_tile a multiple of 32 in (max_rows of
// vlsa_gated_scores_tiling, 256]; ws: n_tiles x 514 floats; pooled [B, 512] fp32 = sum_n softmax(a)_n x_n per bag.  a is written
// whole (no zeroing needed).
extern "C" int vlsa_gated_scores_pool_batch(const void* bag_desc, int B, int x_dtype, int D, const void* prep, int gated,
                                            const int* tile_start, int n_tiles, int rows_per_tile, float* a, const int64_t* a_off,
                                            float* ws, float* pooled, void* stream) {
    if (!bag_table_ok(bag_desc, B, tile_start, n_tiles) || !prep || !a || !a_off || !ws || !pooled) return VLSA_EINVAL;
    if (D != gs::kD || x_dtype != VLSA_DT_BF16) return VLSA_EUNSUPPORTED;
    const GsBatch bt{static_cast<const vlsa_bag_desc*>(bag_desc), tile_start, reinterpret_cast<const long long*>(a_off), B, 0u, 0u, 1.f, 0u};
    return gs_tile_launch(nullptr, 0ll, 0ll, static_cast<const unsigned char*>(prep), gated, a, n_tiles, rows_per_tile, bt, ws, pooled,
                          (hipStream_t)stream);
}

// The same for ONE bag given by pointer (no bag table): ws = vlsa_gated_scores_pool_ws_floats(N) floats, pooled [512].
// fp32 bags (the reference's own format), or VLSA_GS_TILE=0: the same result from ONE host call through the fragment-order score kernel,
// the pooling partials (vlsa_scored_pool_partial) and their merge -- three launches whose Python route (six allocations, three calls,
// an autograd Function) is what bounds a slide-sized bag's module call.
extern "C" int vlsa_pool_num_partials(int64_t N);
extern "C" int vlsa_scored_pool_partial(const void* X, int x_dtype, int64_t N, int64_t ldx, int D, const float* scores, float* pm, float* pl,
                                        float* pacc, void* stream);
extern "C" int vlsa_vlfan_merge(const float* pm, const float* pl, const float* pacc, int G, int P, int D, int normalise, float* m2, float* l,
                                float* out, void* stream);
extern "C" int64_t vlsa_gated_scores_pool_ws_floats(int64_t N) {
    if (N < 1) return 0;
    const int64_t tiles = 514ll * gs_tile_pool_tiles((long long)N);
    const int64_t chain = (int64_t)vlsa_pool_num_partials(N) * (16 + 16 + 512) + 64;      // pm, pl, pacc of the partials + (m2, l)
    return tiles > chain ? tiles : chain;
}
extern "C" int vlsa_gated_scores_pool(const void* X, int x_dtype, int64_t N, int64_t ldx, int D, const void* prep, int gated, float* a,
                                      float* ws, float* pooled, void* stream) {
    if (!X || !prep || !a || !ws || !pooled || N < 1 || ldx < D) return VLSA_EINVAL;
    if (D != gs::kD || (x_dtype != VLSA_DT_BF16 && x_dtype != VLSA_DT_F32)) return VLSA_EUNSUPPORTED;
    const long long esz = x_dtype == VLSA_DT_F32 ? 4 : 2;
    if ((reinterpret_cast<uintptr_t>(X) & 15) || ((ldx * esz) % 16) || 256ll * ldx * esz >= (1ll << 31)) return VLSA_EINVAL;
    if (x_dtype == VLSA_DT_BF16 && gs_tile_min_rows_pooled() <= (long long)N) {
        const GsBatch none{nullptr, nullptr, nullptr, 0, 0u, 0u, 1.f, 0u};
        return gs_tile_launch(X, (long long)N, (long long)ldx, static_cast<const unsigned char*>(prep), gated, a, 0, 0, none, ws, pooled,
                              (hipStream_t)stream);
    }
    int rc = gated_scores_impl(X, x_dtype, N, ldx, D, prep, gated, a, 0.f, 0u, stream);
    if (rc != VLSA_OK) return rc;
    const int G = vlsa_pool_num_partials(N);
    float* pm = ws;
    float* pl = pm + (size_t)G * 16;
    float* pacc = pl + (size_t)G * 16;
    float* ml = pacc + (size_t)G * 512;
    rc = vlsa_scored_pool_partial(X, x_dtype, N, ldx, D, a, pm, pl, pacc, stream);
    if (rc != VLSA_OK) return rc;
    return vlsa_vlfan_merge(pm, pl, pacc, G, 1, D, 1, ml, ml + 16, pooled, stream);
}

// ... and DeepMIL's Adapter head behind it (vlsa_adapter_head: model/deepmil.py:283-286) from the same host call: the whole N-sized and
// head part of DeepMIL.forward(eval) for one bag.  ws: vlsa_gated_scores_pool_ws_floats(N) + R floats; W1 [R, 512], W2 [512, R]; logit [512].
// (Fold + both head layers as ONE single-workgroup launch was built and measured: 27 us for that kernel -- one CU pulls the 0.35 MB of
// tile partials and the 0.5 MB of head weights at 30-50 GB/s -- against 5 + 5 + 5 us for the three grid launches; module call 50-58
// instead of 39-40 us.  The three launches stay.)
extern "C" int vlsa_adapter_head(const float* f, int D, const float* W1, int R, const float* W2, float keep_ratio, float* hidden, float* out,
                                 void* stream);
extern "C" int vlsa_gated_scores_pool_adapter(const void* X, int x_dtype, int64_t N, int64_t ldx, int D, const void* prep, int gated, float* a,
                                              float* ws, float* pooled, const float* W1, int R, const float* W2, float keep_ratio,
                                              float* logit, void* stream) {
    if (!W1 || !W2 || !logit || R < 4 || (R % 4)) return VLSA_EINVAL;
    const int rc = vlsa_gated_scores_pool(X, x_dtype, N, ldx, D, prep, gated, a, ws, pooled, stream);
    if (rc != VLSA_OK) return rc;
    return vlsa_adapter_head(pooled, D, W1, R, W2, keep_ratio, ws + vlsa_gated_scores_pool_ws_floats(N), logit, stream);
}
