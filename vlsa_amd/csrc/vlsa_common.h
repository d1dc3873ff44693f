// Shared device helpers for the gfx950 kernels of libvlsa_hip.so.  CDNA4 only: 64-lane wavefronts,
// MFMA 16x16x32 bf16, LDS transpose reads.  No portability layer on purpose.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/vlsa_hip.h"

// Experiment switches.  The shipped library reads NO process environment (no global state): every A/B hook of the
// measurement tools goes through VLSA_ENV, which is getenv only in a -DVLSA_EXPERIMENT build (tools/*: VLSA_EXTRA_HIPCC_FLAGS) and a
// null pointer -- the hook's name does not even reach the binary -- otherwise.  tests/test_abi_cpu.py greps the default build.
#ifdef VLSA_EXPERIMENT
#include <cstdlib>
#define VLSA_ENV(name) getenv(name)
#else
#define VLSA_ENV(name) (static_cast<const char*>(nullptr))
#endif

// wave priority of the short tail / preparation kernels that co-run with a persistent streaming kernel
#ifndef VLSA_TAIL_PRIO
#define VLSA_TAIL_PRIO 3
#endif

namespace vlsa {

typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) bf16x4* lds_bf16x4_ptr;
typedef __attribute__((address_space(3))) void* lds_void_ptr;
// LDS images are written as raw words (or by LDS-DMA) and read back as typed fragments: every such access goes through
// may_alias types so type-based alias analysis can never reorder a fragment read above the staging write.
typedef u32x4 __attribute__((may_alias)) u32x4_ma;
typedef bf16x8 __attribute__((may_alias)) bf16x8_ma;
typedef bf16x4 __attribute__((may_alias)) bf16x4_ma;
typedef f32x4 __attribute__((may_alias)) f32x4_ma;
typedef float __attribute__((may_alias)) float_ma;
typedef int __attribute__((may_alias)) int_ma;

// The kernels read the public descriptors (vlsa_hip.h) straight from device memory.
static_assert(sizeof(vlsa_bag_desc) == 24, "vlsa_bag_desc is part of the ABI");
static_assert(sizeof(vlsa_rows_desc) == 16, "vlsa_rows_desc is part of the ABI");

constexpr float kLog2e = 1.4426950408889634f;
constexpr float kNormEps = 1e-12f;  // F.normalize eps (model/deepmil.py:187,189)
constexpr int kPStride = 16;        // stride of the per-query m/l arrays

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
    return v;
}
// Sum / max over the 4 lanes {i, i+16, i+32, i+48} (the four 16-lane rows of a wavefront).
__device__ __forceinline__ float quad_rows_sum(float v) {
    v += __shfl_xor(v, 16);
    v += __shfl_xor(v, 32);
    return v;
}
__device__ __forceinline__ float quad_rows_max(float v) {
    v = fmaxf(v, __shfl_xor(v, 16));
    v = fmaxf(v, __shfl_xor(v, 32));
    return v;
}
// sum over the 16 lanes of a DPP row (lanes 16 k .. 16 k + 15), result in every lane: four full-rate VALU adds
__device__ __forceinline__ float row16_sum(float v) {
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x128, 0xf, 0xf, false));  // row_ror:8
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x124, 0xf, 0xf, false));  // row_ror:4
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x122, 0xf, 0xf, false));  // row_ror:2
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x121, 0xf, 0xf, false));  // row_ror:1
    return v;
}
__device__ __forceinline__ float fast_exp2(float x) { return __builtin_amdgcn_exp2f(x); }

// Byte offset of (row, byte_off) in a wave's bf16 slice image (256-byte rows): the 32-byte chunk index is XORed with row & 7.
__device__ __forceinline__ int swz(int row, int byte_off) { return row * 256 + (byte_off ^ ((row & 7) << 5)); }

// Counter-based dropout mask of the fused attention-score kernels (forward and backward recompute the same bits):
// keep(seed, row, unit) = mix32(seed ^ row * 0x9E3779B1 ^ unit * 0x85EBCA6B) >= thr, thr = p * 2^32 (murmur3 finaliser).
// `unit` = hidden unit + 256 * branch; `row` = the row's index in the launch's score array.
__host__ __device__ __forceinline__ unsigned int dropout_bits(unsigned int seed, unsigned int row, unsigned int unit) {
    unsigned int h = seed ^ (row * 0x9E3779B1u) ^ (unit * 0x85EBCA6Bu);
    h ^= h >> 16;
    h *= 0x85EBCA6Bu;
    h ^= h >> 13;
    h *= 0xC2B2AE35u;
    h ^= h >> 16;
    return h;
}

// Seed of bag b in a batched training launch whose seed word is s: bag 0 keeps s (a batch of one bag draws the masks of the
// single-bag path under s), every other bag a hashed seed of its own, so that bags of one launch get independent masks.
__host__ __device__ __forceinline__ unsigned int bag_drop_seed(unsigned int s, int b) {
    return b == 0 ? s : dropout_bits(s ^ 0x5BD1E995u, (unsigned int)b, 0xFFFFFFFFu);
}

__device__ __forceinline__ float load_as_float(const float* p) { return *p; }
__device__ __forceinline__ float load_as_float(const __bf16* p) { return (float)*p; }

// Block-wide sum for 256-thread blocks; `red` is >= 4 floats of LDS. All threads get the result.
__device__ __forceinline__ float block_sum_256(float v, float* red) {
    v = wave_sum(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return red[0] + red[1] + red[2] + red[3];
}

// Opaque prepared-query block layout (see vlsa_prepare_queries).
struct QPrepLayout {
    size_t qeff, qsplit, qhat, qnorm, total;
    __host__ __device__ explicit QPrepLayout(int D) {
        qeff = 0;
        qsplit = qeff + (size_t)16 * D * 4;
        qhat = qsplit + (size_t)3 * 16 * D * 2;
        qnorm = qhat + (size_t)17 * D * 4;
        total = qnorm + 32 * 4;
    }
};

}  // namespace vlsa
