// Plumbing shared by the LDS-DMA streaming kernels (k_vlfan_partial_dma, k_vlfan_partial_dma_batch, k_vlfan_partial_f32_batch,
// k_vlfan_backward_dma_batch, k_vlfan_backward_f32_batch): the barrier, the bag table entry and the row split that fills it,
// the per-wave DMA ring and the walk over a wave's own tiles.  Device code only; what a kernel does with a tile stays in its file.
//
// The including file defines VLSA_STREAM_NT, the cache qualifier of the DMA loads, as a string literal ("nt" or "").
#pragma once
#include "vlsa_common.h"

#ifndef VLSA_STREAM_NT
#error "define VLSA_STREAM_NT (\"nt\" or \"\") before including vlfan_stream.h"
#endif

// LDS accesses of this wave have returned, then a raw barrier (no vmcnt wait: the DMA ring stays in flight across it)
#define VLSA_LDS_BARRIER()                                   \
    do {                                                     \
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   \
        __builtin_amdgcn_s_barrier();                        \
        asm volatile("" ::: "memory");                       \
    } while (0)

namespace vlsa {

constexpr int kStreamD = 512;  // columns of a streamed row

// element (row, col) of a wave's fp32 slice image (16 rows x 128 columns) lives at
// row * 512 + (((col >> 2) ^ row) << 4) + (col & 3) * 4: the 16-B chunk index is XORed with the 4-bit row, so that both the
// score reads (16 rows x one chunk per quarter wave) and the weighted-sum reads (4 rows x 16 words) hit 64 distinct banks
// (the bf16 image's swz is in vlsa_common.h)
__device__ __forceinline__ int fswz(int row, int col) { return row * 512 + ((((col >> 2) ^ (row & 15))) << 4) + ((col & 3) << 2); }

// ---- bag table: one entry of ints per bag in LDS, describing THIS workgroup's rows of the bag.  The first four ints are the
// ring's int4 reload (buffer base, span, pitch); a forward table appends the bag's score rows.
enum StreamEntry : int {
    kEntAddrLo = 0,    // first row of the range: address bits 0..31
    kEntAddrHi,        // ... bits 32..47 (the descriptor's stride field stays 0)
    kEntSpan,          // descriptor span in bytes: anything past the range's last row reads as zero
    kEntPitch,         // row pitch in bytes
    kEntRows,          // rows of the range (0: nothing to stream)
    kEntTiles,         // ... in tiles
    kEntSlot,          // partial slot of this workgroup for this bag
    kEntMine,          // 0: a bag of another workgroup group (global tables only)
    kEntScoreLo,       // forward tables: score row pointer at the range's first row (0: none), bits 0..31
    kEntScoreHi,
    kEntScorePitch,    // ... and the score matrix's row pitch in floats
};

template <int kInts>
struct StreamTab {
    int_ma* t;
    __device__ __forceinline__ int_ma* entry(int bag) const { return t + bag * kInts; }
    __device__ __forceinline__ int get(int bag, int k) const { return __builtin_amdgcn_readfirstlane(t[bag * kInts + k]); }
};

// Row range of virtual workgroup vb out of G for bag d, in units of 1 << kUnitShift rows (= one iteration of the workgroup);
// fills entry e and returns the range's first row.  The workgroup that gets the remainder unit rotates with the bag index (the
// caller's vb) so that the extra iterations even out over the batch.  !mine: an empty range.
template <int kUnitShift, int kElemBytes, int kTile>
__device__ __forceinline__ long long stream_split(const vlsa_bag_desc& d, int G, unsigned int vb, bool mine, int_ma* e) {
    const unsigned long long units = (unsigned long long)((d.N + ((1 << kUnitShift) - 1)) >> kUnitShift);
    const unsigned int uq = (unsigned int)(units / (unsigned int)G), ur = (unsigned int)(units % (unsigned int)G);
    const unsigned long long ubeg = (unsigned long long)vb * uq + (vb < ur ? vb : ur);
    const long long rbeg = (long long)(ubeg << kUnitShift);
    long long rend = (long long)((ubeg + uq + (vb < ur ? 1u : 0u)) << kUnitShift);
    if (rend > d.N) rend = d.N;
    const int nrows = (mine && rend > rbeg) ? (int)(rend - rbeg) : 0;
    const unsigned long long addr = reinterpret_cast<unsigned long long>(d.X) + (unsigned long long)rbeg * d.ldx * (unsigned long long)kElemBytes;
    e[kEntAddrLo] = (int)(unsigned int)addr;
    e[kEntAddrHi] = (int)((addr >> 32) & 0xffffu);
    e[kEntSpan] = nrows > 0 ? (int)(((long long)(nrows - 1) * d.ldx + kStreamD) * kElemBytes) : 0;
    e[kEntPitch] = (int)(d.ldx * kElemBytes);
    e[kEntRows] = nrows;
    e[kEntTiles] = (nrows + kTile - 1) / kTile;
    e[kEntSlot] = (int)vb;
    e[kEntMine] = mine ? 1 : 0;
    return rbeg;
}

// ---- the walk over a wave's own tiles: tiles start, start + kStride, ... of every bag (two row groups: (2, rg); one: (1, 0))
template <int kInts>
__device__ __forceinline__ int stream_first_bag(const StreamTab<kInts>& tab, int bag, int nbags, int start) {
    while (bag < nbags && tab.get(bag, kEntTiles) <= start) ++bag;
    return bag;
}
// the next own tile after (bag, tile): same bag if it has one, else the first of a later bag (nb == nbags: none)
template <int kStride, int kInts>
__device__ __forceinline__ void stream_next(const StreamTab<kInts>& tab, int bag, int tile, int ntiles_bag, int nbags, int start,
                                            int& nb, int& nt) {
    if (tile + kStride < ntiles_bag) {
        nb = bag;
        nt = tile + kStride;
        return;
    }
    nb = bag + 1;
    while (nb < nbags && tab.get(nb, kEntTiles) <= start) ++nb;
    nt = start;
}

// ---- DMA ring.  A tile goes HBM -> LDS in 8 wave-instructions of 1 KiB (buffer_load_dwordx4 ... lds) into one of the two
// 8-KiB slots of the wave's ring; rows past the bound range read as zero through the buffer descriptor's bounds check.  The
// DMA lands lane l at byte 16 l of its piece, so the XOR swizzle of the LDS image is applied on the per-lane SOURCE address.
// The DMA is issued from inline asm on purpose: hipcc would otherwise order every later ds_read of the ring behind ALL
// outstanding LDS-DMA (s_waitcnt vmcnt(0)), which serialises the prefetch; the kernels count vmcnt themselves.
#define VLSA_DMA_PIECE(lds_dst, voff, rsrc, soff)                         \
    do {                                                                  \
        unsigned int keep_;                                               \
        asm volatile(                                                     \
            "s_mov_b32 %0, m0\n\t"                                        \
            "s_mov_b32 m0, %1\n\t"                                        \
            "s_nop 0\n\t"                                                 \
            "buffer_load_dwordx4 %2, %3, %4 offen " VLSA_STREAM_NT " lds\n\t" \
            "s_mov_b32 m0, %0"                                            \
            : "=&s"(keep_)                                                \
            : "s"(lds_dst), "v"(voff), "s"(rsrc), "s"(soff)               \
            : "memory");                                                  \
    } while (0)

constexpr int kDmaSlot = 8192;  // bytes of a ring slot = one wave's slice image of a tile

// What both piece layouts share: the buffer descriptor {base_lo, base_hi (stride 0), num_records, flags} and the row pitch of
// the range the ring streams from, cached in SGPRs and reloaded from the table on a bag change.
struct DmaRingBase {
    i32x4 rsrc = {0, 0, 0, 0x00020000};
    int ldb = 0;        // row pitch in bytes
    int bag = -1;       // table entry the descriptor was loaded from
    unsigned int lds;   // LDS byte address of this wave's ring
    int cw;             // column quarter of this wave

    __device__ __forceinline__ DmaRingBase(unsigned char* ring, int cw_) : lds((unsigned int)(uintptr_t)(lds_void_ptr)ring), cw(cw_) {}
    // the descriptor words of bag table entry `e`
    __device__ __forceinline__ void load(const int_ma* e) {
        const int4 v = *reinterpret_cast<const int4*>(e);
        rsrc[0] = __builtin_amdgcn_readfirstlane(v.x);
        rsrc[1] = __builtin_amdgcn_readfirstlane(v.y);
        rsrc[2] = __builtin_amdgcn_readfirstlane(v.z);
        ldb = __builtin_amdgcn_readfirstlane(v.w);
    }
};

// bf16 rows: tile = 32 rows x 256 B; piece i = rows 4 i .. 4 i + 3, lane l -> row 4 i + (l >> 4), source chunk
// (l & 15) ^ ((row & 7) << 1) with row & 7 = (l >> 4) + 4 (i & 1)
struct DmaRingBf16 : DmaRingBase {
    static constexpr int kTile = 32;
    int lr, chunk_e, chunk_o;
    int voff_e = 0, voff_o = 0;

    __device__ __forceinline__ DmaRingBf16(unsigned char* ring, int lane, int cw_) : DmaRingBase(ring, cw_), lr(lane >> 4) {
        chunk_e = ((lane & 15) ^ (lr << 1)) << 4;
        chunk_o = ((lane & 15) ^ (lr << 1) ^ 8) << 4;
    }
    __device__ __forceinline__ void offsets() {
        voff_e = lr * ldb + cw * 256 + chunk_e;
        voff_o = lr * ldb + cw * 256 + chunk_o;
    }
    // bind to wave-uniform descriptor words (a kernel without a table)
    __device__ __forceinline__ void bind(int addr_lo, int addr_hi, int span, int pitch) {
        rsrc[0] = addr_lo;
        rsrc[1] = addr_hi;
        rsrc[2] = span;
        ldb = pitch;
        offsets();
    }
    // bind to entry `e` of a bag table, the table's entry number `b`
    __device__ __forceinline__ void bind(const int_ma* e, int b) {
        if (b != bag) {
            load(e);
            offsets();
            bag = b;
        }
    }
    __device__ __forceinline__ void issue(int tile, int slot) const {
        const int sbase = tile * kTile * ldb;
        const unsigned int dst = lds + slot * kDmaSlot;
#pragma unroll
        for (int i = 0; i < 8; ++i) VLSA_DMA_PIECE(dst + i * 1024, (i & 1) ? voff_o : voff_e, rsrc, sbase + i * 4 * ldb);
    }
};

// fp32 rows: tile = 16 rows x 512 B; piece i = rows 2 i, 2 i + 1, lane l -> row 2 i + (l >> 5), source chunk (l & 31) ^ row
struct DmaRingF32 : DmaRingBase {
    static constexpr int kTile = 16;
    int lr, lc;
    int voff[8] = {0, 0, 0, 0, 0, 0, 0, 0};

    __device__ __forceinline__ DmaRingF32(unsigned char* ring, int lane, int cw_) : DmaRingBase(ring, cw_), lr(lane >> 5), lc(lane & 31) {}
    __device__ __forceinline__ void bind(const int_ma* e, int b) {
        if (b != bag) {
            load(e);
#pragma unroll
            for (int q = 0; q < 8; ++q) voff[q] = lr * ldb + cw * 512 + ((lc ^ (2 * q + lr)) << 4);
            bag = b;
        }
    }
    __device__ __forceinline__ void issue(int tile, int slot) const {
        const int sbase = tile * kTile * ldb;
        const unsigned int dst = lds + slot * kDmaSlot;
#pragma unroll
        for (int i = 0; i < 8; ++i) VLSA_DMA_PIECE(dst + i * 1024, voff[i], rsrc, sbase + i * 2 * ldb);
    }
};

}  // namespace vlsa
