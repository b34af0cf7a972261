// Weight gradients of the convolutions on bf16 / fp16 MFMA (gfx950).
//
//   dw[tap][co][kc] = sum_m dz[m][co] * x[gather(m, tap)][kc]      (fp32)
//
// GEMM view: rows = co, cols = kc (input channels of one tap), K = output pixels.  Both operands are stored channel-contiguous (NHWC)
// while the reduction runs over pixels, so both MFMA fragments are fetched from LDS with the CDNA4 transposing read
// ds_read_b64_tr_b16 (wg_tr_read; no software transpose).  LDS tiles are [pixels][64 channels] (128-B rows); 32-B granules are
// XOR-swizzled (wg_swz_off, wg_src_piece) so the 8 rows a 32-lane half touches land on 8 distinct bank groups.
//
// The file's five kernels, each described where it is defined:
//   conv_wgrad_kernel                     any tap set, 64 x 64 tiles, fp32 atomics               ("Atomics kernel")
//   conv_wgrad_halo_kernel (+ _pair_,     3x3 / 1x1 on a staged x halo, 64 x 64 tiles, loader     ("halo form")
//     _grouped_ variants of one body)     waves + MFMA waves, split partials in a slab
//   conv_wgrad_stem_kernel                the 7x7 stride-2 stem on raw input rows, same waves     ("Stem weight gradient")
//   conv_wgrad128_persistent_kernel       128-wide tiles, persistent blocks, host-built schedule  ("wg2")
//   wgrad_slab_reduce_group_kernel        sums the split partials of one or more problems         (WgReduceGroup)
// Host side: wg_route() decides which kernel takes a problem; every eligibility test and launcher is stated on it.
#include <string.h>
#include <algorithm>
#include <type_traits>
#include <utility>
#include <vector>
#include "common.h"

typedef const void __attribute__((address_space(1)))* wg_gptr_t;
typedef void __attribute__((address_space(3)))* wg_lptr_t;
typedef const char __attribute__((address_space(3)))* wg_lds_cp;

// The 32-byte-granule swizzle of a [rows][64] tile.  Reader side: element offset of column `col` of row `r`; loader side: the 16-B
// source piece that lane piece `piece` (0..7) of row `r` fetches, so that a linear LDS-DMA write lands swizzled.
static __device__ __forceinline__ int wg_f(int r) { return ((r >> 1) & 1) | (((r >> 3) & 1) << 1); }
static __device__ __forceinline__ int wg_swz_off(int r, int col) { return r * 64 + ((((col >> 4) ^ wg_f(r)) << 4) | (col & 15)); }
static __device__ __forceinline__ int wg_src_piece(int r, int piece) { return (((piece >> 1) ^ wg_f(r)) << 1) | (piece & 1); }

// One MFMA 16x16x32 operand with the K index on LDS rows: two transposing reads of four rows each (k = 8g + q and 8g + 4 + q).
static __device__ __forceinline__ bf16x8 wg_tr_read(wg_lds_cp lo_addr, wg_lds_cp hi_addr) {
    typedef s16x4 __attribute__((address_space(3))) * lds_p;
    const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_p)lo_addr);
    const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_p)hi_addr);
    s16x8 v;
    v[0] = lo[0]; v[1] = lo[1]; v[2] = lo[2]; v[3] = lo[3];
    v[4] = hi[0]; v[5] = hi[1]; v[6] = hi[2]; v[7] = hi[3];
    return __builtin_bit_cast(bf16x8, v);
}
static __device__ __forceinline__ bf16x8 wg_tr_read(const bf16_t* tile, int o0, int o1) {      // element offsets into a tile in LDS
    return wg_tr_read((wg_lds_cp)(const char*)(tile + o0), (wg_lds_cp)(const char*)(tile + o1));
}

// Stores N 16 x 16 fp32 accumulator tiles (16-row groups a = 0..N-1 of one 16-column strip) into a [co][ci] matrix: `o` points at
// (row 0, this lane's column), gq = lane >> 4.
template <int N>
static __device__ __forceinline__ void wg_store_tile(float* o, size_t row_stride, const f32x4 (&acc)[N], int gq) {
#pragma unroll
    for (int a = 0; a < N; ++a)
#pragma unroll
        for (int j = 0; j < 4; ++j) o[(size_t)(a * 16 + 4 * gq + j) * row_stride] = acc[a][j];
}

// ---------------------------------------------------------------------------
// Atomics kernel: any tap set.  One block = one (co tile 64, kc tile 64, tap) over `chunks_per_block` 128-pixel chunks, staged
// through registers into two [128][64] tiles per operand; the 4 waves split every chunk's pixels (32 each) and their 64x64 partial
// tiles are summed through LDS before one fp32 atomic per element.
// ---------------------------------------------------------------------------
static __device__ __forceinline__ bf16x8 tr_frag(const bf16_t* tile, int rbase, int ctile, int lane) {
    // element j of lane l = tile[row rbase + 8*(l>>4) + j][col ctile*16 + (l&15)]
    const int g = lane >> 4, i = lane & 15, q = i >> 2, pp = i & 3;
    const int col = ctile * 16 + 4 * pp;               // 4 consecutive columns = 8 bytes
    const int r0 = rbase + 8 * g + q;
    return wg_tr_read(tile, wg_swz_off(r0, col), wg_swz_off(r0 + 4, col));
}

__global__ __launch_bounds__(256, 2) void conv_wgrad_kernel(const WgradParams p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    bf16_t* sZ = reinterpret_cast<bf16_t*>(smem);        // [2][128*64]  dz tile
    bf16_t* sX = sZ + 2 * 128 * 64;                      // [2][128*64]  x tile

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int piece = tid & 7;
    const int row0 = tid >> 3;

    const int kct = p.Kc >> 6;
    const int cot = p.Co >> 6;
    int bx = blockIdx.x;
    const int tap = bx / (cot * kct);
    bx -= tap * cot * kct;
    const int co0 = (bx / kct) * 64;
    const int kc0 = (bx % kct) * 64;

    const int HW = p.Hs * p.Ws;
    const int chunk_begin = blockIdx.y * p.chunks_per_block;
    const int nchunks_total = (p.M + 127) >> 7;
    int chunk_end = chunk_begin + p.chunks_per_block;
    chunk_end = chunk_end < nchunks_total ? chunk_end : nchunks_total;
    if (chunk_begin >= chunk_end) return;

    const int tir = tap / p.taps.nc;
    const int tic = tap - tir * p.taps.nc;
    const int toff = ((p.taps.dy0 + tir * p.taps.dys) * p.xWp + (p.taps.dx0 + tic * p.taps.dxs)) * p.xC + kc0 + piece * 8;
    const int wsl = p.taps.w0 + tir * p.taps.wrs + tic * p.taps.wcs;

    u32x4 rz[4], rx[4];
    auto load_chunk = [&](int ch) __attribute__((always_inline)) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int m = ch * 128 + row0 + 32 * i;
            if (m < p.M) {
                const int b = m / HW;
                const int r = m - b * HW;
                const int yy = r / p.Ws;
                const int xx = r - yy * p.Ws;
                const size_t zo = ((size_t)(b * p.dzHp + yy + p.dzpad) * p.dzWp + xx + p.dzpad) * p.dzC + co0 + piece * 8;
                rz[i] = *reinterpret_cast<const u32x4*>(p.dz + zo);
                const size_t xo = ((size_t)(b * p.xHp + yy * p.istr) * p.xWp + xx * p.istr) * p.xC + toff;
                rx[i] = *reinterpret_cast<const u32x4*>(p.x + xo);
            } else {
                rz[i] = u32x4{0u, 0u, 0u, 0u};
                rx[i] = u32x4{0u, 0u, 0u, 0u};
            }
        }
    };
    auto store_chunk = [&](int buf) __attribute__((always_inline)) {
        bf16_t* dZ = sZ + buf * 128 * 64;
        bf16_t* dX = sX + buf * 128 * 64;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int r = row0 + 32 * i;
            const int o = wg_swz_off(r, piece * 8);
            *reinterpret_cast<u32x4*>(dZ + o) = rz[i];
            *reinterpret_cast<u32x4*>(dX + o) = rx[i];
        }
    };

    f32x4 acc[4][4];     // [co tile][kc tile]
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) acc[a][b] = f32x4{0.f, 0.f, 0.f, 0.f};

    load_chunk(chunk_begin);
    store_chunk(0);
    __syncthreads();

    for (int ch = chunk_begin; ch < chunk_end; ++ch) {
        const int buf = (ch - chunk_begin) & 1;
        if (ch + 1 < chunk_end) load_chunk(ch + 1);
        const bf16_t* cZ = sZ + buf * 128 * 64;
        const bf16_t* cX = sX + buf * 128 * 64;
        bf16x8 az[4], bx8[4];
#pragma unroll
        for (int a = 0; a < 4; ++a) az[a] = tr_frag(cZ, wave * 32, a, lane);
#pragma unroll
        for (int b = 0; b < 4; ++b) bx8[b] = tr_frag(cX, wave * 32, b, lane);
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int b = 0; b < 4; ++b)
                acc[a][b] = VPD_MFMA16(az[a], bx8[b], acc[a][b]);
        if (ch + 1 < chunk_end) store_chunk(buf ^ 1);
        __syncthreads();
    }

    // cross-wave reduction through LDS: red[wave][co 64][kc 64] fp32 = 64 KiB
    float* red = reinterpret_cast<float*>(smem);
    const int fr = lane & 15, fq = lane >> 4;
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int co = a * 16 + 4 * fq + j;
                const int kc = b * 16 + fr;
                red[(wave * 64 + co) * 64 + kc] = acc[a][b][j];
            }
    __syncthreads();
    float* out = p.dw + ((size_t)wsl * p.Co + co0) * p.Kc + kc0;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const int e = tid + 256 * i;          // 0..4095
        const int co = e >> 6, kc = e & 63;
        const float v = red[e] + red[4096 + e] + red[8192 + e] + red[12288 + e];
        atomicAdd(out + (size_t)co * p.Kc + kc, v);
    }
}

// ---------------------------------------------------------------------------
// 3x3 stride-1 weight gradient, halo form (the bulk of the network).
//
// One block owns a 64(co) x 64(ci) tile for ALL NINE taps over a range of 64-pixel chunks (whole image
// rows; two MFMA K-steps).  Per chunk the dz tile [64 px][64 co] and the x halo
// [NHP px][64 ci] are brought to LDS by LDS-DMA (global_load_lds) issued by four dedicated LOADER waves
// into a 3-stage ring, two chunks ahead (counted vmcnt), while the four MFMA waves (one per SIMD)
// consume the current stage: wave w owns ci columns 16w..16w+15, keeps 9 taps x 4 co-tiles of
// accumulators (144 VGPRs) and reads every operand with ds_read_b64_tr_b16 at 44 chunk-invariant,
// precomputed swizzled offsets.  The x halo is loaded once and serves all nine taps (139 FLOP per
// staged byte instead of 32).  One barrier per chunk: READY_c = "chunk c has landed" and, because the
// MFMA waves only arrive after finishing chunk c-1, also "the stage of chunk c-1 is free".  Partial
// tiles go to an fp32 slab with plain stores (slab[split][tap][Co][Ci]); wgrad_slab_reduce_group_kernel sums
// the splits.
// ---------------------------------------------------------------------------
#define WG_CH 64           // pixels per chunk = two MFMA K-steps (vpd_wgrad_split assumes 64)
#define WG_NS 3            // ring stages

struct WgHaloGeom {
    int TR, multi, HR, NHP, total_pix;   // halo tiling of a 128-pixel chunk (as HaloGeom in conv_igemm.hip)
    int ksplit, cpb;                     // pixel-chunk splits and chunks per block
};

// The down-sampling block's 1x1 branch riding in its 3x3 stride-2 conv1's launch (conv_wgrad_halo_pair_kernel): the branch's dz and
// its slab.  Everything else -- x, the shapes, the split -- is conv1's.
struct WgPair {
    const bf16_t* dz2;
    float* slab2;                        // [split][Co][Ci]
};

// MFMA-wave body of conv_wgrad_halo_kernel for taps [T0, T1): ci columns 16*ctile .. +15, all 64 co.
// BR: the wave also carries the riding 1x1 branch as a further "tap": B operand = the centre tap's x fragments, A operand from the
// branch's dz tiles (ring2: two stages of 64 x 64), accumulated in the order of the one_by_one launch it replaces.
template <int T0, int T1, int NS, bool BR = false>
static __device__ __forceinline__ void wgrad_mfma_half(const WgradParams& p, const WgHaloGeom& g, const bf16_t* ring,
                                                       int STAGE, int nch, int ctile, int lane, int bx, int by,
                                                       const bf16_t* ring2 = nullptr, float* slab2 = nullptr) {
    constexpr int NT = T1 - T0;
    // W, H: OUTPUT dims; the x halo is rows of the padded INPUT (stride S = 1 or 2: input pixel S*y + r, S*x + t)
    const int W = p.Ws, H = p.Hs, Wp = p.xWp, S = p.istr;
    f32x4 acc[NT][4];
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int a = 0; a < 4; ++a) acc[t][a] = f32x4{0.f, 0.f, 0.f, 0.f};
    f32x4 acc2[4];                       // (BR) the branch's tile
#pragma unroll
    for (int a = 0; a < 4; ++a) acc2[a] = f32x4{0.f, 0.f, 0.f, 0.f};

    const int gq = lane >> 4, i16 = lane & 15, q = i16 >> 2, pp = i16 & 3;
    // chunk-invariant LDS element offsets (within a stage) of every transposed read of this lane.
    // dz rows are 32*ks + 8*gq + 4*h + q: the swizzle only looks at row bits 1 and 3, so k-step 1 is +32 rows.
    int offA[4][2], offB[2][NT][2];
    [[maybe_unused]] int offC[2][2];
    {
        const int ra = 8 * gq + q;
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                offA[a][h] = wg_swz_off(ra + 4 * h, a * 16 + 4 * pp);
            }
#pragma unroll
        for (int ks = 0; ks < 2; ++ks)
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const int pk = 32 * ks + 8 * gq + 4 * h + q;      // pixel of the chunk this lane addresses
                const int lr = pk / W;
                const int xx = pk - lr * W;
                const int hrow = g.multi ? (lr / H) * p.xHp + S * (lr % H) : S * lr;
                const int hmv = hrow * Wp + S * xx;
#pragma unroll
                for (int t = 0; t < NT; ++t) {
                    const int tt = T0 + t;
                    const int r = hmv + (p.taps.dy0 + (tt / 3) * p.taps.dys) * Wp + (p.taps.dx0 + (tt % 3) * p.taps.dxs);
                    offB[ks][t][h] = 64 * 64 + wg_swz_off(r, ctile * 16 + 4 * pp);
                }
                if constexpr (BR) {      // the centre tap
                    const int r = hmv + (p.taps.dy0 + p.taps.dys) * Wp + (p.taps.dx0 + p.taps.dxs);
                    offC[ks][h] = 64 * 64 + wg_swz_off(r, ctile * 16 + 4 * pp);
                }
            }
    }
    if constexpr (NS == 2) {
        // the 13-pass launches: hipcc keeps each offset as two addends (row, swizzled column) and folds them into the stage address
        // inside the loop -- twice the registers, spilled.  Opaque values stay one register each.
#pragma unroll
        for (int ks = 0; ks < 2; ++ks)
#pragma unroll
            for (int h = 0; h < 2; ++h) {
#pragma unroll
                for (int t = 0; t < NT; ++t) asm volatile("" : "+v"(offB[ks][t][h]));
                if constexpr (BR) asm volatile("" : "+v"(offC[ks][h]));
            }
    }

    for (int c = 0; c < nch; ++c) {
        __builtin_amdgcn_s_barrier();                             // READY_c
        if (VPD_ABL(p, 2)) continue;
        const bf16_t* st = ring + (c % NS) * STAGE;
        if constexpr (BR) {
            const bf16_t* st2 = ring2 + (c & 1) * WG_CH * 64;
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
                bf16x8 az[4], bx[NT];
#pragma unroll
                for (int a = 0; a < 4; ++a) az[a] = wg_tr_read(st + ks * 32 * 64, offA[a][0], offA[a][1]);
#pragma unroll
                for (int t = 0; t < NT; ++t) bx[t] = wg_tr_read(st, offB[ks][t][0], offB[ks][t][1]);
                const bf16x8 bxc = wg_tr_read(st, offC[ks][0], offC[ks][1]);
                __builtin_amdgcn_sched_barrier(0);
                // co tile by co tile (every accumulator still sees its k-steps in order): once a tile's MFMAs are issued its dz
                // registers take the branch's dz fragment, whose read then hides behind the next tiles' MFMAs -- five A sets at
                // once do not fit the 168 registers of a 12-wave block
#pragma unroll
                for (int a = 0; a < 4; ++a) {
#pragma unroll
                    for (int t = 0; t < NT; ++t) acc[t][a] = VPD_MFMA16(az[a], bx[t], acc[t][a]);
                    az[a] = wg_tr_read(st2 + ks * 32 * 64, offA[a][0], offA[a][1]);
                    __builtin_amdgcn_sched_barrier(0);
                }
#pragma unroll
                for (int a = 0; a < 4; ++a) acc2[a] = VPD_MFMA16(az[a], bxc, acc2[a]);
            }
            continue;
        }
        if constexpr (NT == 4) {
            // the 4-tap wave of a SIMD reads BOTH k-steps up front and then issues its 32 MFMAs in one run, so that
            // the 5-tap wave's second read phase falls into this wave's MFMAs instead of coinciding with a read
            // phase of its own (the two waves leave the barrier together)
            bf16x8 az[2][4], bx[2][NT];
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
#pragma unroll
                for (int a = 0; a < 4; ++a) az[ks][a] = wg_tr_read(st + ks * 32 * 64, offA[a][0], offA[a][1]);
#pragma unroll
                for (int t = 0; t < NT; ++t) bx[ks][t] = wg_tr_read(st, offB[ks][t][0], offB[ks][t][1]);
            }
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int ks = 0; ks < 2; ++ks)
#pragma unroll
                for (int t = 0; t < NT; ++t)
#pragma unroll
                    for (int a = 0; a < 4; ++a)
                        acc[t][a] = VPD_MFMA16(az[ks][a], bx[ks][t], acc[t][a]);
            continue;
        }
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            bf16x8 az[4], bx[NT];
#pragma unroll
            for (int a = 0; a < 4; ++a) az[a] = wg_tr_read(st + ks * 32 * 64, offA[a][0], offA[a][1]);
#pragma unroll
            for (int t = 0; t < NT; ++t) bx[t] = wg_tr_read(st, offB[ks][t][0], offB[ks][t][1]);
            __builtin_amdgcn_sched_barrier(0);      // keep the reads ahead of the MFMA block (hipcc would sink them)
#pragma unroll
            for (int t = 0; t < NT; ++t)
#pragma unroll
                for (int a = 0; a < 4; ++a)
                    acc[t][a] = VPD_MFMA16(az[a], bx[t], acc[t][a]);
        }
    }

    // acc[t][a][j] = partial dW[tap T0+t][co0 + a*16 + 4*gq + j][ci0 + 16*ctile + i16]
    if (VPD_ABL(p, 8)) return;
    const int kct = p.Kc >> 6;
    const int co0 = (bx / kct) * 64;
    const int ci0 = (bx % kct) * 64;
    float* slab = p.slab + (size_t)by * (p.one_by_one ? 1 : 9) * p.Co * p.Kc;
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        const int tt = T0 + t;
        const int wsl = p.one_by_one ? 0 : p.taps.w0 + (tt / 3) * p.taps.wrs + (tt % 3) * p.taps.wcs;
        wg_store_tile(slab + ((size_t)wsl * p.Co + co0) * p.Kc + ci0 + 16 * ctile + i16, p.Kc, acc[t], gq);
    }
    if constexpr (BR) wg_store_tile(slab2 + ((size_t)by * p.Co + co0) * p.Kc + ci0 + 16 * ctile + i16, p.Kc, acc2, gq);
}
// The 64-pixel chunks [*begin, *begin + n) of pixel split `split` at `cpb` chunks per split; returns n (>= 1 by construction of the splits).
static __device__ __forceinline__ int wg_chunk_range(int M, int split, int cpb, int* begin) {
    const int nchunks_total = (M + WG_CH - 1) / WG_CH;
    *begin = split * cpb;
    const int end = *begin + cpb < nchunks_total ? *begin + cpb : nchunks_total;
    return end - *begin;
}
// Loader waves (conv_wgrad_halo_kernel and conv_wgrad_stem_kernel): loader wave lw (0..3) issues a quarter of every tile.
// One dz tile [64 px][64 co] of chunk `ch`: 8 wave-instructions of 8 pixel rows, two per loader wave.  Rows past M read `zero`, 64
// zero channels of a border pixel, and contribute nothing.  (A functor over references to the kernel's own variables, as a lambda
// in the kernel body would be: the same code as a free function taking values costs the halo kernels two registers.)
struct WgIssueDz {
    const WgradParams& p;
    const int& co0;
    const int& lw;
    const int& piece;
    const int& lrow;
    __device__ __forceinline__ void operator()(const bf16_t* dz, const bf16_t* zero, bf16_t* dst, int ch) const {
        const int W = p.Ws, H = p.Hs;
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int row = (lw + 4 * i) * 8 + lrow;
            const int m = ch * WG_CH + row;
            const int cpc = wg_src_piece(row, piece);
            const bf16_t* src = zero + cpc * 8;
            if (m < p.M) {
                const int b = m / (H * W);
                const int r = m - b * H * W;
                const int yy = r / W;
                const int xx = r - yy * W;
                src = dz + ((size_t)(b * p.dzHp + yy + p.dzpad) * p.dzWp + xx + p.dzpad) * p.dzC + co0 + cpc * 8;
            }
            __builtin_amdgcn_global_load_lds((wg_gptr_t)src, (wg_lptr_t)(dst + (lw + 4 * i) * 8 * 64), 16, 0, 0);
        }
    }
};
// The ring schedule of a loader wave over the nch chunks of its block: issue(c) requests chunk c into stage c % NS with PER_CHUNK
// LDS-DMA instructions; chunks 0 and 1 up front, then per chunk a counted wait, the READY_c barrier and chunk c + NS - 1 into the stage
// chunk c - 1 used.  PAIR: issue2(c) requests the riding branch's dz tile of chunk c into its two-stage ring (see wgrad_halo_body).
template <int NS, int PER_CHUNK, bool PAIR, class Issue, class Issue2>
static __device__ __forceinline__ void wg_loader_ring(int nch, Issue issue, Issue2 issue2) {
    if (PAIR) issue2(0);
    issue(0);
    if (NS > 2 && nch > 1) issue(1);
    for (int c = 0; c < nch; ++c) {
        // chunk c has landed when at most the instructions of the NS - 2 younger chunks are still outstanding
        if (NS > 2 && c + 1 < nch) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(PER_CHUNK) : "memory");
        else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();                             // READY_c (MFMA waves have finished chunk c-1)
        if (PAIR && c + 1 < nch) issue2(c + 1);                   // into the slot chunk c-1 used
        if (c + NS - 1 < nch) issue(c + NS - 1);                  // into the stage chunk c-1 used
    }
}

// NPASS: 32-row LDS-DMA passes of the x halo (NHP <= 32*NPASS).  (bx, by) = (output tile, pixel split) of this block.
// PAIR: a second dz tile per chunk (the riding 1x1 branch, WgPair) on a two-stage ring of its own behind the NS stages.  The tile of
// chunk c+1 goes into the slot chunk c-1 used, so it is issued behind READY_c, FIRST in that bundle: the counted wait for chunk c+1
// (at most the PER_CHUNK instructions of chunk c+2 outstanding) then covers it too.
template <int NPASS, int NS = WG_NS, bool PAIR = false>
static __device__ __forceinline__ void wgrad_halo_body(const WgradParams& p, const WgHaloGeom& g, int bx, int by,
                                                       const WgPair& pr = WgPair{nullptr, nullptr}) {
    constexpr int HROWS = 32 * NPASS;
    constexpr int STAGE = (WG_CH + HROWS) * 64;                   // bf16 elements per stage: dz tile, halo
    constexpr int PER_CHUNK = 2 + NPASS;                          // LDS-DMA instructions per loader wave per chunk
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    bf16_t* ring = reinterpret_cast<bf16_t*>(smem);               // [NS][dz 64x64 | halo HROWSx64]
    bf16_t* ring2 = ring + NS * STAGE;                            // (PAIR) [2][dz2 64x64]

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    // waves 0..7: MFMA (ci tile = wave & 3, tap half = wave >> 2: two MFMA waves share each SIMD so one computes
    // while the other waits for its LDS reads); waves 8..11: loaders
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int H = p.Hs, Wp = p.xWp, S = p.istr;
    const int kct = p.Kc >> 6;
    const int co0 = (bx / kct) * 64;
    const int ci0 = (bx % kct) * 64;
    int chunk_begin;
    const int nch = wg_chunk_range(p.M, by, g.cpb, &chunk_begin);

    if (wave >= 8) {
        // ------------------------- loader waves -------------------------
        const int lw = wave - 8;
        const int piece = lane & 7;
        const int lrow = lane >> 3;                               // row within an 8-row wave instruction
        const WgIssueDz issue_dz{p, co0, lw, piece, lrow};
        auto issue2 = [&](int c) __attribute__((always_inline)) { issue_dz(pr.dz2, pr.dz2, ring2 + (c & 1) * WG_CH * 64, chunk_begin + c); };
        auto issue = [&](int c) __attribute__((always_inline)) {
            const int ch = chunk_begin + c;
            bf16_t* st = ring + (c % NS) * STAGE;
            issue_dz(p.dz, p.dz, st, ch);      // zero: the border row of image 0
            // x halo: 4*NPASS wave-instructions; NPASS per loader wave
            const int gr0 = ch * g.TR;
            int prow0;
            if (g.multi) prow0 = (gr0 / H) * p.xHp;
            else { const int b = gr0 / H; prow0 = b * p.xHp + S * (gr0 - b * H); }
            const int gp0 = prow0 * Wp;
#pragma unroll
            for (int i = 0; i < NPASS; ++i) {
                const int hp = (lw + 4 * i) * 8 + lrow;
                int gp = gp0 + hp;
                gp = gp < g.total_pix ? gp : g.total_pix - 1;
                const int cpc = wg_src_piece(hp, piece);
                const bf16_t* src = p.x + (size_t)gp * p.xC + ci0 + cpc * 8;
                __builtin_amdgcn_global_load_lds((wg_gptr_t)src, (wg_lptr_t)(st + WG_CH * 64 + (lw + 4 * i) * 8 * 64), 16, 0, 0);
            }
        };
        if (VPD_ABL(p, 1)) {
            for (int c = 0; c < nch; ++c) __builtin_amdgcn_s_barrier();
            return;
        }
        wg_loader_ring<NS, PER_CHUNK, PAIR>(nch, issue, issue2);
        return;
    }

    // ------------------------- MFMA waves -------------------------
    const int ctile = wave & 3;
    if constexpr (PAIR) {
        // ten "taps" split 5 / 5: waves 4..7 take taps 5..8 and the branch (five accumulator sets each, as the 5-tap waves hold)
        if (wave < 4) wgrad_mfma_half<0, 5, NS>(p, g, ring, STAGE, nch, ctile, lane, bx, by);
        else wgrad_mfma_half<5, 9, NS, true>(p, g, ring, STAGE, nch, ctile, lane, bx, by, ring2, pr.slab2);
        return;
    }
    if (p.one_by_one) {
        // 1x1 convolution = the centre tap alone: waves 0..3 carry it (8 MFMAs per chunk: the launch is bound by the
        // operand stream), waves 4..7 only keep the barrier count
        if (wave < 4) wgrad_mfma_half<4, 5, NS>(p, g, ring, STAGE, nch, ctile, lane, bx, by);
        else
            for (int c = 0; c < nch; ++c) __builtin_amdgcn_s_barrier();
        return;
    }
    if (wave < 4) wgrad_mfma_half<0, 5, NS>(p, g, ring, STAGE, nch, ctile, lane, bx, by);
    else wgrad_mfma_half<5, 9, NS>(p, g, ring, STAGE, nch, ctile, lane, bx, by);
}

template <int NPASS, int NS = WG_NS>
__global__ __launch_bounds__(768) void conv_wgrad_halo_kernel(const WgradParams p, const WgHaloGeom g) {
    wgrad_halo_body<NPASS, NS>(p, g, blockIdx.x, blockIdx.y);
}

// A down-sampling BasicBlock's 3x3 stride-2 conv1 and its 1x1 stride-2 branch in one launch: same input, same halo, same chunks,
// same split; only dz differs.  The halo is staged once; the nine taps' partials go to p.slab, the branch's to pr.slab2.
template <int NPASS, int NS>
__global__ __launch_bounds__(768) void conv_wgrad_halo_pair_kernel(const WgradParams p, const WgHaloGeom g, const WgPair pr) {
    wgrad_halo_body<NPASS, NS, true>(p, g, blockIdx.x, blockIdx.y, pr);
}

// Grouped launch: the weight gradients of SEVERAL convolutions of one ResNet stage in one grid.  A weight gradient
// only needs dz and the saved activation, so it can wait until the stage's backward is done; one launch then
// carries 6-12 problems, which (1) pays the ~10 us fixed cost of a launch once instead of per layer, (2) gives the
// chip thousands of blocks, so each block can take 4x more pixels and the split-K slab shrinks 4x (layer4 needs none:
// its blocks write the gradient itself), and (3) leaves no one-block-per-CU tail between layers.
#define WG_GROUP_MAX 18
struct WgGroup {
    int nprob;
    int task_begin[WG_GROUP_MAX + 1];          // first task of each problem
    int tiles[WG_GROUP_MAX];
    WgradParams p[WG_GROUP_MAX];
    WgHaloGeom g[WG_GROUP_MAX];
};
template <int NPASS>
__global__ __launch_bounds__(768) void conv_wgrad_halo_grouped_kernel(const WgGroup grp) {
    // Tasks are ordered tile-fastest, so consecutive tasks are the output tiles of ONE pixel range: they read the same
    // dz / x chunks (different channel slices).  Workgroups go to the 8 XCDs round-robin (block b -> XCD b % 8, each
    // with its own L2), so block b takes task (b % 8) * (grid / 8) + b / 8: the tiles that share pixels then run on
    // one XCD at the same time and their operands come from its L2 instead of 4-8 separate trips to HBM.
    const int t = (blockIdx.x & 7) * (gridDim.x >> 3) + (blockIdx.x >> 3);
    if (t >= grp.task_begin[grp.nprob]) return;                   // grid padded to a multiple of 8
    int pi = 0;
    for (int i = 1; i < grp.nprob; ++i)
        if (t >= grp.task_begin[i]) pi = i;
    const int local = t - grp.task_begin[pi];
    const int tiles = grp.tiles[pi];
    wgrad_halo_body<NPASS>(grp.p[pi], grp.g[pi], local % tiles, local / tiles);
}

// slab sums of a group in one launch: blockIdx.y = problem (problems whose blocks wrote the gradient directly have ksplit 1
// and are skipped by the launcher)
// dw[e] = sum over all splits of slab[split][e].  A block owns 64 float4 outputs; its `groups` thread groups each sum every
// groups-th split (coalesced 1-KiB rows), then one LDS pass adds the groups.
struct WgReduceGroup {
    int nprob;
    const float4* slab[WG_GROUP_MAX];
    float4* dw[WG_GROUP_MAX];
    long n4[WG_GROUP_MAX];
    int ksplit[WG_GROUP_MAX];
    void add(const float* slab_, float* dw_, long nfloats, int ksplit_) {
        slab[nprob] = reinterpret_cast<const float4*>(slab_); dw[nprob] = reinterpret_cast<float4*>(dw_);
        n4[nprob] = nfloats / 4; ksplit[nprob++] = ksplit_;
    }
};
__global__ __launch_bounds__(1024) void wgrad_slab_reduce_group_kernel(const WgReduceGroup r, int groups) {
    __shared__ float4 sh[16][64];
    const int pi = blockIdx.y;
    const long n4 = r.n4[pi];
    const int ksplit = r.ksplit[pi];
    const float4* slab = r.slab[pi];
    const int o = threadIdx.x & 63, gi = threadIdx.x >> 6;
    const long i = (long)blockIdx.x * 64 + o;
    if ((long)blockIdx.x * 64 >= n4) return;                      // block-uniform
    float4 a = {0.f, 0.f, 0.f, 0.f};
    if (i < n4)
        for (int s2 = gi; s2 < ksplit; s2 += groups) {
            const float4 v = slab[(long)s2 * n4 + i];
            a.x += v.x; a.y += v.y; a.z += v.z; a.w += v.w;
        }
    sh[gi][o] = a;
    __syncthreads();
    if (gi == 0 && i < n4) {
        for (int k = 1; k < groups; ++k) {
            const float4 v = sh[k][o];
            a.x += v.x; a.y += v.y; a.z += v.z; a.w += v.w;
        }
        r.dw[pi][i] = a;
    }
}
// the slab sums of `red` (at most WG_GROUP_MAX problems; none: no launch): the thread groups are those of the problem with the most splits
static void wg_launch_reduce(const WgReduceGroup& red, hipStream_t stream) {
    if (red.nprob < 1) return;
    int max_ks = 1;
    long max_n4 = 0;
    for (int i = 0; i < red.nprob; ++i) {
        max_n4 = red.n4[i] > max_n4 ? red.n4[i] : max_n4;
        max_ks = red.ksplit[i] > max_ks ? red.ksplit[i] : max_ks;
    }
    const int groups = max_ks < 16 ? max_ks : 16;
    hipLaunchKernelGGL(wgrad_slab_reduce_group_kernel, dim3((unsigned)((max_n4 + 63) / 64), red.nprob), dim3(64 * groups), 0, stream,
                       red, groups);
}
// the same launch from flat arguments (vpd_op_wgrad_reduce: the operator tests)
int vpd_wgrad_reduce_max() { return WG_GROUP_MAX; }
hipError_t vpd_launch_wgrad_reduce(int nprob, const float* const* slabs, float* const* dws, const long long* nfloats,
                                   const int* ksplits, hipStream_t stream) {
    if (nprob < 1 || nprob > WG_GROUP_MAX) return hipErrorInvalidValue;
    WgReduceGroup red = {};
    for (int i = 0; i < nprob; ++i) red.add(slabs[i], dws[i], (long)nfloats[i], ksplits[i]);
    wg_launch_reduce(red, stream);
    return hipGetLastError();
}


// ---------------------------------------------------------------------------
// Stem weight gradient (7x7 stride 2, 8-channel border-3 input, 64 output channels):
//   dw[r][co][t*8 + c] += sum_m dz[m][co] * xin[2y + r][2x + t][c]
// Same structure as conv_wgrad_halo_kernel (loader waves, 3-stage ring of 64-pixel chunks, two MFMA waves per
// SIMD with the 7 kernel rows split 4 / 3, slab + reduce), but the x operand is the RAW input rows of the chunk
// (one contiguous range, plain LDS-DMA copy): the transposing read takes a per-lane address, so the 64 values
// (8 column taps x 8 channels) of an output pixel are read in place at its 32-byte pixel pitch -- the gather
// kernel staged 7 x 128 B per output pixel instead of 64 B.
// ---------------------------------------------------------------------------
template <int R0, int R1>
static __device__ __forceinline__ void wgrad_stem_half(const WgradParams& p, const bf16_t* ring, int STAGE, int nch,
                                                       int ctile, int lane) {
    constexpr int NT = R1 - R0;
    const int W0 = p.Ws, Wp = p.xWp;
    f32x4 acc[NT][4];
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int a = 0; a < 4; ++a) acc[t][a] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int gq = lane >> 4, i16 = lane & 15, q = i16 >> 2, pp = i16 & 3;
    int offA[4][2], baseB[2][2];
    {
        const int ra = 8 * gq + q;
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                offA[a][h] = wg_swz_off(ra + 4 * h, a * 16 + 4 * pp);
            }
#pragma unroll
        for (int ks = 0; ks < 2; ++ks)
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const int pk = 32 * ks + 8 * gq + 4 * h + q;      // output pixel of the chunk this lane addresses
                const int lr = pk / W0;
                const int xx = pk - lr * W0;
                baseB[ks][h] = 64 * 64 + (2 * lr * Wp + 2 * xx) * 8 + ctile * 16 + 4 * pp;
            }
    }
    for (int c = 0; c < nch; ++c) {
        __builtin_amdgcn_s_barrier();                             // READY_c
        const bf16_t* st = ring + (c % 3) * STAGE;
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            bf16x8 az[4], bx[NT];
#pragma unroll
            for (int a = 0; a < 4; ++a) az[a] = wg_tr_read(st + ks * 32 * 64, offA[a][0], offA[a][1]);
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                const int ro = (R0 + t) * Wp * 8;
                bx[t] = wg_tr_read(st, baseB[ks][0] + ro, baseB[ks][1] + ro);
            }
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int t = 0; t < NT; ++t)
#pragma unroll
                for (int a = 0; a < 4; ++a)
                    acc[t][a] = VPD_MFMA16(az[a], bx[t], acc[t][a]);
        }
    }
    // acc[t][a][j] = partial dW[row R0+t][co a*16 + 4*gq + j][16*ctile + i16]
    float* slab = p.slab + (size_t)blockIdx.y * 7 * 64 * 64;
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        wg_store_tile(slab + ((size_t)(R0 + t) * 64) * 64 + 16 * ctile + i16, 64, acc[t], gq);
    }
}

__global__ __launch_bounds__(768) void conv_wgrad_stem_kernel(const WgradParams p, int TR, int cpb, long xelems) {
    constexpr int NPASS = 4, HROWS = 32 * NPASS;
    constexpr int STAGE = (64 + HROWS) * 64;
    constexpr int PER_CHUNK = 2 + NPASS;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    bf16_t* ring = reinterpret_cast<bf16_t*>(smem);
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int H0 = p.Hs;
    int chunk_begin;
    const int nch = wg_chunk_range(p.M, blockIdx.y, cpb, &chunk_begin);

    if (wave >= 8) {
        const int lw = wave - 8;
        const int piece = lane & 7;
        const int lrow = lane >> 3;
        const int co0 = 0;                                        // all 64 output channels
        const WgIssueDz issue_dz{p, co0, lw, piece, lrow};
        auto issue = [&](int c) __attribute__((always_inline)) {
            const int ch = chunk_begin + c;
            bf16_t* st = ring + (c % 3) * STAGE;
            issue_dz(p.dz, p.x, st, ch);      // zero: the top border rows of image 0 of the INPUT (dz has no border)
            const int gr0 = ch * TR;
            const int b = gr0 / H0, y0 = gr0 - b * H0;
            const long e0 = ((long)(b * p.xHp + 2 * y0) * p.xWp) * 8;
#pragma unroll
            for (int i = 0; i < NPASS; ++i) {
                const int row = (lw + 4 * i) * 8 + lrow;
                long e = e0 + (long)row * 64 + piece * 8;
                e = e < xelems - 8 ? e : xelems - 8;
                __builtin_amdgcn_global_load_lds((wg_gptr_t)(p.x + e), (wg_lptr_t)(st + 64 * 64 + (lw + 4 * i) * 8 * 64), 16, 0, 0);
            }
        };
        wg_loader_ring<3, PER_CHUNK, false>(nch, issue, [](int) {});
        return;
    }
    const int ctile = wave & 3;
    if (wave < 4) wgrad_stem_half<0, 4>(p, ring, STAGE, nch, ctile, lane);
    else wgrad_stem_half<4, 7>(p, ring, STAGE, nch, ctile, lane);
}

// ---- host side of the atomics, halo and stem kernels: routing, geometry, launchers ----
static int wg_ablate() {
#ifdef VPD_ENABLE_ABLATE
    return vpd_switches().ablate;
#else
    return 0;
#endif
}

static bool wg_stem_eligible(const WgradParams& p, int* TR) {
    if (!(p.slab && p.xC == 8 && p.Kc == 64 && p.Co == 64 && p.istr == 2 && p.taps.nr == 7 && p.taps.nc == 1 &&
          p.taps.dy0 == 0 && p.taps.dys == 1 && p.taps.dx0 == 0 && p.taps.w0 == 0 && p.taps.wrs == 1))
        return false;
    if (p.Ws <= 0 || 64 % p.Ws != 0) return false;
    *TR = 64 / p.Ws;
    if (*TR > p.Hs || p.Hs % *TR != 0 || p.M % 64 != 0) return false;
    return ((2 * *TR + 5) * p.xWp + 7) / 8 <= 128;
}

// Tiling of H x W OUTPUT planes (stride S, padded input planes xHp x xWp) into 64-pixel chunks of whole rows: TR rows per chunk, or
// (multi) TR / H whole images; HR x xWp = NHP padded input pixels hold the 3x3 halo of a chunk.
static bool wg_chunk_tiling(int H, int W, int S, int xHp, int xWp, WgHaloGeom* g) {
    if (W <= 0 || WG_CH % W != 0 || (S != 1 && S != 2)) return false;
    const int TR = WG_CH / W;
    if (TR <= H) { if (H % TR != 0) return false; g->multi = 0; g->HR = S * (TR - 1) + 3; }
    else { if (TR % H != 0) return false; g->multi = 1; g->HR = (TR / H) * xHp; }
    g->TR = TR;
    g->NHP = g->HR * xWp;
    return true;
}
// ... whose halo the halo kernel can stage (5 passes at stride 1, 13 at stride 2)
static bool wg_halo_tiling(int H, int W, int S, int xHp, int xWp, WgHaloGeom* g) {
    return wg_chunk_tiling(H, W, S, xHp, xWp, g) && g->NHP <= (S == 1 ? 160 : 416);
}
static bool wg_halo_geom(const WgradParams& p, WgHaloGeom* g) {
    g->total_pix = p.N * p.xHp * p.xWp;
    return wg_halo_tiling(p.Hs, p.Ws, p.istr, p.xHp, p.xWp, g);
}
// shape test of the halo kernel for a 3x3 pad-1 conv with H x W outputs (independent of the batch size)
bool vpd_wgrad_halo_shape_ok(int H, int W, int stride, int Hin, int Win) {
    if (stride == 2 && (!vpd_switches().wgrad_s2 || Hin != 2 * H || Win != 2 * W)) return false;
    WgHaloGeom g;
    return wg_halo_tiling(H, W, stride, Hin + 2, Win + 2, &g);
}

// A 1x1 pad-0 convolution in the caller's terms (one tap at padded offset (1, 1)) rewritten as the centre tap of the
// 3x3 halo form; false when `p` is not such a conv.
static bool wg_as_one_by_one(const WgradParams& p, WgradParams* q) {
    if (!(p.taps.nr == 1 && p.taps.nc == 1 && p.taps.dy0 == 1 && p.taps.dx0 == 1 && !p.one_by_one)) return false;
    *q = p;
    q->taps.nr = 3; q->taps.nc = 3; q->taps.dy0 = 0; q->taps.dys = 1; q->taps.dx0 = 0; q->taps.dxs = 1;
    q->taps.w0 = 0; q->taps.wrs = 0; q->taps.wcs = 0;
    q->one_by_one = 1;
    return true;
}

// Which kernel takes a problem stated in the caller's terms.  Every kernel but the atomics one OVERWRITES dw (no pre-zeroing needed).
enum WgKernel { WG_ATOMICS, WG_STEM, WG_HALO_3X3, WG_HALO_1X1 };
struct WgRoute {
    WgKernel kernel;
    WgradParams p;                       // as the kernel takes it: a 1x1 on the halo kernel is rewritten (wg_as_one_by_one)
    WgHaloGeom g;                        // halo kernels: the tiling (ksplit, cpb left to the launcher)
    int tr_stem;                         // stem kernel: output rows per chunk
    bool halo() const { return kernel == WG_HALO_3X3 || kernel == WG_HALO_1X1; }
};
static WgRoute wg_route(const WgradParams& p0) {
    WgRoute r;
    r.kernel = WG_ATOMICS; r.p = p0; r.g = WgHaloGeom{}; r.tr_stem = 0;
    if (wg_stem_eligible(p0, &r.tr_stem)) { r.kernel = WG_STEM; return r; }
    WgradParams p = p0;
    // 1x1 convolutions on the halo kernel (centre tap), no atomics.  As ONE launch per conv it is no faster than the atomics
    // kernel (both run at the ~4 TB/s their operand streams allow; ResNet-50: 9.90 vs 9.55 ms per step, ResNet-34: +12 us),
    // but it OVERWRITES its output and adds in a fixed order.  Default: ON where the caller asks for it (WgradParams::
    // prefer_halo_1x1 -- the plan sets it for the BasicBlock students, whose three down-sampling convs were the last fp32
    // atomics of the step: the ResNet-18/34 step is now reproducible bit for bit), otherwise off; VPD_WGRAD_1X1=0/1 forces.
    if (wg_as_one_by_one(p0, &p)) {
        const int env_1x1 = vpd_switches().wgrad_1x1;
        if (env_1x1 >= 0 ? !env_1x1 : !p0.prefer_halo_1x1) return r;
    }
    const bool s1 = p.istr == 1 && p.xHp == p.Hs + 2 && p.xWp == p.Ws + 2;
    // stride 2 (3x3 pad 1 / 1x1 pad 0, even input): taps 0..2 in padded input coordinates, forward order only
    const bool s2 = vpd_switches().wgrad_s2 && p.istr == 2 && p.xHp == 2 * p.Hs + 2 && p.xWp == 2 * p.Ws + 2 && p.taps.dy0 == 0 &&
                    p.taps.dys == 1 && p.taps.dx0 == 0 && p.taps.dxs == 1;
    if (!(p.slab && p.taps.nr == 3 && p.taps.nc == 3 && (s1 || s2) && p.xC == p.Kc && p.taps.dy0 >= 0 &&
          p.taps.dy0 + 2 * p.taps.dys >= 0 && p.taps.dy0 <= 2 &&
          p.taps.dy0 + 2 * p.taps.dys <= 2 && p.taps.dx0 >= 0 && p.taps.dx0 + 2 * p.taps.dxs >= 0 && p.taps.dx0 <= 2 &&
          p.taps.dx0 + 2 * p.taps.dxs <= 2 && wg_halo_geom(p, &r.g)))
        return r;
    r.kernel = p.one_by_one ? WG_HALO_1X1 : WG_HALO_3X3;
    r.p = p;
    return r;
}
// ... for a test that does not depend on the slab address
static WgRoute wg_route_any_slab(const WgradParams& p) {
    WgradParams q = p;
    if (!q.slab) q.slab = reinterpret_cast<float*>(16);
    return wg_route(q);
}
bool vpd_wgrad_overwrites(const WgradParams& p) { return wg_route(p).kernel != WG_ATOMICS; }

size_t vpd_wgrad_slab_bytes() { return (size_t)256 * 9 * 64 * 64 * sizeof(float); }   // ksplit * tiles <= 256

hipError_t vpd_launch_wgrad_reduce(const WgradParams& p, hipStream_t stream) {
    WgReduceGroup red = {};
    red.add(p.slab, p.dw, (long)(p.taps.nr == 1 ? 1 : 9) * p.Co * p.Kc, vpd_wgrad_split(p.M, p.Co, p.Kc, nullptr));
    wg_launch_reduce(red, stream);
    return hipGetLastError();
}

// Dynamic LDS of a halo launch: `ns` stages of a dz tile and `npass` 32-row halo passes; (pair) the branch's two dz tiles behind them
static size_t wg_ring_lds(int npass, int ns, bool pair) {
    return ((size_t)ns * (WG_CH + 32 * npass) + (pair ? 2 * WG_CH : 0)) * 64 * sizeof(bf16_t);
}
// f(integral_constant<int, NPASS>) for the instantiation that stages `npass` halo passes: 3, 4, 5 (stride 1), 10 or 13 (stride 2)
template <class F>
static void wg_npass_dispatch(int npass, F f) {
    if (npass <= 3) f(std::integral_constant<int, 3>{});
    else if (npass == 4) f(std::integral_constant<int, 4>{});
    else if (npass == 5) f(std::integral_constant<int, 5>{});
    else if (npass <= 10) f(std::integral_constant<int, 10>{});
    else f(std::integral_constant<int, 13>{});
}

// ---- grouped launch (see WgGroup) ----
// Split policy.  A problem's K (its 64-pixel chunks) is cut into `ksplit` tasks per output tile; every task beyond the
// first costs a 9*64*64 fp32 partial written to the slab and read back.  Tasks run in rounds of one per CU, so the cost
// of a choice is  rounds * (chunks_per_task * t_chunk + t_fixed) + slab bytes * 2 / bandwidth (+ the reduce launch),
// with the measured t_chunk 1.0 us (grouped launches: 124-242 us for 252 x 114 ... 176 x 256 chunk tasks), t_fixed 4 us,
// 4.5 TB/s.  Every task size from 8 to 512 chunks is tried.
// splits a problem may use at most: its slab share is capped at 16 MB (plan-time allocation)
int vpd_wgrad_group_max_splits(int Co, int Kc, int ntaps) {
    const size_t per = (size_t)ntaps * Co * Kc * 4;
    size_t cap = ((size_t)16 << 20) / per;
    if (cap > 64) cap = 64;
    return cap < 2 ? 1 : (int)cap;
}
size_t vpd_wgrad_group_slab_floats(int, int Co, int Kc, int ntaps) {
    const int cap = vpd_wgrad_group_max_splits(Co, Kc, ntaps);
    return cap <= 1 ? 0 : (size_t)cap * ntaps * Co * Kc;
}
// splits of `nch` chunks (at most `cap`) for tasks of about `target` chunks: equal tasks of *cpb chunks, the last one maybe shorter
static int wg_split_for_target(int nch, int cap, double target, int* cpb) {
    int k = (int)(nch / target + 0.5);
    k = k < 1 ? 1 : (k > cap ? cap : k);
    *cpb = (nch + k - 1) / k;
    return (nch + *cpb - 1) / *cpb;
}
static void wg_group_choose(const WgradParams* ps, int n, int* ksplit) {
    int nch[WG_GROUP_MAX], tiles[WG_GROUP_MAX], cap[WG_GROUP_MAX];
    for (int i = 0; i < n; ++i) {
        nch[i] = (ps[i].M + WG_CH - 1) / WG_CH;
        tiles[i] = (ps[i].Co / 64) * (ps[i].Kc / 64);
        cap[i] = vpd_wgrad_group_max_splits(ps[i].Co, ps[i].Kc, 9);
        if (cap[i] > nch[i]) cap[i] = nch[i];
    }
    const double t_chunk = 1.0, t_fixed = 4.0, bw = 4.5e6;       // us, us, bytes per us
    double best = 1e30;
    for (int target = 8; target <= 512; target += (target < 128 ? 1 : 4)) {
        int ks[WG_GROUP_MAX];
        long tasks = 0;
        int max_cpb = 0;
        double slab = 0.0;
        bool any = false;
        for (int i = 0; i < n; ++i) {
            int cpb;
            const int k = ks[i] = wg_split_for_target(nch[i], cap[i], (double)target, &cpb);
            tasks += (long)tiles[i] * k;
            max_cpb = cpb > max_cpb ? cpb : max_cpb;
            if (k > 1) { slab += (double)k * 9 * ps[i].Co * ps[i].Kc * 4; any = true; }
        }
        const double cost = (double)((tasks + 255) / 256) * (max_cpb * t_chunk + t_fixed) + 2.0 * slab / bw + (any ? 3.0 : 0.0);
        if (cost < best) {
            best = cost;
            for (int i = 0; i < n; ++i) ksplit[i] = ks[i];
        }
    }
}
bool vpd_wgrad_group_eligible(const WgradParams& p) { return wg_route_any_slab(p).halo(); }
// What vpd_launch_wgrad_group does with `n` problems: every problem's tiling and split (wg_group_choose), the task table's extent,
// the grid and the instantiation.  0: fine; 1: a plane the halo tiling does not take; 2: the problems' pass counts differ.
struct WgGroupPlan {
    int npass, inst, tasks, grid;
    int tiles[WG_GROUP_MAX], task_begin[WG_GROUP_MAX + 1];
    WgHaloGeom g[WG_GROUP_MAX];          // ksplit and cpb set
};
static int wg_group_plan(const WgradParams* ps, int n, WgGroupPlan* out) {
    int ks[WG_GROUP_MAX];
    wg_group_choose(ps, n, ks);
    out->tasks = 0; out->npass = 0;
    for (int i = 0; i < n; ++i) {
        const WgradParams& p = ps[i];
        WgHaloGeom g;
        if (!wg_halo_geom(p, &g)) return 1;
        const int np = (g.NHP + 31) / 32;
        if (out->npass == 0) out->npass = np;
        if (np != out->npass) return 2;                           // one stage: one geometry
        const int nchunks = (p.M + WG_CH - 1) / WG_CH;
        g.ksplit = ks[i];
        g.cpb = (nchunks + g.ksplit - 1) / g.ksplit;
        out->tiles[i] = (p.Co / 64) * (p.Kc / 64);
        out->task_begin[i] = out->tasks;
        out->tasks += out->tiles[i] * g.ksplit;
        out->g[i] = g;
    }
    out->task_begin[n] = out->tasks;
    out->grid = ((out->tasks + 7) / 8) * 8;                       // (the kernel's XCD remap wants a multiple of 8)
    // a stage's stride-1 convolutions: 3..5 passes (the group has no instantiation beyond 5)
    wg_npass_dispatch(out->npass, [&](auto np) { out->inst = decltype(np)::value > 5 ? 5 : decltype(np)::value; });
    return 0;
}
// host only: head4 = {pass instantiation, tasks, grid, halo passes}, per3 = {ksplit, cpb, tiles} per problem
int vpd_wgrad_group_dispatch(const WgradParams* ps, int n, int* head4, int* per3) {
    if (n < 1 || n > WG_GROUP_MAX) return -1;
    WgGroupPlan gp;
    if (const int rc = wg_group_plan(ps, n, &gp)) return rc;
    head4[0] = gp.inst; head4[1] = gp.tasks; head4[2] = gp.grid; head4[3] = gp.npass;
    for (int i = 0; i < n; ++i) { per3[3 * i] = gp.g[i].ksplit; per3[3 * i + 1] = gp.g[i].cpb; per3[3 * i + 2] = gp.tiles[i]; }
    return 0;
}
int vpd_wgrad_group_max() { return WG_GROUP_MAX; }
// ps[i].slab must point to vpd_wgrad_group_slab_floats() floats of its own (ignored when that is 0)
hipError_t vpd_launch_wgrad_group(const WgradParams* ps, int n, hipStream_t stream) {
    if (n < 1 || n > WG_GROUP_MAX) return hipErrorInvalidValue;
    const int ablate = wg_ablate();
    WgGroup grp = {};
    WgReduceGroup red = {};
    WgGroupPlan gp;
    if (wg_group_plan(ps, n, &gp) != 0) return hipErrorInvalidValue;
    grp.nprob = n;
    for (int i = 0; i < n; ++i) {
        WgradParams p = ps[i];
        p.ablate = ablate;
        if (gp.g[i].ksplit <= 1) p.slab = p.dw;                   // split 0 of a 1-split problem IS the gradient
        else red.add(p.slab, p.dw, (long)9 * p.Co * p.Kc, gp.g[i].ksplit);
        grp.tiles[i] = gp.tiles[i];
        grp.task_begin[i] = gp.task_begin[i];
        grp.p[i] = p;
        grp.g[i] = gp.g[i];
    }
    grp.task_begin[n] = gp.tasks;
    const size_t lds = wg_ring_lds(gp.npass <= 3 ? 3 : gp.npass, WG_NS, false);
    wg_npass_dispatch(gp.npass, [&](auto np) {
        constexpr int NP = decltype(np)::value > 5 ? 5 : decltype(np)::value;
        VPD_LAUNCH(conv_wgrad_halo_grouped_kernel<NP>, dim3(gp.grid), dim3(768), lds, stream, grp);
    });
    if (!(ablate & 16)) wg_launch_reduce(red, stream);
    return hipGetLastError();
}

// What vpd_launch_wgrad does with a problem: the route, the instantiation, the split and the grid (grid_x, ksplit).  The launcher
// launches exactly this; vpd_wgrad_dispatch reports it.
struct WgLaunchPlan {
    WgRoute r;
    int npass;          // halo kernels: 32-row passes of the halo
    int inst, ns;       // halo kernels: the NPASS instantiation and its ring stages; stem: 4 and 3; atomics: 0 and its 2 LDS buffers
    int ksplit, cpb;    // pixel splits (grid.y) and chunks per split: 64-pixel chunks, the atomics kernel's of 128 pixels
    int grid_x;         // output tiles (atomics kernel: per tap)
};
static bool wg_launch_plan(const WgradParams& p0, WgLaunchPlan* out) {
    if (p0.Kc % 64 != 0 || p0.Co % 64 != 0 || p0.M <= 0) return false;
    WgLaunchPlan& L = *out;
    L.r = wg_route(p0);
    L.npass = 0;
    const WgradParams& p = L.r.p;
    if (L.r.kernel == WG_STEM) {
        const int nchunks = p.M / 64;
        L.ksplit = nchunks < 256 ? nchunks : 256;
        L.cpb = (nchunks + L.ksplit - 1) / L.ksplit;
        L.ksplit = (nchunks + L.cpb - 1) / L.cpb;
        L.inst = 4; L.ns = 3; L.grid_x = 1;
        return true;
    }
    if (L.r.halo()) {
        L.grid_x = (p.Co / 64) * (p.Kc / 64);
        L.ksplit = vpd_wgrad_split(p.M, p.Co, p.Kc, &L.cpb);
        L.npass = (L.r.g.NHP + 31) / 32;                // 3..5 (stride 1), up to 10 / 13 (stride 2)
        wg_npass_dispatch(L.npass, [&](auto np) {
            L.inst = decltype(np)::value;
            L.ns = L.inst > 10 ? 2 : WG_NS;             // the 13-pass halo (layer4.0: four whole input planes) leaves room for two stages
        });
        return true;
    }
    const int tiles = (p.Co / 64) * (p.Kc / 64) * p.taps.nr * p.taps.nc;
    const int nchunks = (p.M + 127) / 128;
    // aim for ~1024 blocks; at least 4 chunks per block to amortise the atomics
    int ksplit = (1024 + tiles - 1) / tiles;
    if (ksplit > nchunks) ksplit = nchunks;
    if (ksplit < 1) ksplit = 1;
    int cpb = (nchunks + ksplit - 1) / ksplit;
    if (cpb < 4) cpb = nchunks < 4 ? nchunks : 4;
    L.ksplit = (nchunks + cpb - 1) / cpb;
    L.cpb = cpb; L.inst = 0; L.ns = 2; L.grid_x = tiles;
    return true;
}
// host only: out9 = {kernel (WgKernel: 0 atomics, 1 stem, 2 halo 3x3, 3 halo 1x1), pass instantiation, ring stages, TR, multi, NHP,
// ksplit, cpb, grid.x}; TR / multi / NHP are the halo tiling's (stem: TR and the input pixels a chunk stages; atomics: 0).  false:
// the launcher refuses the problem.
bool vpd_wgrad_dispatch(const WgradParams& p0, int* out9) {
    WgLaunchPlan L;
    if (!wg_launch_plan(p0, &L)) return false;
    const bool stem = L.r.kernel == WG_STEM, halo = L.r.halo();
    const int v[9] = {(int)L.r.kernel, L.inst, L.ns, stem ? L.r.tr_stem : halo ? L.r.g.TR : 0, halo ? L.r.g.multi : 0,
                      stem ? (2 * L.r.tr_stem + 5) * L.r.p.xWp : halo ? L.r.g.NHP : 0, L.ksplit, L.cpb, L.grid_x};
    memcpy(out9, v, sizeof v);
    return true;
}

hipError_t vpd_launch_wgrad(const WgradParams& p0, hipStream_t stream) {
    WgLaunchPlan L;
    if (!wg_launch_plan(p0, &L)) return hipErrorInvalidValue;
    WgradParams p = L.r.p;
    p.ablate = wg_ablate();
    const dim3 grid(L.grid_x, L.ksplit);
    if (L.r.kernel == WG_STEM) {
        const long xelems = (long)p.N * p.xHp * p.xWp * 8 + 64;
        VPD_LAUNCH(conv_wgrad_stem_kernel, grid, dim3(768), wg_ring_lds(L.inst, L.ns, false), stream, p, L.r.tr_stem, L.cpb, xelems);
        WgReduceGroup red = {};
        red.add(p.slab, p.dw, (long)7 * 64 * 64, L.ksplit);
        wg_launch_reduce(red, stream);
        return hipGetLastError();
    }
    if (L.r.halo()) {
        WgHaloGeom g = L.r.g;
        g.ksplit = L.ksplit; g.cpb = L.cpb;
        wg_npass_dispatch(L.npass, [&](auto np) {
            constexpr int NP = decltype(np)::value;
            constexpr int NS = NP > 10 ? 2 : WG_NS;
            VPD_LAUNCH((conv_wgrad_halo_kernel<NP, NS>), grid, dim3(768), wg_ring_lds(NP, NS, false), stream, p, g);
        });
        if (p.defer_reduce || VPD_ABL(p, 16)) return hipGetLastError();
        return vpd_launch_wgrad_reduce(p0, stream);
    }
    p.chunks_per_block = L.cpb;
    const size_t lds = 64 * 1024;     // max(staging 2*2*16 KiB, reduction 64 KiB)
    VPD_LAUNCH(conv_wgrad_kernel, grid, dim3(256), lds, stream, p);
    return hipGetLastError();
}

// ---- pair launch (conv_wgrad_halo_pair_kernel): a down-sampling BasicBlock's 3x3 stride-2 conv1 (p3) with its 1x1 stride-2 branch (p1),
// both in the caller's terms ----
#ifndef VPD_WG_PAIR_NS
#define VPD_WG_PAIR_NS 3      // stages of the dz + halo ring of the 10-pass pair launch (-DVPD_WG_PAIR_NS=2: two stages of everything)
#endif
// Dynamic LDS of a pair launch whose halo takes `npass` 32-row passes on an `ns`-stage ring (ns 0: the launcher's ring depth), the
// branch's two dz tiles behind it.  false: more than the 160 KB of a CU -- such a layout is never launched.
static bool wg_pair_lds(int npass, int ns, size_t* bytes) {
    if (ns <= 0) ns = npass > 10 ? 2 : VPD_WG_PAIR_NS;
    *bytes = wg_ring_lds(npass <= 10 ? 10 : 13, ns, true);
    return ns >= 2 && npass <= 13 && *bytes <= (size_t)160 * 1024;
}
// Host-only: the LDS bytes of the pair launch for an H x W OUTPUT (input 2H x 2W, border 1).  ns 0: the launcher's ring depth.
// 0: fits; 1: the layout is over 160 KB (the launcher refuses it); -1: no halo geometry for this output size.
int vpd_wgrad_pair_lds_query(int H, int W, int ns, long long* bytes) {
    WgHaloGeom g;
    if (H <= 0 || !wg_halo_tiling(H, W, 2, 2 * H + 2, 2 * W + 2, &g)) return -1;
    size_t b = 0;
    const bool ok = wg_pair_lds((g.NHP + 31) / 32, ns, &b);
    if (bytes) *bytes = (long long)b;
    return ok ? 0 : 1;
}
// p3's route when (p3, p1) can share a launch, else the atomics route
static WgRoute wg_pair_route(const WgradParams& p3, const WgradParams& p1) {
    WgRoute none = {};
    none.kernel = WG_ATOMICS;
    if (!vpd_switches().wgrad_ds_ride) return none;
    const WgRoute r3 = wg_route(p3);
    if (r3.kernel != WG_HALO_3X3 || wg_route(p1).kernel != WG_HALO_1X1 || p1.one_by_one) return none;
    if (p3.istr != 2 || p3.Kc % 64 != 0 || p3.Co % 64 != 0 || p3.M <= 0) return none;
    const bool same = p1.x == p3.x && p1.xHp == p3.xHp && p1.xWp == p3.xWp && p1.xC == p3.xC && p1.N == p3.N && p1.Hs == p3.Hs &&
                      p1.Ws == p3.Ws && p1.istr == p3.istr && p1.Kc == p3.Kc && p1.Co == p3.Co && p1.M == p3.M && p1.dzHp == p3.dzHp &&
                      p1.dzWp == p3.dzWp && p1.dzC == p3.dzC && p1.dzpad == p3.dzpad;
    return same ? r3 : none;
}
bool vpd_wgrad_pair_ok(const WgradParams& p3, const WgradParams& p1) { return wg_pair_route(p3, p1).halo(); }
// one launch sums both slabs: the same split and the same thread groups as a launch of vpd_launch_wgrad_reduce each, element by element
hipError_t vpd_launch_wgrad_pair_reduce(const WgradParams& p3, const WgradParams& p1, hipStream_t stream) {
    const int ksplit = vpd_wgrad_split(p3.M, p3.Co, p3.Kc, nullptr);
    WgReduceGroup red = {};
    red.add(p3.slab, p3.dw, (long)9 * p3.Co * p3.Kc, ksplit);
    red.add(p1.slab, p1.dw, (long)p3.Co * p3.Kc, ksplit);
    wg_launch_reduce(red, stream);
    return hipGetLastError();
}
hipError_t vpd_launch_wgrad_pair(const WgradParams& p3, const WgradParams& p1, hipStream_t stream) {
    const WgRoute r = wg_pair_route(p3, p1);
    if (!r.halo()) return hipErrorInvalidValue;
    WgradParams p = r.p;
    p.ablate = wg_ablate();
    WgHaloGeom g = r.g;
    const int tiles = (p.Co / 64) * (p.Kc / 64);
    g.ksplit = vpd_wgrad_split(p.M, p.Co, p.Kc, &g.cpb);
    const int npass = (g.NHP + 31) / 32;
    size_t lds = 0;
    if (!wg_pair_lds(npass, 0, &lds)) return hipErrorInvalidValue;
    const WgPair pr{p1.dz, p1.slab};
    wg_npass_dispatch(npass, [&](auto np) {
        constexpr int NP = decltype(np)::value <= 10 ? 10 : 13;
        VPD_LAUNCH((conv_wgrad_halo_pair_kernel<NP, (NP > 10 ? 2 : VPD_WG_PAIR_NS)>), dim3(tiles, g.ksplit), dim3(768), lds, stream, p, g, pr);
    });
    if (p.defer_reduce || VPD_ABL(p, 16)) return hipGetLastError();
    return vpd_launch_wgrad_pair_reduce(p3, p1, stream);
}

// ---------------------------------------------------------------------------
// 128(co) x 64(ci) weight-gradient tiles, persistent blocks with a host-built schedule ("wg2").
//
// Why: the grouped 64 x 64 kernel above is bound by its operand stream, not by the matrix cores -- every launch moves
// 24-28 KB of LDS-DMA per 64-pixel chunk and tile, and the chip delivers ~5.4 TB/s of such traffic however many CUs ask
// (layer2's group: 1.2 us per chunk on 256 CUs; layer3's: 0.74 us on the 176 CUs it fills; 0.55 us is the MFMA time).
// A 128 x 64 tile reads the x halo ONCE for twice the output channels: 16 KB of dz + 13-18 KB of halo per chunk for
// twice the FLOPs (-35 % bytes per FLOP).  Its accumulators (9 taps x 128 x 64 fp32 = 288 KB) need all 512 registers of
// every SIMD lane, so there are no loader waves: 8 waves (two per SIMD, 144 accumulator registers each: ci tile =
// wave & 3, co half = wave >> 2) issue their own share of the LDS-DMA right after the chunk barrier and then run
// 72 MFMAs per chunk; a 4-stage ring keeps two chunks in flight.
// Scheduling: a launch takes the weight gradients of one or MORE ResNet stages (layer4's wait for layer3's: 160 + 176
// tasks of equal length fill the 256 CUs exactly where each stage alone leaves a third of the chip idle).  The host
// picks a uniform pixel split per problem with a cost model, orders the (problem, split, tile) tasks longest first and
// deals them to the least loaded block (LPT), blocks of one XCD taking consecutive tasks (the tiles that share pixels
// then stream from that XCD's L2); block b runs its list from a table in device memory.
// ---------------------------------------------------------------------------
#define WG2_NS 4
#define WG2_MAX 18
static_assert(WG2_MAX <= WG_GROUP_MAX, "WgReduceGroup holds one entry per problem of a launch");
struct Wg2Group {
    int nprob;
    const int4* tasks;                         // device: (problem, tile, split, -)
    const int* blk_begin;                      // device: [grid + 1] first task of each block
    int stage_elems;                           // bf16 elements of the whole ring (the launch's dynamic LDS)
    int kind[WG2_MAX];                         // 0: 3x3 (wg2_task); 1 / 2 / 4: 1x1 on 128 x 64 / 128 x 128 / 128 x 256 tiles (wg2_task_1x1); + 16: 256 output channels per tile
    WgradParams p[WG2_MAX];
    WgHaloGeom g[WG2_MAX];
};

template <int N>
static __device__ __forceinline__ void wg2_waitcnt() { asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory"); }
static __device__ __forceinline__ void wg2_wait_allow(int n) {      // n: wave-uniform, one of 0, k, 2k with k in 3..5
    switch (n) {
        case 0: wg2_waitcnt<0>(); break;
        case 3: wg2_waitcnt<3>(); break;
        case 4: wg2_waitcnt<4>(); break;
        case 5: wg2_waitcnt<5>(); break;
        case 6: wg2_waitcnt<6>(); break;
        case 8: wg2_waitcnt<8>(); break;
        case 10: wg2_waitcnt<10>(); break;
        default: wg2_waitcnt<0>(); break;
    }
}

// LDS-DMA of 16 bytes per lane (1 KiB per wave) as inline assembly.  The builtin would make hipcc's wait-count pass put
// s_waitcnt vmcnt(0) in front of the first ds_read that follows it in program order -- a wave that both streams and
// computes would then wait for the tile it has JUST requested before touching the one that landed two chunks ago.  The
// assembly form is opaque to that pass; the kernel's own counted vmcnt waits + the chunk barrier order the ring.
static __device__ __forceinline__ void wg2_lds_dma16(const void* gsrc, unsigned lds_byte_addr) {
    asm volatile("s_mov_b32 m0, %1\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, off" ::"v"(gsrc), "s"(lds_byte_addr) : "memory");
}

// The chunks of a task and the running position of the NEXT chunk to issue: c chunks issued so far; image index b and first
// output row y (non-multi) of that chunk.
struct Wg2Walk {
    int chunk_begin, nch, ipc, c, b, y;
    __device__ __forceinline__ Wg2Walk(const WgradParams& p, const WgHaloGeom& g, int split) {
        nch = wg_chunk_range(p.M, split, g.cpb, &chunk_begin);
        const int cpi = g.multi ? 1 : p.Hs / g.TR;                    // chunks per image (non-multi)
        ipc = g.multi ? g.TR / p.Hs : 1;                              // images per chunk (multi)
        c = 0;
        if (g.multi) { b = chunk_begin * ipc; y = 0; }
        else { b = chunk_begin / cpi; y = (chunk_begin - b * cpi) * g.TR; }
    }
    __device__ __forceinline__ void advance(const WgradParams& p, const WgHaloGeom& g) {
        ++c;
        if (g.multi) b += ipc;
        else { y += g.TR; if (y >= p.Hs) { y = 0; ++b; } }
    }
};
// dz LDS-DMA instruction i of a chunk (64-channel block i >> 3 from channel co0 on, pixel rows (i & 7) * 8 ..): the chunk-invariant
// element offset of this lane's 16 bytes from the chunk's first pixel, and its pixel row in the chunk
static __device__ __forceinline__ void wg2_dz_lane(const WgradParams& p, const WgHaloGeom& g, int i, int co0, int lane, int* zlane, int* zrow) {
    const int piece = lane & 7, row = (i & 7) * 8 + (lane >> 3);
    const int lr = row / p.Ws, xx = row - lr * p.Ws;
    const int img = g.multi ? lr / p.Hs : 0, yy = g.multi ? lr % p.Hs : lr;
    *zlane = ((img * p.dzHp + yy + p.dzpad) * p.dzWp + xx + p.dzpad) * p.dzC + co0 + (i >> 3) * 64 + wg_src_piece(row, piece) * 8;
    *zrow = row;
}
// the NZ dz instructions of this wave for the walk's next chunk, into the stage at LDS byte address st_lds
template <int NZ>
static __device__ __forceinline__ void wg2_issue_dz(const WgradParams& p, const Wg2Walk& w, int wave, const int (&zlane)[NZ],
                                                    const int (&zrow)[NZ], unsigned st_lds) {
    const int ch = w.chunk_begin + w.c;
    const bf16_t* zb = p.dz + ((size_t)w.b * p.dzHp + w.y) * p.dzWp * p.dzC;
#pragma unroll
    for (int k = 0; k < NZ; ++k) {
        const int i = wave * NZ + k;
        const bf16_t* src = (ch * WG_CH + zrow[k] < p.M) ? zb + zlane[k]
                                                         : p.dz + (zlane[k] & 63);      // zero border pixel (0, 0) of image 0
        wg2_lds_dma16(src, st_lds + (unsigned)(i * 8 * 64 * 2));
    }
}
// The pipeline of a task on an NS-stage ring (`per` LDS-DMA instructions per wave and chunk): issue() requests the walk's next chunk
// and ADVANCES w (w.c chunks issued so far),
// compute(c, mid) consumes chunk c and calls mid() between its two k-steps.
template <class Issue, class Compute>
static __device__ __forceinline__ void wg2_pipeline(int NS, int per, int cohalf, Wg2Walk& w, Issue issue, Compute compute) {
    // every wave is done with the previous task's ring (and its stores are on their way) before new tiles land in it
    __builtin_amdgcn_s_barrier();
#pragma unroll
    for (int k = 0; k < 3; ++k)
        if (k < NS - 1 && k < w.nch) issue();
    for (int c = 0; c < w.nch; ++c) {
        // this wave's share of chunk c has landed when at most its instructions of the younger chunks are outstanding
        int ahead = w.nch - 1 - c;
        ahead = ahead < NS - 2 ? ahead : NS - 2;
        wg2_wait_allow(ahead * per);                                  // (NS == 2: 0; NS == 4: per <= 5 by eligibility)
        __builtin_amdgcn_s_barrier();                                 // READY_c: all shares landed; everyone finished chunk c-1
        // chunk c + NS - 1 goes into the stage chunk c - 1 used.  The second wave of every SIMD requests its share between the
        // two k-steps instead, so that the two waves stop running their read / MFMA phases in lockstep (same-box A/B 490 ->
        // 458 us per step for the class; profiles/r02_negative_results.txt has the variants)
        const bool do_issue = w.c < w.nch;
        if (do_issue && !cohalf) issue();
        compute(c, [&]() __attribute__((always_inline)) { if (do_issue && cohalf) issue(); });
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // (already true after the last chunk's wait: belt and braces)
}

static __device__ __forceinline__ void wg2_task(const WgradParams& p, const WgHaloGeom& g, int tile, int split,
                                                bf16_t* ring, int lds_elems) {
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);        // 0..7
    const int ctile = wave & 3, cohalf = wave >> 2;
    const int W = p.Ws, H = p.Hs, Wp = p.xWp, S = p.istr;         // W, H: OUTPUT dims; S = 1 or 2 (3x3 pad 1: input pixel S*y + r)
    const int kct = p.Kc >> 6;
    const int co0 = (tile / kct) * 128;
    const int ci0 = (tile % kct) * 64;
    Wg2Walk w(p, g, split);
    const int nhi = (g.NHP + 7) >> 3;                                 // halo LDS-DMA instructions per chunk (8 pixels each)
    const int nh_mine = (nhi - wave + 7) >> 3;                        // this wave's: wave, wave + 8, ...
    const int per = 2 + nh_mine;                                      // its LDS-DMA instructions per chunk
    // ring of THIS problem: four stages when they fit the launch's LDS (stride 1: 28-36 KB each), else two (stride 2: the
    // halo of a 64-pixel chunk is 306-400 input pixels, 55-66 KB per stage); tasks run one after the other in a block
    const int STAGE = (128 + 8 * nhi) * 64;
    const int NS = 4 * STAGE <= lds_elems ? 4 : 2;

    // ---- LDS-DMA side: chunk-invariant per-lane element offsets (32-bit), the chunk's part is wave-uniform (64-bit) ----
    const int piece = lane & 7, lrow = lane >> 3;
    int zlane[2], zrow[2];
#pragma unroll
    for (int k = 0; k < 2; ++k) wg2_dz_lane(p, g, wave * 2 + k, co0, lane, &zlane[k], &zrow[k]);      // (block i >> 3 = cohalf)
    const unsigned ring_lds = (unsigned)(size_t)(wg_lptr_t)ring;      // LDS byte address of the ring
    auto issue = [&]() __attribute__((always_inline)) {
        const unsigned st_lds = __builtin_amdgcn_readfirstlane(ring_lds + (unsigned)((w.c & (NS - 1)) * STAGE * 2));
        wg2_issue_dz<2>(p, w, wave, zlane, zrow, st_lds);
        const int gp0 = (w.b * p.xHp + S * w.y) * Wp;
        const bf16_t* xb = p.x + ci0;
        for (int k = 0; k < nh_mine; ++k) {
            const int hp = (wave + 8 * k) * 8 + lrow;
            const int cpc = wg_src_piece(hp, piece);
            int gp = gp0 + hp;
            gp = gp < g.total_pix ? gp : g.total_pix - 1;
            const bf16_t* src = xb + (size_t)gp * p.xC + cpc * 8;
            wg2_lds_dma16(src, st_lds + (unsigned)((128 + (wave + 8 * k) * 8) * 64 * 2));
        }
        w.advance(p, g);
    };

    // ---- MFMA side: chunk-invariant LDS BYTE offsets (within a stage) of this lane's transposed reads.  A (dz) operand:
    // co tile a only changes the 32-byte granule, offA(a) = offA(0) ^ (a << 5); B (x halo) operand: one offset per k-step,
    // tap and 4-row half, two 16-bit values per register (a stage is < 64 KiB). ----
    const int gq = lane >> 4, i16 = lane & 15, q = i16 >> 2, pp = i16 & 3;
    int offA0[2];
    unsigned offB[2][9];                                              // [ks][tap]: low half h = 0, high half h = 1 (bytes from the halo's base: < 64 KiB)
    {
        const int ra = 8 * gq + q;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int r = ra + 4 * h;
            offA0[h] = 2 * (cohalf * 64 * 64 + wg_swz_off(r, 4 * pp));
        }
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            int hmv[2];
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const int pk = 32 * ks + 8 * gq + 4 * h + q;
                const int lr = pk / W;
                const int xx = pk - lr * W;
                const int hrow = g.multi ? (lr / H) * p.xHp + S * (lr % H) : S * lr;
                hmv[h] = hrow * Wp + S * xx;
            }
#pragma unroll
            for (int t = 0; t < 9; ++t) {
                unsigned v = 0;
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    const int r = hmv[h] + (p.taps.dy0 + (t / 3) * p.taps.dys) * Wp + (p.taps.dx0 + (t % 3) * p.taps.dxs);
                    const unsigned o = 2u * (unsigned)wg_swz_off(r, ctile * 16 + 4 * pp);      // from the halo's base
                    v |= o << (16 * h);
                }
                offB[ks][t] = v;
            }
        }
    }
    f32x4 acc[9][4];
#pragma unroll
    for (int t = 0; t < 9; ++t)
#pragma unroll
        for (int a = 0; a < 4; ++a) acc[t][a] = f32x4{0.f, 0.f, 0.f, 0.f};

    wg2_pipeline(NS, per, cohalf, w, issue, [&](int c, auto mid) __attribute__((always_inline)) {
        const wg_lds_cp sb = (wg_lds_cp)(const char*)(ring + (c & (NS - 1)) * STAGE);
        // Explicit software pipeline of the LDS reads (pinned with sched_barrier: left alone, hipcc waits for every B
        // fragment right before its four MFMAs): the A fragments of both k-steps are resident (the second set is read
        // during the first k-step's last taps), the B fragment of tap t + 2 is requested before the MFMAs of tap t.
        auto ldA = [&](int ks, int a) __attribute__((always_inline)) {
            const wg_lds_cp a0 = sb + ks * 32 * 128 + offA0[0], a1 = sb + ks * 32 * 128 + offA0[1];
            return wg_tr_read((wg_lds_cp)(size_t)((unsigned)(size_t)a0 ^ (unsigned)(a << 5)), (wg_lds_cp)(size_t)((unsigned)(size_t)a1 ^ (unsigned)(a << 5)));
        };
        auto ldB = [&](int ks, int t) __attribute__((always_inline)) {
            const unsigned v = offB[ks][t];
            return wg_tr_read(sb + 128 * 128 + (v & 0xffffu), sb + 128 * 128 + (v >> 16));
        };
        {
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
                if (ks == 1) mid();
                bf16x8 az[4];
#pragma unroll
                for (int a = 0; a < 4; ++a) az[a] = ldA(ks, a);
#pragma unroll
                for (int tg = 0; tg < 3; ++tg) {
                    bf16x8 bx[3];
#pragma unroll
                    for (int u = 0; u < 3; ++u) bx[u] = ldB(ks, tg * 3 + u);
#pragma unroll
                    for (int u = 0; u < 3; ++u)
#pragma unroll
                        for (int a = 0; a < 4; ++a)
                            acc[tg * 3 + u][a] = VPD_MFMA16(az[a], bx[u], acc[tg * 3 + u][a]);
                }
            }
        }
    });
    // acc[t][a][j] = partial dW[tap t][co0 + 64*cohalf + a*16 + 4*gq + j][ci0 + 16*ctile + i16]
    float* out = g.ksplit > 1 ? p.slab + (size_t)split * 9 * p.Co * p.Kc : p.dw;
#pragma unroll
    for (int t = 0; t < 9; ++t) {
        const int wsl = p.taps.w0 + (t / 3) * p.taps.wrs + (t % 3) * p.taps.wcs;
        wg_store_tile(out + ((size_t)wsl * p.Co + co0 + cohalf * 64) * p.Kc + ci0 + 16 * ctile + i16, p.Kc, acc[t], gq);
    }
}

// 1x1 convolutions (pad 0; stride 1 or 2) as tasks of the same persistent launch: dW[Co][Ci] = sum_m dz[m][Co]^T x[pix(m)][Ci],
// a plain tall-K GEMM.  Tile TCO(co) x TCI(ci), TCO = 128, TCI = 64, 128 or 256; per 64-pixel chunk the dz tile (two [64][64] halves) and the x
// tile (TCI / 64 blocks of [64 px][64 ci], gathered pixel by pixel from the padded activation: (S*y + 1, S*x + 1)) come in by
// LDS-DMA into a 4-stage ring; wave (ctile, cohalf) owns co 64*cohalf .. +63 and ci 16*ctile (+ 64 for the second block):
// 8 or 16 MFMAs per chunk against 24-32 KB of operands -- these tasks are bound by the stream (51-65 FLOP per staged byte),
// like the operator itself at small channel counts; what the launch buys over conv_wgrad_kernel is no atomics (fixed-order
// slab sums), no launch of its own, and tiles that stream 2-4x fewer bytes per FLOP than its 64 x 64 ones.
#ifndef WG2_NS256
#define WG2_NS256 2
#endif
template <int TCI, int TCO = 128>
static __device__ __forceinline__ void wg2_task_1x1(const WgradParams& p, const WgHaloGeom& g, int tile, int split,
                                                    bf16_t* ring) {
    constexpr int NB = TCI / 64;
    constexpr int NZ = TCO / 64;                                      // dz blocks of [64 px][64 co]; a wave owns NZ / 2 of them
    constexpr int NA = NZ * 2;                                        // 16-channel co groups per wave
    constexpr int NS = (TCI == 256 || TCO == 256) ? WG2_NS256 : 4;    // (40-48 KB stages: two of them; three measured equal)
    constexpr int STAGE = (TCO + 64 * NB) * 64;                       // bf16 elements
    constexpr int PER = NZ + NB;                                      // LDS-DMA instructions per wave and chunk
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int ctile = wave & 3, cohalf = wave >> 2;
    const int W = p.Ws, H = p.Hs, S = p.istr;
    const int kct = p.Kc / TCI;
    const int co0 = (tile / kct) * TCO;
    const int ci0 = (tile % kct) * TCI;
    Wg2Walk w(p, g, split);

    const int piece = lane & 7, lrow = lane >> 3;
    int zlane[NZ], zrow[NZ], xlane[NB];
#pragma unroll
    for (int k = 0; k < NZ; ++k) wg2_dz_lane(p, g, wave * NZ + k, co0, lane, &zlane[k], &zrow[k]);
#pragma unroll
    for (int k = 0; k < NB; ++k) {
        const int j = wave * NB + k;                                  // x instruction: block j >> 3, rows (j & 7) * 8 ..
        const int row = (j & 7) * 8 + lrow;
        const int lr = row / W, xx = row - lr * W;
        const int cpc = wg_src_piece(row, piece);
        const int img = g.multi ? lr / H : 0, yy = g.multi ? lr % H : lr;
        xlane[k] = ((img * p.xHp + S * yy + 1) * p.xWp + S * xx + 1) * p.xC + ci0 + (j >> 3) * 64 + cpc * 8;
    }
    const unsigned ring_lds = (unsigned)(size_t)(wg_lptr_t)ring;
    auto issue = [&]() __attribute__((always_inline)) {
        const int ch = w.chunk_begin + w.c;
        const unsigned st_lds = __builtin_amdgcn_readfirstlane(ring_lds + (unsigned)((w.c % NS) * STAGE * 2));
        wg2_issue_dz<NZ>(p, w, wave, zlane, zrow, st_lds);
        const bf16_t* xb = p.x + ((size_t)w.b * p.xHp + S * w.y) * p.xWp * p.xC;
#pragma unroll
        for (int k = 0; k < NB; ++k) {
            const int j = wave * NB + k;
            // rows past the end of a ragged last chunk meet zero dz rows: any finite x will do (the first pixels of the tensor)
            const bf16_t* src = (ch * WG_CH + (j & 7) * 8 + lrow < p.M) ? xb + xlane[k] : p.x + (xlane[k] & 63);
            wg2_lds_dma16(src, st_lds + (unsigned)((TCO + j * 8) * 64 * 2));
        }
        w.advance(p, g);
    };

    const int gq = lane >> 4, i16 = lane & 15, q = i16 >> 2, pp = i16 & 3;
    int offA0[2], offB0[2];                                           // byte offsets within a stage (k-step 0; +32 rows for k-step 1)
    {
        const int ra = 8 * gq + q;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int r = ra + 4 * h;
            offA0[h] = 2 * (cohalf * (TCO / 2) * 64 + wg_swz_off(r, 4 * pp));
            offB0[h] = 2 * (TCO * 64 + wg_swz_off(r, ctile * 16 + 4 * pp));
        }
    }
    f32x4 acc[NB][NA];
#pragma unroll
    for (int u = 0; u < NB; ++u)
#pragma unroll
        for (int a = 0; a < NA; ++a) acc[u][a] = f32x4{0.f, 0.f, 0.f, 0.f};

    wg2_pipeline(NS, PER, cohalf, w, issue, [&](int c, auto mid) __attribute__((always_inline)) {
        const wg_lds_cp sb = (wg_lds_cp)(const char*)(ring + (c % NS) * STAGE);
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            if (ks == 1) mid();
            bf16x8 bx[NB];
            const wg_lds_cp a0 = sb + ks * 32 * 128 + offA0[0], a1 = sb + ks * 32 * 128 + offA0[1];
#pragma unroll
            for (int u = 0; u < NB; ++u)
                bx[u] = wg_tr_read(sb + u * 64 * 128 + ks * 32 * 128 + offB0[0], sb + u * 64 * 128 + ks * 32 * 128 + offB0[1]);
#pragma unroll
            for (int zb = 0; zb < NZ / 2; ++zb) {      // this wave's dz blocks, one at a time (four co groups of fragments live)
                bf16x8 az[4];
#pragma unroll
                for (int a = 0; a < 4; ++a)      // (16-channel group a of the block by the XOR)
                    az[a] = wg_tr_read((wg_lds_cp)(size_t)(((unsigned)(size_t)a0 ^ (unsigned)(a << 5)) + zb * 64 * 128),
                                       (wg_lds_cp)(size_t)(((unsigned)(size_t)a1 ^ (unsigned)(a << 5)) + zb * 64 * 128));
#pragma unroll
                for (int u = 0; u < NB; ++u)
#pragma unroll
                    for (int a = 0; a < 4; ++a)
                        acc[u][zb * 4 + a] = VPD_MFMA16(az[a], bx[u], acc[u][zb * 4 + a]);
            }
        }
    });
    // acc[u][a][j] = partial dW[co0 + (TCO/2)*cohalf + a*16 + 4*gq + j][ci0 + 64*u + 16*ctile + i16]
    float* out = g.ksplit > 1 ? p.slab + (size_t)split * p.Co * p.Kc : p.dw;
#pragma unroll
    for (int u = 0; u < NB; ++u) {
        if (p.transposed) {      // out[ci][co]: this lane's four consecutive co of one ci are 16 contiguous bytes
            float* o = out + (size_t)(ci0 + 64 * u + 16 * ctile + i16) * p.Co + co0 + cohalf * (TCO / 2) + 4 * gq;
#pragma unroll
            for (int a = 0; a < NA; ++a) *reinterpret_cast<f32x4*>(o + a * 16) = acc[u][a];
            continue;
        }
        wg_store_tile(out + (size_t)(co0 + cohalf * (TCO / 2)) * p.Kc + ci0 + 64 * u + 16 * ctile + i16, p.Kc, acc[u], gq);
    }
}

__global__ __launch_bounds__(512) void conv_wgrad128_persistent_kernel(const Wg2Group grp) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    bf16_t* ring = reinterpret_cast<bf16_t*>(smem);
    const int t0 = grp.blk_begin[blockIdx.x], t1 = grp.blk_begin[blockIdx.x + 1];
    for (int t = t0; t < t1; ++t) {
        const int4 tk = grp.tasks[t];
        const int pi = __builtin_amdgcn_readfirstlane(tk.x);
        const int tile = __builtin_amdgcn_readfirstlane(tk.y), split = __builtin_amdgcn_readfirstlane(tk.z);
        const int kind = grp.kind[pi];
        if (kind == 0) wg2_task(grp.p[pi], grp.g[pi], tile, split, ring, grp.stage_elems);
        else if (kind == 1) wg2_task_1x1<64>(grp.p[pi], grp.g[pi], tile, split, ring);
        else if (kind == 2) wg2_task_1x1<128>(grp.p[pi], grp.g[pi], tile, split, ring);
        else if (kind == 4) wg2_task_1x1<256>(grp.p[pi], grp.g[pi], tile, split, ring);
        else if (kind == 17) wg2_task_1x1<64, 256>(grp.p[pi], grp.g[pi], tile, split, ring);
        else wg2_task_1x1<128, 256>(grp.p[pi], grp.g[pi], tile, split, ring);
    }
}

// ---- host side: eligibility, split choice, LPT schedule ----
// kind of a problem for the persistent launch and its chunk geometry: -1 not eligible, 0 3x3, else 1x1 (pad 0: one tap at padded
// offset (1, 1)) on tiles of 128 co x 64 / 128 / 256 ci (1 / 2 / 4), + 16: 256 co
static int wg2_kind_1x1(const WgradParams& p, WgHaloGeom* g) {
    if (!vpd_switches().wg2_1x1 || !(p.taps.nr == 1 && p.taps.nc == 1 && p.taps.dy0 == 1 && p.taps.dx0 == 1) || p.one_by_one) return -1;
    if (p.Co % 128 || p.Kc % 64 || p.xC != p.Kc || p.dzC % 128 || p.dzpad < 1 || (p.istr != 1 && p.istr != 2)) return -1;
    if (p.xHp != p.istr * p.Hs + 2 || p.xWp != p.istr * p.Ws + 2 || p.dzHp != p.Hs + 2 * p.dzpad || p.dzWp != p.Ws + 2 * p.dzpad) return -1;
    *g = WgHaloGeom{};
    if (!wg_chunk_tiling(p.Hs, p.Ws, p.istr, p.xHp, p.xWp, g)) return -1;
    g->NHP = 64; g->HR = 0; g->total_pix = p.N * p.xHp * p.xWp;      // no halo: the 64 pixels of the chunk
    // 128 x 256 tiles: a dz chunk serves four ci blocks.  These tasks are bound by the bytes they stream (the tiles of a pixel range
    // do not run close enough in time to meet in an XCD's 4 MB L2): ResNet-50's grouped launches 1,240 -> 955 us per step, same
    // box.  256 x 256 tiles (64 KB stages, 128 accumulator registers) were slower again, 976 vs 925 us: fewer tiles, more splits
    if (p.Kc % 256 == 0) return 4;
    // few input channels, many output channels (a Bottleneck's closing conv): 256 x 64 / 256 x 128 tiles -- the x chunk serves twice
    // the output channels
    return (p.Kc % 128 == 0 ? 2 : 1) + (vpd_switches().wg2_tco256 && p.Co % 256 == 0 ? 16 : 0);
}
static inline int wg2_nb(int kind) { return kind & 15; }                     // 64-channel ci blocks per tile
static inline int wg2_tco(int kind) { return kind >= 16 ? 256 : 128; }       // output channels per tile
static int wg2_kind(const WgradParams& p, WgHaloGeom* g) {
    if (!vpd_switches().wg2) return -1;
    const int k1 = wg2_kind_1x1(p, g);
    if (k1 > 0) return k1;
    if (p.Co % 128 != 0 || p.Kc % 64 != 0 || (p.istr != 1 && p.istr != 2) || p.one_by_one || p.dzpad < 1 || p.dzC % 128 != 0) return -1;
    if (p.istr == 2 && p.taps.nr != 3) return -1;
    const WgRoute r = wg_route_any_slab(p);
    if (!r.halo()) return -1;
    *g = r.g;
    const int nhi = (g->NHP + 7) / 8;
    // stride 1: four ring stages with at most 5 LDS-DMA instructions per wave and chunk (the counted vmcnt waits);
    // stride 2: two stages that fit 160 KB
    return (p.istr == 1 ? nhi <= 24 : 2 * (128 + 8 * nhi) * 128 <= 160 * 1024) ? 0 : -1;
}
bool vpd_wgrad128_eligible(const WgradParams& p) {
    WgHaloGeom g;
    return wg2_kind(p, &g) >= 0;
}

struct Wg2Schedule {
    std::vector<int> tasks;        // 4 ints per task
    std::vector<int> blk_begin;    // grid + 1
    int ksplit[WG2_MAX];
    int grid = 0;
    double est_us = 0.0;
};

// makespan of the LPT deal of `len` (task lengths, any order) over G blocks; optionally the assignment
static double wg2_lpt(const std::vector<std::pair<double, int>>& sorted, int G, const std::vector<int>& order,
                      std::vector<int>* owner) {
    std::vector<double> load(G, 0.0);
    if (owner) owner->assign(sorted.size(), 0);
    for (size_t i = 0; i < sorted.size(); ++i) {
        int best = order[0];
        for (int k = 1; k < G; ++k) {
            const int b = order[k];
            if (load[b] < load[best] - 1e-9) best = b;
        }
        load[best] += sorted[i].first;
        if (owner) (*owner)[i] = best;
    }
    double mx = 0.0;
    for (double v : load) mx = v > mx ? v : mx;
    return mx;
}

static void wg2_build(const WgradParams* ps, const WgHaloGeom* gs, int n, int G, Wg2Schedule* out, const int* kinds = nullptr) {
    // block order: the blocks of XCD 0 first (b = 0, 8, 16, ...), then XCD 1, ...: equal-length tasks are dealt in task order
    // to equally loaded blocks, so consecutive tasks (the tiles of one pixel range) land on one XCD
    std::vector<int> order;
    for (int x = 0; x < 8; ++x)
        for (int b = x; b < G; b += 8) order.push_back(b);
    int nch[WG2_MAX], tiles[WG2_MAX], cap[WG2_MAX], ntap[WG2_MAX];
    for (int i = 0; i < n; ++i) {
        const int kind = kinds ? kinds[i] : 0;
        nch[i] = (ps[i].M + WG_CH - 1) / WG_CH;
        tiles[i] = kind ? (ps[i].Co / wg2_tco(kind)) * (ps[i].Kc / (64 * wg2_nb(kind))) : (ps[i].Co / 128) * (ps[i].Kc / 64);
        ntap[i] = kind ? 1 : 9;
        cap[i] = vpd_wgrad_group_max_splits(ps[i].Co, ps[i].Kc, ntap[i]);
        if (cap[i] > nch[i]) cap[i] = nch[i];
    }
    // per-chunk time of a 128 x 64 task: the larger of the MFMA time (1.15 us) and the stream (16 KB + halo at ~21 GB/s
    // per CU when every CU streams); per-task fixed cost; slab bytes written and read back at 4.5 TB/s
    const double t_fixed = 5.0, bw = 4.5e6;
    auto tchunk = [&](int i) {
        const int kind = kinds ? kinds[i] : 0;
        if (kind) return (wg2_tco(kind) / 8.0 + 8.0 * wg2_nb(kind)) / 21.0;      // 1x1: the stream alone
        const double st = (16.0 + (gs[i].NHP + 7) / 8) / 21.0;
        return st > 1.15 ? st : 1.15;
    };
    // task list of the splits ks[]: problem-major, split-major, tile-fastest; then stable sort by length (longest first)
    struct T { int prob, tile, split; };
    std::vector<T> tv;
    std::vector<std::pair<double, int>> tl;
    auto list_tasks = [&](const int* ks) {
        tv.clear();
        tl.clear();
        for (int i = 0; i < n; ++i) {
            const int cpb = (nch[i] + ks[i] - 1) / ks[i];
            for (int s = 0; s < ks[i]; ++s) {
                const int c1 = (s + 1) * cpb < nch[i] ? (s + 1) * cpb : nch[i];
                for (int t = 0; t < tiles[i]; ++t) {
                    tl.push_back({(c1 - s * cpb) * tchunk(i) + t_fixed, (int)tv.size()});
                    tv.push_back({i, t, s});
                }
            }
        }
        std::stable_sort(tl.begin(), tl.end(), [](const std::pair<double, int>& a, const std::pair<double, int>& b) { return a.first > b.first; });
    };
    double best = 1e30;
    for (int target = 8; target <= 1024; target += (target < 128 ? 2 : 8)) {
        int ks[WG2_MAX];
        double slab = 0.0;
        bool any = false;
        for (int i = 0; i < n; ++i) {
            int cpb;
            ks[i] = wg_split_for_target(nch[i], cap[i], (double)target, &cpb);
            if (ks[i] > 1) { slab += (double)ks[i] * ntap[i] * ps[i].Co * ps[i].Kc * 4; any = true; }
        }
        list_tasks(ks);
        const double cost = wg2_lpt(tl, G, order, nullptr) + 2.0 * slab / bw + (any ? 3.0 : 0.0);
        if (cost < best) { best = cost; for (int i = 0; i < n; ++i) out->ksplit[i] = ks[i]; }
    }
    list_tasks(out->ksplit);      // the final list; LPT deal
    std::vector<int> owner;
    out->est_us = wg2_lpt(tl, G, order, &owner);
    std::vector<std::vector<int>> per(G);
    for (size_t i = 0; i < tl.size(); ++i) per[owner[i]].push_back(tl[i].second);
    out->tasks.clear();
    out->blk_begin.assign(G + 1, 0);
    for (int b = 0; b < G; ++b) {
        out->blk_begin[b] = (int)out->tasks.size() / 4;
        for (int id : per[b]) {
            out->tasks.push_back(tv[id].prob); out->tasks.push_back(tv[id].tile);
            out->tasks.push_back(tv[id].split); out->tasks.push_back(0);
        }
    }
    out->blk_begin[G] = (int)out->tasks.size() / 4;
    out->grid = G;
}

// Host-only view of the schedule for the tests (no GPU needed): problems as {M, Co, Ci, NHP} quadruples; returns the number of
// tasks and fills ksplit[n], blk_begin[G + 1] and tasks[4 * ntasks] (capacity `cap` tasks; -1 if it does not fit).
extern "C" int vpd_op_wgrad128_schedule(int n, const int* dims4, int G, int* ksplit, int* blk_begin, int* tasks, int cap,
                                        double* est_us) {
    if (n < 1 || n > WG2_MAX || G < 1 || !dims4 || !ksplit || !blk_begin || !tasks) return -1;
    WgradParams ps[WG2_MAX];
    WgHaloGeom gs[WG2_MAX];
    memset(ps, 0, sizeof ps);
    memset(gs, 0, sizeof gs);
    for (int i = 0; i < n; ++i) {
        ps[i].M = dims4[4 * i]; ps[i].Co = dims4[4 * i + 1]; ps[i].Kc = dims4[4 * i + 2]; gs[i].NHP = dims4[4 * i + 3];
        if (ps[i].M < 1 || ps[i].Co % 128 || ps[i].Kc % 64 || gs[i].NHP < 1) return -1;
    }
    Wg2Schedule sch;
    wg2_build(ps, gs, n, G, &sch);
    const int nt = (int)sch.tasks.size() / 4;
    if (nt > cap) return -1;
    for (int i = 0; i < n; ++i) ksplit[i] = sch.ksplit[i];
    for (int b = 0; b <= G; ++b) blk_begin[b] = sch.blk_begin[b];
    for (size_t i = 0; i < sch.tasks.size(); ++i) tasks[i] = sch.tasks[i];
    if (est_us) *est_us = sch.est_us;
    return nt;
}

size_t vpd_wgrad128_table_bytes() { return (size_t)1 << 17; }       // device table of one launch: tasks + block index

// One launch for `n` eligible problems (ps[i].slab: vpd_wgrad_group_slab_floats() floats of its own).  `cache` (may be
// null) keeps the schedule between calls with the same shapes; `dev_table` is vpd_wgrad128_table_bytes() of device
// memory owned by the caller for THIS group (re-uploaded, stream-ordered, only when the shapes change).
struct Wg2Cache {
    int n = 0, ncu = 0;
    int sig[WG2_MAX][4];
    const void* uploaded_to = nullptr;
    Wg2Schedule sch;
};
void* vpd_wgrad128_cache_new() { return new Wg2Cache(); }
void vpd_wgrad128_cache_free(void* c) { delete static_cast<Wg2Cache*>(c); }

hipError_t vpd_launch_wgrad128_group(const WgradParams* ps, int n, void* cache_v, void* dev_table, hipStream_t stream) {
    if (n < 1 || n > WG2_MAX || !dev_table) return hipErrorInvalidValue;
    const int ncu = vpd_cu_budget();
    Wg2Group grp = {};
    WgReduceGroup red = {};
    grp.nprob = n;
    int kinds[WG2_MAX];
    for (int i = 0; i < n; ++i) {
        grp.p[i] = ps[i];
        kinds[i] = grp.kind[i] = wg2_kind(ps[i], &grp.g[i]);
        if (kinds[i] < 0) return hipErrorInvalidValue;
    }
    Wg2Cache local;
    Wg2Cache* c = cache_v ? static_cast<Wg2Cache*>(cache_v) : &local;
    bool same = c->n == n && c->uploaded_to == dev_table && c->ncu == ncu;
    for (int i = 0; i < n && same; ++i)
        same = c->sig[i][0] == ps[i].M && c->sig[i][1] == ps[i].Co && c->sig[i][2] == ps[i].Kc && c->sig[i][3] == grp.g[i].NHP + 1000 * kinds[i];
    if (!same) {
        wg2_build(ps, grp.g, n, ncu, &c->sch, kinds);
        c->n = n; c->ncu = ncu;
        for (int i = 0; i < n; ++i) { c->sig[i][0] = ps[i].M; c->sig[i][1] = ps[i].Co; c->sig[i][2] = ps[i].Kc; c->sig[i][3] = grp.g[i].NHP + 1000 * kinds[i]; }
        const size_t tb = c->sch.tasks.size() * sizeof(int), bb = c->sch.blk_begin.size() * sizeof(int);
        if (tb + bb + 64 > vpd_wgrad128_table_bytes()) return hipErrorInvalidValue;
        hipError_t e = hipMemcpyAsync(dev_table, c->sch.tasks.data(), tb, hipMemcpyHostToDevice, stream);
        if (e != hipSuccess) return e;
        e = hipMemcpyAsync((char*)dev_table + ((tb + 63) & ~(size_t)63), c->sch.blk_begin.data(), bb, hipMemcpyHostToDevice, stream);
        if (e != hipSuccess) return e;
        if (!cache_v) { e = hipStreamSynchronize(stream); if (e != hipSuccess) return e; }      // `local` dies with this call
        c->uploaded_to = dev_table;
    }
    const Wg2Schedule& sch = c->sch;
    grp.tasks = reinterpret_cast<const int4*>(dev_table);
    grp.blk_begin = reinterpret_cast<const int*>((char*)dev_table + ((sch.tasks.size() * sizeof(int) + 63) & ~(size_t)63));
    {
        size_t need = 0;      // every problem's ring: 4 stages (stride 1, and every 1x1) or 2 (3x3 stride 2)
        for (int i = 0; i < n; ++i) {
            const size_t st = kinds[i] ? (size_t)(wg2_tco(kinds[i]) + 64 * wg2_nb(kinds[i])) * 64 : (size_t)(128 + 8 * ((grp.g[i].NHP + 7) / 8)) * 64;
            const size_t want = (kinds[i] >= 4 ? WG2_NS256 : (kinds[i] || ps[i].istr == 1 ? 4 : 2)) * st;      // (kind 4, or + 16)
            need = want > need ? want : need;
        }
        grp.stage_elems = (int)need;
    }
    for (int i = 0; i < n; ++i) {
        WgHaloGeom& g = grp.g[i];
        const int nchunks = (ps[i].M + WG_CH - 1) / WG_CH;
        g.ksplit = sch.ksplit[i];
        g.cpb = (nchunks + g.ksplit - 1) / g.ksplit;
        if (g.ksplit > 1) red.add(ps[i].slab, ps[i].dw, (long)(kinds[i] ? 1 : 9) * ps[i].Co * ps[i].Kc, g.ksplit);
    }
    const size_t lds = (size_t)grp.stage_elems * sizeof(bf16_t);
    if (lds > 160 * 1024) return hipErrorInvalidValue;
    VPD_LAUNCH(conv_wgrad128_persistent_kernel, dim3(sch.grid), dim3(512), lds, stream, grp);
    wg_launch_reduce(red, stream);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------
// Probe for the parity tests: stages one [128][64] bf16 tile exactly like the
// wgrad kernel and dumps the transposed-read fragments, so the
// ds_read_b64_tr_b16 lane mapping is checked on hardware in isolation.
// out: [4 waves][4 ctiles][64 lanes][8] bf16
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void tr_read_probe_kernel(const bf16_t* tile, bf16_t* out) {
    __shared__ __attribute__((aligned(16))) bf16_t s[128 * 64];
    const int tid = threadIdx.x, piece = tid & 7, row0 = tid >> 3;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int r = row0 + 32 * i;
        *reinterpret_cast<uint4*>(s + wg_swz_off(r, piece * 8)) = *reinterpret_cast<const uint4*>(tile + r * 64 + piece * 8);
    }
    __syncthreads();
    const int lane = tid & 63, wave = tid >> 6;
#pragma unroll
    for (int ct = 0; ct < 4; ++ct) {
        const bf16x8 f = tr_frag(s, wave * 32, ct, lane);
        *reinterpret_cast<bf16x8*>(out + ((size_t)(wave * 4 + ct) * 64 + lane) * 8) = f;
    }
}
extern "C" int vpd_op_tr_read_probe(const void* tile, void* out, void* stream) {
    hipLaunchKernelGGL(tr_read_probe_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)tile,
                       (bf16_t*)out);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
