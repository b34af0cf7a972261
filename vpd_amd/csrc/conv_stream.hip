// 1x1 convolutions with few input channels on many pixels (the Bottleneck students' layer1 / layer2: 64 <-> 256, 128 <-> 512
// channels on 262,144 / 65,536 pixels; forward, data gradient, eval) as a persistent STREAMING kernel.
//
// These launches are 8.6 GFLOP over 100-170 MB: memory-bound by a factor of ten.  What they need is bytes in flight and nothing
// in the way of the stores.  conv_igemm_kernel (the gather kernel they ran on) stages through registers one K-step ahead and
// re-reads its weight tile per pixel tile: 3.3-4 TB/s.  Here
//   * the whole [BN][Kc] weight tile is brought to LDS ONCE per block (Kc <= 256: 8-64 KB),
//   * a block walks the pixel tiles t = blockIdx.x, + gridDim.x, ... ; a tile's [BM][Kc] input slice is ONE K extent, brought by
//     LDS-DMA into an NSA-deep ring by four loader waves that run NSA - 1 tiles ahead (counted vmcnt waits: the loaders issue no
//     stores, so nothing but their own tiles stands in their queue),
//   * four MFMA waves multiply a tile out of LDS and leave through the shared epilogue (conv_epilogue.h: statistics, accumulate
//     with the ReLU bit map, eval scale / shift / residual / ReLU) -- residual and old-value fragments requested BEFORE the tile's
//     barrier, so that no round trip is exposed between the MFMAs and the stores,
//   * one workgroup barrier per tile.
// Pixel tiles are whole image rows (BM % Ws == 0, Hs * Ws % BM == 0): a lane's share of a tile sits at the same offsets in every
// tile, and the tile's base address is one scalar division away.  Anything else stays on the other kernels.
#include "common.h"
#include "kernels.h"
#include "conv_epilogue.h"
#include "conv_pws.h"      // gptr_t / lptr_t
#include <string.h>

namespace {

template <int N>
static __device__ __forceinline__ void stream_wait_vm() { asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory"); }
// at most `behind` newer tiles of PER instructions each may still be in flight
template <int PER, int MAXB>
static __device__ __forceinline__ void stream_wait_tiles(int behind) {
    static_assert(PER * MAXB < 64, "vmcnt immediate");
    if constexpr (MAXB >= 7) { if (behind >= 7) { stream_wait_vm<7 * PER>(); return; } }
    if constexpr (MAXB >= 6) { if (behind == 6) { stream_wait_vm<6 * PER>(); return; } }
    if constexpr (MAXB >= 5) { if (behind == 5) { stream_wait_vm<5 * PER>(); return; } }
    if constexpr (MAXB >= 4) { if (behind == 4) { stream_wait_vm<4 * PER>(); return; } }
    if constexpr (MAXB >= 3) { if (behind == 3) { stream_wait_vm<3 * PER>(); return; } }
    if constexpr (MAXB >= 2) { if (behind == 2) { stream_wait_vm<2 * PER>(); return; } }
    if constexpr (MAXB >= 1) { if (behind == 1) { stream_wait_vm<1 * PER>(); return; } }
    stream_wait_vm<0>();
}

struct StreamGeo {
    int mtiles;             // pixel tiles of the launch
    int tiles_per_img;      // Hs * Ws / BM
    int rows_per_tile;      // BM / Ws
};

// LDS of a block: the resident weights [KC / 64][BN][64], NSA ring stages [KC / 64][BM][64], then `coef_rows` rows of BN floats
// (the fused kernels' per-channel coefficients)
constexpr size_t stream_lds_bytes(int KC, int BM, int BN, int NSA, int coef_rows = 0) {
    return (size_t)(KC / 64) * 64 * (BN + NSA * BM) * sizeof(bf16_t) + (size_t)coef_rows * BN * sizeof(float);
}

// What a wave of a streaming block knows about itself: NMW MFMA waves (4 or 8: WM pixel waves x WN channel waves) in front of four
// loader waves, the carve-up of the block's LDS and the block's pixel tiles first, first + lanes, ... (ntile of them).
template <int KC_, int BM_, int BN_, int NSA_, int NMW_>
struct StreamBlock {
    static constexpr int KC = KC_, BM = BM_, BN = BN_, NSA = NSA_, NMW = NMW_;
    static constexpr int KCH = KC / 64;
    static constexpr int WN = BN >= 256 ? 4 : BN / 64, WM = NMW / WN;
    static constexpr int WTM = BM / WM, WTN = BN / WN, MI = WTM / 16, NI = WTN / 16;
    static constexpr int WELEMS = KCH * BN * 64, ASTAGE = KCH * BM * 64;
    unsigned char* smem;
    bf16_t* sW; bf16_t* ring; float* coef;
    int tid, lane, wave, n0, lanes, first, ntile;
    int wm, wn, fr, fq, nw;      // MFMA waves: pixel wave, channel wave, fragment row / quarter, first channel of the wave

    __device__ __forceinline__ StreamBlock(const StreamGeo& sg) {
        extern __shared__ __attribute__((aligned(16))) unsigned char stream_smem[];
        smem = stream_smem;
        sW = reinterpret_cast<bf16_t*>(smem);
        ring = sW + WELEMS;
        coef = reinterpret_cast<float*>(ring + NSA * ASTAGE);
        tid = threadIdx.x;
        lane = tid & 63;
        wave = __builtin_amdgcn_readfirstlane(tid >> 6);
        n0 = blockIdx.y * BN;
        lanes = gridDim.x;
        first = blockIdx.x;
        ntile = first < sg.mtiles ? (sg.mtiles - first + lanes - 1) / lanes : 0;
        wm = wave % WM; wn = wave / WM;
        fr = lane & 15; fq = lane >> 4;
        nw = n0 + wn * WTN;
    }
    // asked BEFORE a wave makes its StreamBlock: the loader branch and the MFMA branch of a kernel each construct their own (one
    // object in front of the branch keeps two more VGPRs live in nearly every instantiation -- a property of the compiler at hand:
    // profiles/stream_shared_resources.txt is the table to regenerate when the toolchain changes)
    static __device__ __forceinline__ bool loader() { return __builtin_amdgcn_readfirstlane(threadIdx.x >> 6) >= NMW; }
    __device__ __forceinline__ int mtile(int it) const { return first + it * lanes; }
    // (MFMA waves) the pixel of fragment row fr in pixel group b of a tile
    __device__ __forceinline__ int pixel(int mtile, int b) const { return mtile * BM + wm * WTM + b * 16 + fr; }
    __device__ __forceinline__ const bf16_t* stage(int it) const { return ring + (it % NSA) * ASTAGE; }
    // coefficient row k: this lane's four channels of group a
    __device__ __forceinline__ float4 coef4(int k, int a) const {
        return *reinterpret_cast<const float4*>(coef + k * BN + wn * WTN + a * 16 + 4 * fq);
    }
};

template <int N>
static __device__ __forceinline__ void stream_barriers() {
#pragma unroll
    for (int k = 0; k < N; ++k) __builtin_amdgcn_s_barrier();
}

// The loader waves' part of a block (the four waves behind the MFMA waves, lw = 0..3): the resident weight tile, then the block's
// pixel tiles through the ring, then the END barrier.  The MFMA waves run workgroup barriers of their own around that, which the
// loaders must run too:
//   PRE   before their first tile (a coefficient prologue), matched here once the first AHEAD tiles are on their way,
//   TAIL  behind the END barrier (stream_tail_barriers).
// DUAL: two convolutions of 64 input channels each on the same pixels (same padded geometry): chunk 0 = (p.x, p.w), chunk 1 =
// (p.x2, p.w2) -- a down-sampling Bottleneck's closing 1x1 and its 1x1 branch (conv1x1_bn2_stream_kernel)
template <class B, int PRE, int TAIL, bool DUAL = false>
static __device__ __forceinline__ void stream_loader(const ConvParams& p, const StreamGeo& sg, const B& blk) {
    constexpr int KCH = B::KCH, BM = B::BM, BN = B::BN, NSA = B::NSA;
    constexpr int A_PER = BM / 32;                     // LDS-DMA instructions per loader wave, chunk and tile
    constexpr int PER_TILE = A_PER * KCH;
    constexpr int W_PER = BN / 32;
    constexpr int AHEAD = NSA - 1;
    static_assert(NSA >= 2 && AHEAD * PER_TILE < 64, "ring depth");
    static_assert(!DUAL || B::KC == 128, "DUAL: two chunks of 64 channels");
    const int lw = blk.wave - B::NMW;
    const int piece = blk.lane & 7;
    const int lrow = blk.lane >> 3;
    // weights: [BN][Kc] rows n0 .. of the one tap, chunk by chunk
    const bf16_t* const wsrc = p.w + (size_t)p.taps.w0 * p.Co * p.Kc;
#pragma unroll
    for (int cc = 0; cc < KCH; ++cc)
#pragma unroll
        for (int i = 0; i < W_PER; ++i) {
            const int n = (lw + 4 * i) * 8 + lrow;
            const bf16_t* const ws = DUAL ? (cc ? p.w2 : p.w) + (size_t)(blk.n0 + n) * 64 : wsrc + (size_t)(blk.n0 + n) * p.Kc + cc * 64;
            __builtin_amdgcn_global_load_lds((gptr_t)(ws + ((piece ^ (n & 7)) << 3)),
                                             (lptr_t)(blk.sW + (cc * BN + (lw + 4 * i) * 8) * 64), 16, 0, 0);
        }
    // this lane's pixel rows of a tile: offsets from the tile's first pixel (same in every tile)
    int aoff[A_PER];
#pragma unroll
    for (int i = 0; i < A_PER; ++i) {
        const int r = (lw + 4 * i) * 8 + lrow;
        const int dy = r / p.Ws;
        const int xx = r - dy * p.Ws;
        aoff[i] = (dy * p.istr * p.xWp + xx * p.istr) * p.xC + ((piece ^ (r & 7)) << 3);
    }
    const int tap_off = (p.taps.dy0 * p.xWp + p.taps.dx0) * p.xC;
    auto issue = [&](int it) __attribute__((always_inline)) {
        const int t = blk.mtile(it);
        const int b = t / sg.tiles_per_img;
        const int r0 = (t - b * sg.tiles_per_img) * sg.rows_per_tile;
        const size_t toff = (size_t)((b * p.xHp + r0 * p.istr) * p.xWp) * p.xC + tap_off;
        const bf16_t* const src = p.x + toff;
        bf16_t* const st = blk.ring + (it % NSA) * B::ASTAGE;
#pragma unroll
        for (int cc = 0; cc < KCH; ++cc)
#pragma unroll
            for (int i = 0; i < A_PER; ++i)
                __builtin_amdgcn_global_load_lds((gptr_t)(DUAL ? (cc ? p.x2 : p.x) + toff + aoff[i] : src + aoff[i] + cc * 64),
                                                 (lptr_t)(st + (cc * BM + (lw + 4 * i) * 8) * 64), 16, 0, 0);
    };
#pragma unroll
    for (int it = 0; it < AHEAD; ++it)
        if (it < blk.ntile) issue(it);
    stream_barriers<PRE>();
    for (int it = 0; it < blk.ntile; ++it) {
        // tile `it` (and the weights, issued before everything) must have landed; the tiles issued behind it may be in flight
        int behind = blk.ntile - 1 - it;
        behind = behind < AHEAD - 1 ? behind : AHEAD - 1;
        stream_wait_tiles<PER_TILE, AHEAD - 1>(behind);
        __builtin_amdgcn_s_barrier();                         // READY_it (stage (it - 1) % NSA is free again)
        if (it + AHEAD < blk.ntile) issue(it + AHEAD);
    }
    if (blk.ntile == 0) stream_wait_vm<0>();
    stream_barriers<1 + TAIL>();                              // END, and the MFMA waves' barriers behind it
}

// One pixel tile out of LDS: acc[a][b] += W[channels wn*WTN + 16a ..][K] . X[pixels wm*WTM + 16b ..][K]
template <int KC, int BM, int BN, int WM, int WN>
static __device__ __forceinline__ void stream_mma(const bf16_t* sW, const bf16_t* cA, f32x4 (&acc)[BN / WN / 16][BM / WM / 16],
                                                  int wm, int wn, int fr, int fq) {
    constexpr int KCH = KC / 64, WTM = BM / WM, WTN = BN / WN, MI = WTM / 16, NI = WTN / 16;
#pragma unroll
    for (int cc = 0; cc < KCH; ++cc)
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) {
            bf16x8 af[NI], bfm[MI];
            const int chunk = kk * 4 + fq;
#pragma unroll
            for (int a = 0; a < NI; ++a) {
                const int r = wn * WTN + a * 16 + fr;
                af[a] = *reinterpret_cast<const bf16x8*>(sW + (cc * BN + r) * 64 + ((chunk ^ (r & 7)) << 3));
            }
#pragma unroll
            for (int b = 0; b < MI; ++b) {
                const int r = wm * WTM + b * 16 + fr;
                bfm[b] = *reinterpret_cast<const bf16x8*>(cA + (cc * BM + r) * 64 + ((chunk ^ (r & 7)) << 3));
            }
#pragma unroll
            for (int a = 0; a < NI; ++a)
#pragma unroll
                for (int b = 0; b < MI; ++b)
                    acc[a][b] = VPD_MFMA16(af[a], bfm[b], acc[a][b]);
        }
}

// per-lane partial sums -> 16 pixel lanes (DPP) -> WM pixel waves (LDS) -> ONE fp64 atomic per channel and block into accumulator
// row blockIdx.x % rows.  MFMA waves only, behind the END barrier; contains ONE workgroup barrier.
template <class B>
static __device__ __forceinline__ void stream_stats_flush(double* rows, int stat_rows, int Co, const B& blk, float (&st1)[B::NI][4],
                                                          float (&st2)[B::NI][4]) {
    constexpr int BN = B::BN, WM = B::WM, NI = B::NI;
    float* red = reinterpret_cast<float*>(blk.smem);          // [WM][2][BN] (the ring is idle now)
#pragma unroll
    for (int a = 0; a < NI; ++a)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float u = row16_sum(st1[a][j]), v = row16_sum(st2[a][j]);
            if (blk.fr == 0) {
                const int c = blk.wn * B::WTN + a * 16 + 4 * blk.fq + j;
                red[(blk.wm * 2 + 0) * BN + c] = u;
                red[(blk.wm * 2 + 1) * BN + c] = v;
            }
        }
    __syncthreads();
    if (rows) {
        const int rmask = (stat_rows ? stat_rows : VPD_STAT_ROWS) - 1;
        for (int i = blk.tid; i < 2 * BN; i += B::NMW * 64) {
            const int which = i / BN;
            const int c = i - which * BN;
            float t = 0.f;
#pragma unroll
            for (int w = 0; w < WM; ++w) t += red[(w * 2 + which) * BN + c];
            atomicAdd(&rows[((size_t)((int)blockIdx.x & rmask) * 2 + which) * Co + blk.n0 + c], (double)t);
        }
    }
}
// ... of two BatchNorms that share sum g (st1): the second flush reuses `red`, so a barrier stands between them
template <class B>
static __device__ __forceinline__ void stream_stats_flush2(double* rows3, double* rowsD, int stat_rows, int Co, const B& blk,
                                                           float (&st1)[B::NI][4], float (&st2)[B::NI][4], float (&st3)[B::NI][4]) {
    stream_stats_flush(rows3, stat_rows, Co, blk, st1, st2);
    __syncthreads();
    stream_stats_flush(rowsD, stat_rows, Co, blk, st1, st3);
}
// Workgroup barriers the MFMA waves run behind the END barrier, which the loader waves run too (stream_loader's TAIL): those of
// the statistics flush above for `nconv` BatchNorms -- one per flush and one between two
constexpr int stream_tail_barriers(bool flush, int nconv) { return flush ? 2 * nconv - 1 : 0; }

template <int KC, int BM, int BN, int NSA, int EPM, int NMW = 4>      // NMW MFMA waves (4 or 8) + 4 loader waves
__global__ __launch_bounds__((NMW + 4) * 64) void conv1x1_stream_kernel(const ConvParams p, const StreamGeo sg) {
    using B = StreamBlock<KC, BM, BN, NSA, NMW>;
    constexpr int WM = B::WM, WN = B::WN, MI = B::MI, NI = B::NI;
    constexpr bool FLUSH = EPM == 1 || EPM == 4;
    static_assert(stream_lds_bytes(KC, BM, BN, NSA) <= 160 * 1024, "LDS");
    const ConvGeo geo = {p.Hs, p.Ws, p.M, p.oph, p.opw};
    if (B::loader()) {
        stream_loader<B, 0, stream_tail_barriers(FLUSH, 1)>(p, sg, B(sg));
        return;
    }
    const B blk(sg);
    float st1[NI][4], st2[NI][4];
#pragma unroll
    for (int a = 0; a < NI; ++a)
#pragma unroll
        for (int j = 0; j < 4; ++j) { st1[a][j] = 0.f; st2[a][j] = 0.f; }
    for (int it = 0; it < blk.ntile; ++it) {
        const int mtile = blk.mtile(it);
        // fragments of the other tensors the epilogue reads: requested before the tile's barrier
        ResFrag<NI, MI> resf;
        AccFrag<NI, MI> accf;
        if (EPM == 3 && p.res) conv_res_prefetch<BM, BN, WM, WN>(p, mtile, blk.n0, geo, resf);
        if (EPM == 2) conv_acc_prefetch<BM, BN, WM, WN>(p, mtile, blk.n0, geo, accf);
        f32x4 acc[NI][MI];
        zero_acc(acc);
        __builtin_amdgcn_s_barrier();                             // READY_it
        stream_mma<KC, BM, BN, WM, WN>(blk.sW, blk.stage(it), acc, blk.wm, blk.wn, blk.fr, blk.fq);
        if (EPM == 3 && p.res) {
            conv_epilogue_res_pre<BM, BN, WM, WN, EPM>(p, acc, mtile, blk.n0, st1, st2, geo, resf);
        } else if (EPM == 2) {
            BstFrag<NI, VPD_BST_MB(MI)> none;
            conv_epilogue_acc_pre<BM, BN, WM, WN, EPM>(p, acc, mtile, blk.n0, st1, st2, geo, none, accf);
        } else {
            conv_epilogue<BM, BN, WM, WN, EPM>(p, acc, mtile, blk.n0, st1, st2, geo);
        }
    }
    __builtin_amdgcn_s_barrier();                                 // END
    if (FLUSH) stream_stats_flush(p.stats, p.stat_rows, p.Co, blk, st1, st2);
}

// ---------------------------------------------------------------------------
// A Bottleneck's closing 1x1 convolution TOGETHER with its BatchNorm (train mode), the convolution computed twice instead of
// written and read back.  z3 = conv3(a2) has 4x the channels of a2 and K is 64 / 128: recomputing a tile is 128 MFMAs per wave,
// writing and re-reading it is 2 x 32 KB through a memory system that is the bound of every launch around it.
//   forward:  [statistics]  conv1x1_stream_kernel<.., 4>: z3 tile -> bf16 -> sum / sum of squares -> the BatchNorm's rows; no store
//             [MODE 1]      z3 tile again -> relu(scale z3 + shift + identity) -> block output + ReLU bit map.  Every block
//                           finalizes the statistics of its own 256 channels in its prologue (bn_finalize_channel, as
//                           bn_fwd_fused_kernel does); the blocks of the first pixel lane store mean / rstd / scale / shift and
//                           update the running statistics.
//   backward: [MODE 2]      z3 tile again; g = d(out) * mask; sum g, sum g z3 -> rows
//             [MODE 3]      z3 tile again; dz3 = A g + B z3 + D (bn_bwd_apply_coef in the prologue, dgamma / dbeta from the first
//                           lane) -> padded dz3 for the weight- and data-gradient launches.
// z3 is rounded to bf16 in registers exactly where the unfused path stores it: the forward is bit-identical to conv + bn_fwd_fused,
// the backward has bn_bwd_apply_fused_kernel's arithmetic.  64 x 256 tiles (eight MFMA waves x 32 pixels x 64 channels; the statistics
// pass keeps the storing launch's four), Kc = 64 / 128.
// ---------------------------------------------------------------------------
constexpr int TAIL_BM = 64, TAIL_BN = 256, TAIL_NMW = 8;      // the fused kernels' tile and MFMA waves (2 pixel x 4 channel waves)
constexpr int TAIL_THREADS = (TAIL_NMW + 4) * 64;

struct StreamBnSide {                                      // one BatchNorm
    const double* rows;                                    // MODE 1 / 3: the sums to finalize ([VPD_FUSED_ROWS][2][Co])
    const float* gamma; const float* beta;
    float* mean; float* rstd; float* scale; float* shift;  // MODE 1: written (first lane); MODE 3: mean / rstd read
    float* rm; float* rv;                                  // MODE 1: running statistics (may be null)
    double* rows_out;                                      // MODE 2: rows to add sum g / sum g z to
    float* dgamma; float* dbeta;                           // MODE 3 (first lane)
    bf16_t* dz;                                            // MODE 3: output (p.y = d(out), dense, with p.acc_mask = the bit map)
};
struct StreamBn {
    float count, momentum, eps;
    unsigned char* mask_out;                               // MODE 1: ReLU bit map [M][Co / 8] (may be null)
    int dzHp, dzWp, dzpad;                                 // MODE 3: geometry of every side's dz
    int frozen;                                            // MODE 1: mean / rstd from rm / rv (read only); MODE 3: B = D = 0 (every side)
    StreamBnSide s;                                        // the closing convolution's BatchNorm
};

// ---- coefficient prologues: one channel `ch` per thread ----
// MODE 1: scale / shift of the channel; the blocks of the first pixel lane publish the BatchNorm's vectors
static __device__ __forceinline__ void stream_bn_finalize(const StreamBnSide& s, const StreamBn& bn, int Co, int ch, float* coef_scale,
                                                          float* coef_shift) {
    float mu, r, sc, sh; double var;
    bn_finalize_channel(s.rows, Co, ch, bn.count, bn.eps, s.gamma[ch], s.beta[ch], &mu, &r, &sc, &sh, &var, bn.frozen, s.rm, s.rv);
    *coef_scale = sc; *coef_shift = sh;
    if (blockIdx.x == 0) {
        s.mean[ch] = mu; s.rstd[ch] = r; s.scale[ch] = sc; s.shift[ch] = sh;
        if (s.rm && !bn.frozen) {
            const double unb = bn.count > 1.f ? var * (double)bn.count / ((double)bn.count - 1.0) : var;
            s.rm[ch] = (1.f - bn.momentum) * s.rm[ch] + bn.momentum * mu;
            s.rv[ch] = (1.f - bn.momentum) * s.rv[ch] + bn.momentum * (float)unb;
        }
    }
}
// MODE 3: A / B / D into three coefficient rows of BN floats at `coef`, entry i; dgamma / dbeta from the first lane
template <int BN>
static __device__ __forceinline__ void stream_bn_bwd_coef(const StreamBnSide& s, const StreamBn& bn, int Co, int ch, float* coef, int i) {
    bn_bwd_apply_coef(s.rows, Co, ch, bn.count, s.gamma[ch], s.mean[ch], s.rstd[ch], coef, coef + BN, coef + 2 * BN, s.dgamma, s.dbeta,
                      blockIdx.x == 0, i, bn.frozen);
}

// ---- a lane's four channels of one group ----
static __device__ __forceinline__ void stream_unpack4(const uint2& v, float (&f)[4]) {
    f[0] = bf2f((unsigned short)(v.x & 0xffff)); f[1] = bf2f((unsigned short)(v.x >> 16));
    f[2] = bf2f((unsigned short)(v.y & 0xffff)); f[3] = bf2f((unsigned short)(v.y >> 16));
}
// a coefficient row of StreamBlock::coef4 (kept as the float4 it is loaded as and taken apart at its use: the same rows as an
// indexable vector type put the two-convolution MODE 3 kernel into scratch)
static __device__ __forceinline__ void stream_coef4(const float4& k, float (&c)[4]) { c[0] = k.x; c[1] = k.y; c[2] = k.z; c[3] = k.w; }
static __device__ __forceinline__ uint2 stream_pack4(const float (&v)[4]) { return uint2{pack2bf(v[0], v[1]), pack2bf(v[2], v[3])}; }
// z as the unfused path stores it
static __device__ __forceinline__ void stream_round4(const f32x4& acc, float (&z)[4]) {
    stream_unpack4(uint2{pack2bf(acc[0], acc[1]), pack2bf(acc[2], acc[3])}, z);
}
// g = d(out) * mask: this lane's four bits of group a in the pixel's bits of the wave's channel range, and channel j of them
static __device__ __forceinline__ unsigned stream_mask4(unsigned long long mbits, int a, int fq) { return (unsigned)(mbits >> (a * 16 + 4 * fq)); }
static __device__ __forceinline__ float stream_masked_g(unsigned bits, int j, float d) { return ((bits >> j) & 1u) ? d : 0.f; }

static __device__ __forceinline__ unsigned stream_relu_bits(const uint4& ov) {
    // [half != 0] of eight stored non-negative bf16 values as one byte (bn_fwd_fused_kernel's form)
    const unsigned w[4] = {ov.x, ov.y, ov.z, ov.w};
    unsigned acc = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        unsigned f1;
        asm("v_pk_min_u16 %0, %1, %2" : "=v"(f1) : "v"(w[j]), "v"(0x00010001u));
        acc |= f1 << (2 * j);
    }
    return (acc | (acc >> 15)) & 0xffu;
}

// element offset of output pixel m (every row of a tile is a pixel: M % BM == 0) in the padded tensor a MODE writes: p.y
// (MODE 1) or every side's dz (MODE 3)
template <int MODE>
static __device__ __forceinline__ size_t stream_out_off(const ConvParams& p, const StreamBn& bn, const PixSplit& ps, int m) {
    int bi, yy, xx;
    pix_split(ps, m, bi, yy, xx);
    if (MODE == 1) return ((size_t)(bi * p.yHp + yy + p.ypad) * p.yWp + (xx + p.ypad)) * p.yC;
    return ((size_t)(bi * bn.dzHp + yy + bn.dzpad) * bn.dzWp + (xx + bn.dzpad)) * p.Co;
}
// MODE 1: eight channels from `chan` on of pixel m (element offset off in p.y) and their byte of the ReLU bit map
static __device__ __forceinline__ void stream_store_out(const ConvParams& p, const StreamBn& bn, size_t off, int m, int chan, const uint4& ov) {
    vpd_store16<VPD_CP_EPI>(p.y + off + chan, ov);
    if (bn.mask_out) bn.mask_out[(size_t)m * (p.Co >> 3) + (chan >> 3)] = (unsigned char)stream_relu_bits(ov);
}
// MODE 2 of one convolution of the two-convolution kernel: sum g -> sg (WITH_G), sum g z -> sz, z rounded as stored (the
// one-convolution kernel forms the same sums inside its one tile loop: through this function its K = 64 instantiation lost a wave)
template <bool WITH_G, int NI, int MI>
static __device__ __forceinline__ void stream_bwd_sums(const f32x4 (&acc)[NI][MI], const AccFrag<NI, MI>& accf, int fq, float (&sg)[NI][4],
                                                       float (&sz)[NI][4]) {
#pragma unroll
    for (int b = 0; b < MI; ++b)
#pragma unroll
        for (int a0 = 0; a0 < NI; a0 += 2) {
            uint2 dv[2];
            frag_pair_unpack(accf.old[b].q[a0 / 2], dv[0], dv[1]);
#pragma unroll
            for (int ai = 0; ai < 2; ++ai) {
                const int a = a0 + ai;
                float z[4], d[4];
                stream_round4(acc[a][b], z);
                stream_unpack4(dv[ai], d);
                const unsigned bits = stream_mask4(accf.bits[b], a, fq);
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const float g = stream_masked_g(bits, j, d[j]);
                    if (WITH_G) sg[a][j] += g;
                    sz[a][j] += g * z[j];
                }
            }
        }
}

template <int KC, int NSA, int MODE>
__global__ __launch_bounds__(TAIL_THREADS) void conv1x1_bn_stream_kernel(const ConvParams p, const StreamGeo sg, const StreamBn bn) {
    // eight MFMA waves (two per SIMD: one's fragment reads and epilogue arithmetic under the other's MFMAs -- with four, the
    // statistics passes ran at 1.8-3 TB/s on phases that do not overlap inside one wave) x 32 pixels x 64 channels
    using B = StreamBlock<KC, TAIL_BM, TAIL_BN, NSA, TAIL_NMW>;
    constexpr int BM = B::BM, BN = B::BN, WM = B::WM, WN = B::WN, MI = B::MI, NI = B::NI;
    constexpr int PRE = MODE == 2 ? 0 : 1;
    static_assert(stream_lds_bytes(KC, BM, BN, NSA, 3) <= 160 * 1024, "LDS");
    if (B::loader()) {
        stream_loader<B, PRE, stream_tail_barriers(MODE == 2, 1)>(p, sg, B(sg));
        return;
    }
    const B blk(sg);
    const int fq = blk.fq;
    // ---- coefficient prologue (the first BN of the MFMA waves' threads): (scale, shift) or (A, B, D) ----
    if (PRE && blk.tid < BN) {
        const int ch = blk.n0 + blk.tid;
        if (MODE == 1) stream_bn_finalize(bn.s, bn, p.Co, ch, blk.coef + blk.tid, blk.coef + BN + blk.tid);
        else stream_bn_bwd_coef<BN>(bn.s, bn, p.Co, ch, blk.coef, blk.tid);
    }
    float4 k0[NI] = {}, k1[NI] = {}, k2[NI] = {};      // this lane's channels' coefficients
    if (PRE) {
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
#pragma unroll
        for (int a = 0; a < NI; ++a) {
            k0[a] = blk.coef4(0, a);
            k1[a] = blk.coef4(1, a);
            if (MODE == 3) k2[a] = blk.coef4(2, a);
        }
    }
    float st1[NI][4], st2[NI][4];
#pragma unroll
    for (int a = 0; a < NI; ++a)
#pragma unroll
        for (int j = 0; j < 4; ++j) { st1[a][j] = 0.f; st2[a][j] = 0.f; }
    const ConvGeo geo = {p.Hs, p.Ws, p.M, p.oph, p.opw};
    const PixSplit ps = pix_split_init(p, geo);
    for (int it = 0; it < blk.ntile; ++it) {
        const int mtile = blk.mtile(it);
        ResFrag<NI, MI> resf;      // MODE 1: the identity path (padded activation)
        AccFrag<NI, MI> accf;      // MODE 2 / 3: d(out) (dense) and its ReLU bits
        if (MODE == 1) conv_res_prefetch<BM, BN, WM, WN>(p, mtile, blk.n0, geo, resf);
        else conv_acc_prefetch<BM, BN, WM, WN>(p, mtile, blk.n0, geo, accf);
        f32x4 acc[NI][MI];
        zero_acc(acc);
        __builtin_amdgcn_s_barrier();                             // READY_it
        stream_mma<KC, BM, BN, WM, WN>(blk.sW, blk.stage(it), acc, blk.wm, blk.wn, blk.fr, fq);
#pragma unroll
        for (int b = 0; b < MI; ++b) {
            const int m = blk.pixel(mtile, b);
            const size_t poff = stream_out_off<MODE>(p, bn, ps, m);
#pragma unroll
            for (int a0 = 0; a0 < NI; a0 += 2) {
                uint2 ov2[2], ovs[2];      // the residual (MODE 1) or d(out) (MODE 2 / 3), back in the MFMA layout; what leaves
                frag_pair_unpack(MODE == 1 ? resf.r[b].q[a0 / 2] : accf.old[b].q[a0 / 2], ov2[0], ov2[1]);
#pragma unroll
                for (int ai = 0; ai < 2; ++ai) {
                    const int a = a0 + ai;
                    float z[4], o[4], v[4], c0[4], c1[4], c2[4];
                    stream_round4(acc[a][b], z);
                    stream_unpack4(ov2[ai], o);
                    stream_coef4(k0[a], c0);
                    stream_coef4(k1[a], c1);
                    stream_coef4(k2[a], c2);
                    if (MODE == 1) {
#pragma unroll
                        for (int j = 0; j < 4; ++j) {
                            v[j] = __builtin_fmaf(z[j], c0[j], c1[j]) + o[j];
                            v[j] = v[j] > 0.f ? v[j] : 0.f;
                        }
                    } else {
                        const unsigned bits = stream_mask4(accf.bits[b], a, fq);
#pragma unroll
                        for (int j = 0; j < 4; ++j) {
                            const float g = stream_masked_g(bits, j, o[j]);
                            if (MODE == 2) { st1[a][j] += g; st2[a][j] += g * z[j]; }
                            else v[j] = __builtin_fmaf(c0[j], g, __builtin_fmaf(c1[j], z[j], c2[j]));
                        }
                    }
                    if (MODE != 2) ovs[ai] = stream_pack4(v);
                }
                if (MODE == 2) continue;
                const uint4 ov = frag_pair_pack(ovs[0], ovs[1]);
                const int c = blk.nw + frag_pair_chan(a0, fq);
                if (MODE == 1) stream_store_out(p, bn, poff, m, c, ov);
                else vpd_store16<VPD_CP_EPI>(bn.s.dz + poff + c, ov);
            }
        }
    }
    __builtin_amdgcn_s_barrier();                                 // END
    if (MODE == 2) stream_stats_flush(bn.s.rows_out, VPD_FUSED_ROWS, p.Co, blk, st1, st2);
}

// ---------------------------------------------------------------------------
// The same for a DOWN-SAMPLING Bottleneck whose two 1x1 convolutions have 64 input channels each and stride 1 (layer1's first
// block): out = relu(BatchNorm3(conv3(a2)) + BatchNormD(convD(x))).  Both weight tiles are resident, a ring stage holds the
// a2 tile and the x tile of the same pixels, two accumulator sets per wave.  Neither z3 nor zd is ever stored.
//   MODE 1: both BatchNorms finalized in the prologue; out + ReLU bit map
//   MODE 2: g = d(out) * mask; sum g, sum g z3 -> BatchNorm3's rows; sum g, sum g zd -> BatchNormD's rows
//   MODE 3: dz3 = A3 g + B3 z3 + D3, dzd = Ad g + Bd zd + Dd -> two padded tensors; dgamma / dbeta of both
// (the statistics passes are two launches of conv1x1_stream_kernel<.., 4>, one per convolution)
// ---------------------------------------------------------------------------
template <int NSA, int MODE>
__global__ __launch_bounds__(TAIL_THREADS) void conv1x1_bn2_stream_kernel(const ConvParams p, const StreamGeo sg, const StreamBn bn,
                                                                          const StreamBnSide bd) {      // bn.s: BatchNorm3, bd: the branch's
    using B = StreamBlock<128, TAIL_BM, TAIL_BN, NSA, TAIL_NMW>;      // chunk 0: conv3, chunk 1: the branch
    constexpr int BM = B::BM, BN = B::BN, WM = B::WM, WN = B::WN, MI = B::MI, NI = B::NI;
    constexpr int PRE = MODE == 2 ? 0 : 1;
    constexpr int NK = MODE == 1 ? 2 : 3;              // coefficient rows per BatchNorm: (scale, shift) or (A, B, D)
    static_assert(stream_lds_bytes(128, BM, BN, NSA, 6) <= 160 * 1024, "LDS");
    if (B::loader()) {
        stream_loader<B, PRE, stream_tail_barriers(MODE == 2, 2), true>(p, sg, B(sg));
        return;
    }
    const B blk(sg);
    const int fq = blk.fq;
    if (PRE && blk.tid < BN) {
        const int ch = blk.n0 + blk.tid;
        if (MODE == 1) {
            stream_bn_finalize(bn.s, bn, p.Co, ch, blk.coef + blk.tid, blk.coef + BN + blk.tid);
            stream_bn_finalize(bd, bn, p.Co, ch, blk.coef + 2 * BN + blk.tid, blk.coef + 3 * BN + blk.tid);
        } else {
            stream_bn_bwd_coef<BN>(bn.s, bn, p.Co, ch, blk.coef, blk.tid);
            stream_bn_bwd_coef<BN>(bd, bn, p.Co, ch, blk.coef + 3 * BN, blk.tid);
        }
    }
    if (PRE) {
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
    }
    float st1[NI][4], st2[NI][4], st3[NI][4];
#pragma unroll
    for (int a = 0; a < NI; ++a)
#pragma unroll
        for (int j = 0; j < 4; ++j) { st1[a][j] = 0.f; st2[a][j] = 0.f; st3[a][j] = 0.f; }
    const ConvGeo geo = {p.Hs, p.Ws, p.M, p.oph, p.opw};
    const PixSplit ps = pix_split_init(p, geo);
    for (int it = 0; it < blk.ntile; ++it) {
        const int mtile = blk.mtile(it);
        AccFrag<NI, MI> accf;      // MODE 2 / 3: d(out) (dense) and its ReLU bits
        if (MODE != 1) conv_acc_prefetch<BM, BN, WM, WN>(p, mtile, blk.n0, geo, accf);
        f32x4 acc3[NI][MI], accd[NI][MI];
        zero_acc(acc3);
        zero_acc(accd);
        __builtin_amdgcn_s_barrier();                             // READY_it
        const bf16_t* const stg = blk.stage(it);
        if (MODE == 2) {
            // one accumulator set at a time (three sum sets of 16 registers beside it): conv3's sums, then the branch's
            stream_mma<64, BM, BN, WM, WN>(blk.sW, stg, acc3, blk.wm, blk.wn, blk.fr, fq);
            stream_bwd_sums<true>(acc3, accf, fq, st1, st2);
            zero_acc(acc3);
            stream_mma<64, BM, BN, WM, WN>(blk.sW + BN * 64, stg + BM * 64, acc3, blk.wm, blk.wn, blk.fr, fq);
            stream_bwd_sums<false>(acc3, accf, fq, st1, st3);
            continue;
        }
        stream_mma<64, BM, BN, WM, WN>(blk.sW, stg, acc3, blk.wm, blk.wn, blk.fr, fq);
        stream_mma<64, BM, BN, WM, WN>(blk.sW + BN * 64, stg + BM * 64, accd, blk.wm, blk.wn, blk.fr, fq);
        size_t poff[MI];           // this lane's pixels in the padded outputs (out, or dz3 / dzd: same geometry)
#pragma unroll
        for (int b = 0; b < MI; ++b) poff[b] = stream_out_off<MODE>(p, bn, ps, blk.pixel(mtile, b));
#pragma unroll
        for (int a0 = 0; a0 < NI; a0 += 2) {
            // the pair's coefficient rows, BatchNorm3's NK then the branch's NK: MODE 1 (scale3, shift3, scaleD, shiftD),
            // MODE 3 (A3, B3, D3, Ad, Bd, Dd) -- so a side's first two rows are [0], [1] / [NK], [NK + 1] and D is its last
            float4 kq[2][2 * NK];
#pragma unroll
            for (int ai = 0; ai < 2; ++ai)
#pragma unroll
                for (int q = 0; q < 2 * NK; ++q) kq[ai][q] = blk.coef4(q, a0 + ai);
            const int c = blk.nw + frag_pair_chan(a0, fq);
#pragma unroll
            for (int b = 0; b < MI; ++b) {
                uint2 dv[2], o3[2], od[2];
                if (MODE == 3) frag_pair_unpack(accf.old[b].q[a0 / 2], dv[0], dv[1]);
#pragma unroll
                for (int ai = 0; ai < 2; ++ai) {
                    const int a = a0 + ai;
                    float z3[4], zd[4], v[4], w[4], k[2 * NK][4];
#pragma unroll
                    for (int q = 0; q < 2 * NK; ++q) stream_coef4(kq[ai][q], k[q]);
                    stream_round4(acc3[a][b], z3);
                    stream_round4(accd[a][b], zd);
                    if (MODE == 1) {
#pragma unroll
                        for (int j = 0; j < 4; ++j) {
                            v[j] = __builtin_fmaf(z3[j], k[0][j], k[1][j]) + __builtin_fmaf(zd[j], k[NK][j], k[NK + 1][j]);
                            v[j] = v[j] > 0.f ? v[j] : 0.f;
                        }
                    } else {
                        float d[4];
                        stream_unpack4(dv[ai], d);
                        const unsigned bits = stream_mask4(accf.bits[b], a, fq);
#pragma unroll
                        for (int j = 0; j < 4; ++j) {
                            const float g = stream_masked_g(bits, j, d[j]);
                            v[j] = __builtin_fmaf(k[0][j], g, __builtin_fmaf(k[1][j], z3[j], k[NK - 1][j]));
                            w[j] = __builtin_fmaf(k[NK][j], g, __builtin_fmaf(k[NK + 1][j], zd[j], k[2 * NK - 1][j]));
                        }
                        od[ai] = stream_pack4(w);
                    }
                    o3[ai] = stream_pack4(v);
                }
                const uint4 ov = frag_pair_pack(o3[0], o3[1]);
                if (MODE == 1) {
                    stream_store_out(p, bn, poff[b], blk.pixel(mtile, b), c, ov);
                } else {
                    vpd_store16<VPD_CP_EPI>(bn.s.dz + poff[b] + c, ov);
                    vpd_store16<VPD_CP_EPI>(bd.dz + poff[b] + c, frag_pair_pack(od[0], od[1]));
                }
            }
        }
    }
    __builtin_amdgcn_s_barrier();                                 // END
    if (MODE == 2) stream_stats_flush2(bn.s.rows_out, bd.rows_out, VPD_FUSED_ROWS, p.Co, blk, st1, st2, st3);
}

// pixel lanes (gridDim.x) of a launch with NT channel tiles on `mtiles` pixel tiles
int stream_lanes(int mtiles, int NT) {
    int lanes = vpd_cu_budget() / NT;
    lanes -= lanes % 8;                      // blocks b and b + 8 share an XCD: the NT channel tiles of a pixel tile meet in its L2
    if (lanes < 8) lanes = 8;
    if (lanes > mtiles) lanes = mtiles;
    return lanes;
}
// ring depths of the fused kernels (K = 64, K = 128, the two-convolution kernel)
constexpr int BN_NSA_K64 = 8, BN_NSA_K128 = 5, BN2_NSA = 5;

// tile shape for (Kc, Co): wide channel tiles take 64-pixel tiles (64 accumulator registers beside the prefetched fragments)
void stream_shape(int Kc, int Co, int* bm, int* bn) {
    int n = Co % 256 == 0 ? 256 : Co % 128 == 0 ? 128 : 64;      // (only the instantiated widths: Co = 192 runs on 64-wide tiles)
    if (Kc == 256 && n > 128) n = 128;      // 64 KB of weights + the ring
    *bn = n;
    // 256 input channels: 32 KB per 64 pixels -- small tiles keep 96 KB per CU in flight (128-pixel tiles with two stages
    // and 64 x 128 with three: 4.0-4.3 TB/s; these: +0.9 % on the ResNet-50 step, same box)
    *bm = n == 256 ? 64 : (Kc == 256 ? (n == 64 ? 64 : 32) : 128);
}

StreamGeo stream_geo(const ConvParams& p, int BM) {
    StreamGeo sg;
    sg.mtiles = p.M / BM;
    sg.tiles_per_img = (p.Hs * p.Ws) / BM;
    sg.rows_per_tile = BM / p.Ws;
    return sg;
}

template <int KC, int BM, int BN, int NSA>
hipError_t launch_stream(const ConvParams& p, hipStream_t stream) {
    const StreamGeo sg = stream_geo(p, BM);
    const int NT = p.Co / BN;
    const dim3 grid(stream_lanes(sg.mtiles, NT), NT);
    constexpr size_t lds = stream_lds_bytes(KC, BM, BN, NSA);
    if (!Conv1x1StreamModes::visit(conv_ep_mode(p), [&](auto m) {
            VPD_LAUNCH((conv1x1_stream_kernel<KC, BM, BN, NSA, decltype(m)::value>), grid, dim3(512), lds, stream, p, sg);
        })) return hipErrorInvalidValue;
    return hipGetLastError();
}

}  // namespace

// 1x1, one tap, one class, <= 256 input channels, whole-row pixel tiles, enough tiles for every CU to stream
bool vpd_conv1x1_stream_eligible(const ConvParams& p) {
    if (!vpd_switches().conv1x1_stream) return false;
    if (p.taps.nr != 1 || p.taps.nc != 1 || p.ncls > 1 || p.alt_w || p.x2 || p.bst_z || p.bst_z2 || p.pool_y) return false;
    if (p.osub != 1 || p.oph != 0 || p.opw != 0 || (p.istr != 1 && p.istr != 2)) return false;
    if (p.Kc != 64 && p.Kc != 128 && p.Kc != 256) return false;
    if (p.xC != p.Kc || p.Co % 64 != 0) return false;
    if (p.accumulate && (p.ypad != 0 || p.yWp != p.Ws || p.yHp != p.Hs)) return false;      // (prefetched old values: dense y)
    int bm, bn;
    stream_shape(p.Kc, p.Co, &bm, &bn);
    if (p.Co % bn != 0) return false;
    if (p.Ws <= 0 || bm % p.Ws != 0 || (p.Hs * p.Ws) % bm != 0) return false;
    if (p.M != p.N * p.Hs * p.Ws || p.M / bm < 2 * vpd_cu_budget()) return false;
    if (p.M >= VPD_FDIV_MAX) return false;
    return (long)p.N * p.xHp * p.xWp * p.xC < (1l << 31) && (long)p.Co * p.Kc * (p.taps.w0 + 1) < (1l << 31);
}

hipError_t vpd_launch_conv1x1_stream(const ConvParams& p, hipStream_t stream) {
    int bm, bn;
    stream_shape(p.Kc, p.Co, &bm, &bn);
    switch (p.Kc) {
        case 64:
            if (bn == 64) return launch_stream<64, 128, 64, 6>(p, stream);
            if (bn == 128) return launch_stream<64, 128, 128, 6>(p, stream);
            return launch_stream<64, 64, 256, 8>(p, stream);
        case 128:
            if (bn == 64) return launch_stream<128, 128, 64, 4>(p, stream);
            if (bn == 128) return launch_stream<128, 128, 128, 4>(p, stream);
            return launch_stream<128, 64, 256, 6>(p, stream);
        case 256:
            if (bn == 64) return launch_stream<256, 64, 64, 4>(p, stream);
            return launch_stream<256, 32, 128, 6>(p, stream);
        default: break;
    }
    return hipErrorInvalidValue;
}

// host-side reporting (vpd_conv_dispatch): the tile the launcher above picks for `p` and its pixel lanes
void vpd_conv1x1_stream_grid(const ConvParams& p, int* bm, int* bn, int* lanes) {
    stream_shape(p.Kc, p.Co, bm, bn);
    *lanes = stream_lanes(p.M / *bm, p.Co / *bn);
}

// ---- the closing 1x1 convolution of a Bottleneck with its BatchNorm (conv1x1_bn_stream_kernel) ----
bool vpd_conv1x1_bn_eligible(const ConvParams& p) {
    if (!vpd_switches().bneck_recompute || !vpd_conv1x1_stream_eligible(p)) return false;
    if (p.istr != 1 || (p.Kc != 64 && p.Kc != 128) || p.Co % TAIL_BN != 0 || p.accumulate || p.ep_scale) return false;
    return p.M % TAIL_BM == 0 && TAIL_BM % p.Ws == 0 && (p.Hs * p.Ws) % TAIL_BM == 0;
}

namespace {
// what the BatchNorms of a launch share; BN_TAIL_BWD_APPLY writes every dz padded by dzpad
StreamBn stream_bn(float count, float momentum, float eps, unsigned char* mask_out, const ConvParams& p, int dzpad) {
    StreamBn bn;
    memset(&bn, 0, sizeof bn);
    bn.count = count; bn.momentum = momentum; bn.eps = eps; bn.mask_out = mask_out;
    bn.dzHp = p.Hs + 2 * dzpad; bn.dzWp = p.Ws + 2 * dzpad; bn.dzpad = dzpad;
    return bn;
}
// BN_TAIL_FWD: one BatchNorm of a BnFusedFwd
StreamBnSide stream_side_fwd(const BnFwdSide& f) {
    StreamBnSide s;
    memset(&s, 0, sizeof s);
    s.rows = f.rows; s.gamma = f.gamma; s.beta = f.beta; s.mean = f.mean; s.rstd = f.rstd; s.scale = f.scale; s.shift = f.shift;
    s.rm = f.rm; s.rv = f.rv;
    return s;
}
// BN_TAIL_BWD_SUMS: the rows to add to; BN_TAIL_BWD_APPLY: the same rows to finalize, with the forward's mean / rstd and the dz to write
StreamBnSide stream_side_bwd(const BnBwdSide& b, BnTailPass pass) {
    StreamBnSide s;
    memset(&s, 0, sizeof s);
    if (pass == BN_TAIL_BWD_SUMS) { s.rows_out = b.rows; return s; }
    s.rows = b.rows; s.gamma = b.gamma; s.dgamma = b.dgamma; s.dbeta = b.dbeta;
    s.mean = const_cast<float*>(b.mean); s.rstd = const_cast<float*>(b.rstd); s.dz = b.dz;
    return s;
}
// what a forward / a backward launch's BatchNorms share
StreamBn stream_bn_fwd(const BnTailLaunch& t, const ConvParams& p) {
    StreamBn bn = stream_bn(t.fwd->count, t.fwd->momentum, t.fwd->eps, t.mask_out, p, 0);
    bn.frozen = t.fwd->frozen;
    return bn;
}
StreamBn stream_bn_bwd(const BnTailLaunch& t, const ConvParams& p) {
    StreamBn bn = stream_bn(t.bwd->count, 0.f, 0.f, nullptr, p, t.dzpad);
    bn.frozen = t.bwd->frozen;
    return bn;
}
bool stream_side_apply_ok(const BnBwdSide& b) { return b.dz && b.mean && b.rstd; }
// the backward passes read p.y = d(out), dense, with its bit map
bool stream_bwd_operands(const ConvParams& p) {
    return p.y && p.acc_mask && p.ypad == 0 && p.yC == p.Co && p.yHp == p.Hs && p.yWp == p.Ws;
}

template <int KC, int NSA>
hipError_t launch_bn_stream(const ConvParams& p, const StreamBn& bn, BnTailPass pass, hipStream_t stream) {
    constexpr int BM = TAIL_BM, BN = TAIL_BN;
    const StreamGeo sg = stream_geo(p, BM);
    const int NT = p.Co / BN;
    const dim3 grid(stream_lanes(sg.mtiles, NT), NT), block(TAIL_THREADS);
    constexpr size_t lds = stream_lds_bytes(KC, BM, BN, NSA, 3);
    switch (pass) {
        // (four MFMA waves as the storing launch: the same pixels per lane, so the same fp32 partial sums -- the fused forward is
        //  bit-identical to conv + BatchNorm launches; eight waves were no faster here, 16.4-18.2 vs 17.8-19.4 us)
        case BN_TAIL_STATS: VPD_LAUNCH((conv1x1_stream_kernel<KC, BM, BN, NSA, 4>), grid, dim3(512), lds, stream, p, sg); break;
        case BN_TAIL_FWD: VPD_LAUNCH((conv1x1_bn_stream_kernel<KC, NSA, 1>), grid, block, lds, stream, p, sg, bn); break;
        case BN_TAIL_BWD_SUMS: VPD_LAUNCH((conv1x1_bn_stream_kernel<KC, NSA, 2>), grid, block, lds, stream, p, sg, bn); break;
        case BN_TAIL_BWD_APPLY: VPD_LAUNCH((conv1x1_bn_stream_kernel<KC, NSA, 3>), grid, block, lds, stream, p, sg, bn); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}
}  // namespace

// one pass (BnTailPass, kernels.h) of the tail: t.fwd->s[0] / t.bwd->s[0] is the BatchNorm
hipError_t vpd_launch_conv1x1_bn(const ConvParams& p, const BnTailLaunch& t, hipStream_t stream) {
    if (!vpd_conv1x1_bn_eligible(p)) return hipErrorInvalidValue;
    StreamBn bn = stream_bn(0.f, 0.f, 0.f, nullptr, p, 0);
    if (t.pass == BN_TAIL_STATS) {
        if (!p.stats || p.stat_rows != VPD_FUSED_ROWS) return hipErrorInvalidValue;
    } else if (t.pass == BN_TAIL_FWD) {
        if (!t.fwd || !p.res || !p.y || p.ypad != 1 || p.yC != p.Co || p.rC != p.Co) return hipErrorInvalidValue;
        if (t.fwd->frozen && (!t.fwd->s[0].rm || !t.fwd->s[0].rv)) return hipErrorInvalidValue;
        bn = stream_bn_fwd(t, p);
        bn.s = stream_side_fwd(t.fwd->s[0]);
    } else {
        if (!t.bwd || !stream_bwd_operands(p)) return hipErrorInvalidValue;
        if (t.pass == BN_TAIL_BWD_APPLY && !stream_side_apply_ok(t.bwd->s[0])) return hipErrorInvalidValue;
        bn = stream_bn_bwd(t, p);
        bn.s = stream_side_bwd(t.bwd->s[0], t.pass);
    }
    if (p.Kc == 64) return launch_bn_stream<64, BN_NSA_K64>(p, bn, t.pass, stream);
    return launch_bn_stream<128, BN_NSA_K128>(p, bn, t.pass, stream);
}

// ---- ... of a down-sampling Bottleneck with two 64-channel stride-1 1x1 convolutions (conv1x1_bn2_stream_kernel): p.x / p.w =
// the closing convolution, p.x2 / p.w2 = the branch (same padded input geometry).  t.fwd / t.bwd: s[0] = BatchNorm3, s[1] = the
// branch's.  Every pass but BN_TAIL_STATS (the statistics passes are two launches of vpd_launch_conv1x1_bn).
bool vpd_conv1x1_bn2_eligible(const ConvParams& p) {
    if (!(p.x2 && p.w2 && p.Kc == 64 && p.Kc2 == 64 && p.Co == TAIL_BN)) return false;
    ConvParams q = p;
    q.x2 = nullptr; q.w2 = nullptr; q.Kc2 = 0;
    return vpd_conv1x1_bn_eligible(q);
}
hipError_t vpd_launch_conv1x1_bn2(const ConvParams& p, const BnTailLaunch& t, hipStream_t stream) {
    if (!vpd_conv1x1_bn2_eligible(p)) return hipErrorInvalidValue;
    StreamBn bn;
    StreamBnSide bd;
    if (t.pass == BN_TAIL_FWD) {
        if (!t.fwd || !t.fwd->s[1].rows || !p.y || p.ypad != 1 || p.yC != p.Co) return hipErrorInvalidValue;
        if (t.fwd->frozen && (!t.fwd->s[0].rm || !t.fwd->s[0].rv || !t.fwd->s[1].rm || !t.fwd->s[1].rv)) return hipErrorInvalidValue;
        bn = stream_bn_fwd(t, p);
        bn.s = stream_side_fwd(t.fwd->s[0]);
        bd = stream_side_fwd(t.fwd->s[1]);
    } else if (t.pass == BN_TAIL_BWD_SUMS || t.pass == BN_TAIL_BWD_APPLY) {
        if (!t.bwd || !t.bwd->s[1].rows || !stream_bwd_operands(p)) return hipErrorInvalidValue;
        if (t.pass == BN_TAIL_BWD_APPLY && !(stream_side_apply_ok(t.bwd->s[0]) && stream_side_apply_ok(t.bwd->s[1]))) return hipErrorInvalidValue;
        bn = stream_bn_bwd(t, p);
        bn.s = stream_side_bwd(t.bwd->s[0], t.pass);
        bd = stream_side_bwd(t.bwd->s[1], t.pass);
    } else return hipErrorInvalidValue;
    constexpr int BM = TAIL_BM, BN = TAIL_BN, NSA = BN2_NSA;
    const StreamGeo sg = stream_geo(p, BM);
    const dim3 grid(stream_lanes(sg.mtiles, 1), 1), block(TAIL_THREADS);
    constexpr size_t lds = stream_lds_bytes(128, BM, BN, NSA, 6);
    switch (t.pass) {
        case BN_TAIL_FWD: VPD_LAUNCH((conv1x1_bn2_stream_kernel<NSA, 1>), grid, block, lds, stream, p, sg, bn, bd); break;
        case BN_TAIL_BWD_SUMS: VPD_LAUNCH((conv1x1_bn2_stream_kernel<NSA, 2>), grid, block, lds, stream, p, sg, bn, bd); break;
        default: VPD_LAUNCH((conv1x1_bn2_stream_kernel<NSA, 3>), grid, block, lds, stream, p, sg, bn, bd); break;
    }
    return hipGetLastError();
}

// host-side reporting (vpd_op_conv1x1_bn_dispatch): the grid of the launches above for an eligible `p` -- pixel lanes, channel
// tiles, pixel tiles of the busiest block, ring depth
void vpd_conv1x1_bn_grid(const ConvParams& p, bool two, int out4[4]) {
    const int mtiles = p.M / TAIL_BM;
    const int NT = two ? 1 : p.Co / TAIL_BN;
    const int lanes = stream_lanes(mtiles, NT);
    out4[0] = lanes; out4[1] = NT; out4[2] = (mtiles + lanes - 1) / lanes;
    out4[3] = two ? BN2_NSA : p.Kc == 64 ? BN_NSA_K64 : BN_NSA_K128;
}
