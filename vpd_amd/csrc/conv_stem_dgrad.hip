// Data gradient of the stem convolution (7x7, stride 2, padding 3; models/module.py:58 through loss.backward(), models/util.py:52):
//   dx = conv_transpose2d(dz, w, stride 2, padding 3, output_padding 1)
// dz: dense NHWC [N][H/2][W/2][64] elements, w: the fp32 master weight [64][Cin][7][7] (rounded to the element type here, as
// vpd_pack_weights rounds it), dx: fp32 NCHW [N][Cin][H][W].  Training never needs it (nothing sits in front of the stem); it is
// the input gradient of the autograd path (vpd_backward_ext).
//
// Split by output parity, the transposed convolution is a GEMM per output row Y = 2 t + par:
//   rows     M  the column pairs j (X = 2 j + xpar)
//   columns  N = 16 = (xpar, input channel padded to 8)
//   depth    K  = (dox in -1..2) x (kernel-row slot s) x (64 output channels): kernel row ky = 2 s + 1 - par (3 rows for even Y,
//               4 for odd Y), dz row oy = t + 1 + par - s, dz column ox = j + dox, kernel column kx = xpar + 3 - 2 dox (the slot
//               is zero when kx is outside 0..6: xpar = 0, dox = 2)
// The B matrix (both row parities, 24 + 32 K-steps of 32) is built once per block in LDS, already in the lane order of
// v_mfma_f32_16x16x32's B fragment.  Blocks are persistent over tiles of 8 output rows x 64 column pairs of one image: the 7 dz
// rows x 67 dz columns a tile reads are staged in LDS (zeros outside the image: dz has no border), one plane per 16-byte channel
// chunk so that the A-fragment reads (16 pixels x 4 chunks per K-step) are conflict-free; the next tile's rows are fetched into
// registers while the current one is multiplied.  Wave w owns output row 8 rb + w: 4 accumulator tiles of 16 pairs.  Both column
// parities of a pair sit in one accumulator tile (lanes l and l ^ 8): one lane exchange, then every lane stores 4 consecutive X.
#include "common.h"
#include "kernels.h"

#define SD_TJ 64            // column pairs per tile
#define SD_ROWS 7           // dz rows a tile of 8 output rows reads
#define SD_PXU 67           // dz columns it reads (TJ + 3)
#define SD_PX 80            // pixel slots of a chunk plane (a multiple of 16: planes are 256-byte multiples apart)
#define SD_KS0 24           // K-steps of an even output row (4 dox x 3 kernel rows x 2 halves of the 64 channels)
#define SD_KS1 32           // ... of an odd one (4 kernel rows)
#define SD_ITEMS (SD_ROWS * 9 * 64)      // 16-byte items staged per tile: 9 groups of 8 pixels x 8 chunks per row
#define SD_LDS ((size_t)((SD_KS0 + SD_KS1) * 64 + SD_ROWS * 8 * SD_PX) * 16)

namespace {

struct StemDgradTile { int b, rb, j0; };
static __device__ __forceinline__ StemDgradTile sd_tile(int t, int nrb, int nct) {
    StemDgradTile q;
    const int ct = t % nct;
    const int u = t / nct;
    q.rb = u % nrb; q.b = u / nrb; q.j0 = ct * SD_TJ;
    return q;
}

// the tile's dz range into registers: thread `tid` takes items tid + 512 k; item i = (row, group of 8 pixels, chunk, pixel in
// group) with the pixel fastest inside 8 lanes -- a wave reads 1 KiB of contiguous NHWC and writes 8 x 128 contiguous LDS bytes
static __device__ __forceinline__ void sd_fetch(const bf16_t* dz, const StemDgradTile& q, int Hz, int Wz, int tid, uint4 (&pre)[8]) {
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const int i = tid + 512 * k;
        const int g = i >> 6, r = g / 9, pg = g - r * 9;
        const int p = pg * 8 + (i & 7), c = (i >> 3) & 7;
        const int oy = q.rb * 4 - 1 + r, ox = q.j0 - 1 + p;
        uint4 v = uint4{0u, 0u, 0u, 0u};
        if (i < SD_ITEMS && p < SD_PXU && oy >= 0 && oy < Hz && ox >= 0 && ox < Wz)
            v = *reinterpret_cast<const uint4*>(dz + (((size_t)q.b * Hz + oy) * Wz + ox) * 64 + c * 8);
        pre[k] = v;
    }
}
static __device__ __forceinline__ void sd_stage(uint4* sA, int tid, const uint4 (&pre)[8]) {
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const int i = tid + 512 * k;
        const int g = i >> 6, r = g / 9, pg = g - r * 9;
        const int p = pg * 8 + (i & 7), c = (i >> 3) & 7;
        if (i < SD_ITEMS) sA[(r * 8 + c) * SD_PX + p] = pre[k];      // (p <= 71 < SD_PX; slots 67.. are never read)
    }
}

// one output row of parity PAR: acc[mt] += A(16 pairs of tile mt) x B over the parity's K-steps
template <int PAR>
static __device__ __forceinline__ void sd_row(const uint4* sA, const uint4* sB, int tl, int lane, int nmt, f32x4 (&acc)[4]) {
    constexpr int NKY = 3 + PAR;
    const uint4* bp = sB + (PAR ? SD_KS0 * 64 : 0) + lane;
    const uint4* ap = sA + (lane >> 4) * SD_PX + (lane & 15);
#pragma unroll
    for (int doxi = 0; doxi < 4; ++doxi) {
#pragma unroll
        for (int s = 0; s < NKY; ++s) {
            const int r = tl + 2 + PAR - s;                          // staged row of oy = t + 1 + PAR - s
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const bf16x8 bf = __builtin_bit_cast(bf16x8, bp[((doxi * NKY + s) * 2 + h) * 64]);
                const uint4* a = ap + (r * 8 + h * 4) * SD_PX + doxi;
#pragma unroll
                for (int mt = 0; mt < 4; ++mt)
                    if (mt < nmt) acc[mt] = VPD_MFMA16(__builtin_bit_cast(bf16x8, a[mt * 16]), bf, acc[mt]);
            }
        }
    }
}

template <bool VEC4>
__global__ __launch_bounds__(512) void conv_stem_dgrad_kernel(const bf16_t* __restrict__ dz, const float* __restrict__ w,
                                                              float* __restrict__ dx, int Cin, int H, int W, int ntiles,
                                                              int nrb, int nct) {
    extern __shared__ __attribute__((aligned(16))) unsigned char sd_smem[];
    uint4* sB = reinterpret_cast<uint4*>(sd_smem);                   // [24 + 32 K-steps][64 lanes] B fragments
    uint4* sA = sB + (SD_KS0 + SD_KS1) * 64;                         // [7 rows][8 chunks][SD_PX pixels]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int Hz = H >> 1, Wz = W >> 1;

    uint4 pre[8];
    int t = blockIdx.x;
    StemDgradTile q = sd_tile(t, nrb, nct);
    sd_fetch(dz, q, Hz, Wz, tid, pre);

    // B: lane l of K-step ks holds B[k = 8 (l >> 4) + e][column l & 15], e = 0..7
    for (int i = tid; i < (SD_KS0 + SD_KS1) * 64; i += 512) {
        const int ks = i >> 6, l = i & 63;
        const int par = ks >= SD_KS0 ? 1 : 0;
        const int k2 = ks - par * SD_KS0, nky = 3 + par;
        const int h = k2 & 1, pr = k2 >> 1;
        const int doxi = pr / nky, s = pr - doxi * nky;
        const int col = l & 15, xpar = col >> 3, ch = col & 7;
        const int ky = 2 * s + 1 - par, kx = xpar + 5 - 2 * doxi;    // dox = doxi - 1
        const int co0 = h * 32 + 8 * (l >> 4);
        float v[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = 0.f;
        if (ch < Cin && kx >= 0 && kx <= 6) {
#pragma unroll
            for (int e = 0; e < 8; ++e) v[e] = w[((size_t)(co0 + e) * Cin + ch) * 49 + ky * 7 + kx];
        }
        sB[i] = pack8(v);
    }

    const int qd = lane >> 4, col = lane & 15, xpar = col >> 3, ch = col & 7;
    for (; t < ntiles; t += gridDim.x) {
        sd_stage(sA, tid, pre);
        __syncthreads();
        const StemDgradTile cur = q;
        if (t + (int)gridDim.x < ntiles) {
            q = sd_tile(t + gridDim.x, nrb, nct);
            sd_fetch(dz, q, Hz, Wz, tid, pre);
        }
        const int Y = cur.rb * 8 + wave;
        const int left = Wz - cur.j0;                                // pairs of this column tile inside the image (>= 1)
        const int nmt = left >= SD_TJ ? 4 : (left + 15) >> 4;
        if (Y < H) {                                                 // (wave-uniform)
            f32x4 acc[4];
#pragma unroll
            for (int mt = 0; mt < 4; ++mt) acc[mt] = f32x4{0.f, 0.f, 0.f, 0.f};
            if (wave & 1) sd_row<1>(sA, sB, wave >> 1, lane, nmt, acc);
            else sd_row<0>(sA, sB, wave >> 1, lane, nmt, acc);
            // accumulator: column = (xpar, ch) on the lane, pair 4 qd + reg in the registers.  Lanes l and l ^ 8 hold the two
            // parities of the same pairs: the xpar = 0 lane ends up with X = 8 qd + 0..3, the xpar = 1 lane with 8 qd + 4..7
            float* row = dx + (((size_t)cur.b * Cin + (ch < Cin ? ch : 0)) * H + Y) * W;
#pragma unroll
            for (int mt = 0; mt < 4; ++mt) {
                if (mt < nmt) {                                      // (block-uniform)
                    const f32x4 a = acc[mt];
                    const float r0 = __shfl_xor(xpar ? a[0] : a[2], 8, 64);
                    const float r1 = __shfl_xor(xpar ? a[1] : a[3], 8, 64);
                    const float4 o = xpar ? float4{r0, a[2], r1, a[3]} : float4{a[0], r0, a[1], r1};
                    const int ja = cur.j0 + mt * 16 + 4 * qd + 2 * xpar;      // first of this lane's two pairs
                    if (ch < Cin) {
                        if (VEC4) {                                  // W % 4 == 0: Wz even, both pairs inside together
                            if (ja < Wz) *reinterpret_cast<float4*>(row + 2 * ja) = o;
                        } else {
                            if (ja < Wz) *reinterpret_cast<float2*>(row + 2 * ja) = float2{o.x, o.y};
                            if (ja + 1 < Wz) *reinterpret_cast<float2*>(row + 2 * ja + 2) = float2{o.z, o.w};
                        }
                    }
                }
            }
        }
        __syncthreads();
    }
}

}  // namespace

hipError_t vpd_launch_stem_dgrad(const bf16_t* dz, const float* w_oihw, float* dx_nchw, int N, int Cin, int H, int W,
                                 hipStream_t s) {
    const int nrb = (H + 7) / 8, nct = (W / 2 + SD_TJ - 1) / SD_TJ;
    const long long nt = (long long)N * nrb * nct;
    if (nt < 1 || nt > 0x7fffffffLL) return hipErrorInvalidValue;
    if (reinterpret_cast<size_t>(dx_nchw) & 7) return hipErrorInvalidValue;      // the pair stores are 8 bytes wide
    const int ntiles = (int)nt;
    const int ncu = vpd_cu_budget();
    const int grid = ntiles < ncu ? ntiles : ncu;
    const bool vec4 = (W & 3) == 0 && (reinterpret_cast<size_t>(dx_nchw) & 15) == 0;
    if (vec4)
        hipLaunchKernelGGL((conv_stem_dgrad_kernel<true>), dim3(grid), dim3(512), SD_LDS, s, dz, w_oihw, dx_nchw, Cin, H, W, ntiles, nrb, nct);
    else
        hipLaunchKernelGGL((conv_stem_dgrad_kernel<false>), dim3(grid), dim3(512), SD_LDS, s, dz, w_oihw, dx_nchw, Cin, H, W, ntiles, nrb, nct);
    return hipGetLastError();
}
