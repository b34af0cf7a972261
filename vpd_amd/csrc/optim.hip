// Layout conversion at the reference boundary (fp32 NCHW / OIHW <-> internal
// bf16 NHWC / packed-tap weights) and the fused AdamW step.
#include "../../include/vpd_hip.h"
#include "common.h"
#include "kernels.h"

// f32 [N][C][H][W] -> bf16 [N][Hp][Wp][Cp] interior (zero border is pre-set and never written).
// A thread converts 4 consecutive pixels of a row: one float4 per channel plane in, four 16-byte pixels out.
// CT: the channel count as a compile-time constant (3, 5, 6), or 0 = run-time C with CLAMPED unconditional loads -- a
// per-channel "load or zero" on a run-time condition makes hipcc branch around every load and wait for each one
// (54 us for 84 MB; /opt/skills/guides/cdna_hip_programming.md, "three .s-level traps" (c))
template <int CT>
__global__ __launch_bounds__(256) void pack_input_kernel(const float* x, int N, int C, int H, int W, bf16_t* out,
                                                         int Hp, int Wp, int pad, int Cp) {
    const int W4 = W >> 2;
    const long total = (long)N * H * W4;
    const long plane = (long)H * W;
    const int Cn = CT ? CT : C;
    // (item -> (image, row, pixel quad): the 64-bit divisions of the generic form were most of an item's vector instructions -- 40 us
    //  for 157 MB; item counts below 2^21 split exactly with the float reciprocal, vpd_fdiv)
    const bool fast = total < VPD_FDIV_MAX;
    const float rW4 = 1.0f / (float)W4, rH = 1.0f / (float)H;
    for (long it = (long)blockIdx.x * blockDim.x + threadIdx.x; it < total; it += (long)gridDim.x * blockDim.x) {
        int b, y, x0;
        if (fast) {
            const int q = vpd_fdiv((int)it, rW4);              // b * H + y
            x0 = ((int)it - q * W4) << 2;
            b = vpd_fdiv(q, rH);
            y = q - b * H;
        } else {
            b = (int)(it / ((long)H * W4));
            const long r4 = it - (long)b * H * W4;
            y = (int)(r4 / W4);
            x0 = (int)(r4 - (long)y * W4) << 2;
        }
        const float* src = x + (size_t)b * Cn * plane + (size_t)y * W + x0;
        float4 f[8];
        if (CT) {
#pragma unroll
            for (int c = 0; c < 8; ++c)
                f[c] = c < CT ? *reinterpret_cast<const float4*>(src + (size_t)c * plane) : float4{0.f, 0.f, 0.f, 0.f};
        } else {
#pragma unroll
            for (int c = 0; c < 8; ++c) {
                const int cc = c < Cn ? c : Cn - 1;
                f[c] = *reinterpret_cast<const float4*>(src + (size_t)cc * plane);
            }
#pragma unroll
            for (int c = 0; c < 8; ++c)
                if (c >= Cn) f[c] = float4{0.f, 0.f, 0.f, 0.f};
        }
        float v[4][8];
#pragma unroll
        for (int c = 0; c < 8; ++c) { v[0][c] = f[c].x; v[1][c] = f[c].y; v[2][c] = f[c].z; v[3][c] = f[c].w; }
        bf16_t* dst = out + ((size_t)(b * Hp + y + pad) * Wp + x0 + pad) * Cp;
#pragma unroll
        for (int q = 0; q < 4; ++q) *reinterpret_cast<uint4*>(dst + q * Cp) = pack8(v[q]);
    }
}
// widths that are not a multiple of 4: one pixel per thread
__global__ __launch_bounds__(256) void pack_input_px_kernel(const float* x, int N, int C, int H, int W, bf16_t* out,
                                                            int Hp, int Wp, int pad, int Cp) {
    const long total = (long)N * H * W;
    const long plane = (long)H * W;
    for (long it = (long)blockIdx.x * blockDim.x + threadIdx.x; it < total; it += (long)gridDim.x * blockDim.x) {
        const int b = (int)(it / plane);
        const long r = it - (long)b * plane;
        const int y = (int)(r / W);
        const int xx = (int)(r - (long)y * W);
        float v[8];
#pragma unroll
        for (int c = 0; c < 8; ++c) v[c] = c < C ? x[((size_t)b * C + c) * plane + r] : 0.f;
        *reinterpret_cast<uint4*>(out + ((size_t)(b * Hp + y + pad) * Wp + xx + pad) * Cp) = pack8(v);
    }
}
// Rows of a multiple of 64 pixels (the 128 x 128 crops of every BASELINE config): a wave takes 256 consecutive pixels of an image --
// one float4 per lane and channel plane in (1 KB per instruction), through its own 8 KB of LDS ([plane][256 pixels]: written four
// pixels per lane, read one pixel per lane), one 16-byte pixel per lane out: every store instruction covers 1 KB of one padded row.
// (pack_input_kernel's lanes write 64-byte pieces 64 bytes apart with four instructions that each touch 64 different lines.)
template <int CT>
__global__ __launch_bounds__(256) void pack_input_rows_kernel(const float* x, int N, int H, int W, bf16_t* out, int Hp, int Wp,
                                                              int pad) {
    __shared__ float lds[4][CT][256];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long plane = (long)H * W;
    const long nwork = (long)N * plane / 256;                          // (H * W % 256 == 0: checked by the launcher)
    const int per_img = (int)(plane / 256);
    float (*my)[256] = lds[wave];
    for (long it = (long)blockIdx.x * 4 + wave; it < nwork; it += (long)gridDim.x * 4) {
        const int b = (int)(it / per_img);
        const int p0 = (int)(it - (long)b * per_img) * 256;            // first pixel of the image
        const float* src = x + (size_t)b * CT * plane + p0 + 4 * lane;
        float4 f[CT];
#pragma unroll
        for (int c = 0; c < CT; ++c) f[c] = *reinterpret_cast<const float4*>(src + (size_t)c * plane);
#pragma unroll
        for (int c = 0; c < CT; ++c) *reinterpret_cast<float4*>(&my[c][4 * lane]) = f[c];
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int p = p0 + q * 64 + lane;
            const int y = p / W, xx = p - y * W;
            float v[8];
#pragma unroll
            for (int c = 0; c < 8; ++c) v[c] = c < CT ? my[c][q * 64 + lane] : 0.f;
            *reinterpret_cast<uint4*>(out + ((size_t)(b * Hp + y + pad) * Wp + xx + pad) * 8) = pack8(v);
        }
        __builtin_amdgcn_wave_barrier();
    }
}
hipError_t vpd_launch_pack_input(const float* x, int N, int C, int H, int W, bf16_t* out, int Hp, int Wp, int pad,
                                 int Cp, hipStream_t s) {
    if (Cp != 8 || C > 8) return hipErrorInvalidValue;
    const bool quad = (W & 3) == 0 && (reinterpret_cast<size_t>(x) & 15) == 0;
    long items = quad ? (long)N * H * (W / 4) : (long)N * H * W;
    long g = (items + 255) / 256;
    if (g > 8192) g = 8192;
    if (!quad) {
        hipLaunchKernelGGL(pack_input_px_kernel, dim3(g < 1 ? 1 : (int)g), dim3(256), 0, s, x, N, C, H, W, out, Hp, Wp, pad, Cp);
        return hipGetLastError();
    }
    if ((W & 63) == 0 && ((long)H * W) % 256 == 0 && (C == 5 || C == 3 || C == 6)) {
        long gb = ((long)N * H * W / 256 + 3) / 4;
        if (gb > 4096) gb = 4096;
        const dim3 gr((unsigned)(gb < 1 ? 1 : gb));
        if (C == 5) hipLaunchKernelGGL(pack_input_rows_kernel<5>, gr, dim3(256), 0, s, x, N, H, W, out, Hp, Wp, pad);
        else if (C == 3) hipLaunchKernelGGL(pack_input_rows_kernel<3>, gr, dim3(256), 0, s, x, N, H, W, out, Hp, Wp, pad);
        else hipLaunchKernelGGL(pack_input_rows_kernel<6>, gr, dim3(256), 0, s, x, N, H, W, out, Hp, Wp, pad);
        return hipGetLastError();
    }
    const dim3 grid(g < 1 ? 1 : (int)g);
    if (C == 5) hipLaunchKernelGGL(pack_input_kernel<5>, grid, dim3(256), 0, s, x, N, C, H, W, out, Hp, Wp, pad, Cp);
    else if (C == 3) hipLaunchKernelGGL(pack_input_kernel<3>, grid, dim3(256), 0, s, x, N, C, H, W, out, Hp, Wp, pad, Cp);
    else if (C == 6) hipLaunchKernelGGL(pack_input_kernel<6>, grid, dim3(256), 0, s, x, N, C, H, W, out, Hp, Wp, pad, Cp);
    else hipLaunchKernelGGL(pack_input_kernel<0>, grid, dim3(256), 0, s, x, N, C, H, W, out, Hp, Wp, pad, Cp);
    return hipGetLastError();
}

#define PACK_CHUNK 1024

// master fp32 OIHW -> bf16 forward layout [tap][Co][Ci] and dgrad layout [tap][Ci][Co].
// One block transposes a 32(co) x 32(ci) x taps tile through LDS: the OIHW reads are 32 contiguous runs of
// 32*taps floats, the forward layout is written in 64-byte runs along ci and the dgrad layout in 64-byte runs
// along co (a plain element-wise gather re-fetched every source line ~5x: FETCH_SIZE 410 MB for 85 MB of weights).
// The stem (7x7, Ci <= 8, row-tap packing with zero fill) keeps the element-wise form.
__global__ __launch_bounds__(256) void pack_weights_kernel(const PackDesc* descs, const int* blockmap,
                                                           const float* master, bf16_t* arena) {
    __shared__ float tile[32][32 * 9 + 1];
    const PackDesc d = descs[blockmap[2 * blockIdx.x]];
    const int chunk = blockmap[2 * blockIdx.x + 1];
    const float* src = master + d.src_off;
    const int khw = d.kh * d.kw;
    if (d.stem) {
        const long e0 = (long)chunk * PACK_CHUNK;
        const long nf = (long)d.ntaps * d.Co * d.Kc;
        for (long e = e0 + threadIdx.x; e < e0 + PACK_CHUNK && e < nf; e += 256) {
            const int kc = (int)(e % d.Kc);
            const long q = e / d.Kc;
            const int co = (int)(q % d.Co);
            const int tap = (int)(q / d.Co);      // tap = kernel row r; kc = t*8 + c
            const int t = kc >> 3, c = kc & 7;
            float v = 0.f;
            if (t < d.kw && c < d.Ci) v = src[((size_t)(co * d.Ci + c) * d.kh + tap) * d.kw + t];
            arena[d.fwd_off + e] = (bf16_t)v;
        }
        return;
    }
    const int tci = d.Ci >> 5;
    const int co0 = (chunk / tci) * 32, ci0 = (chunk % tci) * 32;
    const int run = 32 * khw;                      // contiguous floats per co row of the tile
    if ((reinterpret_cast<size_t>(src) & 15) == 0) {   // 16-byte loads (run and the row starts are multiples of 4 floats)
        const int run4 = run >> 2;
        for (int i = threadIdx.x; i < 32 * run4; i += 256) {
            const int r = i / run4, k = (i - r * run4) << 2;
            const float4 f = *reinterpret_cast<const float4*>(src + ((size_t)(co0 + r) * d.Ci + ci0) * khw + k);
            tile[r][k] = f.x; tile[r][k + 1] = f.y; tile[r][k + 2] = f.z; tile[r][k + 3] = f.w;
        }
    } else {
        for (int i = threadIdx.x; i < 32 * run; i += 256) {
            const int r = i / run, k = i - r * run;
            tile[r][k] = src[((size_t)(co0 + r) * d.Ci + ci0) * khw + k];
        }
    }
    __syncthreads();
    // forward: dst[(tap*Co + co)*Ci + ci]: a lane converts 8 consecutive ci -> one 16-byte store, 4 lanes per 64-byte run
    for (int i = threadIdx.x; i < 128 * khw; i += 256) {
        const int q = i & 3, co = (i >> 2) & 31, tap = i >> 7;
        float f[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) f[j] = tile[co][(q * 8 + j) * khw + tap];
        *reinterpret_cast<uint4*>(arena + d.fwd_off + ((size_t)tap * d.Co + co0 + co) * d.Ci + ci0 + q * 8) = pack8(f);
    }
    // dgrad: dst[(tap*Ci + ci)*Co + co]: 8 consecutive co per lane
    if (d.dgr_off >= 0)
        for (int i = threadIdx.x; i < 128 * khw; i += 256) {
            const int q = i & 3, ci = (i >> 2) & 31, tap = i >> 7;
            float f[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) f[j] = tile[q * 8 + j][ci * khw + tap];
            *reinterpret_cast<uint4*>(arena + d.dgr_off + ((size_t)tap * d.Ci + ci0 + ci) * d.Co + co0 + q * 8) = pack8(f);
        }
}
hipError_t vpd_launch_pack_weights(const PackDesc* d_descs, int ndesc, const int* d_blockmap, int nblocks,
                                   const float* master, bf16_t* arena, hipStream_t s) {
    (void)ndesc;
    hipLaunchKernelGGL(pack_weights_kernel, dim3(nblocks), dim3(256), 0, s, d_descs, d_blockmap, master, arena);
    return hipGetLastError();
}

// Gradient of every conv of a bucket -> flat gradient buffer in the reference's OIHW order, one launch.
// Every conv's weight gradient sits in the wgrad scratch as [tap][Co][Kc] fp32: gather into OIHW (element-wise: the
// strided 4-byte reads are absorbed by L2; an LDS-tiled transpose like pack_weights_kernel measured 48 % slower, one
// thread per (co, ci) pair -- coalesced reads, 36-byte-strided stores -- 40 % slower).
__global__ __launch_bounds__(256) void unpack_grads_kernel(const PackDesc* descs, const int* blockmap, const float* wg,
                                                           float* grads) {
    const PackDesc d = descs[blockmap[2 * blockIdx.x]];
    const long e0 = (long)blockmap[2 * blockIdx.x + 1] * PACK_CHUNK;
    const int khw = d.kh * d.kw;
    const long ns = (long)d.Co * d.Ci * khw;
    const float* src = wg + d.wg_off;
    for (long e = e0 + threadIdx.x; e < e0 + PACK_CHUNK && e < ns; e += 256) {
        const int tap = (int)(e % khw);
        const long q = e / khw;
        const int ci = (int)(q % d.Ci);
        const int co = (int)(q / d.Ci);
        float v;
        if (d.stem) {
            const int r = tap / d.kw, t = tap - r * d.kw;
            v = src[((size_t)r * d.Co + co) * d.Kc + t * 8 + ci];
        } else {
            v = src[((size_t)tap * d.Co + co) * d.Kc + ci];
        }
        grads[d.src_off + e] = v;
    }
}
hipError_t vpd_launch_unpack_grads(const PackDesc* d_descs, int ndesc, const int* d_blockmap, int nblocks,
                                   const float* wg, float* grads, hipStream_t s) {
    (void)ndesc;
    hipLaunchKernelGGL(unpack_grads_kernel, dim3(nblocks), dim3(256), 0, s, d_descs, d_blockmap, wg, grads);
    return hipGetLastError();
}

// Fused AdamW over the whole flat parameter buffer.  Ungrouped (AdamHyper / AdamHyperDyn): every tensor shares the
// hyper-parameters, as train_vpd_model.py:104's one param group with wd on all.  Grouped (AdamGroupHyper / AdamGroupHyperDyn,
// kernels.h): lr and weight decay per parameter group, found through the segment table; the arithmetic is this one function.
// (explicit fma placement: the flat kernel and the fused AdamW + repack kernel must round identically)
static __device__ __forceinline__ void adamw1(float& p, float g, float& m, float& v, const AdamHyper& h) {
#pragma clang fp contract(off)
    g *= h.gscale;      // 1 / loss scale: exact for the powers of two a LossScaler uses, and for 1
    p *= h.decay;
    m = fmaf(g - m, h.omb1, m);
    v = fmaf(h.omb2 * g, g, v * h.b2);
    const float den = fmaf(sqrtf(v), h.inv_sqrt_bc2, h.eps);
    p = fmaf(-h.step_size, m / den, p);
}
static __device__ __forceinline__ void adamw4(float4& pp, const float4& gg, float4& mm, float4& vv, const AdamHyper& h) {
    adamw1(pp.x, gg.x, mm.x, vv.x, h); adamw1(pp.y, gg.y, mm.y, vv.y, h);
    adamw1(pp.z, gg.z, mm.z, vv.z, h); adamw1(pp.w, gg.w, mm.w, vv.w, h);
}
static AdamHyper adam_hyper(const AdamArgs& a, int step, float gscale) {
    const double bc1 = 1.0 - pow(a.b1, step);
    const double bc2 = 1.0 - pow(a.b2, step);
    return AdamHyper{(float)(1.0 - a.lr * a.wd), (float)(1.0 - a.b1), (float)a.b2, (float)(1.0 - a.b2), (float)(a.lr / bc1),
                     (float)(1.0 / sqrt(bc2)), (float)a.eps, gscale};
}
// (step 1 / gscale 1 are place-holders: adam_live replaces step_size, inv_sqrt_bc2 and gscale from the device block)
static AdamHyperDyn adam_hyper_dyn(const AdamArgs& a) { return AdamHyperDyn{adam_hyper(a, 1, 1.f), a.st, a.lr, a.b1, a.b2}; }

// H: AdamHyper as the host computed it (every launch without a dynamic loss scaler), or AdamHyperDyn -- the same plus the
// scaler's device block (vpd_scale_state, include/vpd_hip.h): gradient factor 1 / scale, bias corrections from the number of
// steps APPLIED so far, which only the device knows after a skipped step (in double, rounded to float: adam_hyper), and when the
// non-finite word is set the launch writes nothing at all -- scaler.step(optimizer) of models/util.py:56.
static __device__ __forceinline__ const AdamHyper& adam_live(const AdamHyper& h, bool& live) {
    live = true;
    return h;
}
static __device__ __forceinline__ AdamHyper adam_live(const AdamHyperDyn& d, bool& live) {
    AdamHyper h = d.h;
    live = d.st->found == 0;
    if (live) {
        const double step = (double)(d.st->applied_steps + 1);
        h.step_size = (float)(d.lr / (1.0 - pow(d.b1, step)));
        h.inv_sqrt_bc2 = (float)(1.0 / sqrt(1.0 - pow(d.b2, step)));
        h.gscale = 1.0f / d.st->scale;
    }
    return h;
}

// ---- parameter groups: the grouped instantiations of both kernels (the ungrouped ones take none of this: if constexpr) ----
template <class H> struct AdamGrouped { static constexpr bool on = false; };
template <> struct AdamGrouped<AdamGroupHyper> { static constexpr bool on = true; };
template <> struct AdamGrouped<AdamGroupHyperDyn> { static constexpr bool on = true; };
// What is shared (betas, eps, inv_sqrt_bc2, gscale), as the ungrouped launch forms it; bc1: the first moment's bias correction under
// a device block, from which adam_pick forms a group's step_size exactly as adam_live(AdamHyperDyn) forms the single one
static __device__ __forceinline__ AdamHyper adam_live(const AdamGroupHyper& g, bool& live, double& bc1) {
    live = true;
    bc1 = 1.0;
    return g.h;
}
static __device__ __forceinline__ AdamHyper adam_live(const AdamGroupHyperDyn& d, bool& live, double& bc1) {
    AdamHyper h = d.g.h;
    live = d.st->found == 0;
    bc1 = 1.0;
    if (live) {
        const double step = (double)(d.st->applied_steps + 1);
        bc1 = 1.0 - pow(d.b1, step);
        h.inv_sqrt_bc2 = (float)(1.0 / sqrt(1.0 - pow(d.b2, step)));
        h.gscale = 1.0f / d.st->scale;
    }
    return h;
}
// `h` with group gid's decay and step_size (gid < VPD_MAX_PARAM_GROUPS: vpd_adam_groups_init refuses any other table)
static __device__ __forceinline__ void adam_pick(const AdamGroupHyper& g, double, int gid, AdamHyper& h) {
    gid &= VPD_MAX_PARAM_GROUPS - 1;      // (never leaves the argument, whatever the table holds)
    h.decay = g.decay[gid];
    h.step_size = g.step_size[gid];
}
static __device__ __forceinline__ void adam_pick(const AdamGroupHyperDyn& d, double bc1, int gid, AdamHyper& h) {
    gid &= VPD_MAX_PARAM_GROUPS - 1;
    h.decay = d.g.decay[gid];
    h.step_size = (float)(d.lr[gid] / bc1);
}
static __device__ __forceinline__ const void* adam_table(const AdamGroupHyper& g) { return g.table; }
static __device__ __forceinline__ const void* adam_table(const AdamGroupHyperDyn& d) { return d.g.table; }
// The segment table (layout: kernels.h) and the segment of element e by binary search: the last s with begin[s] <= e, so an e
// behind the table's end falls into the last segment.  Plain loads of device memory a host-to-device copy wrote.
struct SegTable { const long long* begin; const int* group; int nseg; };
static __device__ __forceinline__ SegTable seg_table(const void* table) {
    const int* hd = reinterpret_cast<const int*>(table);
    const int nseg = hd[0];
    const long long* begin = reinterpret_cast<const long long*>(hd + 4);
    return SegTable{begin, reinterpret_cast<const int*>(begin + nseg + 1), nseg};
}
static __device__ __forceinline__ int seg_find(const SegTable& t, long e) {
    int lo = 0, hi = t.nseg - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (t.begin[mid] <= e) lo = mid; else hi = mid - 1;
    }
    return lo;
}
// ... forward from segment s (e not in front of it)
static __device__ __forceinline__ int seg_walk(const SegTable& t, int s, long e) {
    while (s + 1 < t.nseg && t.begin[s + 1] <= e) ++s;
    return s;
}

template <class H>
__global__ __launch_bounds__(256) void adamw_kernel(float4* p, const float4* g, float4* m, float4* v, long n4,
                                                    const H hh) {
    if constexpr (AdamGrouped<H>::on) {
        // a float4 inside one segment takes the vector path with that segment's group; one that straddles a boundary (segments may
        // begin at any element) is done element by element
        bool live;
        double bc1;
        AdamHyper h = adam_live(hh, live, bc1);
        if (!live) return;
        const SegTable t = seg_table(adam_table(hh));
        for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (long)gridDim.x * blockDim.x) {
            float4 pp = p[i], gg = g[i], mm = m[i], vv = v[i];
            const long e = i << 2;
            int s = seg_find(t, e);
            adam_pick(hh, bc1, t.group[s], h);
            if (s + 1 >= t.nseg || t.begin[s + 1] >= e + 4) {
                adamw4(pp, gg, mm, vv, h);
            } else {
                adamw1(pp.x, gg.x, mm.x, vv.x, h);
                s = seg_walk(t, s, e + 1); adam_pick(hh, bc1, t.group[s], h);
                adamw1(pp.y, gg.y, mm.y, vv.y, h);
                s = seg_walk(t, s, e + 2); adam_pick(hh, bc1, t.group[s], h);
                adamw1(pp.z, gg.z, mm.z, vv.z, h);
                s = seg_walk(t, s, e + 3); adam_pick(hh, bc1, t.group[s], h);
                adamw1(pp.w, gg.w, mm.w, vv.w, h);
            }
            p[i] = pp; m[i] = mm; v[i] = vv;
        }
    } else {
        bool live;
        const AdamHyper h = adam_live(hh, live);
        if (!live) return;
        for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (long)gridDim.x * blockDim.x) {
            float4 pp = p[i], gg = g[i], mm = m[i], vv = v[i];
            adamw4(pp, gg, mm, vv, h);
            p[i] = pp; m[i] = mm; v[i] = vv;
        }
    }
}
hipError_t vpd_launch_adamw(float* p, const float* g, float* m, float* v, long n, const AdamArgs& a, hipStream_t s) {
    if (n % 4) return hipErrorInvalidValue;
    const long n4 = n / 4;
    long gsz = (n4 + 255) / 256;
    if (gsz > 4096) gsz = 4096;
    const dim3 grid(gsz < 1 ? 1 : (int)gsz);
    if (!a.st)
        hipLaunchKernelGGL(adamw_kernel<AdamHyper>, grid, dim3(256), 0, s, (float4*)p, (const float4*)g, (float4*)m, (float4*)v,
                           n4, adam_hyper(a, a.step, a.gscale));
    else
        hipLaunchKernelGGL(adamw_kernel<AdamHyperDyn>, grid, dim3(256), 0, s, (float4*)p, (const float4*)g, (float4*)m, (float4*)v,
                           n4, adam_hyper_dyn(a));
    return hipGetLastError();
}
// Per group exactly what adam_hyper computes for the one (lr, wd): the same doubles, rounded to float once
static AdamGroupHyper adam_group_hyper(const AdamGroupArgs& a, int step, float gscale) {
    AdamGroupHyper gh;
    gh.h = adam_hyper(AdamArgs{a.lr[0], a.b1, a.b2, a.eps, a.wd[0], step, gscale, a.st}, step, gscale);
    gh.table = a.table;
    const double bc1 = 1.0 - pow(a.b1, step);
    for (int i = 0; i < VPD_MAX_PARAM_GROUPS; ++i) {
        gh.decay[i] = i < a.ngroups ? (float)(1.0 - a.lr[i] * a.wd[i]) : 1.f;
        gh.step_size[i] = i < a.ngroups ? (float)(a.lr[i] / bc1) : 0.f;
    }
    return gh;
}
static AdamGroupHyperDyn adam_group_hyper_dyn(const AdamGroupArgs& a) {
    AdamGroupHyperDyn d;
    d.g = adam_group_hyper(a, 1, 1.f);      // (place-holders, as adam_hyper_dyn's)
    d.st = a.st; d.b1 = a.b1; d.b2 = a.b2;
    for (int i = 0; i < VPD_MAX_PARAM_GROUPS; ++i) d.lr[i] = i < a.ngroups ? a.lr[i] : 0.0;
    return d;
}
static bool adam_groups_ok(const AdamGroupArgs& a) {
    return a.table && a.lr && a.wd && a.ngroups >= 1 && a.ngroups <= VPD_MAX_PARAM_GROUPS && (reinterpret_cast<size_t>(a.table) & 15) == 0;
}
hipError_t vpd_launch_adamw_groups(float* p, const float* g, float* m, float* v, long n, const AdamGroupArgs& a, hipStream_t s) {
    if (n % 4 || !adam_groups_ok(a)) return hipErrorInvalidValue;
    const long n4 = n / 4;
    long gsz = (n4 + 255) / 256;
    if (gsz > 4096) gsz = 4096;
    const dim3 grid(gsz < 1 ? 1 : (int)gsz);
    if (!a.st)
        hipLaunchKernelGGL(adamw_kernel<AdamGroupHyper>, grid, dim3(256), 0, s, (float4*)p, (const float4*)g, (float4*)m,
                           (float4*)v, n4, adam_group_hyper(a, a.step, a.gscale));
    else
        hipLaunchKernelGGL(adamw_kernel<AdamGroupHyperDyn>, grid, dim3(256), 0, s, (float4*)p, (const float4*)g, (float4*)m,
                           (float4*)v, n4, adam_group_hyper_dyn(a));
    return hipGetLastError();
}

// AdamW and the repack of the bf16 weight layouts in ONE pass over the parameters (the train step's optimizer):
// a block updates a 32(co) x 32(ci) x taps tile of a conv weight in place (p, m, v: 16-byte accesses of the OIHW
// runs), keeps the new values in LDS and writes both bf16 layouts from there -- pack_weights_kernel's tile without
// re-reading the 85 MB of master weights.  Ranges that are not conv weights (BatchNorm, fc, motion head) are
// `stem == 2` descriptors updated element-wise; so is the stem conv, whose row-tap packing gathers across the whole
// tensor and is done by a 28-block pack_weights_kernel launch afterwards.
#define ADAM_PLAIN_CHUNK 2048
// wg != null: the conv weight gradients are read where the weight-gradient kernels left them -- the fp32 scratch in
// [tap][Co][Ci] order (PackDesc::wg_off) -- instead of from the OIHW gradient buffer: the unpack pass in between (170 MB of
// traffic, 67 us per step) disappears.  The stem and every non-conv tensor still come from `g`.
template <int KHW>
static __device__ __forceinline__ float4 adamw_gather_g(const float* wgc, int Co, int Kc, int co, int ci0, int k) {
    float v[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int kk = k + j;
        const int ci = kk / KHW, tap = kk - ci * KHW;
        v[j] = wgc[((size_t)tap * Co + co) * Kc + ci0 + ci];
    }
    return float4{v[0], v[1], v[2], v[3]};
}
template <class H>      // AdamHyper | AdamHyperDyn | their grouped forms (a skipped step leaves the packed weights alone too: they already hold these parameters)
__global__ __launch_bounds__(256) void adamw_pack_kernel(const PackDesc* descs, const int* blockmap, float* p,
                                                         const float* g, float* m, float* v, bf16_t* arena,
                                                         const H hh, const float* wg) {
    __shared__ unsigned short tile[32][32 * 9 + 2];      // the new weights, already rounded to bf16 (18 KB: 8 blocks per CU)
    constexpr bool grouped = AdamGrouped<H>::on;
    bool live;
    [[maybe_unused]] double bc1 = 1.0;
    [[maybe_unused]] SegTable t{};
    AdamHyper h;
    if constexpr (grouped) h = adam_live(hh, live, bc1); else h = adam_live(hh, live);
    if (!live) return;
    if constexpr (grouped) t = seg_table(adam_table(hh));
    const PackDesc d = descs[blockmap[2 * blockIdx.x]];
    const int chunk = blockmap[2 * blockIdx.x + 1];
    const int khw = d.kh * d.kw;
    if (d.stem == 2) {
        // (grouped: a plain range spans tensors of several groups -- BatchNorm weight and bias are 64 floats each -- so the group is
        //  resolved per element: a search for a thread's first element, a walk forward for its next ones)
        const long e0 = d.src_off + (long)chunk * ADAM_PLAIN_CHUNK;
        const long e1 = d.src_off + d.numel;
        [[maybe_unused]] int seg = -1, gid = -1;
        for (long e = e0 + threadIdx.x; e < e0 + ADAM_PLAIN_CHUNK && e < e1; e += 256) {
            if constexpr (grouped) {
                seg = seg < 0 ? seg_find(t, e) : seg_walk(t, seg, e);
                if (t.group[seg] != gid) { gid = t.group[seg]; adam_pick(hh, bc1, gid, h); }
            }
            float pp = p[e], mm = m[e], vv = v[e];
            adamw1(pp, g[e], mm, vv, h);
            p[e] = pp; m[e] = mm; v[e] = vv;
        }
        return;
    }
    // (grouped: a conv weight lies inside one segment -- vpd_adam_groups_init refuses any other table --: one lookup per block)
    if constexpr (grouped) adam_pick(hh, bc1, t.group[seg_find(t, d.src_off)], h);
    const int tci = d.Ci >> 5;
    const int co0 = (chunk / tci) * 32, ci0 = (chunk % tci) * 32;
    const int run4 = (32 * khw) >> 2;
    const float* wgc = wg ? wg + d.wg_off : nullptr;
    for (int i = threadIdx.x; i < 32 * run4; i += 256) {
        const int r = i / run4, k = (i - r * run4) << 2;
        const size_t e = d.src_off + ((size_t)(co0 + r) * d.Ci + ci0) * khw + k;
        float4 pp = *reinterpret_cast<const float4*>(p + e);
        float4 mm = *reinterpret_cast<const float4*>(m + e);
        float4 vv = *reinterpret_cast<const float4*>(v + e);
        float4 gg;
        if (!wgc) gg = *reinterpret_cast<const float4*>(g + e);
        else if (khw == 9) gg = adamw_gather_g<9>(wgc, d.Co, d.Kc, co0 + r, ci0, k);
        else if (khw == 1) gg = *reinterpret_cast<const float4*>(wgc + (size_t)(co0 + r) * d.Kc + ci0 + k);
        else {
            float t4[4];
            for (int j = 0; j < 4; ++j) {
                const int ci = (k + j) / khw, tap = (k + j) - ci * khw;
                t4[j] = wgc[((size_t)tap * d.Co + co0 + r) * d.Kc + ci0 + ci];
            }
            gg = float4{t4[0], t4[1], t4[2], t4[3]};
        }
        adamw4(pp, gg, mm, vv, h);
        *reinterpret_cast<float4*>(p + e) = pp;
        *reinterpret_cast<float4*>(m + e) = mm;
        *reinterpret_cast<float4*>(v + e) = vv;
        tile[r][k] = __builtin_bit_cast(unsigned short, (bf16_t)pp.x);
        tile[r][k + 1] = __builtin_bit_cast(unsigned short, (bf16_t)pp.y);
        tile[r][k + 2] = __builtin_bit_cast(unsigned short, (bf16_t)pp.z);
        tile[r][k + 3] = __builtin_bit_cast(unsigned short, (bf16_t)pp.w);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < 128 * khw; i += 256) {
        const int q = i & 3, co = (i >> 2) & 31, tap = i >> 7;
        unsigned int w[4];
#pragma unroll
        for (int j = 0; j < 4; ++j)
            w[j] = (unsigned int)tile[co][(q * 8 + 2 * j) * khw + tap] | ((unsigned int)tile[co][(q * 8 + 2 * j + 1) * khw + tap] << 16);
        *reinterpret_cast<uint4*>(arena + d.fwd_off + ((size_t)tap * d.Co + co0 + co) * d.Ci + ci0 + q * 8) = uint4{w[0], w[1], w[2], w[3]};
    }
    if (d.dgr_off >= 0)
        for (int i = threadIdx.x; i < 128 * khw; i += 256) {
            const int q = i & 3, ci = (i >> 2) & 31, tap = i >> 7;
            unsigned int w[4];
#pragma unroll
            for (int j = 0; j < 4; ++j)
                w[j] = (unsigned int)tile[q * 8 + 2 * j][ci * khw + tap] | ((unsigned int)tile[q * 8 + 2 * j + 1][ci * khw + tap] << 16);
            *reinterpret_cast<uint4*>(arena + d.dgr_off + ((size_t)tap * d.Ci + ci0 + ci) * d.Co + co0 + q * 8) = uint4{w[0], w[1], w[2], w[3]};
        }
}
hipError_t vpd_launch_adamw_pack(const PackDesc* d_descs, const int* d_blockmap, int nblocks, float* p, const float* g,
                                 float* m, float* v, bf16_t* arena, const AdamArgs& a, hipStream_t s, const float* wg) {
    if ((reinterpret_cast<size_t>(p) | reinterpret_cast<size_t>(g) | reinterpret_cast<size_t>(m) |
         reinterpret_cast<size_t>(v)) & 15)
        return hipErrorInvalidValue;
    if (!a.st)
        hipLaunchKernelGGL(adamw_pack_kernel<AdamHyper>, dim3(nblocks), dim3(256), 0, s, d_descs, d_blockmap, p, g, m, v, arena,
                           adam_hyper(a, a.step, a.gscale), wg);
    else
        hipLaunchKernelGGL(adamw_pack_kernel<AdamHyperDyn>, dim3(nblocks), dim3(256), 0, s, d_descs, d_blockmap, p, g, m, v,
                           arena, adam_hyper_dyn(a), wg);
    return hipGetLastError();
}
hipError_t vpd_launch_adamw_pack_groups(const PackDesc* d_descs, const int* d_blockmap, int nblocks, float* p, const float* g,
                                        float* m, float* v, bf16_t* arena, const AdamGroupArgs& a, hipStream_t s, const float* wg) {
    if ((reinterpret_cast<size_t>(p) | reinterpret_cast<size_t>(g) | reinterpret_cast<size_t>(m) |
         reinterpret_cast<size_t>(v)) & 15)
        return hipErrorInvalidValue;
    if (!adam_groups_ok(a)) return hipErrorInvalidValue;
    if (!a.st)
        hipLaunchKernelGGL(adamw_pack_kernel<AdamGroupHyper>, dim3(nblocks), dim3(256), 0, s, d_descs, d_blockmap, p, g, m, v,
                           arena, adam_group_hyper(a, a.step, a.gscale), wg);
    else
        hipLaunchKernelGGL(adamw_pack_kernel<AdamGroupHyperDyn>, dim3(nblocks), dim3(256), 0, s, d_descs, d_blockmap, p, g, m, v,
                           arena, adam_group_hyper_dyn(a), wg);
    return hipGetLastError();
}

// ---- dynamic loss scaling (vpd_scale_state): the inf / NaN search over the gradients and the scale's update rule ----
// A float is inf or NaN exactly when its eight exponent bits are all ones.
static __device__ __forceinline__ unsigned nonfinite1(float f) {
    return (__float_as_uint(f) & 0x7f800000u) == 0x7f800000u ? 1u : 0u;
}
static __device__ __forceinline__ unsigned nonfinite4(const float4& f) {
    return nonfinite1(f.x) | nonfinite1(f.y) | nonfinite1(f.z) | nonfinite1(f.w);
}
// What the four range walkers (check_finite_kernel, ema_update_kernel, grad_accum_kernel, grad_sqsum_kernel) share.  A float range of any alignment
// and length, split by the 16-byte phase of `x`: `head` floats (at most three) in front, the aligned middle of `n4` float4 at
// x + head, and the floats from `tail` on (at most three)
struct RangeSplit { long head, n4, tail; };
static __device__ __forceinline__ RangeSplit split_range(const float* x, long n) {
    long head = (long)((16 - (reinterpret_cast<size_t>(x) & 15)) & 15) >> 2;
    if (head > n) head = n;
    const long n4 = (n - head) >> 2;
    return RangeSplit{head, n4, head + (n4 << 2)};
}
// ... and a wave's four consecutive 1 KB rows of one operand: one address, the rows behind it by the instruction's offset field
struct Rows4 { f32x4 a, b, c, d; };
static __device__ __forceinline__ Rows4 load_rows4(const f32x4* p) { return Rows4{p[0], p[64], p[128], p[192]}; }
// Every range of `r` (float ranges of any alignment) in one launch: a range's 16-byte aligned middle is read with 16-byte loads,
// four in flight per thread, the up to three floats in front of it and behind it one by one.  A wave votes; a block issues ONE
// atomic OR, and only when one of its waves found something -- a clean step (all of them but a handful) writes nothing.
__global__ __launch_bounds__(256) void check_finite_kernel(const FiniteRanges r, unsigned* found) {
    __shared__ unsigned blk;
    if (threadIdx.x == 0) blk = 0u;
    __syncthreads();
    const long tid = (long)blockIdx.x * 256 + threadIdx.x, nth = (long)gridDim.x * 256;
    unsigned bad = 0u;
    for (int k = 0; k < r.count; ++k) {
        const float* x = r.ptr[k];
        const long n = r.n[k];
        const RangeSplit sp = split_range(x, n);
        const long head = sp.head, n4 = sp.n4, tail = sp.tail;
        const float4* x4 = reinterpret_cast<const float4*>(x + head);
        long i = tid;
        for (; i + 3 * nth < n4; i += 4 * nth) {
            const float4 a = x4[i], b = x4[i + nth], c = x4[i + 2 * nth], d = x4[i + 3 * nth];
            bad |= nonfinite4(a) | nonfinite4(b) | nonfinite4(c) | nonfinite4(d);
        }
        for (; i < n4; i += nth) bad |= nonfinite4(x4[i]);
        if (tid < head) bad |= nonfinite1(x[tid]);
        if (tid < n - tail) bad |= nonfinite1(x[tail + tid]);
    }
    if (__any(bad != 0u) && (threadIdx.x & 63) == 0) blk = 1u;      // (every writer stores the same value)
    __syncthreads();
    if (threadIdx.x == 0 && blk) atomicOr(found, 1u);
}
hipError_t vpd_launch_check_finite(const FiniteRanges& r, vpd_scale_state* st, hipStream_t s) {
    const int grid = vpd_grad_sqsum_grid(r.n, r.count, 2048);      // at most 2048 blocks = 8 per CU: enough loads in flight for the fabric
    if (grid == 0) return hipSuccess;
    hipLaunchKernelGGL(check_finite_kernel, dim3(grid), dim3(256), 0, s, r, &st->found);
    return hipGetLastError();
}

// scaler.update() (models/util.py:57) on one thread, torch's rule (_amp_update_scale_: a growth that would leave fp32's range is
// not taken, nothing else is clamped)
__global__ void scale_update_kernel(vpd_scale_state* st, float growth, float backoff, int interval) {
    if (st->found) {
        st->scale *= backoff;
        st->growth_tracker = 0;
        st->skipped_steps += 1;
    } else {
        st->applied_steps += 1;
        const int t = st->growth_tracker + 1;
        if (t == interval) {
            const float grown = st->scale * growth;
            if (grown <= 3.4028235e38f) st->scale = grown;
            st->growth_tracker = 0;
        } else {
            st->growth_tracker = t;
        }
    }
    st->found = 0u;
}
hipError_t vpd_launch_scale_update(vpd_scale_state* st, float growth, float backoff, int interval, hipStream_t s) {
    hipLaunchKernelGGL(scale_update_kernel, dim3(1), dim3(1), 0, s, st, growth, backoff, interval);
    return hipGetLastError();
}

// ---- exponential moving average of the weights (vpd_ema_update): dst += (1 - d) * (src - dst) over up to EMA_MAX ranges, one launch ----
// Streaming: 4 bytes read twice and written once per element, nothing reused.  A range is split like check_finite_kernel's by the
// alignment of `dst`: up to three floats in front, the 16-byte aligned middle -- 16 KB tiles with four 16-byte loads of each operand
// in flight per thread, then what is left of it one float4 per thread -- and up to three floats behind.  When `src` does not share dst's 16-byte phase its middle is read float by float.
// st != null (a DynamicLossScaler's step in flight): nothing is written when the non-finite word is set -- the AdamW before this
// launch wrote nothing either -- and t, the number of updates so far, is the applied-step count minus its value at enable time.
static __device__ __forceinline__ float ema1(float s, float d, float omd) {
#pragma clang fp contract(off)
    return fmaf(omd, s - d, d);
}
static __device__ __forceinline__ f32x4 ema4(const f32x4& s, const f32x4& d, float omd) {
    return f32x4{ema1(s.x, d.x, omd), ema1(s.y, d.y, omd), ema1(s.z, d.z, omd), ema1(s.w, d.w, omd)};
}
// (at most 64 registers: the capped grid of 2048 blocks = 8 waves per SIMD is resident at once)
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(8, 8))) void ema_update_kernel(const EmaRanges r, double decay, int warmup, int t, int t0,
                                                         const vpd_scale_state* st) {
    if (st) {
        if (st->found != 0u) return;
        t = st->applied_steps - t0;
        if (t < 0) t = 0;
    }
    double d = decay;
    if (warmup) {      // timm's rule: min(decay, (1 + t) / (10 + t))
        const double w = (1.0 + (double)t) / (10.0 + (double)t);
        d = w < d ? w : d;
    }
    const float omd = (float)(1.0 - d);
    const long tid = (long)blockIdx.x * 256 + threadIdx.x, nth = (long)gridDim.x * 256;
    for (int k = 0; k < r.count; ++k) {
        const float* x = r.src[k];
        float* y = r.dst[k];
        const long n = r.n[k];
        const RangeSplit sp = split_range(y, n);
        const long head = sp.head, n4 = sp.n4, tail = sp.tail;
        f32x4* y4 = reinterpret_cast<f32x4*>(y + head);
        long i = tid;
        if ((reinterpret_cast<size_t>(x + head) & 15) == 0) {
            const f32x4* x4 = reinterpret_cast<const f32x4*>(x + head);
            // tiles of 1024 float4 (16 KB) per block: a wave takes four consecutive 1 KB rows of each operand -- one address per
            // operand, the rows behind it by the instruction's offset field
            const long ntile = n4 >> 10;
            for (long tl = blockIdx.x; tl < ntile; tl += gridDim.x) {
                const long e = (tl << 10) + (threadIdx.x >> 6) * 256 + (threadIdx.x & 63);
                const f32x4* xp = x4 + e;
                f32x4* yp = y4 + e;
                Rows4 rs = load_rows4(xp), rd = load_rows4(yp);
                // every loaded value passes through one opaque point: all eight loads are issued before the first is consumed
                // (left alone, hipcc sinks each pair of loads to its use and waits for it there: two in flight per thread)
                asm volatile("" : "+v"(rs.a), "+v"(rs.b), "+v"(rs.c), "+v"(rs.d), "+v"(rd.a), "+v"(rd.b), "+v"(rd.c), "+v"(rd.d));
                yp[0] = ema4(rs.a, rd.a, omd);
                yp[64] = ema4(rs.b, rd.b, omd);
                yp[128] = ema4(rs.c, rd.c, omd);
                yp[192] = ema4(rs.d, rd.d, omd);
            }
            for (i += ntile << 10; i < n4; i += nth) y4[i] = ema4(x4[i], y4[i], omd);
        } else {
            const float* xs = x + head;
            for (; i < n4; i += nth) {
                const f32x4 s = {xs[4 * i], xs[4 * i + 1], xs[4 * i + 2], xs[4 * i + 3]};
                y4[i] = ema4(s, y4[i], omd);
            }
        }
        if (tid < head) y[tid] = ema1(x[tid], y[tid], omd);
        if (tid < n - tail) y[tail + tid] = ema1(x[tail + tid], y[tail + tid], omd);
    }
}
hipError_t vpd_launch_ema_update(const EmaRanges& r, double decay, int warmup, int t, int t0, const vpd_scale_state* st,
                                 hipStream_t s) {
    const int grid = vpd_grad_sqsum_grid(r.n, r.count, 2048);      // capped like check_finite_kernel's grid: 2048 blocks = 8 per CU
    if (grid == 0) return hipSuccess;
    hipLaunchKernelGGL(ema_update_kernel, dim3(grid), dim3(256), 0, s, r, decay, warmup, t, t0, st);
    return hipGetLastError();
}

// ---- gradient-norm clipping (vpd_clip_state): sum of squares over float ranges, then norm, coefficient and the effective scale ----
// torch.nn.utils.clip_grad_norm_ decided on the device.  grad_sqsum_kernel streams the ranges of check_finite_kernel (same split:
// up to three floats in front, the 16-byte aligned middle, up to three behind) with ema_update_kernel's loads: 32 KB tiles, a wave
// takes four consecutive 1 KB rows in each half of the tile -- one address per half, the rows behind it by the offset field, eight
// 16-byte loads in flight per thread, kept from sinking to their use.  Every element is widened to double and squared there, into
// four accumulators per thread (one per float4 lane): no square overflows, and n * 2^-53 bounds the summation error.  A wave
// reduces by shuffles, the block through LDS, both in a fixed order; thread 0 stores the block's double into its own slot.  No
// atomics: the same input gives the same bits on every launch and on every data-parallel rank.
static __device__ __forceinline__ void sq4(const f32x4& f, double& a0, double& a1, double& a2, double& a3) {
    const double x = (double)f.x, y = (double)f.y, z = (double)f.z, w = (double)f.w;
    a0 = fma(x, x, a0); a1 = fma(y, y, a1); a2 = fma(z, z, a2); a3 = fma(w, w, a3);
}
static __device__ __forceinline__ double wave_sum_f64(double s) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off, 64);
    return s;      // (lane 0 holds the wave's sum)
}
// ... and a block's: the four waves' sums through `wsum`, added as (w0 + w1) + (w2 + w3) (every thread returns the block's sum)
static __device__ __forceinline__ double block_sum_f64(double s, double* wsum) {
    s = wave_sum_f64(s);
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = s;
    __syncthreads();
    return (wsum[0] + wsum[1]) + (wsum[2] + wsum[3]);
}
// (at most 64 registers, as ema_update_kernel: the capped grid of 2048 blocks = 8 waves per SIMD is resident at once)
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(8, 8))) void grad_sqsum_kernel(const FiniteRanges r, double* partials) {
    __shared__ double wsum[4];
    const long tid = (long)blockIdx.x * 256 + threadIdx.x, nth = (long)gridDim.x * 256;
    double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
    for (int k = 0; k < r.count; ++k) {
        const float* x = r.ptr[k];
        const long n = r.n[k];
        const RangeSplit sp = split_range(x, n);
        const long head = sp.head, n4 = sp.n4, tail = sp.tail;
        const f32x4* x4 = reinterpret_cast<const f32x4*>(x + head);
        // tiles of 2048 float4: the last element a tile touches is (tl << 11) + 1024 + 3 * 256 + 63 + 192 = (tl << 11) + 2047 < n4
        const long ntile = n4 >> 11;
        for (long tl = blockIdx.x; tl < ntile; tl += gridDim.x) {
            const f32x4* xa = x4 + (tl << 11) + (threadIdx.x >> 6) * 256 + (threadIdx.x & 63);
            const f32x4* xb = xa + 1024;
            Rows4 f = load_rows4(xa), g = load_rows4(xb);
            // (all eight loads are issued before the first is consumed: ema_update_kernel)
            asm volatile("" : "+v"(f.a), "+v"(f.b), "+v"(f.c), "+v"(f.d), "+v"(g.a), "+v"(g.b), "+v"(g.c), "+v"(g.d));
            sq4(f.a, a0, a1, a2, a3); sq4(f.b, a0, a1, a2, a3); sq4(f.c, a0, a1, a2, a3); sq4(f.d, a0, a1, a2, a3);
            sq4(g.a, a0, a1, a2, a3); sq4(g.b, a0, a1, a2, a3); sq4(g.c, a0, a1, a2, a3); sq4(g.d, a0, a1, a2, a3);
        }
        for (long i = (ntile << 11) + tid; i < n4; i += nth) sq4(x4[i], a0, a1, a2, a3);
        if (tid < head) { const double v = (double)x[tid]; a0 = fma(v, v, a0); }
        if (tid < n - tail) { const double v = (double)x[tail + tid]; a1 = fma(v, v, a1); }
    }
    const double s = block_sum_f64((a0 + a1) + (a2 + a3), wsum);
    if (threadIdx.x == 0) partials[blockIdx.x] = s;
}
// The grid of one launch of a range walker (this one, check_finite_kernel, ema_update_kernel): a function of the ranges' lengths
// alone (the bits of a norm depend on it), at most `cap` blocks; 0 = nothing to do
int vpd_grad_sqsum_grid(const long* n, int count, int cap) {
    long total = 0;
    for (int k = 0; k < count; ++k) total += n[k] > 0 ? n[k] : 0;
    if (count <= 0 || total == 0) return 0;
    long gsz = (total / 4 + 255) / 256;
    if (gsz > cap) gsz = cap;
    return gsz < 1 ? 1 : (int)gsz;
}
hipError_t vpd_launch_grad_sqsum(const FiniteRanges& r, int grid, double* partials, hipStream_t s) {
    if (grid <= 0) return hipSuccess;
    hipLaunchKernelGGL(grad_sqsum_kernel, dim3(grid), dim3(256), 0, s, r, partials);
    return hipGetLastError();
}

// One block: the used slots summed in a fixed order (thread t takes slots t, t + 256, ...; then the wave and block order above),
// everything in double, every stored value rounded to float once.  norm = sqrt(sum) / scale, coef = min(1, max_norm / (norm + 1e-6))
// -- torch's formula and clamp -- and eff.scale = scale / coef, so that the AdamW that reads `eff` multiplies by coef / scale.
// A sum of squares is non-finite exactly when an element is: eff.found then says so, to the source block as well.
__global__ __launch_bounds__(256) void clip_finalize_kernel(vpd_clip_state* clip, int used, double max_norm, vpd_scale_state* src,
                                                            float host_scale) {
    __shared__ double wsum[4];
    const double* partials = reinterpret_cast<const double*>(clip + 1);
    double a = 0.0;
    for (int i = threadIdx.x; i < used; i += 256) a += partials[i];
    const double sum = block_sum_f64(a, wsum);
    if (threadIdx.x != 0) return;
    const bool bad = (__double_as_longlong(sum) & 0x7ff0000000000000LL) == 0x7ff0000000000000LL;      // inf or NaN
    const double scale = src ? (double)src->scale : (double)host_scale;
    const double norm = sqrt(sum) / scale;
    double coef = max_norm / (norm + 1e-6);
    coef = coef < 1.0 ? coef : 1.0;
    if (bad) coef = 1.0;      // (the step is skipped: nothing reads it)
    const float fnorm = (float)norm;
    clip->total_norm = fnorm;
    clip->coef = (float)coef;
    clip->eff.scale = (float)(scale / coef);
    unsigned found = bad ? 1u : 0u;
    if (src) {
        found |= src->found != 0u ? 1u : 0u;
        if (bad) src->found = 1u;
        clip->eff.applied_steps = src->applied_steps;
    }
    clip->eff.found = found;
    if (bad) {
        clip->nonfinite_steps += 1;
    } else {
        if (coef < 1.0) clip->clipped_steps += 1;
        if (!nonfinite1(fnorm) && fnorm > clip->norm_max) clip->norm_max = fnorm;
    }
}
hipError_t vpd_launch_clip_finalize(vpd_clip_state* clip, int used, double max_norm, vpd_scale_state* src, float host_scale,
                                    hipStream_t s) {
    hipLaunchKernelGGL(clip_finalize_kernel, dim3(1), dim3(256), 0, s, clip, used, max_norm, src, host_scale);
    return hipGetLastError();
}

// Zero up to ZR_MAX float ranges in ONE launch (accumulator rows of the BN statistics + the fp32 weight-gradient
// ranges the atomics kernel adds into): hipMemsetAsync costs 5-12 us per call on this runtime.
__global__ __launch_bounds__(256) void zero_ranges_kernel(const ZeroRanges z) {
    float4* p = reinterpret_cast<float4*>(z.ptr[blockIdx.y]);
    const long n4 = z.n4[blockIdx.y];
    const float4 zero = {0.f, 0.f, 0.f, 0.f};
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long)gridDim.x * 256) p[i] = zero;
}
hipError_t vpd_launch_zero_ranges(const ZeroRanges& z, hipStream_t s) {
    if (z.count <= 0) return hipSuccess;
    long mx = 0;
    for (int i = 0; i < z.count; ++i) mx = z.n4[i] > mx ? z.n4[i] : mx;
    long gx = (mx + 255) / 256;
    if (gx > 512) gx = 512;
    hipLaunchKernelGGL(zero_ranges_kernel, dim3((unsigned)(gx < 1 ? 1 : gx), z.count), dim3(256), 0, s, z);
    return hipGetLastError();
}

// ---- gradient accumulation (vpd_op_grad_accumulate): dst = src (ADD false) or dst += src (ADD true) over up to GA_MAX range pairs ----
// ema_update_kernel's walk with a plain fp32 add in place of the fma: a pair is split by the 16-byte phase of `dst`, the aligned
// middle goes in 16 KB tiles (a wave takes four consecutive 1 KB rows of each operand from one address, every load issued before the
// first use), what is left of it one float4 per thread, `src` float by float when it does not share dst's phase.  The store mode
// (the first micro-batch of a window) never reads dst: whatever the accumulator held, NaN included, is gone.
static __device__ __forceinline__ float acc1(float d, float s) {
#pragma clang fp contract(off)
    return d + s;
}
static __device__ __forceinline__ f32x4 acc4(const f32x4& d, const f32x4& s) {
    return f32x4{acc1(d.x, s.x), acc1(d.y, s.y), acc1(d.z, s.z), acc1(d.w, s.w)};
}
// (at most 64 registers, as ema_update_kernel: the capped grid of 2048 blocks = 8 waves per SIMD is resident at once)
template <bool ADD>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(8, 8))) void grad_accum_kernel(const AccumRanges r) {
    const long tid = (long)blockIdx.x * 256 + threadIdx.x, nth = (long)gridDim.x * 256;
    for (int k = 0; k < r.count; ++k) {
        const float* x = r.src[k];
        float* y = r.dst[k];
        const long n = r.n[k];
        const RangeSplit sp = split_range(y, n);
        const long head = sp.head, n4 = sp.n4, tail = sp.tail;
        f32x4* y4 = reinterpret_cast<f32x4*>(y + head);
        long i = tid;
        if ((reinterpret_cast<size_t>(x + head) & 15) == 0) {
            const f32x4* x4 = reinterpret_cast<const f32x4*>(x + head);
            // tiles of 1024 float4: the last element a tile touches is (tl << 10) + 3 * 256 + 63 + 192 = (tl << 10) + 1023 < n4
            const long ntile = n4 >> 10;
            for (long tl = blockIdx.x; tl < ntile; tl += gridDim.x) {
                const long e = (tl << 10) + (threadIdx.x >> 6) * 256 + (threadIdx.x & 63);
                const f32x4* xp = x4 + e;
                f32x4* yp = y4 + e;
                Rows4 rs = load_rows4(xp);
                if constexpr (ADD) {
                    Rows4 rd = load_rows4(yp);
                    // (all eight loads are issued before the first is consumed: ema_update_kernel)
                    asm volatile("" : "+v"(rs.a), "+v"(rs.b), "+v"(rs.c), "+v"(rs.d), "+v"(rd.a), "+v"(rd.b), "+v"(rd.c), "+v"(rd.d));
                    yp[0] = acc4(rd.a, rs.a);
                    yp[64] = acc4(rd.b, rs.b);
                    yp[128] = acc4(rd.c, rs.c);
                    yp[192] = acc4(rd.d, rs.d);
                } else {
                    asm volatile("" : "+v"(rs.a), "+v"(rs.b), "+v"(rs.c), "+v"(rs.d));
                    yp[0] = rs.a;
                    yp[64] = rs.b;
                    yp[128] = rs.c;
                    yp[192] = rs.d;
                }
            }
            for (i += ntile << 10; i < n4; i += nth) {
                if constexpr (ADD) y4[i] = acc4(y4[i], x4[i]); else y4[i] = x4[i];
            }
        } else {
            const float* xs = x + head;
            for (; i < n4; i += nth) {
                const f32x4 s = {xs[4 * i], xs[4 * i + 1], xs[4 * i + 2], xs[4 * i + 3]};
                if constexpr (ADD) y4[i] = acc4(y4[i], s); else y4[i] = s;
            }
        }
        if (tid < head) y[tid] = ADD ? acc1(y[tid], x[tid]) : x[tid];
        if (tid < n - tail) y[tail + tid] = ADD ? acc1(y[tail + tid], x[tail + tid]) : x[tail + tid];
    }
}
hipError_t vpd_launch_grad_accum(const AccumRanges& r, bool add, hipStream_t s) {
    if (r.count < 0 || r.count > GA_MAX) return hipErrorInvalidValue;
    const int grid = vpd_grad_sqsum_grid(r.n, r.count, 2048);      // capped like ema_update_kernel's grid: 2048 blocks = 8 per CU
    if (grid == 0) return hipSuccess;
    if (add) hipLaunchKernelGGL(grad_accum_kernel<true>, dim3(grid), dim3(256), 0, s, r);
    else hipLaunchKernelGGL(grad_accum_kernel<false>, dim3(grid), dim3(256), 0, s, r);
    return hipGetLastError();
}
