// Compile-time-geometry instantiations of conv3x3_pws_kernel (conv_pws.h, "compile-time geometry"): the image width W and the tap
// orientation are template parameters, so a pixel fragment's LDS address is a per-lane register + an immediate.  One translation
// unit of their own: they compile beside conv_igemm.hip.
//
// Reference shapes: models/module.py:61-67 (layer2 / layer3 / layer4 of the 128 x 128 student: W = 16 / 8 / 4).
#include <hip/hip_runtime.h>

#include "conv_pws.h"
#include "kernels.h"

namespace {

template <int KC, int WC, bool INT>
bool launch_geo(bool flip, const ConvParams& q, const HaloGeom& g, const PwsGrid& sg, dim3 grid, dim3 block, size_t lds,
                hipStream_t stream) {
    static_assert(conv3x3_tile_class(KC), "a 3x3 tile class");
    constexpr Conv3x3Tile T = conv3x3_tile(KC);
    if (!flip) return Conv3x3GeoFwdModes::visit(conv_ep_mode(q), [&](auto m) {
        VPD_LAUNCH((conv3x3_pws_kernel<T.bm, T.bn, T.hrows, T.ns, decltype(m)::value, T.nmw, T.pipe, WC, false, INT>), grid, block, lds, stream, q, g, sg);
    });
    return Conv3x3GeoFlipModes::visit(conv_ep_mode(q), [&](auto m) {
        VPD_LAUNCH((conv3x3_pws_kernel<T.bm, T.bn, T.hrows, T.ns, decltype(m)::value, T.nmw, T.pipe, WC, true, INT>), grid, block, lds, stream, q, g, sg);
    });
}

}  // namespace

// Image width of the compile-time-geometry instantiation that takes this launch of a 3x3 tile class (and its tap orientation), or
// 0: none does
int vpd_pws_geo_width(int kclass, const ConvParams& q, const HaloGeom& g, bool* flip_out) {
    const TapSet& t = q.taps;
    const bool fwd = t.dy0 == 0 && t.dys == 1 && t.dx0 == 0 && t.dxs == 1;
    const bool flip = t.dy0 == 2 && t.dys == -1 && t.dx0 == 2 && t.dxs == -1;
    if (!fwd && !flip) return 0;
    // (the swizzle key the kernel's bases are built from: halo_geom, conv_igemm.hip)
    if (q.Ws >= 8 ? !(g.kmask == 7 && g.kshift == 0 && g.rowmask == 0) : !(g.kmask == 3 && g.kshift == 2 && g.rowmask == 1)) return 0;
    const int mode = conv_ep_mode(q);
    if (flip ? !Conv3x3GeoFlipModes::has(mode) : !Conv3x3GeoFwdModes::has(mode)) return 0;
    *flip_out = flip;
    if (kclass == 6) return q.Ws == 16 || q.Ws == 8 ? q.Ws : 0;
    if (kclass == 3) return q.Ws == 4 ? 4 : 0;
    // (round 6, measured and removed -- profiles/r06_ab_geo8.txt: the same loop on class 1's eight-wave 256 x 128 tile, whose 168-register
    //  budget it does not fit without spilling and whose two MFMA waves per SIMD already cover each other's reads, 676 vs 636 us per step
    //  for its class at 512 crops; with it and the 128 x 128 tile of layer4 the apply forward read 389 k against 393 k crops/s)
    return 0;
}

bool vpd_launch_pws_geo(int kclass, const ConvParams& q, const HaloGeom& g, const PwsGrid& sg, dim3 grid, dim3 block, size_t lds,
                        hipStream_t stream) {
    bool flip = false;
    // HaloGeom::interior (vpd_conv_dispatch) picks the interior-loader twin of the same kernel: same MFMA side, same results
    switch (vpd_pws_geo_width(kclass, q, g, &flip)) {      // (widths 16 / 8: class 6 only, width 4: class 3 only)
        case 16: return g.interior ? launch_geo<6, 16, true>(flip, q, g, sg, grid, block, lds, stream)
                                   : launch_geo<6, 16, false>(flip, q, g, sg, grid, block, lds, stream);
        case 8: return g.interior ? launch_geo<6, 8, true>(flip, q, g, sg, grid, block, lds, stream)
                                  : launch_geo<6, 8, false>(flip, q, g, sg, grid, block, lds, stream);
        case 4: return g.interior ? launch_geo<3, 4, true>(flip, q, g, sg, grid, block, lds, stream)
                                  : launch_geo<3, 4, false>(flip, q, g, sg, grid, block, lds, stream);
        default: return false;
    }
}
