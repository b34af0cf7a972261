// Host-only table of every decision of the convolution launcher over a sweep of shapes (no device needed: the launcher assumes 256
// CUs without one).  One row per problem: its arguments, the 12 values of vpd_op_conv2d_dispatch, vpd_op_conv2d_interior and
// vpd_conv_xcd_tile_px.  Two builds of the library agree on every decision when their tables are equal row for row
// (profiles/conv_launch_refactor.txt); the launcher reads its switches once per process, so each setting is one run.
//   hipcc -O1 -std=c++17 --offload-arch=gfx950 -I vpd_amd/csrc -I include tools/conv_dispatch_sweep.hip -L <dir of libvpdhip.so>
//         -lvpdhip -Wl,-rpath,<dir> -o sweep && VPD_PWS=0 ./sweep > table.txt
// The last line on stderr counts the rows that pass vpd_launch_conv's preconditions and, of those, the rows whose epilogue mode the
// chosen kernel family does not instantiate (conv_epilogue.h's lists): the launchers return hipErrorInvalidValue for such a row.
#include <stdio.h>

#include "common.h"
#include "conv_epilogue.h"
#include "kernels.h"
#include "vpd_hip.h"

namespace {
const double present = 0.0;      // the launcher's decisions read pointers only as present / absent

// the ConvParams of vpd_op_conv2d_dispatch (ops.hip) for the same arguments
ConvParams params(const int* a, const int* taps, int accumulate, int flags) {
    TapSet t;
    t.nr = taps[0]; t.nc = taps[1]; t.dy0 = taps[2]; t.dys = taps[3]; t.dx0 = taps[4]; t.dxs = taps[5]; t.w0 = taps[6]; t.wrs = taps[7]; t.wcs = taps[8];
    ConvParams q = vpd_conv_params(nullptr, a[1], a[2], a[3], nullptr, a[0], a[8], a[9], a[13], a[14], a[15], t);
    q.yHp = a[4]; q.yWp = a[5]; q.yC = a[6]; q.ypad = a[7];
    q.osub = a[10]; q.oph = a[11]; q.opw = a[12]; q.accumulate = accumulate;
    if (flags & 1) q.stats = const_cast<double*>(&present);
    if (flags & 2) { q.ep_scale = (const float*)&present; q.ep_shift = (const float*)&present; }
    if (flags & 4) q.acc_mask = (const unsigned char*)&present;
    if (flags & 8) { q.bst_z = (const bf16_t*)&present; q.bst_mask = (const unsigned char*)&present; vpd_conv_set_bn_rows(q, const_cast<double*>(&present)); }
    if (flags & 16) { q.bst_z2 = (const bf16_t*)&present; q.stats2 = const_cast<double*>(&present); }
    return q;
}

// the epilogue modes of the kernel family the dispatch values name
bool family_has_mode(const int* v) {
    const int kclass = v[0], c64x2 = v[3], ws1x1 = v[4], stream1x1 = v[5], halo = v[6], mode = v[9];
    switch (kclass) {
        case 0: return c64x2 ? mode == 3 : ConvC64Modes::has(mode);
        case 1: case 2: case 3: case 6: return Conv3x3WsModes::has(mode);      // (a geo instantiation or the run-time-geometry kernel)
        case 5: return mode == 0 || mode == 1;                                 // the stem kernel: plain store or statistics
        default: break;
    }
    if (stream1x1) return Conv1x1StreamModes::has(mode);
    if (ws1x1) return Conv1x1WsModes::has(mode);
    if (halo) return mode <= 3;                                                // conv3x3_halo_kernel decides at run time, no sums branch
    return ConvGatherModes::has(mode);
}
}  // namespace

int main() {
    const int crops[] = {1, 5, 13, 64, 101, 256, 401, 512, 1000};
    const int sizes[] = {4, 8, 16, 32};
    // channel pairs of ResNet-18 / 34 (3x3 and 1x1 branch) and ResNet-50 (Bottleneck 1x1s, 3x3s, branches), both directions
    const int pairs[][2] = {{64, 64}, {64, 128}, {128, 64}, {128, 128}, {128, 256}, {256, 128}, {256, 256}, {256, 512}, {512, 256},
                            {512, 512}, {64, 256}, {256, 64}, {128, 512}, {512, 128}, {256, 1024}, {1024, 256}, {512, 1024},
                            {1024, 512}, {512, 2048}, {2048, 512}, {1024, 2048}, {2048, 1024}};
    // forward 3x3, the data gradient's mirrored 3x3, stride-2 3x3 forward, 1x1
    const int tapsets[4][9] = {{3, 3, 0, 1, 0, 1, 0, 3, 1}, {3, 3, 2, -1, 2, -1, 0, 3, 1}, {3, 3, 0, 1, 0, 1, 0, 3, 1}, {1, 1, 1, 1, 1, 1, 0, 1, 1}};
    const char* tapnames[4] = {"fwd", "flip", "s2", "1x1"};
    const int flagset[] = {0, 1, 2, 4, 8, 8 | 16};
    long rows = 0, launchable = 0, missing = 0;
    for (int n : crops) for (int hw : sizes) for (const auto& c : pairs) for (int ts = 0; ts < 4; ++ts)
        for (int ypad = 0; ypad < 2; ++ypad) for (int acc = 0; acc < 2; ++acc) for (int flags : flagset) {
            const int istr = ts == 2 ? 2 : 1;
            // (n, xHp, xWp, xC, yHp, yWp, yC, ypad, Hs, Ws, osub, oph, opw, istr, Kc, Co)
            const int a[16] = {n, hw * istr + 2, hw * istr + 2, c[0], hw + 2 * ypad, hw + 2 * ypad, c[1], ypad, hw, hw, 1, 0, 0, istr, c[0], c[1]};
            int v[12] = {0}, interior = -1, xcd = -1;
            const int rc = vpd_op_conv2d_dispatch(a[0], a[1], a[2], a[3], a[4], a[5], a[6], a[7], a[8], a[9], a[10], a[11], a[12], a[13], a[14],
                                                  a[15], tapsets[ts], acc, flags, v);
            if (rc == 0) {
                vpd_op_conv2d_interior(a[0], a[1], a[2], a[3], a[4], a[5], a[6], a[7], a[8], a[9], a[10], a[11], a[12], a[13], a[14], a[15],
                                       tapsets[ts], acc, flags, &interior);
                xcd = vpd_conv_xcd_tile_px(params(a, tapsets[ts], acc, flags));
            }
            printf("n %d hw %d ci %d co %d %s ypad %d acc %d flags %d : rc %d |", n, hw, c[0], c[1], tapnames[ts], ypad, acc, flags, rc);
            for (int k = 0; k < 12; ++k) printf(" %d", v[k]);
            printf(" | interior %d xcd_px %d\n", interior, xcd);
            ++rows;
            if (rc != 0 || ((flags & 8) && !v[11])) continue;      // vpd_launch_conv refuses BatchNorm sums no kernel takes
            ++launchable;
            if (!family_has_mode(v)) { ++missing; fprintf(stderr, "mode %d outside the family's list: n %d hw %d ci %d co %d %s ypad %d acc %d flags %d\n", v[9], n, hw, c[0], c[1], tapnames[ts], ypad, acc, flags); }
        }
    fprintf(stderr, "%ld rows, %ld pass vpd_launch_conv's preconditions, %ld of those with a mode outside the chosen family's list\n",
            rows, launchable, missing);
    return missing != 0;
}
