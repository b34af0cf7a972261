// The A/B switches of the native library: every environment variable libvpdhip.so reads, declared once (what each selects:
// SWITCHES.md).  Unset: the default; set: atoi(value).  All of them are read together, once per process, at the library's first use
// of any switch (vpd_switches()), so a plan and the launchers it calls always see the same values.  "Off" sites test !x; a switch
// whose value is more than on / off interprets it where it is used:
//   wgrad_1x1     -1: no override (WgradParams::prefer_halo_1x1 decides); 0 / 1 forces       (vpd_wgrad_overwrites)
//   pws_blocks    only values > 0 replace the CU count                                       (pws_cu_count)
//   reserve_cus   rounded up to whole octets, clamped to leave 8 CUs                          (vpd_cu_budget)
//   bn_xcd_force  -1: not forced; read in -DVPD_ENABLE_ABLATE builds only, like ablate        (vpd_launch_bn_fwd_fused)
#pragma once
#include <stdlib.h>

#define VPD_SWITCHES(X)                                        \
    X(fused_bn,           "VPD_FUSED_BN",          1)          \
    X(bn_pair,            "VPD_BN_PAIR",           1)          \
    X(bn_xcd,             "VPD_BN_XCD",            1)          \
    X(bn_xcd_force,       "VPD_BN_XCD_FORCE",     -1)          \
    X(dgrad_sums,         "VPD_DGRAD_SUMS",        1)          \
    X(dgrad_sums_l1,      "VPD_DGRAD_SUMS_L1",     1)          \
    X(dgrad_sums_s2,      "VPD_DGRAD_SUMS_S2",     1)          \
    X(dgrad_sums_pair,    "VPD_DGRAD_SUMS_PAIR",   1)          \
    X(dgrad_sums_1x1,     "VPD_DGRAD_SUMS_1X1",    1)          \
    X(relu_bits,          "VPD_RELU_BITS",         1)          \
    X(poolbwd_fold,       "VPD_POOLBWD_FOLD",      1)          \
    X(ds_merge,           "VPD_DS_MERGE",          1)          \
    X(pws,                "VPD_PWS",               1)          \
    X(pws_blocks,         "VPD_PWS_BLOCKS",        0)          \
    X(ws_256x64,          "VPD_WS_256x64",         1)          \
    X(ws_mw8,             "VPD_WS_MW8",            1)          \
    X(no_ws,              "VPD_NO_WS",             0)          \
    X(pws_geo,            "VPD_PWS_GEO",           1)          \
    X(pws_rot,            "VPD_PWS_ROT",           1)          \
    X(pws_interior,       "VPD_PWS_INTERIOR",      1)          \
    X(reserve_cus,        "VPD_RESERVE_CUS",       0)          \
    X(c64x2,              "VPD_C64X2",             1)          \
    X(conv1x1_ws,         "VPD_CONV1X1_WS",        1)          \
    X(conv_s2_ws,         "VPD_CONV_S2_WS",        1)          \
    X(conv_s2_dgrad_ws,   "VPD_CONV_S2_DGRAD_WS",  1)          \
    X(wg2,                "VPD_WG2",               1)          \
    X(wg2_1x1,            "VPD_WG2_1X1",           1)          \
    X(wg2_tco256,         "VPD_WG2_TCO256",        1)          \
    X(conv1x1_stream,     "VPD_CONV1X1_STREAM",    1)          \
    X(bneck_recompute,    "VPD_BNECK_RECOMPUTE",   1)          \
    X(wg_group,           "VPD_WG_GROUP",          1)          \
    X(wg_merge,           "VPD_WG_MERGE",          1)          \
    X(wgrad_1x1,          "VPD_WGRAD_1X1",        -1)          \
    X(wgrad_s2,           "VPD_WGRAD_S2",          1)          \
    X(wgrad_ds_ride,      "VPD_WGRAD_DS_RIDE",     1)          \
    X(stem_lds_store,     "VPD_STEM_LDS_STORE",    1)          \
    X(stem_pair,          "VPD_STEM_PAIR",         1)          \
    X(stem_quad,          "VPD_STEM_QUAD",         1)          \
    X(stem_poolsums,      "VPD_STEM_POOLSUMS",     1)          \
    X(stem_pool_fused,    "VPD_STEM_POOL_FUSED",   1)          \
    X(ablate,             "VPD_ABLATE",            0)

struct VpdSwitches {
#define VPD_SWITCH_FIELD(field, env, dflt) int field;
    VPD_SWITCHES(VPD_SWITCH_FIELD)
#undef VPD_SWITCH_FIELD
};

inline const VpdSwitches& vpd_switches() {
    static const VpdSwitches s = [] {
        VpdSwitches v;
#define VPD_SWITCH_READ(field, env, dflt) { const char* e = getenv(env); v.field = e ? atoi(e) : (dflt); }
        VPD_SWITCHES(VPD_SWITCH_READ)
#undef VPD_SWITCH_READ
        return v;
    }();
    return s;
}
