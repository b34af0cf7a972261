"""ctypes binding of libvpdhip.so (C ABI in include/vpd_hip.h).

The library is the product: there is no PyTorch / CPU fallback for the hot
path.  ``lib()`` raises if the shared object is missing or lacks a symbol.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# VPD_LIB_PATH: A/B another build of the same ABI on the same GPU (devices differ by several % in clocks)
LIB_PATH = os.environ.get("VPD_LIB_PATH") or os.path.join(_HERE, "libvpdhip.so")
# the same sources built with fp16 elements (vpd_amd/csrc/Makefile, common.h "Element type"): training and inference
LIB_PATH_F16 = os.environ.get("VPD_LIB_PATH_F16") or os.path.join(_HERE, "libvpdhip_f16.so")
ABI_VERSION = 5

c_int_p = C.POINTER(C.c_int)
c_ll_p = C.POINTER(C.c_longlong)
c_dbl_p = C.POINTER(C.c_double)
vp = C.c_void_p

# name -> (restype, argtypes); mirrors include/vpd_hip.h one to one
SIGNATURES = {
    "vpd_last_error": (C.c_char_p, []),
    "vpd_abi_version": (C.c_int, []),
    "vpd_elem_dtype": (C.c_char_p, []),
    "vpd_plan_create": (C.c_int, [C.c_char_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                  C.POINTER(vp)]),
    "vpd_plan_destroy": (None, [vp]),
    "vpd_plan_num_tensors": (C.c_int, [vp]),
    "vpd_plan_tensor_info": (C.c_int, [vp, C.c_int, c_int_p, c_int_p, c_ll_p, c_ll_p, c_int_p, c_int_p]),
    "vpd_plan_param_numel": (C.c_longlong, [vp]),
    "vpd_plan_num_bn": (C.c_int, [vp]),
    "vpd_plan_bn_info": (C.c_int, [vp, C.c_int, c_int_p, c_ll_p, c_ll_p]),
    "vpd_plan_bn_numel": (C.c_longlong, [vp]),
    "vpd_plan_num_buckets": (C.c_int, [vp]),
    "vpd_plan_bucket_range": (C.c_int, [vp, C.c_int, c_ll_p, c_ll_p]),
    "vpd_plan_workspace_bytes": (C.c_size_t, [vp]),
    "vpd_plan_init_workspace": (C.c_int, [vp, vp, vp]),
    "vpd_pack_weights": (C.c_int, [vp, vp, vp, vp, vp]),
    "vpd_forward_eval": (C.c_int, [vp, vp, vp, C.c_int, vp, vp, vp, vp, vp, vp]),
    "vpd_forward_train": (C.c_int, [vp, vp, vp, vp, vp, C.c_int, vp, vp, vp, vp, vp]),
    "vpd_backward": (C.c_int, [vp, vp, vp, C.c_int, C.POINTER(vp), vp, vp]),
    "vpd_backward_ext": (C.c_int, [vp, vp, vp, vp, C.c_int, vp, C.POINTER(vp), vp, vp]),
    "vpd_adamw_step": (C.c_int, [vp, vp, vp, vp, C.c_longlong, C.c_double, C.c_double, C.c_double, C.c_double,
                                 C.c_double, C.c_int, vp]),
    "vpd_plan_adamw_step": (C.c_int, [vp, vp, vp, vp, vp, C.c_longlong, C.c_double, C.c_double, C.c_double, C.c_double,
                                      C.c_double, C.c_int, vp, vp]),
    "vpd_augment_crops": (C.c_int, [vp, vp, vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_float),
                                    C.c_float, vp, vp, vp]),
    "vpd_plan_stage_crops": (C.c_int, [vp, vp, vp, vp, vp, vp, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_float),
                                       C.c_float, vp, vp, vp]),
    "vpd_plan_stage_views": (C.c_int, [vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_float), vp, vp]),
    "vpd_augment_views": (C.c_int, [vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_float), vp, vp, vp]),
    "vpd_plan_stage_views_jitter": (C.c_int, [vp, vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                              C.POINTER(C.c_float), vp, vp, vp]),
    "vpd_graph_capture_eval": (C.c_int, [vp, vp, vp, C.c_int, vp, vp, vp]),
    "vpd_graph_launch_eval": (C.c_int, [vp, C.c_int, vp]),
    "vpd_plan_sync_errors": (C.c_int, [vp, vp, vp, C.POINTER(C.c_uint)]),
    "vpd_plan_set_lazy_grads": (C.c_int, [vp, C.c_int]),
    "vpd_plan_set_loss_scale": (C.c_int, [vp, C.c_float]),
    "vpd_plan_set_scale_state": (C.c_int, [vp, vp]),
    "vpd_plan_check_grads": (C.c_int, [vp, vp, C.c_longlong, vp, vp, vp]),
    "vpd_op_check_finite": (C.c_int, [vp, C.c_longlong, vp, vp]),
    "vpd_adamw_step_scaled": (C.c_int, [vp, vp, vp, vp, C.c_longlong, C.c_double, C.c_double, C.c_double, C.c_double,
                                        C.c_double, vp, vp]),
    "vpd_plan_adamw_step_scaled": (C.c_int, [vp, vp, vp, vp, vp, C.c_longlong, C.c_double, C.c_double, C.c_double, C.c_double,
                                             C.c_double, vp, vp, vp]),
    "vpd_scale_state_update": (C.c_int, [vp, C.c_float, C.c_float, C.c_int, vp]),
    "vpd_ema_update": (C.c_int, [C.POINTER(vp), C.POINTER(vp), c_ll_p, C.c_int, C.c_double, C.c_int, C.c_int, C.c_int, vp, vp]),
    "vpd_clip_state_bytes": (C.c_size_t, []),
    "vpd_op_grad_norm": (C.c_int, [C.POINTER(vp), c_ll_p, C.c_int, C.c_double, vp, C.c_float, vp, vp]),
    "vpd_plan_grad_norm": (C.c_int, [vp, vp, C.c_longlong, C.c_double, vp, C.c_float, vp, vp, vp]),
    "vpd_adam_groups_bytes": (C.c_size_t, [C.c_int]),
    "vpd_adam_groups_init": (C.c_int, [vp, vp, c_ll_p, c_int_p, C.c_int, C.c_longlong, C.c_int, vp]),
    "vpd_adamw_step_groups": (C.c_int, [vp, vp, vp, vp, C.c_longlong, vp, c_dbl_p, c_dbl_p, C.c_int, C.c_double, C.c_double,
                                        C.c_double, C.c_int, C.c_float, vp, vp]),
    "vpd_plan_adamw_step_groups": (C.c_int, [vp, vp, vp, vp, vp, C.c_longlong, vp, c_dbl_p, c_dbl_p, C.c_int, C.c_double,
                                             C.c_double, C.c_double, C.c_int, vp, vp, vp]),
    "vpd_op_grad_accumulate": (C.c_int, [C.POINTER(vp), C.POINTER(vp), c_ll_p, C.c_int, C.c_int, vp]),
    "vpd_plan_grad_accum_numel": (C.c_longlong, [vp]),
    "vpd_plan_grad_accumulate": (C.c_int, [vp, vp, C.c_longlong, vp, C.c_int, vp, vp]),
    "vpd_plan_bucket_scratch_range": (C.c_int, [vp, C.c_int, C.POINTER(C.c_longlong), C.POINTER(C.c_longlong)]),
    "vpd_plan_grads_pending": (C.c_int, [vp]),
    "vpd_plan_materialize_grads": (C.c_int, [vp, vp, vp, vp]),
    "vpd_plan_set_bn_frozen": (C.c_int, [vp, C.c_int]),
    "vpd_plan_set_param_grads": (C.c_int, [vp, C.c_int]),
    "vpd_plan_set_timing": (C.c_int, [vp, C.c_int]),
    "vpd_plan_read_timing": (C.c_int, [vp, C.POINTER(C.c_double), C.c_int]),
    "vpd_op_conv2d": (C.c_int, [vp, vp, vp, vp] + [C.c_int] * 16 + [c_int_p, C.c_int, vp]),
    "vpd_op_conv_bm": (C.c_int, [C.c_int, C.c_int]),
    "vpd_op_conv2d_ep": (C.c_int, [vp, vp, vp] + [C.c_int] * 13 + [c_int_p, vp, vp, vp, C.c_int, C.c_int, vp, vp]),
    "vpd_op_conv2d_bnsums": (C.c_int, [vp] * 6 + [C.c_int] * 8 + [c_int_p, C.c_int, vp]),
    "vpd_op_conv2d_bnsums2": (C.c_int, [vp] * 8 + [C.c_int] * 8 + [c_int_p, vp]),
    "vpd_op_conv2d_dispatch": (C.c_int, [C.c_int] * 16 + [c_int_p, C.c_int, C.c_int, c_int_p]),
    "vpd_op_conv2d_interior": (C.c_int, [C.c_int] * 16 + [c_int_p, C.c_int, C.c_int, c_int_p]),
    "vpd_op_bn_forward": (C.c_int, [vp] * 13 + [C.c_int] * 5 + [C.c_float, C.c_float, vp]),
    "vpd_op_set_bn_frozen": (C.c_int, [C.c_int]),
    "vpd_op_bn_forward2": (C.c_int, [vp] * 22 + [C.c_int] * 5 + [C.c_float, C.c_float, vp]),
    "vpd_op_bn_finalize": (C.c_int, [vp] * 9 + [C.c_int, C.c_int, C.c_float, C.c_float, vp]),
    "vpd_op_bn_apply": (C.c_int, [vp] * 6 + [C.c_int, vp] + [C.c_int] * 5 + [vp]),
    "vpd_op_bn_backward_apply": (C.c_int, [vp] * 10 + [C.c_int] * 4 + [vp]),
    "vpd_op_bn_backward_apply2": (C.c_int, [vp] * 18 + [C.c_int] * 4 + [vp]),
    "vpd_op_conv1x1_bn": (C.c_int, [C.c_int, vp, vp] + [C.c_int] * 6 + [vp] * 5 + [C.c_float, C.c_float] + [vp] * 12),
    "vpd_op_conv1x1_bn2": (C.c_int, [C.c_int] + [vp] * 4 + [C.c_int] * 6 + [vp] * 18 + [C.c_float, C.c_float] + [vp] * 10),
    "vpd_op_conv1x1_bn_dispatch": (C.c_int, [C.c_int] * 6 + [c_int_p]),
    "vpd_op_stem_pool_forward": (C.c_int, [vp] * 5 + [C.c_int] * 5 + [vp]),
    "vpd_op_stem_dgrad": (C.c_int, [vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, vp]),
    "vpd_op_stem_pool_backward": (C.c_int, [vp] * 15 + [C.c_int] * 4 + [vp]),
    "vpd_op_bn_backward": (C.c_int, [vp] * 15 + [C.c_int] + [vp, vp] + [C.c_int] * 6 + [vp]),
    "vpd_op_bn_backward_pair": (C.c_int, [vp] * 20 + [C.c_int] * 4 + [vp]),
    "vpd_op_bn_backward_residency": (C.c_int, [C.c_int, C.c_int, C.c_int, c_int_p]),
    "vpd_op_avgpool": (C.c_int, [vp] + [C.c_int] * 5 + [vp, vp]),
    "vpd_op_avgpool_bwd": (C.c_int, [vp] + [C.c_int] * 4 + [vp, vp]),
    "vpd_op_sgemm": (C.c_int, [vp] * 4 + [C.c_int] * 6 + [vp]),
    "vpd_op_colsum": (C.c_int, [vp, C.c_int, C.c_int, vp, vp]),
    "vpd_op_relu_mask": (C.c_int, [vp, vp, C.c_longlong, vp]),
    "vpd_op_mse": (C.c_int, [vp, vp, C.c_longlong, vp, vp, vp, vp]),
    "vpd_op_wgrad": (C.c_int, [vp, vp, vp] + [C.c_int] * 13 + [c_int_p, vp, vp]),
    "vpd_op_wgrad_slab_bytes": (C.c_size_t, []),
    "vpd_op_wgrad_dispatch": (C.c_int, [C.c_int] * 13 + [c_int_p, C.c_int, C.c_int, c_int_p]),
    "vpd_op_wgrad_group_slab_floats": (C.c_size_t, [C.c_int, C.c_int]),
    "vpd_op_wgrad_group_dispatch": (C.c_int, [C.c_int, c_int_p, c_int_p]),
    "vpd_op_wgrad_group": (C.c_int, [C.c_int, vp, vp, vp, vp, c_int_p, vp]),
    "vpd_op_wgrad_pair": (C.c_int, [vp] * 5 + [C.c_int] * 13 + [c_int_p, vp, vp, vp]),
    "vpd_op_wgrad_pair_lds_bytes": (C.c_int, [C.c_int, C.c_int, C.c_int, c_ll_p]),
    "vpd_op_tr_read_probe": (C.c_int, [vp, vp, vp]),
    "vpd_op_wgrad128_table_bytes": (C.c_size_t, []),
    "vpd_op_wgrad128_slab_floats": (C.c_size_t, [C.c_int, C.c_int]),
    "vpd_op_wgrad128_group": (C.c_int, [C.c_int, vp, vp, vp, vp, c_int_p, vp, vp]),
    "vpd_op_wgrad128_schedule": (C.c_int, [C.c_int, c_int_p, C.c_int, c_int_p, c_int_p, c_int_p, C.c_int,
                                           C.POINTER(C.c_double)]),
    "vpd_op_pack_input": (C.c_int, [vp] + [C.c_int] * 4 + [vp] + [C.c_int] * 3 + [vp]),
    "vpd_op_pack_weights": (C.c_int, [vp] + [C.c_int] * 4 + [vp, vp, vp]),
    "vpd_op_unpack_grads": (C.c_int, [vp] + [C.c_int] * 5 + [vp, vp]),
    "vpd_op_adamw_pack": (C.c_int, [C.c_int, c_int_p, c_ll_p, C.c_longlong] + [vp] * 6 + [C.c_double] * 5 + [C.c_int, C.c_float, vp]),
    "vpd_op_adamw_pack_groups": (C.c_int, [C.c_int, c_int_p, c_ll_p, C.c_longlong] + [vp] * 6 + [c_ll_p, c_int_p, C.c_int, c_dbl_p,
                                           c_dbl_p, C.c_int] + [C.c_double] * 3 + [C.c_int, C.c_float, vp, vp]),
    "vpd_op_wgrad_reduce": (C.c_int, [C.c_int, C.POINTER(vp), C.POINTER(vp), c_ll_p, c_int_p, vp]),
    "vpd_op_zero_ranges": (C.c_int, [C.POINTER(vp), c_ll_p, C.c_int, vp]),
}

# what an OLDER build of the library may lack when it is A/B-ed through VPD_LIB_PATH / VPD_LIB_PATH_F16 (and every vpd_op_*
# operator-level test entry point); the in-tree library must export every declared symbol
OPTIONAL_SYMBOLS = ("vpd_elem_dtype", "vpd_plan_set_loss_scale", "vpd_backward_ext", "vpd_plan_set_bn_frozen",
                    "vpd_plan_set_param_grads", "vpd_ema_update", "vpd_clip_state_bytes", "vpd_plan_grad_norm",
                    "vpd_adam_groups_bytes", "vpd_adam_groups_init", "vpd_adamw_step_groups", "vpd_plan_adamw_step_groups",
                    "vpd_plan_grad_accum_numel", "vpd_plan_grad_accumulate")

_libs = {}


class VpdHipError(RuntimeError):
    pass


def lib(dtype="bf16"):
    """Load libvpdhip.so (dtype "bf16": training and inference) or libvpdhip_f16.so ("fp16": the same, behind a loss scaler), once each.
    Raises -- never falls back -- when the library is absent, lacks a symbol or was built for another element type."""
    if dtype in _libs:
        return _libs[dtype]
    if dtype not in ("bf16", "fp16"):
        raise VpdHipError("unknown element type %r (bf16 | fp16)" % (dtype,))
    path = LIB_PATH if dtype == "bf16" else LIB_PATH_F16
    name = os.path.basename(path)
    if not os.path.isfile(path):
        raise VpdHipError(
            "%s not found at %s: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "or `make -C vpd_amd/csrc`.  vpd_amd has no PyTorch/CPU fallback." % (name, path))
    # torch first: its libamdhip64 becomes the process's HIP runtime and the library binds to it by soname.  Loaded before torch,
    # the library would pull in the system ROCm's runtime and torch would still map its own (its libraries ask for the unversioned
    # name): two runtimes in one process, and the library's sees no device
    import torch  # noqa: F401
    h = C.CDLL(path)
    # VPD_LIB_PATH / VPD_LIB_PATH_F16 (same-box A/B against an OLDER build of the library, tools/build_head_lib.sh): the operator-level test entry
    # points that build does not have yet are skipped; the in-tree library must export every declared symbol
    ab_build = ("VPD_LIB_PATH" if dtype == "bf16" else "VPD_LIB_PATH_F16") in os.environ
    for sym, (res, args) in SIGNATURES.items():
        try:
            fn = getattr(h, sym)
        except AttributeError as e:
            # (an OLDER library, same-box A/B: the entry points added since are optional there -- OPTIONAL_SYMBOLS, require())
            if ab_build and (sym.startswith("vpd_op_") or sym in OPTIONAL_SYMBOLS):
                continue
            raise VpdHipError("%s lacks symbol %s declared in include/vpd_hip.h" % (name, sym)) from e
        fn.restype = res
        fn.argtypes = args
    # (VPD_LIB_ALLOW_ABI=<n>: a same-box A/B against round n's library, whose train-step entry points have the same signatures)
    if h.vpd_abi_version() != ABI_VERSION and not (ab_build and os.environ.get("VPD_LIB_ALLOW_ABI") == str(h.vpd_abi_version())):
        raise VpdHipError("%s ABI version %d != expected %d" % (name, h.vpd_abi_version(), ABI_VERSION))
    if hasattr(h, "vpd_elem_dtype") and h.vpd_elem_dtype().decode() != dtype:
        raise VpdHipError("%s was built with %s elements, %s asked for" % (path, h.vpd_elem_dtype().decode(), dtype))
    _libs[dtype] = h
    return h


def has(L, symbol):
    """whether this library exports `symbol` of OPTIONAL_SYMBOLS (every other symbol is there, or lib() had raised)"""
    assert symbol in OPTIONAL_SYMBOLS, symbol
    return hasattr(L, symbol)


def require(L, symbol, what=None):
    """An entry point of OPTIONAL_SYMBOLS is about to be called: RuntimeError when this (older, A/B) library lacks it.
    what: the feature's name in the message, in front of the symbol's"""
    if not has(L, symbol):
        raise RuntimeError("this libvpdhip has no %s" % (symbol if what is None else "%s (%s)" % (what, symbol)))


def check(rc, what="", dtype="bf16"):
    if rc != 0:
        msg = lib(dtype).vpd_last_error()
        raise VpdHipError("%s failed: %s" % (what or "libvpdhip call", msg.decode() if msg else "unknown error"))
