"""ctypes bindings of the native libraries.  Loading fails LOUDLY: there is no CPU fallback
for the product path (the CPU oracle lives under oracle/ and is test infrastructure)."""
from __future__ import annotations

import ctypes
import os

from . import _build

c_float_p = ctypes.POINTER(ctypes.c_float)
c_int_p = ctypes.POINTER(ctypes.c_int)


class KernelStat(ctypes.Structure):
    _fields_ = [("name", ctypes.c_char * 48), ("launches", ctypes.c_int32), ("total_ms", ctypes.c_float),
                ("flops", ctypes.c_double), ("bytes", ctypes.c_double)]


class BlockDesc(ctypes.Structure):
    """sayuri_hip_blockdesc"""
    _fields_ = [(n, ctypes.c_int32) for n in ("type", "apply_se", "se_size", "bottleneck_channels", "feedforward_channels", "dw_filter")]


class NetDesc(ctypes.Structure):
    """sayuri_hip_netdesc"""
    _fields_ = [(n, ctypes.c_int32) for n in ("version", "input_channels", "residual_channels", "residual_blocks", "policy_head_channels",
                                              "value_head_channels", "probabilities_channels", "pass_probability_outputs",
                                              "ownership_channels", "value_misc_outputs", "default_act", "policy_head_type",
                                              "policy_dw_filter")] + [("blocks", ctypes.POINTER(BlockDesc))]


def fp(a):
    return a.ctypes.data_as(c_float_p)


def ip(a):
    return a.ctypes.data_as(c_int_p)


# The C-ABI of include/sayuri_hip.h: name -> (restype, argtypes) of every function it declares, applied by hip() to what the
# loaded library exports.  A context (sayuri_hip_ctx*) and packed records are c_void_p: a Python int or an address goes in whole.
_I, _U, _Z, _V, _F, _IP = ctypes.c_int, ctypes.c_uint, ctypes.c_size_t, ctypes.c_void_p, c_float_p, c_int_p
_OUT = [_F] * 4  # prob, pass, misc, own
_STAT = ctypes.POINTER(KernelStat)
_W12 = ctypes.POINTER(c_float_p)  # weights12 of the head taps
HIP_ABI = {
    "sayuri_hip_device_count": (_I, []),
    "sayuri_hip_create": (_V, [_I, _V, _I, _I, _I]),
    "sayuri_hip_create_ex": (_V, [_I, _V, _I, _I, _I, _U]),
    "sayuri_hip_load_tensor": (_I, [_V, _I, _I, _F, _Z]),
    "sayuri_hip_reload_begin": (_I, [_V, _V]),
    "sayuri_hip_reload_prepare": (_I, [_V]),
    "sayuri_hip_reload_commit": (_I, [_V]),
    "sayuri_hip_reload_abort": (_I, [_V]),
    "sayuri_hip_weights_generation": (_I, [_V]),
    "sayuri_hip_forward": (_I, [_V, _I, _F, _IP] + _OUT),
    "sayuri_hip_upload": (_I, [_V, _I, _F, _IP]),
    "sayuri_hip_run": (_I, [_V]),
    "sayuri_hip_sync": (_I, [_V]),
    "sayuri_hip_download": (_I, [_V] + _OUT),
    "sayuri_hip_submit": (_I, [_V, _I, _F, _IP] + _OUT + [_IP]),
    "sayuri_hip_forward_packed": (_I, [_V, _I, _V, _I, _IP] + _OUT),
    "sayuri_hip_submit_packed": (_I, [_V, _I, _V, _I, _IP] + _OUT + [_IP]),
    "sayuri_hip_forward_packed_symm": (_I, [_V, _I, _V, _I, _I, _IP, _IP, _IP] + _OUT),
    "sayuri_hip_submit_packed_symm": (_I, [_V, _I, _V, _I, _I, _IP, _IP, _IP] + _OUT + [_IP]),
    "sayuri_hip_wait": (_I, [_V, _I]),
    "sayuri_hip_query": (_I, [_V, _I]),
    "sayuri_hip_time_runs": (_I, [_V, _I, _F]),
    "sayuri_hip_profile_run": (_I, [_V, _STAT, _I]),
    "sayuri_hip_mark_kernel": (_I, [_V, ctypes.c_char_p]),
    "sayuri_hip_timed_stat": (_I, [_V, _STAT]),
    "sayuri_hip_host_alloc": (_V, [_Z]),
    "sayuri_hip_host_free": (None, [_V]),
    "sayuri_hip_device_bytes": (_Z, [_V]),
    "sayuri_hip_last_chains": (_I, [_V]),
    "sayuri_hip_tower_state": (_I, [_V]),
    "sayuri_hip_latency_state": (_I, [_V]),
    "sayuri_hip_split_ring_plan": (_I, [_I, _IP, _I, _I, _I, _I]),
    "sayuri_hip_last_split_ring": (_I, [_V]),
    "sayuri_hip_pw_plan": (_I, [_I, _IP, _I, _I, _I, _I, _IP]),
    "sayuri_hip_last_pw_launches": (_I, [_V]),
    "sayuri_hip_dw_plan": (_I, [_I, _IP, _I, _I, _I, _I, _IP]),
    "sayuri_hip_last_dw_launches": (_I, [_V]),
    "sayuri_hip_destroy": (None, [_V]),
    "sayuri_hip_last_error": (ctypes.c_char_p, []),
    # the layer taps: device, (use_fp16,) n, board_sizes, max_board, shape ..., tensors
    "sayuri_hip_test_conv": (_I, [_I] * 3 + [_IP] + [_I] * 7 + [_F] * 5),
    "sayuri_hip_test_conv_split": (_I, [_I] * 2 + [_IP] + [_I] * 4 + [_F] * 5 + [_I] * 2),
    "sayuri_hip_test_last_conv_kind": (_I, []),
    "sayuri_hip_test_se_unit": (_I, [_I] * 3 + [_IP] + [_I] * 4 + [_F] * 8),
    "sayuri_hip_test_head_tail": (_I, [_I] * 3 + [_IP] + [_I] * 7 + [_F, _F, _W12] + _OUT),
    "sayuri_hip_test_conv_se": (_I, [_I] * 2 + [_IP] + [_I] * 5 + [_F] * 9),
    "sayuri_hip_test_last_se_form": (_I, []),
    "sayuri_hip_test_tower_run": (_I, [_I] * 2 + [_IP] + [_I] * 4 + [_IP, _IP, _F, _F, _I, _I] + [_F] * 4 + [_I, _F, _F]),
    "sayuri_hip_test_last_tower_run": (_I, [_IP]),
    "sayuri_hip_test_conv_sx": (_I, [_I] * 2 + [_IP] + [_I] * 4 + [_F] * 9),
    "sayuri_hip_test_last_sx_kts": (_I, []),
    "sayuri_hip_test_head_board": (_I, [_I] * 2 + [_IP] + [_I] * 8 + [_F] * 5 + [_W12] + _OUT),
    # device, use_fp16, n, board_sizes, max_board, cin, planes, records, n_records, binary, src, symm, perm, n0, ns, stage_batch, in_place,
    # sentinel, guard_rows, image
    "sayuri_hip_test_pack_input": (_I, [_I] * 3 + [_IP] + [_I] * 2 + [_F, _V, _I, _I] + [_IP] * 3 + [_I] * 4 + [ctypes.c_float, _I, _F]),
    "sayuri_hip_test_last_pack": (_I, [_IP]),
}
# A layer tap whose one Python caller is in the package (hipraw.conv_pw_layer), not in tests/_taps.py: same header, same binder.
HIP_PACKAGE_TAPS = {
    "sayuri_hip_test_conv_pw": (_I, [_I] * 2 + [_IP] + [_I] * 4 + [_F] * 5 + [_I]),
    "sayuri_hip_test_conv_dw": (_I, [_I] * 3 + [_IP] + [_I] * 4 + [_F] * 4 + [_I, _F]),
    "sayuri_hip_test_last_dw_pad": (_I, [_I, ctypes.POINTER(ctypes.c_uint16), _I]),
}
HIP_SYMBOLS = list(HIP_ABI) + list(HIP_PACKAGE_TAPS)

_hip = None
_host = None


def _require(path: str) -> str:
    if not os.path.exists(path):
        raise RuntimeError(
            f"native library {path} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
            "(there is no CPU fallback for the MI355X forward pipe)")
    return path


def hip() -> ctypes.CDLL:
    global _hip
    if _hip is None:
        path = _build.HIP_SO
        fake = os.environ.get("SAYURI_FAKE_HIP_LIB")
        if fake:
            # TEST HOOK (tests/fake_hip): a CPU stand-in for the DEVICE side of include/sayuri_hip.h, loaded ahead of the real
            # library so that the host side can be run without a GPU.  Never set in production; said out loud when it is.
            import sys
            print(f"[sayuri_amd] SAYURI_FAKE_HIP_LIB is set: the device side is the test stand-in {fake}, NOT the MI355X engine",
                  file=sys.stderr)
            path = fake
        lib = ctypes.CDLL(_require(path), mode=ctypes.RTLD_GLOBAL)
        # a device library may lack entry points (the stand-in knows the ABI it was written against and has no kernels to tap)
        for name, (restype, argtypes) in {**HIP_ABI, **HIP_PACKAGE_TAPS}.items():
            if hasattr(lib, name):
                fn = getattr(lib, name)
                fn.restype, fn.argtypes = restype, argtypes
        _hip = lib
    return _hip


def host() -> ctypes.CDLL:
    global _host
    if _host is None:
        hip()
        lib = ctypes.CDLL(_require(_build.HOST_SO))
        lib.sayuri_host_last_error.restype = ctypes.c_char_p
        lib.sayuri_weights_load.restype = ctypes.c_void_p
        lib.sayuri_weights_load.argtypes = [ctypes.c_char_p]
        lib.sayuri_weights_free.argtypes = [ctypes.c_void_p]
        lib.sayuri_weights_info.argtypes = [ctypes.c_void_p, c_int_p]
        lib.sayuri_weights_block_info.argtypes = [ctypes.c_void_p, ctypes.c_int, c_int_p]
        lib.sayuri_weights_tensor.restype = ctypes.c_long
        lib.sayuri_weights_tensor.argtypes = [ctypes.c_void_p, ctypes.c_char_p, c_float_p, ctypes.c_long]
        lib.sayuri_pipe_create.restype = ctypes.c_void_p
        lib.sayuri_pipe_create.argtypes = [ctypes.c_char_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                           ctypes.c_int]
        lib.sayuri_pipe_create_ex.restype = ctypes.c_void_p
        lib.sayuri_pipe_create_ex.argtypes = [ctypes.c_char_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                              ctypes.c_int, ctypes.c_uint]
        lib.sayuri_pipe_create_ens.restype = ctypes.c_void_p
        lib.sayuri_pipe_create_ens.argtypes = [ctypes.c_char_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                               ctypes.c_int, ctypes.c_uint, ctypes.c_int]
        lib.sayuri_pipe_accepts_ensemble.argtypes = [ctypes.c_void_p]
        lib.sayuri_pipe_ensemble_fallbacks.restype = ctypes.c_long
        lib.sayuri_pipe_ensemble_fallbacks.argtypes = [ctypes.c_void_p]
        lib.sayuri_pipe_forward_ensemble.argtypes = [ctypes.c_void_p, c_float_p, ctypes.c_int, ctypes.c_float, ctypes.c_int, c_float_p]
        lib.sayuri_pipe_ensemble_mix.argtypes = [ctypes.c_void_p, ctypes.c_int, c_float_p, c_int_p, c_float_p, c_int_p, c_int_p,
                                                 ctypes.c_int, c_float_p, c_int_p]
        lib.sayuri_packed_symmetry.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p]
        lib.sayuri_pipe_destroy.argtypes = [ctypes.c_void_p]
        lib.sayuri_pipe_num_workers.argtypes = [ctypes.c_void_p]
        lib.sayuri_pipe_ctx.restype = ctypes.c_void_p
        lib.sayuri_pipe_ctx.argtypes = [ctypes.c_void_p, ctypes.c_int]
        lib.sayuri_pipe_reconstruct.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int]
        lib.sayuri_pipe_eval.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, c_float_p,
                                         c_int_p, c_float_p, c_int_p, c_float_p]
        lib.sayuri_pipe_accepts_reload.argtypes = [ctypes.c_void_p]
        lib.sayuri_pipe_reload.argtypes = [ctypes.c_void_p, ctypes.c_char_p]
        lib.sayuri_pipe_weights_generation.argtypes = [ctypes.c_void_p]
        lib.sayuri_pipe_accepts_group.argtypes = [ctypes.c_void_p]
        lib.sayuri_pipe_group_eval.argtypes = [ctypes.c_void_p, ctypes.c_int, c_float_p, c_int_p, c_float_p, c_int_p, c_float_p]
        lib.sayuri_pipe_pump_times.restype = None
        lib.sayuri_pipe_pump_times.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_double),
                                               ctypes.POINTER(ctypes.c_long), ctypes.POINTER(ctypes.c_long)]
        lib.sayuri_pipe_netbench.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_double, ctypes.c_int,
                                             ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_long)]
        _host = lib
    return _host
