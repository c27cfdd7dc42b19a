"""tests/emu/emu_capi_host.cpp -- the host arithmetic of csrc/capi.hip that lives in csrc/cclqr_internal.h -- compiled for the CPU and loaded"""
import ctypes as C

from build_common import host_library


def emu_capi_host():
    """compiled for the host the way plant_tracking_common.emu_tracking_plan compiles its source"""
    lib = host_library("libemu_capi_host.so", ["emu/emu_capi_host.cpp"])
    lib.emu_k_pad.restype = C.c_longlong
    lib.emu_gain_row_overrun.restype = C.c_longlong
    lib.emu_gain_row_overrun.argtypes = [C.c_int] * 4
    lib.emu_gain_table_layout.restype = None
    lib.emu_gain_table_layout.argtypes = [C.c_int] * 4 + [C.c_longlong] * 2 + [C.POINTER(C.c_longlong)]
    lib.emu_ric_p_rows.restype = C.c_int
    lib.emu_ric_p_rows.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int]
    return lib


__all__ = ["emu_capi_host"]
