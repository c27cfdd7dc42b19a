"""tests/emu/emu_capi_host.cpp -- the host arithmetic of csrc/capi.hip that lives in csrc/cclqr_internal.h -- compiled for the CPU and loaded"""
import ctypes as C
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def emu_capi_host():
    """compiled for the host the way plant_tracking_common.emu_tracking_plan compiles its source"""
    d = os.path.join(ROOT, "tests", "emu")
    so, src = os.path.join(d, "libemu_capi_host.so"), os.path.join(d, "emu_capi_host.cpp")
    csrc = os.path.join(ROOT, "constrainedcontrol.jl_amd", "csrc")
    deps = [src] + [os.path.join(csrc, h) for h in ("cclqr_dev.h", "cclqr_internal.h")]
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(f) for f in deps):
        subprocess.check_call(["/opt/rocm/bin/hipcc", "-O2", "-std=c++17", "-fPIC", "-ffp-contract=off", "--offload-arch=gfx950", "-shared", "-o", so, src])
    lib = C.CDLL(so)
    lib.emu_k_pad.restype = C.c_longlong
    lib.emu_gain_row_overrun.restype = C.c_longlong
    lib.emu_gain_row_overrun.argtypes = [C.c_int] * 4
    lib.emu_gain_table_layout.restype = None
    lib.emu_gain_table_layout.argtypes = [C.c_int] * 4 + [C.c_longlong] * 2 + [C.POINTER(C.c_longlong)]
    lib.emu_ric_p_rows.restype = C.c_int
    lib.emu_ric_p_rows.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int]
    return lib


__all__ = ["emu_capi_host"]
