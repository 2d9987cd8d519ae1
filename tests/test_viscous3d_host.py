"""The host side of the 3D viscous operators without a GPU: the refusals fnx_add_viscosity and fnx_set_wall_bcs_stick make before any
launch (on dummy host pointers that nothing may read), and the arguments of examples/plume.py."""
import ctypes
import importlib.util
import os

import pytest

from fluidnet_cxx_amd import build
from util import FnxGrid


def test_plume_driver_takes_viscosity():
    """examples/plume.py --viscosity NU for any --depth; the help text names the stable range of both dimensions"""
    spec = importlib.util.spec_from_file_location("plume_example", os.path.join(os.path.dirname(build.HERE), "examples", "plume.py"))
    plume = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(plume)
    assert plume.parse_args([]).viscosity == 0.0
    assert plume.parse_args(["--viscosity", "0.5"]).viscosity == 0.5
    a = plume.parse_args(["--res", "64", "--depth", "64", "--viscosity", "0.5", "--iters", "20"])
    assert (a.depth, a.viscosity) == (64, 0.5)
    with pytest.raises(SystemExit):
        plume.parse_args(["--viscosity=-0.1"])
    text = " ".join(plume.parser().format_help().split())
    assert "1/6 in 3D" in text and "1/4 in 2D" in text


def test_operator_refusals_before_any_launch():
    """fnx_add_viscosity and fnx_set_wall_bcs_stick on dummy host pointers that nothing may read: ref_quirks has no 3D form, the output
    must not alias the input, 3D addViscosity takes whole grids only -- each with its code and text; and a 2D grid is not refused for
    ref_quirks (the flag is 3D only)"""
    build.build_all()
    lib = ctypes.CDLL(build.LIB)
    lib.fnx_last_error.restype = ctypes.c_char_p
    vp, cf = ctypes.c_void_p, ctypes.c_float
    G = ctypes.POINTER(FnxGrid)
    lib.fnx_add_viscosity.argtypes = [G, cf, vp, vp, vp, cf, vp]
    lib.fnx_set_wall_bcs_stick.argtypes = [G, vp, vp, vp, vp, vp]
    a, b, f, s = (ctypes.cast(ctypes.create_string_buffer(64), vp).value for _ in range(4))
    EINVAL = 1

    def visc(g, uin, uout):
        return lib.fnx_add_viscosity(ctypes.byref(g), 0.1, uin, uout, f, 0.5, None), lib.fnx_last_error().decode()

    def stick(g, uin, uout):
        return lib.fnx_set_wall_bcs_stick(ctypes.byref(g), uin, uout, f, s, None), lib.fnx_last_error().decode()

    g3 = dict(B=1, D=9, H=20, W=66, is3D=1)
    rc, msg = visc(FnxGrid(ref_quirks=1, **g3), a, b)
    assert rc == EINVAL and msg.startswith("add_viscosity: no 3D form with ref_quirks"), msg
    rc, msg = stick(FnxGrid(ref_quirks=1, **g3), a, b)
    assert rc == EINVAL and msg.startswith("set_wall_bcs_stick: no 3D form with ref_quirks"), msg
    for view in (dict(k_begin=2, k_end=5), dict(z_offset=3, D_global=16)):
        assert visc(FnxGrid(**g3, **view), a, b) == (EINVAL, "add_viscosity: no compute window or z-slab view (whole grids only)")
    for g in (FnxGrid(**g3), FnxGrid(B=1, D=1, H=20, W=66, ref_quirks=1)):
        assert visc(g, a, a) == (EINVAL, "add_viscosity: U_out must not alias U_in")
        assert stick(g, a, a) == (EINVAL, "set_wall_bcs_stick: U_out must not alias U_in")
    assert visc(FnxGrid(**g3), None, b) == (EINVAL, "add_viscosity: NULL tensor")
