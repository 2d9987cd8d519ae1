"""The sizes and layouts the MultiScale net's host code hands to its callers, and the refusals of its entry points (no GPU: nothing here
reaches the device).  Callers size and keep weight images, tapes and workspaces, so these numbers are part of the ABI.  Every literal
below was read from the library of the commit BEFORE the net's plan, blob offsets, tower sizes and workspace layout became one statement
each (ABI 35), through the same ctypes calls; the other tests hold the same quantities to a rule, this one to the value."""
import ctypes
import os
import re

import pytest

from fluidnet_cxx_amd import build
from util import FnxGrid as _FnxGrid

vp, sz, ci = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int
HDR = open(os.path.join(os.path.dirname(build.HERE), "include", "fluidnet_hip.h")).read()


def _enum(name):
    return int(re.search(name + r" = (\d+)", HDR).group(1))


N_TAPE = 19


class _Entry(ctypes.Structure):
    _fields_ = [("name", ctypes.c_char * 8), ("offset", sz), ("C", ci), ("H", ci), ("W", ci)]


class _Entry3D(ctypes.Structure):
    _fields_ = [("name", ctypes.c_char * 8), ("offset", sz), ("C", ci), ("D", ci), ("H", ci), ("W", ci)]


# the images: floats of the blob, bytes of the packed and of the transposed image, for 2D and 3D
IMAGES = {"weight_floats": (418643, 1276755), "packed_bytes": (12622080, 38030592), "packed_t_bytes": (14793984, 43572480)}
# (B, D, H, W) -> fnx_workspace_bytes(FNX_OP_FLUIDNET), the backward's and the training forward + backward's workspace, the tape's floats
# and every entry's (name, offset, C, [D,] H, W)
SIZES = {
    (2, 1, 37, 53): {
        "fluidnet_ws": 4177664, "backward_ws": 22911232, "train_ws": 23005952, "tape_floats": 1633280,
        "tape": [("xq", 0, 2, 9, 13), ("y0", 512, 32, 9, 13), ("y1", 8000, 64, 9, 13), ("y2", 22976, 32, 9, 13), ("y3", 30464, 1, 9, 13),
                 ("in2", 30720, 3, 18, 26), ("y4", 33536, 32, 18, 26), ("y5", 63488, 64, 18, 26), ("y6", 123392, 128, 18, 26),
                 ("y7", 243200, 64, 18, 26), ("y8", 303104, 32, 18, 26), ("y9", 333056, 1, 18, 26), ("in1", 334016, 3, 37, 53),
                 ("y10", 345792, 32, 37, 53), ("y11", 471296, 64, 37, 53), ("y12", 722304, 128, 37, 53), ("y13", 1224320, 64, 37, 53),
                 ("y14", 1475328, 32, 37, 53), ("y15", 1600832, 8, 37, 53)]},
    (1, 1, 4, 4): {
        "fluidnet_ws": 35072, "backward_ws": 18891520, "train_ws": 18892544, "tape_floats": 8064,
        "tape": [("xq", 0, 2, 1, 1), ("y0", 64, 32, 1, 1), ("y1", 128, 64, 1, 1), ("y2", 192, 32, 1, 1), ("y3", 256, 1, 1, 1),
                 ("in2", 320, 3, 2, 2), ("y4", 384, 32, 2, 2), ("y5", 512, 64, 2, 2), ("y6", 768, 128, 2, 2), ("y7", 1280, 64, 2, 2),
                 ("y8", 1536, 32, 2, 2), ("y9", 1664, 1, 2, 2), ("in1", 1728, 3, 4, 4), ("y10", 1792, 32, 4, 4), ("y11", 2304, 64, 4, 4),
                 ("y12", 3328, 128, 4, 4), ("y13", 5376, 64, 4, 4), ("y14", 6400, 32, 4, 4), ("y15", 6912, 8, 4, 4)]},
    (2, 6, 10, 37): {
        "fluidnet_ws": 4714240, "backward_ws": 23441408, "train_ws": 23584256, "tape_floats": 1650560,
        "tape": [("xq", 0, 2, 1, 2, 9), ("y0", 128, 32, 1, 2, 9), ("y1", 1280, 64, 1, 2, 9), ("y2", 3584, 32, 1, 2, 9), ("y3", 4736, 1, 1, 2, 9),
                 ("in2", 4800, 3, 3, 5, 18), ("y4", 6464, 32, 3, 5, 18), ("y5", 23744, 64, 3, 5, 18), ("y6", 58304, 128, 3, 5, 18),
                 ("y7", 127424, 64, 3, 5, 18), ("y8", 161984, 32, 3, 5, 18), ("y9", 179264, 1, 3, 5, 18), ("in1", 179840, 3, 6, 10, 37),
                 ("y10", 193216, 32, 6, 10, 37), ("y11", 335296, 64, 6, 10, 37), ("y12", 619456, 128, 6, 10, 37), ("y13", 1187776, 64, 6, 10, 37),
                 ("y14", 1471936, 32, 6, 10, 37), ("y15", 1614016, 8, 6, 10, 37)]},
    (1, 4, 4, 4): {
        "fluidnet_ws": 84992, "backward_ws": 18940672, "train_ws": 18942720, "tape_floats": 25216,
        "tape": [("xq", 0, 2, 1, 1, 1), ("y0", 64, 32, 1, 1, 1), ("y1", 128, 64, 1, 1, 1), ("y2", 192, 32, 1, 1, 1), ("y3", 256, 1, 1, 1, 1),
                 ("in2", 320, 3, 2, 2, 2), ("y4", 384, 32, 2, 2, 2), ("y5", 640, 64, 2, 2, 2), ("y6", 1152, 128, 2, 2, 2),
                 ("y7", 2176, 64, 2, 2, 2), ("y8", 2688, 32, 2, 2, 2), ("y9", 2944, 1, 2, 2, 2), ("in1", 3008, 3, 4, 4, 4),
                 ("y10", 3200, 32, 4, 4, 4), ("y11", 5248, 64, 4, 4, 4), ("y12", 9344, 128, 4, 4, 4), ("y13", 17536, 64, 4, 4, 4),
                 ("y14", 21632, 32, 4, 4, 4), ("y15", 23680, 8, 4, 4, 4)]},
}


@pytest.fixture(scope="module")
def lib():
    build.build_all()
    lib = ctypes.CDLL(build.LIB)
    lib.fnx_last_error.restype = ctypes.c_char_p
    G = ctypes.POINTER(_FnxGrid)
    for f in ("fnx_scalenet_weight_floats", "fnx_scalenet_packed_bytes"):
        getattr(lib, f).restype, getattr(lib, f).argtypes = sz, [ci]
    for f in ("fnx_scalenet_packed_t_bytes", "fnx_scalenet3d_packed_t_bytes"):
        getattr(lib, f).restype, getattr(lib, f).argtypes = sz, []
    for f in ("fnx_multiscale_backward_ws_bytes", "fnx_multiscale3d_backward_ws_bytes", "fnx_fluidnet_train_ws_bytes", "fnx_fluidnet3d_train_ws_bytes"):
        getattr(lib, f).restype, getattr(lib, f).argtypes = sz, [G]
    lib.fnx_workspace_bytes.restype, lib.fnx_workspace_bytes.argtypes = sz, [G, ci]
    lib.fnx_multiscale_tape_layout.restype, lib.fnx_multiscale_tape_layout.argtypes = sz, [G, ctypes.POINTER(_Entry)]
    lib.fnx_multiscale3d_tape_layout.restype, lib.fnx_multiscale3d_tape_layout.argtypes = sz, [G, ctypes.POINTER(_Entry3D)]
    lib.fnx_multiscale_forward.argtypes = [G, vp, vp, vp, ci, vp, sz, vp]
    lib.fnx_multiscale_forward_crop.argtypes = [G, vp, vp, vp, ci, ctypes.POINTER(ci), vp, sz, vp]
    lib.fnx_fluidnet_forward.argtypes = [G, vp, vp, ctypes.c_float, vp, vp, ci, vp, sz, vp]
    return lib


def measure_images(lib):
    return {"weight_floats": (lib.fnx_scalenet_weight_floats(0), lib.fnx_scalenet_weight_floats(1)),
            "packed_bytes": (lib.fnx_scalenet_packed_bytes(0), lib.fnx_scalenet_packed_bytes(1)),
            "packed_t_bytes": (lib.fnx_scalenet_packed_t_bytes(), lib.fnx_scalenet3d_packed_t_bytes())}


def measure_sizes(lib, shape):
    B, D, H, W = shape
    is3d = D > 1
    g = _FnxGrid(B=B, D=D, H=H, W=W, is3D=int(is3d))
    r = ctypes.byref(g)
    entries = ((_Entry3D if is3d else _Entry) * N_TAPE)()
    floats = (lib.fnx_multiscale3d_tape_layout if is3d else lib.fnx_multiscale_tape_layout)(r, entries)
    dims = (lambda e: (e.C, e.D, e.H, e.W)) if is3d else (lambda e: (e.C, e.H, e.W))
    return {"fluidnet_ws": lib.fnx_workspace_bytes(r, _enum("FNX_OP_FLUIDNET")),
            "backward_ws": (lib.fnx_multiscale3d_backward_ws_bytes if is3d else lib.fnx_multiscale_backward_ws_bytes)(r),
            "train_ws": (lib.fnx_fluidnet3d_train_ws_bytes if is3d else lib.fnx_fluidnet_train_ws_bytes)(r),
            "tape_floats": floats,
            "tape": [(e.name.decode(), e.offset) + dims(e) for e in entries]}


def test_image_sizes(lib):
    assert measure_images(lib) == IMAGES


@pytest.mark.parametrize("shape", sorted(SIZES))
def test_workspace_and_tape_layouts(lib, shape):
    assert measure_sizes(lib, shape) == SIZES[shape]


def test_refusal_texts(lib):
    """before any device call (host memory here): the crop's own refusals and a workspace that is too small, word for word"""
    a = ctypes.cast(ctypes.create_string_buffer(64), vp)
    einval, ews = _enum("FNX_EINVAL"), _enum("FNX_EWORKSPACE")
    big = 1 << 40

    def crop(g, trim, ws_bytes=big):
        rc = lib.fnx_multiscale_forward_crop(ctypes.byref(g), a, a, a, 0, (ci * 4)(*trim), a, ws_bytes, None)
        return rc, lib.fnx_last_error().decode()

    g3 = _FnxGrid(B=1, D=24, H=12, W=37, is3D=1)
    assert crop(g3, [8, 3, 4, 0]) == (einval, "multiscale_forward_crop: trim[1] = 3 must be a non-negative multiple of 4")
    assert crop(g3, [8, 4, -4, 0]) == (einval, "multiscale_forward_crop: trim[2] = -4 must be a non-negative multiple of 4")
    assert crop(g3, [4, 4, 8, 0]) == (einval, "multiscale_forward_crop: the half-resolution window must contain the full-resolution one")
    assert crop(g3, [8, 4, 4, 8]) == (einval, "multiscale_forward_crop: the half-resolution window must contain the full-resolution one")
    assert crop(g3, [12, 12, 0, 0]) == (einval, "multiscale_forward_crop: D = 24 must be a multiple of 4 and leave at least 4 planes (trims 12 + 12)")
    assert crop(_FnxGrid(B=1, D=22, H=12, W=37, is3D=1), [4, 0, 0, 0]) == (
        einval, "multiscale_forward_crop: D = 22 must be a multiple of 4 and leave at least 4 planes (trims 4 + 0)")
    assert crop(_FnxGrid(B=1, D=1, H=12, W=37), [4, 0, 0, 0]) == (einval, "multiscale_forward_crop: z windows need a 3D grid")
    assert crop(g3, [8, 4, 4, 0], ws_bytes=4096) == (ews, "fnx_multiscale_forward_crop: workspace of 4096 bytes is too small")
    g2 = _FnxGrid(B=2, D=1, H=37, W=53)
    assert lib.fnx_multiscale_forward(ctypes.byref(g2), a, a, a, 0, a, 0, None) == ews
    assert lib.fnx_last_error().decode() == "fnx_multiscale_forward: workspace of 0 bytes is too small"
    need = lib.fnx_workspace_bytes(ctypes.byref(g2), _enum("FNX_OP_FLUIDNET"))
    assert lib.fnx_fluidnet_forward(ctypes.byref(g2), a, a, 1e-3, a, a, 0, a, need - 1, None) == ews
    assert lib.fnx_last_error().decode() == f"fnx_fluidnet_forward: workspace of {need - 1} bytes is too small"
    # the order of the shared checks: null argument, precision mode, the net's smallest grid, then the workspace
    assert lib.fnx_fluidnet_forward(ctypes.byref(g2), None, a, 1e-3, a, a, 0, a, 0, None) == einval
    assert lib.fnx_last_error().decode() == "fnx_fluidnet_forward: null argument"
    assert lib.fnx_multiscale_forward(ctypes.byref(g2), a, a, a, 99, a, 0, None) == einval
    assert lib.fnx_last_error().decode() == ("fnx_multiscale_forward: unknown precision_mode 99 (FNX_PRECISION_FP32, _FP32_DIRECT, _BF16X6, "
                                             "_BF16X3, _FP32_F4 or _FP32_F2)")
    assert lib.fnx_multiscale_forward(ctypes.byref(_FnxGrid(B=1, D=1, H=3, W=8)), a, a, a, 0, a, 0, None) == einval
    assert lib.fnx_last_error().decode() == "fnx_multiscale_forward: the three-scale net needs at least 4 cells per axis (D 1, H 3, W 8)"
