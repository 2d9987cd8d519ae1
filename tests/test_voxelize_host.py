"""3D obstacles from geometry without a GPU: the C ABI's checks (before anything reads a pointer), the voxeliser's workspace size, the OBJ
reader, the driver's --obstacle option and the resources the kernels compile to for gfx950."""
import ctypes
import importlib.util
import os
import re
import subprocess

import numpy as np
import pytest

from fluidnet_cxx_amd import build
from util import FnxGrid

REPO = os.path.dirname(build.HERE)


@pytest.fixture(scope="module")
def lib():
    build.build_all()
    lib = ctypes.CDLL(build.LIB)
    lib.fnx_last_error.restype = ctypes.c_char_p
    lib.fnx_abi_version.restype = ctypes.c_int
    vp, G, dbl, flt, i32 = ctypes.c_void_p, ctypes.POINTER(FnxGrid), ctypes.c_double, ctypes.c_float, ctypes.c_int
    lib.fnx_create_sphere.restype = i32
    lib.fnx_create_sphere.argtypes = [G, vp, dbl, dbl, dbl, dbl, i32, vp]
    lib.fnx_create_box3d.restype = i32
    lib.fnx_create_box3d.argtypes = [G, vp, flt, flt, flt, flt, flt, flt, i32, vp]
    lib.fnx_voxelize_mesh_ws_bytes.restype = ctypes.c_size_t
    lib.fnx_voxelize_mesh_ws_bytes.argtypes = [G]
    lib.fnx_voxelize_mesh.restype = i32
    lib.fnx_voxelize_mesh.argtypes = [G, vp, vp, i32, vp, i32, i32, vp, vp, ctypes.c_size_t, vp]
    return lib


def _header():
    return open(os.path.join(REPO, "include", "fluidnet_hip.h")).read()


def _code(name):
    return int(re.search(name + r" = (\d+)", _header()).group(1))


def test_abi_version_and_symbols(lib):
    want = int(re.search(r"#define FNX_ABI_VERSION (\d+)", _header()).group(1))
    assert want >= 36 and lib.fnx_abi_version() == want
    for name in ("fnx_create_sphere", "fnx_create_box3d", "fnx_voxelize_mesh_ws_bytes", "fnx_voxelize_mesh"):
        assert hasattr(lib, name) and name + "(" in _header()


def test_workspace_formula(lib):
    """one toggle bit per (k, j, i0), i0 in 0..W, in 32-bit words by rows, plus the two counters; the face count does not enter"""
    for D, H, W in ((3, 3, 3), (4, 6, 31), (4, 6, 32), (4, 6, 33), (4, 6, 63), (4, 6, 64), (3, 5, 2100), (12, 20, 36), (256, 256, 256)):
        for B in (1, 3):
            g = FnxGrid(B=B, D=D, H=H, W=W, is3D=1)
            assert lib.fnx_voxelize_mesh_ws_bytes(ctypes.byref(g)) == (D * H * -(-(W + 1) // 32) + 2) * 4, (B, D, H, W)
    for g, what in ((FnxGrid(B=1, D=1, H=16, W=16, is3D=0), "3D grids only"),
                    (FnxGrid(B=1, D=8, H=16, W=16, is3D=1, k_begin=2, k_end=6), "whole domains only"),
                    (FnxGrid(B=1, D=8, H=16, W=16, is3D=1, z_offset=2, D_global=16), "whole domains only"),
                    (FnxGrid(B=1, D=2, H=16, W=16, is3D=1), "D >= 3")):
        assert lib.fnx_voxelize_mesh_ws_bytes(ctypes.byref(g)) == 0
        assert what in lib.fnx_last_error().decode()
    assert lib.fnx_voxelize_mesh_ws_bytes(None) == 0 and "NULL" in lib.fnx_last_error().decode()


def test_entry_point_checks_before_the_device(lib):
    """each bad call is refused with its own message, on host pointers (nothing may read them)"""
    vp = ctypes.c_void_p
    flags, verts, faces, report, ws = (ctypes.cast(ctypes.create_string_buffer(64), vp) for _ in range(5))
    g3 = lambda **kw: FnxGrid(**dict(dict(B=2, D=8, H=16, W=16, is3D=1), **kw))      # noqa: E731
    g2 = FnxGrid(B=1, D=1, H=16, W=16, is3D=0)
    need = lib.fnx_voxelize_mesh_ws_bytes(ctypes.byref(g3()))

    def sphere(g, f=flags, sample=-1):
        return lib.fnx_create_sphere(ctypes.byref(g), f, 8.0, 8.0, 4.0, 3.0, sample, None)

    def box(g, f=flags, sample=-1):
        return lib.fnx_create_box3d(ctypes.byref(g), f, 2.0, 5.0, 2.0, 5.0, 2.0, 5.0, sample, None)

    def mesh(g, f=flags, v=verts, fc=faces, nv=4, nf=4, sample=-1, rep=report, w=ws, wbytes=need):
        return lib.fnx_voxelize_mesh(ctypes.byref(g), f, v, nv, fc, nf, sample, rep, w, wbytes, None)

    def refused(rc, code, what):
        assert rc == _code(code), (what, rc, lib.fnx_last_error())
        assert re.search(what, lib.fnx_last_error().decode()), (what, lib.fnx_last_error())

    for call, name in ((sphere, "create_sphere"), (box, "create_box3d"), (mesh, "voxelize_mesh")):
        refused(call(g3(), f=None), "FNX_EINVAL", name + ": NULL tensor")
        refused(call(g2), "FNX_EINVAL", name + ": 3D grids only")
        refused(call(g3(k_begin=2, k_end=6)), "FNX_EINVAL", name + ": whole domains only, not a compute window or a z-slab view")
        refused(call(g3(z_offset=2, D_global=16)), "FNX_EINVAL", name + ": whole domains only, not a compute window or a z-slab view")
        refused(call(g3(), sample=2), "FNX_EINVAL", name + ": sample 2 out of range for B=2")
        refused(call(g3(), sample=-2), "FNX_EINVAL", name + ": sample -2 out of range")
        refused(call(g3(D=2)), "FNX_EINVAL", "D >= 3")
        refused(call(g3(H=2)), "FNX_EINVAL", "Dimension mismatch")
    refused(mesh(g3(), v=None), "FNX_EINVAL", "voxelize_mesh: NULL tensor")
    refused(mesh(g3(), fc=None), "FNX_EINVAL", "voxelize_mesh: NULL tensor")
    refused(mesh(g3(), nf=-1), "FNX_EINVAL", "n_faces=-1 must not be negative")
    refused(mesh(g3(), nv=-3), "FNX_EINVAL", "n_vertices=-3")
    refused(mesh(g3(), wbytes=need - 1), "FNX_EWORKSPACE", "voxelize_mesh: workspace too small")
    refused(mesh(g3(), w=None), "FNX_EWORKSPACE", "voxelize_mesh: workspace too small")
    refused(mesh(g3(), w=vp(ws.value + 2)), "FNX_EINVAL", "4-byte aligned")
    assert lib.fnx_create_sphere(None, flags, 1.0, 1.0, 1.0, 1.0, -1, None) == _code("FNX_EINVAL") and "NULL" in lib.fnx_last_error().decode()
    assert lib.fnx_voxelize_mesh(None, flags, verts, 1, faces, 1, -1, None, ws, need, None) == _code("FNX_EINVAL")


def test_python_surface():
    import inspect
    from fluidnet_cxx_amd import fluid
    from fluidnet_cxx_amd._ext import ext
    names = lambda f: list(inspect.signature(f).parameters)       # noqa: E731
    assert names(fluid.createSphere) == ["batch_dict", "centerX", "centerY", "centerZ", "radius", "sample"]
    assert names(fluid.createBox3D) == ["batch_dict", "x0", "x1", "y0", "y1", "z0", "z1", "sample"]
    assert names(fluid.voxelizeMesh) == ["batch_dict", "vertices", "faces", "sample", "check"]
    assert inspect.signature(fluid.voxelizeMesh).parameters["check"].default is True
    assert all(inspect.signature(f).parameters["sample"].default is None for f in (fluid.createSphere, fluid.createBox3D, fluid.voxelizeMesh))
    for name in ("createSphere", "createBox3D", "voxelizeMesh", "load_obj"):
        assert name in fluid.__all__
    for name in ("create_sphere_", "create_box3d_", "voxelize_mesh_", "voxelize_mesh_ws_bytes"):
        assert hasattr(ext, name)
    # the 2D generators keep their signatures
    assert names(fluid.createCylinder) == ["batch_dict", "centerX", "centerY", "radius"]
    assert names(fluid.createBox2D) == ["batch_dict", "x0", "x1", "y0", "y1"]


def test_load_obj_round_trip(tmp_path):
    from fluidnet_cxx_amd import fluid
    import voxel_reference as VR
    v, f = VR.placed(VR.icosphere(1), 2.5, (4.0, 5.0, 6.0))
    path = tmp_path / "ball.obj"
    with open(path, "w") as fh:
        fh.write("# a comment\no ball\n")
        for p in v:
            fh.write("v %s %s %s\n" % tuple(repr(float(t)) for t in p))
        fh.write("vn 0 0 1\nvt 0.5 0.5\ns off\n\n")
        for n, t in enumerate(f):
            fh.write("f %d %d %d\n" % tuple(t + 1) if n % 2 else "f %d/1/1 %d//1 %d/1\n" % tuple(t + 1))
    v2, f2 = fluid.load_obj(str(path))
    assert v2.dtype == np.float32 and f2.dtype == np.int32
    assert np.array_equal(v2, v) and np.array_equal(f2, f)
    # a quad, a pentagon (fans) and indices relative to the end
    path = tmp_path / "poly.obj"
    path.write_text("v 0 0 0\nv 1 0 0\nv 1 1 0\nv 0 1 0\nv 0.5 1.5 0\nf 1 2 3 4\nf 1 2 3 5 4\nf -5 -4 -3\nl 1 2\n")
    v3, f3 = fluid.load_obj(str(path))
    assert v3.shape == (5, 3)
    assert f3.tolist() == [[0, 1, 2], [0, 2, 3], [0, 1, 2], [0, 2, 4], [0, 4, 3], [0, 1, 2]]
    empty = tmp_path / "empty.obj"
    empty.write_text("# nothing\n")
    v4, f4 = fluid.load_obj(str(empty))
    assert v4.shape == (0, 3) and f4.shape == (0, 3)


def test_plume_driver_takes_an_obstacle():
    spec = importlib.util.spec_from_file_location("plume_example", os.path.join(REPO, "examples", "plume.py"))
    plume = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(plume)
    assert plume.parse_args([]).obstacle is None and plume.parse_args(["--depth", "16"]).obstacle is None
    for what in ("sphere", "box", "some/wing.obj", "UPPER.OBJ"):
        assert plume.parse_args(["--depth", "16", "--obstacle", what]).obstacle == what
    for bad in (["--obstacle", "sphere"], ["--obstacle", "box", "--depth", "1"], ["--obstacle", "wing.obj"],
                ["--obstacle", "cone", "--depth", "16"], ["--obstacle", "wing.stl", "--depth", "16"]):
        with pytest.raises(SystemExit):
            plume.parse_args(bad)


def test_kernels_use_no_scratch(tmp_path):
    """the unit compiles for gfx950 without scratch or VGPR spills (build_lib refuses a spilling build too); prints what hipcc reports"""
    unit = "fnx_voxelize.hip"
    assert "-ffp-contract=off" in build.HIP_UNITS[unit] and "-Rpass-analysis=kernel-resource-usage" in build.HIP_UNITS[unit]
    kernels, _ = build.SCRATCH_FREE[unit]
    want = {"geometry3d_kernel": 2, "voxel_faces_kernel": 1, "voxel_fill_kernel": 1}       # sphere and box
    assert sorted(kernels) == sorted(want)
    src = open(os.path.join(build.CSRC, unit)).read()
    assert sorted(set(re.findall(r"__global__[^\n]*void (\w+)\(", src))) == sorted(want), "every kernel of the unit is on the list"
    cmd = ([build.HIPCC] + build.COMMON + build.HIP_UNITS[unit] +
           ["--cuda-device-only", "-c", os.path.join(build.CSRC, unit), "-o", str(tmp_path / "voxelize.o")])
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert p.returncode == 0, p.stdout[-4000:]
    for kernel in kernels:
        bad, seen = build._scratch_users(p.stdout, kernel)
        assert seen == want[kernel], f"{kernel}: {want[kernel]} instantiations, saw {seen} remarks"
        assert not bad, f"{kernel} uses scratch / spills VGPRs: {bad}"
        for name, vgprs, occ in re.findall(r"Function Name: (\S*" + kernel + r"\S*).*?VGPRs: (\d+).*?Occupancy \[waves/SIMD\]: (\d+)", p.stdout, re.S):
            print(f"\n{name}: {vgprs} VGPRs, {occ} waves/SIMD")
