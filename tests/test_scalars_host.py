"""Passive scalars without a GPU: the C ABI's checks (before anything reads a pointer), the workspace size, the refusal of the z-slab
drivers, the driver's --dyes option and the resources the kernels compile to for gfx950."""
import ctypes
import importlib.util
import os
import re
import subprocess

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
    vp = ctypes.c_void_p
    lib.fnx_advect_scalars_workspace_bytes.restype = ctypes.c_size_t
    lib.fnx_advect_scalars_workspace_bytes.argtypes = [ctypes.POINTER(FnxGrid), ctypes.c_int]
    lib.fnx_advect_scalars.restype = ctypes.c_int
    lib.fnx_advect_scalars.argtypes = [ctypes.POINTER(FnxGrid), ctypes.c_float, ctypes.c_int, vp, vp, vp, vp, ctypes.c_int, ctypes.c_int,
                                       ctypes.c_int, ctypes.c_float, vp, ctypes.c_size_t, vp]
    return lib


def _header():
    return open(os.path.join(REPO, "include", "fluidnet_hip.h")).read()


def _code(name):
    return int(re.search(name + r" = (\d+)", _header()).group(1))


def test_abi_version_and_symbols(lib):
    want = int(re.search(r"#define FNX_ABI_VERSION (\d+)", _header()).group(1))
    assert want >= 28 and lib.fnx_abi_version() == want
    assert hasattr(lib, "fnx_advect_scalars") and hasattr(lib, "fnx_advect_scalars_workspace_bytes")


def test_entry_point_checks_before_the_device(lib):
    """each bad call is refused with its own message, on host pointers (nothing may read them)"""
    vp = ctypes.c_void_p
    src, U, flags, dst, ws = (ctypes.cast(ctypes.create_string_buffer(64), vp) for _ in range(5))
    g2 = lambda **kw: FnxGrid(**dict(dict(B=1, D=1, H=16, W=16, is3D=0), **kw))      # noqa: E731
    g3 = lambda **kw: FnxGrid(**dict(dict(B=1, D=8, H=16, W=16, is3D=1), **kw))      # noqa: E731
    MAC, EULER = 1, 0

    def call(g, channels=3, s=src, u=U, f=flags, d=dst, method=MAC, bnd=1, w=ws, wbytes=1 << 30):
        return lib.fnx_advect_scalars(ctypes.byref(g), 0.1, channels, s, u, f, d, method, bnd, 0, 0.75, w, wbytes, None)

    def refused(rc, code, what):
        assert rc == _code(code), (what, rc, lib.fnx_last_error())
        assert re.search(what, lib.fnx_last_error().decode()), (what, lib.fnx_last_error())

    for g in (g2(), g3()):
        for kw in (dict(s=None), dict(u=None), dict(f=None), dict(d=None)):
            refused(call(g, **kw), "FNX_EINVAL", "advect_scalars: NULL tensor")
        refused(call(g, channels=0), "FNX_EINVAL", "channels < 1")
        refused(call(g, channels=-2), "FNX_EINVAL", "channels < 1")
        refused(call(g, d=src), "FNX_EINVAL", "dst must not alias src")
        refused(call(g, method=2), "FNX_EMETHOD", "Advection method not supported")
        refused(call(g, bnd=2), "FNX_EINVAL", "boundary_width == 1")
        need = lib.fnx_advect_scalars_workspace_bytes(ctypes.byref(g), 3)
        refused(call(g, wbytes=need - 1), "FNX_EWORKSPACE", "advect_scalars: workspace too small")
        refused(call(g, w=None), "FNX_EWORKSPACE", "advect_scalars: workspace too small")
    refused(call(g3(k_begin=2, k_end=6)), "FNX_EINVAL", "single-domain")
    refused(call(g3(z_offset=2, D_global=16)), "FNX_EINVAL", "single-domain")
    refused(call(g3(k_begin=2, k_end=6), method=EULER), "FNX_EINVAL", "single-domain")
    refused(call(g2(H=2)), "FNX_EINVAL", "Dimension mismatch")
    refused(call(g3(B=8, D=4096, H=4, W=4), channels=33), "FNX_EINVAL", r"B\*channels\*ceil\(D/16\) > 65535")
    assert lib.fnx_advect_scalars(None, 0.1, 1, src, U, flags, dst, MAC, 1, 0, 0.75, ws, 1 << 30, None) == _code("FNX_EINVAL")
    assert "NULL" in lib.fnx_last_error().decode()


def test_workspace_grows_with_the_channels(lib):
    for g in (FnxGrid(B=2, D=1, H=20, W=33, is3D=0), FnxGrid(B=2, D=9, H=12, W=70, is3D=1)):
        n = g.B * g.D * g.H * g.W
        sizes = [lib.fnx_advect_scalars_workspace_bytes(ctypes.byref(g), c) for c in (1, 2, 5, 8)]
        assert sizes[0] >= (4 if g.is3D else 2) * 4 * n > 0                    # a forward field, the traced cell, 3D: 8-byte clamp bounds
        assert all(b > a for a, b in zip(sizes, sizes[1:]))
        assert sizes[3] - sizes[0] > 7 * 4 * n - 256                          # a forward field per channel (sizes round up to 256)
        assert lib.fnx_advect_scalars_workspace_bytes(ctypes.byref(g), 0) == 0
    win = FnxGrid(B=1, D=8, H=16, W=16, is3D=1, k_begin=2, k_end=6)
    assert lib.fnx_advect_scalars_workspace_bytes(ctypes.byref(win), 2) == 0
    assert "single-domain" in lib.fnx_last_error().decode()


def test_existing_workspace_sizes_are_untouched(lib):
    """the step's and the operators' workspaces are fnx_advect.hip's own: the new unit adds nothing to them"""
    src = open(os.path.join(build.CSRC, "fnx_api.hip")).read()
    assert "advect_scalars_workspace" not in src[src.index("fnx::StepLayout carve_step"):src.index("size_t ws_step")]
    body = src[src.index("size_t fnx_workspace_bytes"):src.index("static int advect_run")]
    assert "scalars" not in body


def test_python_surface_and_slab_refusal(lib):
    import inspect
    from fluidnet_cxx_amd import fluid, slab
    from fluidnet_cxx_amd._ext import ext
    sig = inspect.signature(fluid.advectScalars)
    assert [n for n, p in sig.parameters.items() if p.kind is not p.KEYWORD_ONLY] == [
        "dt", "src", "U", "flags", "method", "boundary_width", "sample_outside_fluid", "maccormack_strength"]
    assert [n for n, p in sig.parameters.items() if p.kind is p.KEYWORD_ONLY] == ["geom"]
    assert sig.parameters["maccormack_strength"].default == 0.75 and sig.parameters["method"].default == "maccormackFluidNet"
    assert "advectScalars" in fluid.__all__ and hasattr(ext, "advect_scalars")
    cfg = dict(dt=0.1, pTol=0.0, jacobiIter=4)
    lay = slab.SlabLayout(16, 1, 0, 5)
    for sim in (slab.NativeSlabSimulator(lay, cfg), slab.SlabSimulator(lay, cfg, ops=object())):
        with pytest.raises(ValueError, match="single-domain only"):
            sim.step(dict(scalars=None))


def test_plume_driver_takes_dyes():
    spec = importlib.util.spec_from_file_location("plume_example", os.path.join(REPO, "examples", "plume.py"))
    plume = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(plume)
    assert plume.parse_args([]).dyes is None
    for n in (1, 2, 3):
        assert plume.parse_args(["--dyes", str(n)]).dyes == n
    for bad in ("0", "4", "-1"):
        with pytest.raises(SystemExit):
            plume.parse_args(["--dyes=" + bad])


def test_kernels_use_no_scratch(tmp_path):
    """every instantiation (2D; 3D with and without quirks; both sample_outside modes) compiles for gfx950 without scratch or VGPR
    spills (build_lib refuses a spilling build too); prints what hipcc reports"""
    unit = "fnx_scalars.hip"
    assert "-ffp-contract=off" in build.HIP_UNITS[unit] and "-Rpass-analysis=kernel-resource-usage" in build.HIP_UNITS[unit]
    kernels, _ = build.SCRATCH_FREE[unit]
    # instantiations: forward / backward 2D x 2 and 3D x 2 x 2 (quirks, sample_outside).  The 3D clamp-bounds reduction is fnx_advect.hip's
    # box_minmax_kernel: tests/test_advect3d_resources.py makes this check of its two instantiations
    want = {"advect_scalars_fwd_kernel": 6, "advect_scalars_bwd_kernel": 6}
    assert sorted(kernels) == sorted(want)
    assert "box_minmax_kernel" in build.SCRATCH_FREE["fnx_advect.hip"][0]
    cmd = ([build.HIPCC] + build.COMMON + build.HIP_UNITS[unit] +
           ["--cuda-device-only", "-c", os.path.join(build.CSRC, unit), "-o", str(tmp_path / "scalars.o")])
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert p.returncode == 0, p.stdout[-4000:]
    for kernel in kernels:
        bad, seen = build._scratch_users(p.stdout, kernel)
        assert seen == want[kernel], f"{kernel}: {want[kernel]} instantiations, saw {seen} remarks"
        assert not bad, f"{kernel} uses scratch / spills VGPRs: {bad}"
        for name, vgprs, occ in re.findall(r"Function Name: (\S*" + kernel + r"\S*).*?VGPRs: (\d+).*?Occupancy \[waves/SIMD\]: (\d+)", p.stdout, re.S):
            print(f"\n{name}: {vgprs} VGPRs, {occ} waves/SIMD")
