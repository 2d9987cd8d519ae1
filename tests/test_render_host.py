"""Volume rendering without a GPU: the numpy statement of the arithmetic (tests/render_reference.py) against independent statements of
it, the C ABI's checks (before anything reads a pointer), the resources the kernels compile to for gfx950, and the driver's arguments."""
import ctypes
import importlib.util
import itertools
import os
import re
import subprocess

import numpy as np
import pytest

import render_reference as rr
from fluidnet_cxx_amd import build

REPO = os.path.dirname(build.HERE)
f32 = np.float32


@pytest.fixture(scope="module")
def built():
    build.build_all()
    return build


def _fluid(B, D, H, W):
    return np.ones((B, D, H, W), f32)


# ---- the model against independent statements ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("view", rr.DIRECTIONS)
def test_uniform_column_against_repeated_multiplication_and_the_closed_form(view):
    """uniform rho, no obstacle, headlight: T is n fp32 multiplications by (1 - a); C agrees with the float64 closed form
    sum_i (T_i a)(ambient + (1 - ambient) T_i), T_i = (1 - a)^i -- with k_light = k_view the arriving light equals the transmittance"""
    shape = (1, 6, 9, 11)
    n = shape[rr._axis(view)[0]]
    rho, k = f32(0.4), f32(0.3)
    img = rr.render(np.full(shape, rho, f32), _fluid(*shape), view, view, k_view=k, k_light=k, ambient=0.25, bnd=0)
    a = f32(k * rho)
    T = f32(1)
    for _ in range(n):
        T = f32(T * f32(f32(1) - a))
    assert img.shape == (1, 2) + rr.image_shape(shape, view)
    assert (img[:, 1] == T).all()
    a64 = float(a)
    Ti = (1.0 - a64) ** np.arange(n)
    C64 = float(np.sum(Ti * a64 * (0.25 + 0.75 * Ti)))
    assert np.abs(img[:, 0].astype(np.float64) - C64).max() <= 1e-6 * C64


def test_obstacle_plane():
    """an obstacle plane at z = 3 seen along +z with the light along -y: T == 0 behind it, C the hand-computed sum"""
    shape = (1, 6, 5, 4)
    flags = _fluid(*shape)
    flags[:, 3] = rr.TYPE_OBSTACLE
    rho, kv, kl = f32(0.5), f32(0.25), f32(0.5)
    img = rr.render(np.full(shape, rho, f32), flags, "+z", "-y", k_view=kv, k_light=kl, ambient=0.25, albedo_smoke=1.0, albedo_obstacle=0.5,
                    bnd=0)
    assert (img[:, 1] == 0).all()
    H = shape[2]
    amb, oma = f32(0.25), f32(1) - f32(0.25)
    av, al = f32(kv * rho), f32(kl * rho)
    for y in range(H):
        Ls = f32(1)                                       # light arriving at row y of a smoke plane: H-1-y cells above it
        for _ in range(H - 1 - y):
            Ls = f32(Ls * f32(f32(1) - al))
        Lo = f32(1) if y == H - 1 else f32(0)             # in the obstacle plane only the top row is lit
        T, C = f32(1), f32(0)
        for _ in range(3):
            C = f32(C + f32(f32(T * av) * f32(f32(1) * f32(amb + f32(oma * Ls)))))
            T = f32(T * f32(f32(1) - av))
        C = f32(C + f32(T * f32(f32(0.5) * f32(amb + f32(oma * Lo)))))
        assert (img[0, 0, y] == C).all(), y


def test_empty_volume():
    shape = (2, 4, 5, 6)
    for view, light in (("-z", "-y"), ("+x", "+x"), ("-y", "+y")):
        img = rr.render(np.zeros(shape, f32), _fluid(*shape), view, light, bnd=1)
        assert (img[:, 0] == 0).all() and (img[:, 1] == 1).all()


def test_border_rule():
    """emptyDomain's wall is invisible with bnd = 1 and opaque with bnd = 0; a 2D grid has no z faces"""
    shape = (1, 6, 7, 8)
    flags = _fluid(*shape)
    flags[:, 0] = flags[:, -1] = rr.TYPE_OBSTACLE
    flags[:, :, 0] = flags[:, :, -1] = rr.TYPE_OBSTACLE
    flags[:, :, :, 0] = flags[:, :, :, -1] = rr.TYPE_OBSTACLE
    for view in rr.DIRECTIONS:
        seen = rr.render(np.zeros(shape, f32), flags, view, "-y", bnd=1)
        assert (seen[:, 0] == 0).all() and (seen[:, 1] == 1).all(), view
        wall = rr.render(np.zeros(shape, f32), flags, view, "-y", bnd=0)
        assert (wall[:, 1] == 0).all() and (wall[:, 0] > 0).all(), view
    flat = np.full((1, 1, 7, 8), 0.5, f32)
    img = rr.render(flat, _fluid(1, 1, 7, 8), "-z", "-z", k_view=1.0, k_light=1.0, bnd=1)
    assert (img[0, 1, 1:-1, 1:-1] == 0.5).all() and (img[0, 1, 0] == 1).all() and (img[0, 1, :, 0] == 1).all()


def _case(shape, seed=0):
    rng = np.random.default_rng(seed)
    density = rng.uniform(-0.2, 1.3, shape).astype(f32)
    density[rng.random(shape) < 0.5] = 0
    flags = _fluid(*shape)
    flags[rng.random(shape) < 0.05] = rr.TYPE_OBSTACLE
    return density, flags


def permuted_direction(direction, perm):
    """the name of `direction` after the volume's (z, y, x) axes were transposed by `perm` (new axis i = old axis perm[i])"""
    old = {"z": 0, "y": 1, "x": 2}[direction[1]]
    return direction[0] + "zyx"[perm.index(old)]


@pytest.mark.parametrize("perm", list(itertools.permutations(range(3))))
def test_model_symmetry(perm):
    """permuting the volume's axes together with the direction names permutes the image, bit for bit"""
    shape = (2, 5, 6, 7)
    density, flags = _case(shape)
    tp = (0,) + tuple(p + 1 for p in perm)
    dp, fp = np.ascontiguousarray(density.transpose(tp)), np.ascontiguousarray(flags.transpose(tp))
    for view, light in (("-z", "-y"), ("+x", "-y"), ("+y", "+y"), ("-x", "+x"), ("+z", "+x"), ("-y", "-z")):
        # equal extents per axis are not needed: the absorptions are given, not derived from the shape
        want = rr.render(density, flags, view, light, k_view=0.9, k_light=1.7, bnd=1)
        got = rr.render(dp, fp, permuted_direction(view, perm), permuted_direction(light, perm), k_view=0.9, k_light=1.7, bnd=1)
        rest = [a for a in range(3) if "zyx"[a] != view[1]]                     # image axes of the original, as volume axes
        new_rest = sorted(perm.index(a) for a in rest)                          # ... of the permuted volume
        order = [rest.index(perm[a]) for a in new_rest]
        assert np.array_equal(got, want.transpose([0, 1] + [2 + o for o in order])), (view, light)


# ---- header and library ---------------------------------------------------------------------------------------------------------------
class _FnxGrid(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int) for n in ("B", "D", "H", "W", "is3D", "ref_quirks", "z_offset", "D_global", "k_begin", "k_end")]


class _Prm(ctypes.Structure):
    _fields_ = [("view_dir", ctypes.c_int), ("light_dir", ctypes.c_int), ("k_view", ctypes.c_float), ("k_light", ctypes.c_float),
                ("ambient", ctypes.c_float), ("one_minus_ambient", ctypes.c_float), ("albedo_smoke", ctypes.c_float),
                ("albedo_obstacle", ctypes.c_float), ("bnd", ctypes.c_int)]


def _header():
    return open(os.path.join(REPO, "include", "fluidnet_hip.h")).read()


def _prm(**kw):
    return _Prm(**dict(dict(view_dir=5, light_dir=3, k_view=0.5, k_light=0.5, ambient=0.25, one_minus_ambient=0.75, albedo_smoke=1.0,
                            albedo_obstacle=0.5, bnd=1), **kw))


def test_abi_version_symbols_and_struct(built):
    lib = ctypes.CDLL(built.LIB)
    lib.fnx_abi_version.restype = ctypes.c_int
    want = int(re.search(r"#define FNX_ABI_VERSION (\d+)", _header()).group(1))
    assert want >= 24 and lib.fnx_abi_version() == want
    assert hasattr(lib, "fnx_render_volume") and hasattr(lib, "fnx_render_volume_ws_bytes")
    body = re.search(r"typedef struct FnxRenderParams \{(.*?)\} FnxRenderParams;", _header(), re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [n for decl in re.findall(r"(?:int|float)\s+([^;]+);", body) for n in re.split(r",\s*", decl.strip())]
    assert names == [n for n, _ in _Prm._fields_]


def test_entry_point_checks_before_the_device(built):
    """each bad call is refused with FNX_EINVAL and its own message, on host pointers (nothing may read them)"""
    lib = ctypes.CDLL(built.LIB)
    lib.fnx_last_error.restype = ctypes.c_char_p
    vp = ctypes.c_void_p
    lib.fnx_render_volume.argtypes = [ctypes.POINTER(_FnxGrid), vp, vp, ctypes.POINTER(_Prm), vp, vp, ctypes.c_size_t, vp]
    lib.fnx_render_volume_ws_bytes.argtypes = [ctypes.POINTER(_FnxGrid), ctypes.POINTER(_Prm)]
    lib.fnx_render_volume_ws_bytes.restype = ctypes.c_size_t
    einval = int(re.search(r"FNX_EINVAL = (\d+)", _header()).group(1))
    rho, fl, img, ws = (ctypes.cast(ctypes.create_string_buffer(64), vp) for _ in range(4))
    g3 = lambda **kw: _FnxGrid(**dict(dict(B=1, D=8, H=16, W=16, is3D=1), **kw))       # noqa: E731
    big = 1 << 20

    def refused(g, prm, what, density=rho, flags=fl, image=img, wsp=ws, ws_bytes=big):
        rc = lib.fnx_render_volume(ctypes.byref(g) if g is not None else None, density, flags,
                                   ctypes.byref(prm) if prm is not None else None, image, wsp, ws_bytes, None)
        assert rc == einval, what
        assert re.search(what, lib.fnx_last_error().decode()), (what, lib.fnx_last_error())

    refused(g3(), _prm(), "NULL tensor", density=None)
    refused(g3(), _prm(), "NULL tensor", flags=None)
    refused(g3(), _prm(), "NULL tensor", image=None)
    refused(g3(), None, "NULL parameters")
    refused(None, _prm(), "NULL")
    for bad in (dict(view_dir=6), dict(view_dir=-1), dict(light_dir=6), dict(light_dir=-1)):
        refused(g3(), _prm(**bad), "direction outside 0..5")
    refused(g3(), _prm(bnd=-1), "bnd < 0")
    for bad in (dict(k_view=-0.5), dict(k_light=-1.0), dict(k_view=float("inf")), dict(k_light=float("nan")), dict(k_view=float("nan"))):
        refused(g3(), _prm(**bad), "finite and not negative")
    need = lib.fnx_render_volume_ws_bytes(ctypes.byref(g3()), ctypes.byref(_prm()))
    refused(g3(), _prm(), "workspace too small", ws_bytes=need - 1)
    refused(g3(), _prm(), "workspace too small", wsp=None)
    refused(g3(k_begin=2, k_end=6), _prm(), "compute window or z-slab view \\(whole grids only\\)")
    refused(g3(z_offset=2, D_global=16), _prm(), "compute window or z-slab view \\(whole grids only\\)")
    refused(g3(H=2), _prm(), "Dimension mismatch")


def test_workspace_bytes(built):
    """0 for the six headlight pairs (one march, no L in memory), one float per cell rounded up to 256 bytes otherwise"""
    lib = ctypes.CDLL(built.LIB)
    lib.fnx_render_volume_ws_bytes.argtypes = [ctypes.POINTER(_FnxGrid), ctypes.POINTER(_Prm)]
    lib.fnx_render_volume_ws_bytes.restype = ctypes.c_size_t
    for g in (_FnxGrid(B=2, D=5, H=7, W=9, is3D=1), _FnxGrid(B=1, D=1, H=37, W=53, is3D=0), _FnxGrid(B=1, D=64, H=64, W=64, is3D=1)):
        cells = g.B * g.D * g.H * g.W
        for v in range(6):
            for l in range(6):
                got = lib.fnx_render_volume_ws_bytes(ctypes.byref(g), ctypes.byref(_prm(view_dir=v, light_dir=l)))
                assert got == (0 if v == l else (4 * cells + 255) // 256 * 256), (v, l)
    assert lib.fnx_render_volume_ws_bytes(ctypes.byref(_FnxGrid(B=1, D=8, H=16, W=16, is3D=1)), ctypes.byref(_prm(view_dir=7))) == 0


def test_python_surface(built):
    import inspect
    from fluidnet_cxx_amd import fluid, output
    from fluidnet_cxx_amd._ext import ext
    sig = inspect.signature(fluid.renderVolume)
    assert [n for n, p in sig.parameters.items() if p.kind is not p.KEYWORD_ONLY] == ["density", "flags", "view", "light"]
    assert {n: p.default for n, p in sig.parameters.items() if p.kind is p.KEYWORD_ONLY} == dict(
        absorption=None, light_absorption=None, ambient=0.25, albedo_smoke=1.0, albedo_obstacle=0.5, bnd=1)
    assert sig.parameters["view"].default == "-z" and sig.parameters["light"].default == "-y"
    assert "renderVolume" in fluid.__all__ and hasattr(ext, "render_volume")
    assert tuple(fluid.ops.RENDER_DIRECTIONS) == rr.DIRECTIONS
    assert inspect.signature(output.save_state).parameters["render"].default is None
    assert inspect.signature(output.save_render).parameters["views"].default == (("-z", "-y"),)
    assert inspect.signature(output.render_image).parameters["background"].default == 1.0


# ---- build remarks ----------------------------------------------------------------------------------------------------------------------
def test_render_kernels_use_no_scratch(tmp_path):
    """every instantiation (light / view / headlight of the y-z march and of the x march) compiles for gfx950 without scratch or VGPR
    spills (build_lib refuses such a build too), and the x march's LDS tiles leave room for several workgroups per CU"""
    unit = "fnx_render.hip"
    assert "-ffp-contract=off" in build.HIP_UNITS[unit] and "-Rpass-analysis=kernel-resource-usage" in build.HIP_UNITS[unit]
    kernels, _ = build.SCRATCH_FREE[unit]
    assert kernels == ["render_march_kernel", "render_march_x_kernel"]
    cmd = ([build.HIPCC] + build.COMMON + build.HIP_UNITS[unit] +
           ["--cuda-device-only", "-c", os.path.join(build.CSRC, unit), "-o", str(tmp_path / "render.o")])
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert p.returncode == 0, p.stdout[-4000:]
    for kernel in kernels:
        bad, seen = build._scratch_users(p.stdout, kernel)
        assert seen == 3, f"one resource-usage remark per mode of {kernel}"
        assert not bad, f"{kernel} uses scratch / spills VGPRs: {bad}"
    found = re.findall(r"Function Name: \S*(render_march\w*?_kernel)\S*.*?VGPRs: (\d+).*?LDS Size \[bytes/block\]: (\d+)", p.stdout, re.S)
    assert len(found) == 6, "resource remark format"
    for name, vgprs, lds in found:
        print(f"\n{name}: {vgprs} VGPRs, {lds} B LDS")
        assert int(vgprs) <= 128
        assert int(lds) == 0 if name == "render_march_kernel" else int(lds) <= 40 * 1024


# ---- the driver's arguments -------------------------------------------------------------------------------------------------------------
def _plume_module():
    spec = importlib.util.spec_from_file_location("plume_example", os.path.join(REPO, "examples", "plume.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_driver_arguments(built, capsys):
    mod = _plume_module()
    a = mod.parse_args([])
    assert a.depth == 1 and a.render is False
    a = mod.parse_args(["--depth", "24", "--render", "--method", "pcg", "--vorticity", "0.3"])
    assert a.depth == 24 and a.render is True
    assert mod.RENDER_VIEWS == (("-z", "-y"), ("+x", "-y"))
    with pytest.raises(SystemExit):
        mod.parse_args(["--depth", "8", "--method", "convnet", "--weights", "w.pth"])
    assert "no 3D weights can be trained here" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        mod.parse_args(["--depth", "2"])
