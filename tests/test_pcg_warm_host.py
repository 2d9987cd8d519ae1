"""The warm-started pressure solve (fnx_pcg_from, FnxStepParams.method 3 'hybrid' and 4) without a GPU: the C ABI's checks (before
anything reads a pointer), the z-slab driver's refusal, the resources the guess kernel compiles to for gfx950 and the plume driver's
arguments."""
import ctypes
import os
import re
import subprocess
import sys

import pytest

from fluidnet_cxx_amd import build

REPO = os.path.dirname(build.HERE)

# FnxStepParams as it was before the hybrid projection: methods 3 and 4 are values of `method`, no field was added
STEP_PARAMS_FIELDS = ["dt", "maccormack_strength", "sample_outside_fluid", "buoyancy_scale", "gravity_vec", "operating_density", "p_tol",
                      "jacobi_iter", "method", "normalize_threshold", "precision_mode", "static_flags", "viscosity", "gravity_scale",
                      "correct_scalar", "periodic", "pcg_tol", "pcg_iter", "vorticity_confinement"]
STATE_FIELDS = ["p", "U", "density", "flags", "UBC", "UBCInvMask", "densityBC", "densityBCInvMask", "net", "bc_class", "flags_stick",
                "density_bc_applied"]


@pytest.fixture(scope="module")
def lib():
    build.build_all()
    lib = ctypes.CDLL(build.LIB)
    lib.fnx_last_error.restype = ctypes.c_char_p
    return lib


class _FnxGrid(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int) for n in ("B", "D", "H", "W", "is3D", "ref_quirks", "z_offset", "D_global", "k_begin", "k_end")]


def _header(comments=True):
    hdr = open(os.path.join(REPO, "include", "fluidnet_hip.h")).read()
    return hdr if comments else re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)


def _structs():
    """ctypes mirrors of FnxStepParams and FnxState, read from the header"""
    hdr = _header(comments=False)
    body = re.search(r"typedef struct FnxStepParams \{(.*?)\} FnxStepParams;", hdr, re.S).group(1)
    fields = []
    for typ, name, dim in re.findall(r"(float|int)\s+(\w+)(?:\[(\d+)\])?;", body):
        t = ctypes.c_float if typ == "float" else ctypes.c_int
        fields.append((name, t * int(dim) if dim else t))
    Prm = type("Prm", (ctypes.Structure,), {"_fields_": fields})
    sbody = re.search(r"typedef struct FnxState \{(.*?)\} FnxState;", hdr, re.S).group(1)
    sfields = []
    for decl in sbody.split(";"):
        decl = decl.strip()
        if decl:
            sfields.append((re.search(r"(\w+)$", decl).group(1), ctypes.c_void_p if "*" in decl else ctypes.c_int))
    St = type("St", (ctypes.Structure,), {"_fields_": sfields})
    return Prm, St


def _einval():
    return int(re.search(r"FNX_EINVAL = (\d+)", _header()).group(1))


def _buf(n=64):
    return ctypes.cast(ctypes.create_string_buffer(n), ctypes.c_void_p)


def test_abi_27_symbols_and_unchanged_structs(lib):
    lib.fnx_abi_version.restype = ctypes.c_int
    want = int(re.search(r"#define FNX_ABI_VERSION (\d+)", _header()).group(1))
    assert want >= 27 and lib.fnx_abi_version() == want
    assert hasattr(lib, "fnx_pcg_from") and hasattr(lib, "fnx_pcg_from_verbose")
    Prm, St = _structs()
    assert [n for n, _ in Prm._fields_] == STEP_PARAMS_FIELDS
    assert [n for n, _ in St._fields_] == STATE_FIELDS
    assert re.search(r"3 = 'hybrid'", _header()) and re.search(r"4 = 'pcg' started from st->p", _header())


def test_pcg_from_checks_before_the_device(lib):
    """each bad call is refused with its own message, on host pointers (nothing may read them)"""
    vp = ctypes.c_void_p
    fn = lib.fnx_pcg_from
    fn.argtypes = [ctypes.POINTER(_FnxGrid), vp, vp, vp, vp, vp, ctypes.c_float, ctypes.c_int, vp, vp, ctypes.c_size_t, vp]
    f, div, p0, p, ws = (_buf() for _ in range(5))
    g3 = lambda **kw: _FnxGrid(**dict(dict(B=1, D=8, H=16, W=16, is3D=1), **kw))

    def refused(g, flags, div, p0, p, max_iter, what):
        assert fn(ctypes.byref(g), flags, div, p0, p, None, 1e-5, max_iter, None, ws, 64, None) == _einval(), what
        assert re.search(what, lib.fnx_last_error().decode()), (what, lib.fnx_last_error())

    for args in ((None, div, p0, p), (f, None, p0, p), (f, div, p0, None), (None, div, None, p)):
        refused(g3(), *args, 4, "NULL tensor")
    refused(g3(), f, div, p0, div, 4, "must not alias")
    refused(g3(), f, div, p0, p, -1, "negative")
    refused(g3(), f, div, None, p, -1, "negative")
    refused(g3(k_begin=2, k_end=6), f, div, p0, p, 4, "compute window or z-slab")
    refused(g3(z_offset=2, D_global=16), f, div, p0, p, 4, "compute window or z-slab")
    # max_iter 0 and p0 == p pass these checks: the call gets as far as the workspace size (64 bytes are too few)
    eworkspace = int(re.search(r"FNX_EWORKSPACE = (\d+)", _header()).group(1))
    assert fn(ctypes.byref(g3()), f, div, p, p, None, 1e-5, 0, None, ws, 64, None) == eworkspace
    assert "workspace too small" in lib.fnx_last_error().decode()
    # fnx_pcg keeps its own bound
    lib.fnx_pcg.argtypes = [ctypes.POINTER(_FnxGrid), vp, vp, vp, vp, ctypes.c_float, ctypes.c_int, vp, vp, ctypes.c_size_t, vp]
    assert lib.fnx_pcg(ctypes.byref(g3()), f, div, p, None, 1e-5, 0, None, ws, 64, None) == _einval()
    assert "At least 1 iteration" in lib.fnx_last_error().decode()


def test_simulate_step_method_checks(lib):
    Prm, St = _structs()
    vp = ctypes.c_void_p
    lib.fnx_simulate_step.argtypes = [ctypes.POINTER(_FnxGrid), ctypes.POINTER(Prm), ctypes.POINTER(St), vp, ctypes.c_size_t, vp]
    bufs = [_buf() for _ in range(5)]
    g = _FnxGrid(B=1, D=8, H=16, W=16, is3D=1)

    def refused(prm, st, what, grid=g):
        assert lib.fnx_simulate_step(ctypes.byref(grid), ctypes.byref(prm), ctypes.byref(st), bufs[4], 64, None) == _einval(), what
        assert re.search(what, lib.fnx_last_error().decode()), (what, lib.fnx_last_error())

    st = St(p=bufs[0].value, U=bufs[1].value, flags=bufs[2].value)
    refused(Prm(dt=0.1, method=3, pcg_iter=10), st, "hybrid method needs packed weights")
    refused(Prm(dt=0.1, method=5, pcg_iter=10), st, "not supported.*hybrid")
    refused(Prm(dt=0.1, method=-1), st, "not supported.*hybrid")
    with_net = St(p=bufs[0].value, U=bufs[1].value, flags=bufs[2].value, net=bufs[3].value)
    refused(Prm(dt=0.1, method=3, pcg_iter=10, precision_mode=99), with_net, "precision_mode")
    for method in (3, 4):
        refused(Prm(dt=0.1, method=method, pcg_iter=0), with_net, "pcg_iter < 1")
        refused(Prm(dt=0.1, method=method, pcg_iter=10), with_net, "compute window or z-slab",
                _FnxGrid(B=1, D=8, H=16, W=16, is3D=1, k_begin=2, k_end=6))


def test_slab_step_refuses_the_warm_solves(lib):
    """methods 3 and 4 get the single-domain message of method 2.  The refusal comes before the driver object is looked at: a block
    of zeros stands in for it (the entry point's failure path reads cfg.nranks, 0 here, and nothing else)"""
    Prm, St = _structs()
    vp = ctypes.c_void_p
    lib.fnx_slab_step.argtypes = [vp, ctypes.POINTER(Prm), ctypes.POINTER(St), vp, ctypes.c_size_t, vp]
    bufs = [_buf() for _ in range(5)]
    slab = _buf(1 << 20)
    st = St(p=bufs[0].value, U=bufs[1].value, flags=bufs[2].value, density=bufs[3].value)
    for method in (2, 3, 4):
        prm = Prm(dt=0.1, method=method, pcg_iter=10)
        assert lib.fnx_slab_step(slab, ctypes.byref(prm), ctypes.byref(st), bufs[4], 64, None) == _einval()
        msg = lib.fnx_last_error().decode()
        assert f"method {method} (PCG) is single-domain only" in msg, msg
    prm = Prm(dt=0.1, method=5)
    assert lib.fnx_slab_step(slab, ctypes.byref(prm), ctypes.byref(st), bufs[4], 64, None) == _einval()
    assert "unknown method 5" in lib.fnx_last_error().decode()


def test_python_surface(lib):
    import inspect
    from fluidnet_cxx_amd import fluid, training
    from fluidnet_cxx_amd._ext import ext
    sig = inspect.signature(fluid.solveLinearSystemPCG)
    assert [n for n, p in sig.parameters.items() if p.kind is not p.KEYWORD_ONLY] == ["flags", "div", "is_3d", "p_tol", "max_iter", "verbose"]
    assert [n for n, p in sig.parameters.items() if p.kind is p.KEYWORD_ONLY] == ["geom", "p0"]
    assert "p0" in ext.solve_linear_system_pcg.__doc__ and "pcg_warm" in ext.simulate_step_.__doc__
    sig = inspect.signature(training.hybrid_iterations)
    assert list(sig.parameters) == ["net", "batches", "tol", "max_iter"]
    assert sig.parameters["tol"].default == 1e-5 and sig.parameters["max_iter"].default == 100


def test_guess_kernel_uses_no_scratch(tmp_path):
    """the new vector kernel compiles for gfx950 without scratch or VGPR spills (build_lib refuses a spilling build too)"""
    unit = "fnx_pcg.hip"
    assert "-Rpass-analysis=kernel-resource-usage" in build.HIP_UNITS[unit]
    kernels, _ = build.SCRATCH_FREE[unit]
    assert kernels == ["pcg_guess_kernel"]
    cmd = ([build.HIPCC] + build.COMMON + build.HIP_UNITS[unit] +
           ["--cuda-device-only", "-c", os.path.join(build.CSRC, unit), "-o", str(tmp_path / "pcg.o")])
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert p.returncode == 0, p.stdout[-4000:]
    bad, seen = build._scratch_users(p.stdout, "pcg_guess_kernel")
    assert seen == 1, "one resource-usage remark for the kernel"
    assert not bad, f"pcg_guess_kernel uses scratch / spills VGPRs: {bad}"
    found = re.findall(r"Function Name: \S*pcg_guess_kernel\S*.*?VGPRs: (\d+).*?LDS Size \[bytes/block\]: (\d+)", p.stdout, re.S)
    assert len(found) == 1, "resource remark format"
    print(f"\npcg_guess_kernel: {found[0][0]} VGPRs, {found[0][1]} B LDS")
    # 256 threads per workgroup at full occupancy (8 waves per SIMD): at most 64 VGPRs; LDS only for the partial sums
    assert int(found[0][0]) <= 64 and int(found[0][1]) <= 1024


def test_plume_driver_arguments():
    plume = os.path.join(REPO, "examples", "plume.py")
    p = subprocess.run([sys.executable, plume, "--method", "hybrid"], capture_output=True, text=True)
    assert p.returncode == 2 and "--method hybrid needs --weights CKPT" in p.stderr, p.stderr[-2000:]
    p = subprocess.run([sys.executable, plume, "--method", "hybrid", "--depth", "8"], capture_output=True, text=True)
    assert p.returncode == 2 and "--method hybrid with --depth > 1 needs --weights3d CKPT" in p.stderr, p.stderr[-2000:]
    p = subprocess.run([sys.executable, plume, "--method", "jacobi", "--pcg-warm"], capture_output=True, text=True)
    assert p.returncode == 2 and "--pcg-warm is only read by --method pcg" in p.stderr, p.stderr[-2000:]
    p = subprocess.run([sys.executable, plume, "--help"], capture_output=True, text=True)
    assert p.returncode == 0 and "--pcg-warm" in p.stdout and "hybrid" in p.stdout
