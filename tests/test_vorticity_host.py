"""Vorticity confinement without a GPU: the C ABI's checks (before anything reads a pointer), the refusals of the z-slab drivers, and
the resources the two kernels compile to for gfx950."""
import ctypes
import os
import re
import subprocess

import pytest

from fluidnet_cxx_amd import build

REPO = os.path.dirname(build.HERE)


@pytest.fixture(scope="module")
def built():
    build.build_all()
    return build


class _FnxGrid(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int) for n in ("B", "D", "H", "W", "is3D", "ref_quirks", "z_offset", "D_global", "k_begin", "k_end")]


def _header():
    return open(os.path.join(REPO, "include", "fluidnet_hip.h")).read()


def test_abi_version_and_symbol(built):
    lib = ctypes.CDLL(built.LIB)
    lib.fnx_abi_version.restype = ctypes.c_int
    want = int(re.search(r"#define FNX_ABI_VERSION (\d+)", _header()).group(1))
    assert want >= 22 and lib.fnx_abi_version() == want
    assert hasattr(lib, "fnx_add_vorticity_confinement")
    assert re.search(r"float\s+vorticity_confinement;", _header())
    # appended behind pcg_iter: a caller's older initialiser list keeps its meaning
    body = re.search(r"typedef struct FnxStepParams \{(.*?)\} FnxStepParams;", _header(), re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = re.findall(r"(\w+)(?:\[\d+\])?;", body)
    assert names[-2:] == ["pcg_iter", "vorticity_confinement"], names[-3:]


def test_entry_point_checks_before_the_device(built):
    """each bad call is refused with its own message, on host pointers (nothing may read them)"""
    lib = ctypes.CDLL(built.LIB)
    lib.fnx_last_error.restype = ctypes.c_char_p
    vp = ctypes.c_void_p
    lib.fnx_add_vorticity_confinement.argtypes = [ctypes.POINTER(_FnxGrid), vp, vp, vp, ctypes.c_float, vp]
    einval = int(re.search(r"FNX_EINVAL = (\d+)", _header()).group(1))
    a = ctypes.cast(ctypes.create_string_buffer(64), vp)
    b = ctypes.cast(ctypes.create_string_buffer(64), vp)
    f = ctypes.cast(ctypes.create_string_buffer(64), vp)
    g3 = lambda **kw: _FnxGrid(**dict(dict(B=1, D=8, H=16, W=16, is3D=1), **kw))

    def refused(g, U_in, U_out, flags, what):
        assert lib.fnx_add_vorticity_confinement(ctypes.byref(g), U_in, U_out, flags, 0.5, None) == einval, what
        assert re.search(what, lib.fnx_last_error().decode()), (what, lib.fnx_last_error())

    for args in ((None, b, f), (a, None, f), (a, b, None)):
        refused(g3(), *args, "NULL tensor")
    refused(g3(), a, a, f, "must not alias")
    refused(g3(k_begin=2, k_end=6), a, b, f, "compute window or z-slab")
    refused(g3(z_offset=2, D_global=16), a, b, f, "compute window or z-slab")
    refused(g3(H=2), a, b, f, "Dimension mismatch")
    refused(g3(D=2), a, b, f, "D >= 3")
    refused(_FnxGrid(B=1, D=4, H=16, W=16, is3D=0), a, b, f, "zdepth")
    assert lib.fnx_add_vorticity_confinement(None, a, b, f, 0.5, None) == einval
    assert "NULL" in lib.fnx_last_error().decode()


def test_pre_projection_refuses_a_window_with_confinement(built):
    """the stage entry point too, ahead of any launch (host pointers)"""
    lib = ctypes.CDLL(built.LIB)
    lib.fnx_last_error.restype = ctypes.c_char_p
    hdr = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
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
        if not decl:
            continue
        name = re.search(r"(\w+)$", decl).group(1)
        sfields.append((name, ctypes.c_void_p if "*" in decl else ctypes.c_int))
    St = type("St", (ctypes.Structure,), {"_fields_": sfields})
    vp = ctypes.c_void_p
    lib.fnx_pre_projection.argtypes = [ctypes.POINTER(_FnxGrid), ctypes.POINTER(Prm), ctypes.POINTER(St), vp, vp, vp, vp]
    bufs = [ctypes.cast(ctypes.create_string_buffer(64), vp) for _ in range(4)]
    prm = Prm(dt=0.1, vorticity_confinement=0.5)
    st = St(U=bufs[0].value, flags=bufs[1].value, p=bufs[2].value)
    g = _FnxGrid(B=1, D=8, H=16, W=16, is3D=1, k_begin=2, k_end=6)
    einval = int(re.search(r"FNX_EINVAL = (\d+)", hdr).group(1))
    assert lib.fnx_pre_projection(ctypes.byref(g), ctypes.byref(prm), ctypes.byref(st), bufs[3], None, None, None) == einval
    assert "vorticity confinement takes no compute window" in lib.fnx_last_error().decode()


def test_slab_drivers_refuse_the_stage(built):
    """fnx_slab_step (source: the check sits with the other optional stages, ahead of the workspace carve) and both Python drivers"""
    src = open(os.path.join(build.CSRC, "fnx_slab.hip")).read()
    body = src[src.index("static int slab_step_body"):]
    assert body.index("prm->vorticity_confinement > 0.f") < body.index("Work W;")
    from fluidnet_cxx_amd import slab
    cfg = dict(dt=0.1, pTol=0.0, jacobiIter=4, vorticityConfinementAmp=0.5)
    lay = slab.SlabLayout(16, 1, 0, 5)
    with pytest.raises(ValueError, match="vorticity confinement"):
        slab.NativeSlabSimulator(lay, cfg)
    with pytest.raises(ValueError, match="vorticity confinement"):
        slab.SlabSimulator(lay, cfg, ops=object())
    slab._refuse_vorticity(dict(cfg, vorticityConfinementAmp=0))      # off: accepted


def test_python_surface(built):
    import inspect
    from fluidnet_cxx_amd import fluid
    from fluidnet_cxx_amd._ext import ext
    sig = inspect.signature(fluid.addVorticityConfinement)
    assert [n for n, p in sig.parameters.items() if p.kind is not p.KEYWORD_ONLY] == ["U", "flags", "strength"]
    assert [n for n, p in sig.parameters.items() if p.kind is p.KEYWORD_ONLY] == ["geom"]
    assert "addVorticityConfinement" in fluid.__all__ and hasattr(ext, "add_vorticity_confinement_")
    assert "vorticity_confinement" in ext.simulate_step_.__doc__


def test_kernels_use_no_scratch_and_fit_two_workgroups_per_cu(tmp_path):
    """Both instantiations compile for gfx950 without scratch or VGPR spills (build_lib refuses a spilling build too), within the
    budget their occupancy needs: two 8-wave workgroups per CU are 4 waves per SIMD, i.e. at most 128 VGPRs of the 512 per lane,
    and half of the CU's 160 KiB of LDS each."""
    unit = "fnx_vorticity.hip"
    assert "-ffp-contract=off" in build.HIP_UNITS[unit] and "-Rpass-analysis=kernel-resource-usage" in build.HIP_UNITS[unit]
    kernels, _ = build.SCRATCH_FREE[unit]
    assert kernels == ["vorticity_confinement_kernel"]
    cmd = ([build.HIPCC] + build.COMMON + build.HIP_UNITS[unit] +
           ["--cuda-device-only", "-c", os.path.join(build.CSRC, unit), "-o", str(tmp_path / "vort.o")])
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert p.returncode == 0, p.stdout[-4000:]
    bad, seen = build._scratch_users(p.stdout, "vorticity_confinement_kernel")
    assert seen == 2, "one resource-usage remark each for the 2D and the 3D kernel"
    assert not bad, f"vorticity_confinement_kernel uses scratch / spills VGPRs: {bad}"
    found = re.findall(r"Function Name: \S*vorticity_confinement_kernel\S*.*?VGPRs: (\d+).*?LDS Size \[bytes/block\]: (\d+)", p.stdout, re.S)
    assert len(found) == 2, "resource remark format"
    for vgprs, lds in found:
        print(f"\nvorticity_confinement_kernel: {vgprs} VGPRs, {lds} B LDS")
        assert int(vgprs) <= 128 and int(lds) <= 80 * 1024
