"""The 'FluidNet' bank net in the native step (fnx_simulate_step_net, ABI 35) without a GPU: the symbol and the kinds, every refusal the
entry point makes before its first launch (the Conv3d bank net's kind among them: the step does not take it yet), the step workspace
(what it was before ABI 35, and large enough for the bank nets) and `step_net` on the five net classes."""
import ctypes
import os
import re

import pytest
import torch

from fluidnet_cxx_amd import build
from util import FnxGrid

REPO = os.path.dirname(build.HERE)
MCONF = dict(inputChannels=dict(div=True, pDiv=False, UDiv=False), normalizeInput=True, normalizeInputChan="UDiv",
             normalizeInputThreshold=1e-5, inputDim=2, is3D=False)
FN = "fnx_simulate_step_net"

# (B, D, H, W): fnx_workspace_bytes(FNX_OP_STEP), (FNX_OP_STEP_STATIC) of the commit before ABI 35 (a build of it, queried once)
STEP_BYTES_BEFORE = {
    (1, 1, 8, 8): (103424, 103424),
    (1, 1, 36, 68): (2685440, 2685440),
    (2, 1, 36, 68): (5367808, 5367808),
    (64, 1, 128, 128): (1143030016, 1143030016),
    (1, 1, 1024, 1024): (1142003200, 1142003200),
    (1, 4, 4, 4): (102912, 103168),
    (1, 12, 24, 36): (11231232, 11272704),
    (2, 12, 24, 36): (22460160, 22543104),
    (4, 64, 64, 64): (1134073088, 1138267392),
    (1, 256, 256, 256): (18144136448, 18211245312),
}


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


def _code(name):
    return int(re.search(name + r" = (\d+)", _header()).group(1))


@pytest.fixture(scope="module")
def lib():
    build.build_all()
    lib = ctypes.CDLL(build.LIB)
    lib.fnx_last_error.restype = ctypes.c_char_p
    lib.fnx_workspace_bytes.restype = lib.fnx_banknet_ws_bytes.restype = lib.fnx_banknet3d_ws_bytes.restype = ctypes.c_size_t
    G = ctypes.POINTER(FnxGrid)
    lib.fnx_workspace_bytes.argtypes = lib.fnx_banknet_ws_bytes.argtypes = lib.fnx_banknet3d_ws_bytes.argtypes = [G, ctypes.c_int]
    return lib


def test_abi_35_symbol_and_kinds(lib):
    hdr = _header()
    want = int(re.search(r"#define FNX_ABI_VERSION (\d+)", hdr).group(1))
    assert want >= 35 and lib.fnx_abi_version() == want
    assert hasattr(lib, FN) and re.search(r"\bint " + FN + r"\(const FnxGrid\* g, const FnxStepParams\* prm, const FnxState\* st, int net_kind,",
                                          _header(comments=False))
    assert (_code("FNX_NET_SCALENET"), _code("FNX_NET_BANK"), _code("FNX_NET_BANK3D")) == (0, 1, 2)
    # the structs are what they were: no trailing field for the kind
    Prm, St = _structs()
    assert [n for n, _ in Prm._fields_][-1] == "vorticity_confinement" and [n for n, _ in St._fields_][-1] == "density_bc_applied"


def test_refusals_before_the_first_launch(lib):
    """fnx_simulate_step_net on dummy host pointers that nothing may read: each refusal with its code, the bank units' wording and the
    entry point's name in front"""
    Prm, St = _structs()
    vp = ctypes.c_void_p
    fn = getattr(lib, FN)
    fn.argtypes = [ctypes.POINTER(FnxGrid), ctypes.POINTER(Prm), ctypes.POINTER(St), ctypes.c_int, vp, ctypes.c_size_t, vp]
    bufs = [ctypes.cast(ctypes.create_string_buffer(64), vp) for _ in range(5)]
    st = St(p=bufs[0].value, U=bufs[1].value, flags=bufs[2].value, net=bufs[3].value)
    EINVAL, EWORKSPACE = _code("FNX_EINVAL"), _code("FNX_EWORKSPACE")
    modes = {k: int(v) for k, v in re.findall(r"(FNX_PRECISION_\w+) = (\d+)", _header())}
    g2, g3 = dict(B=2, D=1, H=36, W=68, is3D=0), dict(B=2, D=12, H=24, W=36, is3D=1)

    def call(grid, kind, method=1, **prm):
        rc = fn(ctypes.byref(FnxGrid(**grid)), ctypes.byref(Prm(dt=0.1, method=method, pcg_iter=10, **prm)), ctypes.byref(st), kind, bufs[4], 64, None)
        return rc, lib.fnx_last_error().decode()

    for method in (1, 3):
        for kind in (3, -1, 99):
            rc, msg = call(g2, kind, method)
            assert rc == EINVAL and msg.startswith(FN + ": ") and f"unknown net_kind {kind}" in msg, msg
        rc, msg = call(g3, 1, method)                            # FNX_NET_BANK on a 3D grid
        assert rc == EINVAL and msg.startswith(FN + ": ") and "'FluidNet' model) is 2D only" in msg, msg
        for grid in (g2, g3):                                    # FNX_NET_BANK3D: not in the step, on any grid
            rc, msg = call(grid, 2, method)
            assert rc == EINVAL and msg.startswith(FN + ": ") and "FNX_NET_BANK3D is not built into the step" in msg, msg
        for axis, v in (("H", 38), ("W", 66), ("H", 0)):
            rc, msg = call(dict(g2, **{axis: v}), 1, method)
            if v:
                assert rc == EINVAL and msg.startswith(FN + ": ") and f"{axis} = {v} must be a positive multiple of 4" in msg, msg
            else:
                assert rc == EINVAL, msg                         # (the grid check's own refusal comes first)
        for m in ("FNX_PRECISION_BF16X6", "FNX_PRECISION_BF16X3"):
            rc, msg = call(g2, 1, method, precision_mode=modes[m])
            assert rc == EINVAL and msg.startswith(FN + ": ") and "fp32 arithmetic only" in msg and "bf16" in msg, msg
        # a view is a 3D grid, which the 2D kind refuses as such; the ScaleNet kind takes it as far as its own checks
        for view in (dict(k_begin=4, k_end=8), dict(z_offset=4, D_global=24)):
            rc, msg = call(dict(g3, **view), 1, method)
            assert rc == EINVAL and msg.startswith(FN + ": ") and "2D only" in msg, (method, msg)
        # a call that passes them gets as far as the workspace (64 bytes are too few), for each kind on its grid
        for grid, kind in ((g2, 0), (g2, 1), (g3, 0)):
            rc, msg = call(grid, kind, method)
            assert rc == EWORKSPACE and "workspace too small" in msg, msg
    # 3D flags_stick stays refused with its text, whatever the kind (behind the workspace check: a workspace of the right size, never read)
    need = lib.fnx_workspace_bytes(ctypes.byref(FnxGrid(**g3)), 3)
    stick = St(p=bufs[0].value, U=bufs[1].value, flags=bufs[2].value, net=bufs[3].value, flags_stick=bufs[2].value)
    rc = fn(ctypes.byref(FnxGrid(**g3)), ctypes.byref(Prm(dt=0.1, method=1)), ctypes.byref(stick), 0, bufs[4], need, None)
    assert rc == EINVAL and "simulate_step: flags_stick is 2D only" in lib.fnx_last_error().decode(), lib.fnx_last_error()
    # methods 0, 2 and 4 do not look at the kind: the same call gets as far as the workspace with any value
    for method in (0, 2, 4):
        for kind in (0, 1, 2, 99):
            rc, msg = call(g3, kind, method)
            assert rc == EWORKSPACE and "workspace too small" in msg, (method, kind, msg)


def test_step_workspace_is_what_it_was_and_holds_the_bank_nets(lib):
    """fnx_workspace_bytes(FNX_OP_STEP) and (FNX_OP_STEP_STATIC) equal the values of the commit before, and the bank nets' whole forward
    (its flags copy, the layout the step carves and the net's own workspace: more than the step takes of it) fits in the step's scratch
    tail."""
    op_step, op_static = _code("FNX_OP_STEP"), _code("FNX_OP_STEP_STATIC")
    for (B, D, H, W), (step, static) in STEP_BYTES_BEFORE.items():
        is3D = int(D > 1)
        g = FnxGrid(B=B, D=D, H=H, W=W, is3D=is3D)
        assert lib.fnx_workspace_bytes(ctypes.byref(g), op_step) == step, (B, D, H, W)
        assert lib.fnx_workspace_bytes(ctypes.byref(g), op_static) == static, (B, D, H, W)
        if H % 4 or W % 4 or (is3D and D % 4):
            continue
        whole = (lib.fnx_banknet3d_ws_bytes if is3D else lib.fnx_banknet_ws_bytes)(ctypes.byref(g), 1)
        # the tail is the largest need of its users, and the ScaleNet's whole forward (FNX_OP_FLUIDNET) is one of them
        tail_at_least = lib.fnx_workspace_bytes(ctypes.byref(g), _code("FNX_OP_FLUIDNET"))
        assert 0 < whole <= tail_at_least < step, ((B, D, H, W), whole, tail_at_least)


def test_step_net_on_the_five_classes():
    from fluidnet_cxx_amd import FluidNet, FluidNetBankTrain, FluidNetBankTrain3D, FluidNetTrain, FluidNetTrain3D
    m3 = dict(MCONF, inputDim=3, is3D=True)
    nets = [FluidNet(MCONF), FluidNet(dict(MCONF, model="FluidNet")), FluidNet(dict(m3, model="FluidNet3D")), FluidNetTrain(MCONF),
            FluidNetTrain3D(m3), FluidNetBankTrain(dict(MCONF, model="FluidNet")), FluidNetBankTrain3D(dict(m3, model="FluidNet3D"))]
    for net in nets:
        assert callable(getattr(net, "step_net", None)), type(net).__name__
    # the Conv3d bank nets say that the native step does not take them (simulate() keeps them on the operator path)
    for net in (nets[2], nets[6]):
        with pytest.raises(RuntimeError, match="'FluidNet3D' bank model, which the native step does not take"):
            net.step_net("cuda")
    # packed_for and packed keep raising for the bank nets (the z-slab drivers rely on it)
    for net in (nets[1], nets[2], nets[5], nets[6]):
        for what in (lambda: net.packed_for("cuda"), lambda: net.packed):
            with pytest.raises(RuntimeError, match="bank model"):
                what()


def test_simulate_asks_step_net_and_falls_back_to_packed_for():
    """simulate() asks net.step_net(device) where the net has it and packed_for(device) where it does not, and hands the kind to
    ext.simulate_step_ (seen through a stand-in for the extension: no GPU)"""
    from fluidnet_cxx_amd import _simulate
    seen = {}

    class Ext:
        @staticmethod
        def simulate_step_(*args, **kw):
            seen["net"], seen["kind"] = args[8], kw["net_kind"]

    class WithStepNet:
        is_bank = True

        def step_net(self, device):
            return "bank", "bank image"

        def packed_for(self, device):
            raise AssertionError("packed_for asked of a net with step_net")

    class ThirdParty:
        def packed_for(self, device):
            return "scalenet image"

    cfg = dict(dt=0.1, maccormackStrength=0.6, sampleOutsideFluid=False, buoyancyScale=0, gravityScale=0)
    bd = dict(p=torch.zeros(1, 1, 1, 8, 8), U=torch.zeros(1, 2, 1, 8, 8), flags=torch.ones(1, 1, 1, 8, 8), density=torch.zeros(1, 1, 1, 8, 8))
    real, _simulate.ext = _simulate.ext, Ext
    try:
        for method in ("convnet", "hybrid"):
            _simulate.simulate(cfg, dict(bd), WithStepNet(), method)
            assert seen == dict(net="bank image", kind="bank")
            _simulate.simulate(cfg, dict(bd), ThirdParty(), method)
            assert seen == dict(net="scalenet image", kind="scalenet")
        _simulate.simulate(cfg, dict(bd), None, "jacobi")
        assert seen == dict(net=None, kind="scalenet")
    finally:
        _simulate.ext = real
