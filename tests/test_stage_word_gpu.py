"""The 3D step on the stage word (csrc/fnx_stage_word.h: one uint32 per cell in the place of seven flag values and seven class bytes in
stage3d_kernel and post_projection_kernel) against the same step on the float kernels, bit for bit.

The float path is three steps with static_flags = 0 (no class map, so no word); the word path the same three steps with static_flags 0, 3,
7 on a workspace of ext.step_workspace_bytes (FNX_OP_STEP_STATIC): the second step builds the class map and the word, the third reuses
both.  Grids: W in {61, 64, 67} x H in {6, 9} x D in {3, 5}, B = 2 -- one and two 64-column blocks, two and three 4-row blocks, ragged in
both, one interior plane and three.  Flags are random per sample (obstacles, EMPTY cells, open border cells, one cell of type 8), with
obstacle and EMPTY cells placed on both sides of the 64-column and 4-row block edges; the BC arrays are the identity on most cells of
sample 0 (whole waves take the no-BC-load path next to cells that do not) and on about two thirds of sample 1, masks in {0, 1, 0.5},
values that include -0 (not the identity)."""
import ctypes
import re

import numpy as np
import pytest
import torch

from util import PLUME_CFG

pytestmark = pytest.mark.gpu

SHAPES = [(W, H, D) for W in (61, 64, 67) for H in (6, 9) for D in (3, 5)]
B = 2
CFG = dict(PLUME_CFG, jacobiIter=5, gravityVec=dict(x=0.3, y=-1.0, z=0.6), operatingDensity=0.1, pcgIter=4, pcgTol=0.0)
KEYS = ("U", "p", "density")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ext():
    from fluidnet_cxx_amd._ext import ext
    return ext


def make_state(W, H, D, seed):
    rng = np.random.default_rng(seed)
    shape = (B, 1, D, H, W)
    kinds = np.array([1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 2.0, 4.0], np.float32)
    f = rng.choice(kinds, size=shape)
    border = np.ones(shape, bool)
    border[:, :, 1:-1, 1:-1, 1:-1] = False
    f[border & (rng.random(shape) < 0.8)] = 2.0                 # most of the shell is wall, the rest open (fluid / EMPTY) border cells
    # both sides of the block edges: columns 63 | 64 (W = 67) and rows 3 | 4, in an interior plane
    k = D // 2
    f[:, :, k, 3, 5] = 2.0; f[:, :, k, 4, 5] = 1.0; f[:, :, k, 3, 9] = 1.0; f[:, :, k, 4, 9] = 4.0
    f[:, :, k, 3, 12] = 4.0; f[:, :, k, 4, 12] = 2.0
    if W > 65:
        f[:, :, k, 2, 63] = 2.0; f[:, :, k, 2, 64] = 1.0; f[:, :, k, 3, 63] = 1.0; f[:, :, k, 3, 64] = 4.0
        f[:, :, k, 4, 63] = 4.0; f[:, :, k, 4, 64] = 2.0
    f[0, 0, k, 2, 20] = 8.0                                     # a type the stages compare with nothing
    f[1, 0, k, 2, 30] = 1.0; f[1, 0, k, 2, 31] = 8.0; f[1, 0, k, 2, 32] = 1.0

    def bc(shape_):
        dense = np.zeros(shape_, bool)
        dense[0] = rng.random(shape_[1:]) < 0.02               # sample 0: scattered single cells, identity waves all around them
        dense[1] = rng.random(shape_[1:]) < 0.35
        m = np.where(dense, rng.choice(np.array([0.0, 0.0, 0.5], np.float32), size=shape_), 1.0).astype(np.float32)
        v = np.where(dense, rng.standard_normal(shape_), 0.0).astype(np.float32)
        v[rng.random(shape_) < 0.01] = -0.0                     # mask 1 with -0 is not the identity (x + -0 keeps a -0)
        return m, v

    UM, UV = bc((B, 3, D, H, W))
    RM, RV = bc(shape)
    return dict(p=(rng.standard_normal(shape) * 0.1).astype(np.float32), U=(rng.standard_normal((B, 3, D, H, W)) * 0.4).astype(np.float32),
                flags=f.astype(np.float32), density=rng.random(shape).astype(np.float32), UBC=UV, UBCInvMask=UM, densityBC=RV,
                densityBCInvMask=RM)


def to_dev(st, dev, density=True):
    bd = {k: torch.from_numpy(v.copy()).to(dev) for k, v in st.items()}
    if not density:
        for k in ("density", "densityBC", "densityBCInvMask"):
            del bd[k]
    return bd


def run(ext, dev, st, shape, static, method="jacobi", cfg=CFG, density=True, geom=None, fused=True, then=None):
    """three steps; `static`: the three static_flags.  then = (change, static_flags): a fourth step after `change(flags)` in place"""
    from fluidnet_cxx_amd import simulate
    W, H, D = shape
    bd = to_dev(st, dev, density)
    ws = torch.empty(ext.step_workspace_bytes(B, D, H, W, True), dtype=torch.uint8, device=dev)
    for it in range(3):
        if fused:
            simulate(cfg, bd, None, method, workspace=ws, static_flags=static[it], geom=geom)
        else:
            simulate(cfg, bd, None, method, fused=False, geom=geom)
    if then is not None:
        then[0](bd["flags"])
        simulate(cfg, bd, None, method, workspace=ws, static_flags=then[1], geom=geom)
    torch.cuda.synchronize()
    return {k: bd[k].clone() for k in KEYS}


def same_bits(a, b, what):
    for k in KEYS:
        assert a[k].dtype == torch.float32
        assert torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)), f"{what}: {k} differs in {int((a[k].view(torch.int32) != b[k].view(torch.int32)).sum())} cells"


def test_the_workspace_has_room_for_the_word(ext):
    """what ext.step_workspace_bytes gives is FNX_OP_STEP_STATIC: with less the step would quietly stay on the float kernels and the
    comparisons below would compare them with themselves"""
    import os
    from fluidnet_cxx_amd import build
    from util import FnxGrid
    lib = ctypes.CDLL(build.LIB)
    lib.fnx_workspace_bytes.restype = ctypes.c_size_t
    lib.fnx_workspace_bytes.argtypes = [ctypes.POINTER(FnxGrid), ctypes.c_int]
    hdr = open(os.path.join(os.path.dirname(build.HERE), "include", "fluidnet_hip.h")).read()
    op_step = int(re.search(r"FNX_OP_STEP = (\d+)", hdr).group(1))
    for W, H, D in SHAPES:
        g = FnxGrid(B=B, D=D, H=H, W=W, is3D=1)
        step = lib.fnx_workspace_bytes(ctypes.byref(g), op_step)
        assert ext.step_workspace_bytes(B, D, H, W, True) >= (step + 255) // 256 * 256 + 4 * B * D * H * W


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("variant", ["density", "no_density", "gravity", "quirks"])
def test_word_path_equals_float_path(ext, dev, shape, variant):
    """Jacobi step (stage with wall BCs and divergence, post-projection pass), three steps, static_flags 0, 3, 7 against 0, 0, 0"""
    st = make_state(*shape, seed=3)
    kw = dict(density=variant != "no_density", cfg=dict(CFG, gravityScale=1.3) if variant == "gravity" else CFG,
              geom=ext.Geom(ref_quirks=True) if variant == "quirks" else None)
    want = run(ext, dev, st, shape, (0, 0, 0), **kw)
    same_bits(run(ext, dev, st, shape, (0, 3, 7), **kw), want, "static_flags 0, 3, 7")
    same_bits(run(ext, dev, st, shape, (3, 3, 7), **kw), want, "static_flags 3, 3, 7")     # the word built in two calls running
    assert all(bool(torch.isfinite(v).all()) for v in want.values())


@pytest.mark.parametrize("shape", [(67, 9, 5), (61, 6, 3)], ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("variant", ["pcg", "periodic", "confinement", "confinement_quirks", "no_buoyancy"])
def test_the_other_stage_instances(ext, dev, shape, variant):
    """the launches the Jacobi step does not make: the PCG step's tail; the stage without the divergence and the tail between the periodic
    patches; the stage cut around the vorticity confinement (its second launch leaves out the first setConstVals and the density)"""
    st = make_state(*shape, seed=5)
    method = "pcg" if variant == "pcg" else "jacobi"
    cfg = {"pcg": CFG, "periodic": {**CFG, "periodic-x": True, "periodic-y": True}, "confinement": dict(CFG, vorticityConfinementAmp=0.4),
           "confinement_quirks": dict(CFG, vorticityConfinementAmp=0.4), "no_buoyancy": dict(CFG, buoyancyScale=0.0)}[variant]
    geom = ext.Geom(ref_quirks=True) if variant == "confinement_quirks" else None
    want = run(ext, dev, st, shape, (0, 0, 0), method=method, cfg=cfg, geom=geom)
    same_bits(run(ext, dev, st, shape, (0, 3, 7), method=method, cfg=cfg, geom=geom), want, variant)


def test_convnet_stage_on_the_word(ext, dev):
    """the convnet's stage has no wall BCs (its tail stays on the float kernel): static_flags 0, 3, 7 against 0, 0, 0"""
    from fluidnet_cxx_amd import FluidNet, simulate
    from fluidnet_cxx_amd.weights import make_scalenet_weights
    shape = (67, 9, 5)
    W, H, D = shape
    st = make_state(*shape, seed=7)
    cfg = dict(CFG, model="ScaleNet", inputChannels=dict(div=True, pDiv=False, UDiv=False), normalizeInput=True, normalizeInputChan="UDiv", is3D=True)
    net = FluidNet.from_weights(cfg, make_scalenet_weights(0, ndim=3), dev)
    outs = []
    for static in ((0, 0, 0), (0, 3, 7)):
        bd = to_dev(st, dev)
        ws = torch.empty(ext.step_workspace_bytes(B, D, H, W, True), dtype=torch.uint8, device=dev)
        for it in range(3):
            simulate(cfg, bd, net, "convnet", workspace=ws, static_flags=static[it])
        outs.append({k: bd[k].clone() for k in KEYS})
    same_bits(outs[1], outs[0], "convnet")


@pytest.mark.parametrize("shape", [(67, 9, 5), (64, 6, 3)], ids=lambda s: "x".join(map(str, s)))
def test_word_path_equals_operator_path(ext, dev, shape):
    """one case against fused=False, operator by operator"""
    st = make_state(*shape, seed=11)
    same_bits(run(ext, dev, st, shape, (0, 3, 7)), run(ext, dev, st, shape, None, fused=False), "fused=False")


@pytest.mark.parametrize("shape", [(67, 9, 5), (61, 6, 5)], ids=lambda s: "x".join(map(str, s)))
def test_changed_flags_rebuild_the_word(ext, dev, shape):
    """after three static steps `flags` changes in place and the caller promises the BC arrays only (static_flags 6: bits 1 and 2, not bit
    0): the word is rebuilt, the step equals the float path's on the new flags -- and differs from a step on the old ones"""
    W, H, D = shape
    st = make_state(*shape, seed=13)

    def change(flags):
        k = D // 2
        flags[:, :, k, 2:5, 20:40] = 2.0         # a wall where fluid was ...
        flags[:, :, k, 5, 41:48] = 1.0           # ... fluid, EMPTY and a type-8 cell where anything was
        flags[:, :, 1, 1, 1:W - 1] = 4.0
        flags[0, 0, k, 3, 50] = 8.0

    want = run(ext, dev, st, shape, (0, 0, 0), then=(change, 0))
    same_bits(run(ext, dev, st, shape, (0, 3, 7), then=(change, 6)), want, "static_flags 6 after a change of flags")
    same_bits(run(ext, dev, st, shape, (0, 3, 7), then=(change, 2)), want, "static_flags 2 after a change of flags")
    unchanged = run(ext, dev, st, shape, (0, 0, 0), then=(lambda flags: None, 0))
    assert not torch.equal(unchanged["U"], want["U"])            # (the change matters: a stale word would have shown)
