"""Passive scalars on the GPU.  fluid.advectScalars is defined by fluid.advectScalar: every channel must come out with the bits that
operator gives for it alone (any plan, both methods, both sample_outside_fluid modes, 3D with and without ref_quirks).  Then the
stage in simulate(), the output files and the driver's --dyes."""
import importlib.util
import os

import numpy as np
import pytest
import torch

from util import PLUME_CFG, assert_bitexact, plume_state, random_state

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAC, EULER = "maccormackFluidNet", "eulerFluidNet"
# (B, C, D, H, W): W = 70 crosses the 64-wide segment of the 3D tile kernels the comparator runs; C = 5: more channels than a sample has
# velocity components.  3d_deep crosses every tile edge of the clamp-bounds reduction: D = 19 its 16-plane chunk, H = 35 its 32-row
# workgroup, W = 70 its 62-column wave, and B = 2 x C = 3 tells a channel's plane stack from its sample's flags
SHAPES = {"2d": (2, 5, 1, 20, 33), "3d": (2, 5, 9, 12, 70), "2d_c1": (2, 1, 1, 20, 33), "3d_c1": (2, 1, 9, 12, 70),
          "3d_deep": (2, 3, 19, 35, 70)}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ext():
    from fluidnet_cxx_amd._ext import ext
    return ext


def T(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(dev)


def N(t):
    return t.cpu().numpy()


_CASES = {}


def _case(name):
    """flags with boxes, U of sigma 3 (with dt = 1 the traces hit obstacles and borders) and C fields; with C = 5 channel 1 carries a
    NaN and an Inf cell in the interior and channel 2 is all zero, so a min / max or a flag shared wrongly between channels shows"""
    if name not in _CASES:
        B, C, D, H, W = SHAPES[name]
        s = random_state(B, D, H, W, sigma=3, seed=11 + D, boxes=True)
        rng = np.random.default_rng(5 + C)
        src = rng.random((B, C, D, H, W)).astype(np.float32)
        if C > 2:
            src[0, 1, D // 2, H // 2 + 2, W // 2 + 3] = np.nan
            src[1, 1, D // 2, 3, W - 5] = np.inf
            src[:, 2] = 0.0
        _CASES[name] = dict(s, src=src)
    return _CASES[name]


def _per_channel(fluid, dev, c, dt, method, so, strength, geom, plan):
    tU, tf = T(c["U"], dev), T(c["flags"], dev)
    return [N(fluid.advectScalar(dt, T(c["src"][:, ch:ch + 1], dev), tU, tf, method, 1, so, strength, geom=geom, plan=plan))
            for ch in range(c["src"].shape[1])]


@pytest.mark.parametrize("so", [False, True])
@pytest.mark.parametrize("method", [MAC, EULER])
@pytest.mark.parametrize("name", ["2d", "2d_c1"])
def test_channels_equal_advect_scalar_2d(dev, ext, oracle, name, method, so):
    from fluidnet_cxx_amd import fluid
    c = _case(name)
    got = N(fluid.advectScalars(1.0, T(c["src"], dev), T(c["U"], dev), T(c["flags"], dev), method, 1, so, 0.6))
    assert got.shape == c["src"].shape
    # the extension's entry point by itself (fluid.advectScalars hands a single field to advectScalar)
    assert_bitexact(N(ext.advect_scalars(1.0, T(c["src"], dev), T(c["U"], dev), T(c["flags"], dev), method, 1, so, 0.6)), got, "ext.advect_scalars")
    for plan in ("auto", "cells"):
        for ch, want in enumerate(_per_channel(fluid, dev, c, 1.0, method, so, 0.6, None, plan)):
            assert_bitexact(got[:, ch:ch + 1], want, f"{name} {method} so={so} plan={plan}: channel {ch}")
    for ch in range(c["src"].shape[1]):
        want = oracle.advect_scalar(1.0, np.ascontiguousarray(c["src"][:, ch:ch + 1]), c["U"], c["flags"], method, 1, so, 0.6)
        assert_bitexact(got[:, ch:ch + 1], want, f"{name} {method} so={so}: channel {ch} vs the oracle")
    if name == "2d":
        assert np.isfinite(got[:, [0, 2, 3, 4]]).all(), "the NaN and the Inf stay in their channel"
        assert (got[:, 2] == 0).all(), "the zero channel stays zero"


@pytest.mark.parametrize("quirks", [0, 1])
@pytest.mark.parametrize("so", [False, True])
@pytest.mark.parametrize("method", [MAC, EULER])
@pytest.mark.parametrize("name", ["3d", "3d_c1", "3d_deep"])
def test_channels_equal_advect_scalar_3d(dev, ext, name, method, so, quirks):
    from fluidnet_cxx_amd import fluid
    c = _case(name)
    geom = ext.Geom(ref_quirks=bool(quirks))
    got = N(fluid.advectScalars(1.0, T(c["src"], dev), T(c["U"], dev), T(c["flags"], dev), method, 1, so, 0.6, geom=geom))
    assert_bitexact(N(ext.advect_scalars(1.0, T(c["src"], dev), T(c["U"], dev), T(c["flags"], dev), method, 1, so, 0.6, None, geom)), got,
                    "ext.advect_scalars")
    for plan in ("auto", "cells"):
        for ch, want in enumerate(_per_channel(fluid, dev, c, 1.0, method, so, 0.6, geom, plan)):
            assert_bitexact(got[:, ch:ch + 1], want, f"{name} {method} so={so} quirks={quirks} plan={plan}: channel {ch}")
    if name == "3d":
        assert (got[:, 2] == 0).all(), "the zero channel stays zero"
        assert np.isfinite(got[:, [0, 2, 3, 4]]).all(), "the NaN and the Inf stay in their channel"


@pytest.mark.parametrize("name", ["2d", "3d"])
def test_permuting_the_channels_permutes_the_output(dev, name):
    from fluidnet_cxx_amd import fluid
    c = _case(name)
    tU, tf = T(c["U"], dev), T(c["flags"], dev)
    perm = [3, 0, 4, 2, 1]
    a = N(fluid.advectScalars(1.0, T(c["src"], dev), tU, tf, MAC, 1, False, 0.6))
    b = N(fluid.advectScalars(1.0, T(c["src"][:, perm], dev), tU, tf, MAC, 1, False, 0.6))
    again = N(fluid.advectScalars(1.0, T(c["src"], dev), tU, tf, MAC, 1, False, 0.6))
    assert_bitexact(b, a[:, perm], f"{name}: permuted channels")
    assert_bitexact(again, a, f"{name}: second call")
    assert_bitexact(N(tU), c["U"], "U after the calls"); assert_bitexact(N(tf), c["flags"], "flags after the calls")


def test_refusals(dev, ext):
    from fluidnet_cxx_amd import fluid
    c = _case("3d")
    src, U, f = T(c["src"], dev), T(c["U"], dev), T(c["flags"], dev)
    with pytest.raises(RuntimeError, match="dst must not alias src"):
        ext.advect_scalars(1.0, src, U, f, MAC, 1, False, 0.6, None, None, src)
    for geom in (ext.Geom(k_begin=2, k_end=6), ext.Geom(z_offset=2, D_global=40)):
        with pytest.raises(RuntimeError, match="single-domain"):
            fluid.advectScalars(1.0, src, U, f, geom=geom)
        with pytest.raises(RuntimeError, match="single-domain"):
            ext.advect_scalars(1.0, src[:, :1].contiguous(), U, f, MAC, 1, False, 0.6, None, geom)
        with pytest.raises(AssertionError, match="single-domain"):
            fluid.advectScalars(1.0, src[:, :1].contiguous(), U, f, geom=geom)
    with pytest.raises(AssertionError, match="Dimension mismatch"):
        fluid.advectScalars(1.0, src[0], U, f)
    with pytest.raises(AssertionError, match="Size mismatch"):
        fluid.advectScalars(1.0, src[:, :, :, :, :60].contiguous(), U, f)
    with pytest.raises(AssertionError, match="Size mismatch"):
        fluid.advectScalars(1.0, src[:1].contiguous(), U, f)
    with pytest.raises(RuntimeError, match="Size mismatch"):
        ext.advect_scalars(1.0, src[:, :, :, :, :60].contiguous(), U, f, MAC, 1, False, 0.6)
    with pytest.raises(RuntimeError, match="workspace too small"):
        ext.advect_scalars(1.0, src, U, f, MAC, 1, False, 0.6, torch.empty(256, dtype=torch.uint8, device=dev))
    with pytest.raises(AssertionError, match="not supported"):
        fluid.advectScalars(1.0, src, U, f, method="upwind")
    c2 = _case("2d")
    with pytest.raises(AssertionError, match="no channel"):
        fluid.advectScalars(1.0, T(c2["src"][:, :0], dev), T(c2["U"], dev), T(c2["flags"], dev))
    # a caller's workspace of the advertised size serves
    B, C, D, H, W = SHAPES["3d"]
    ws = torch.empty(ext.advect_scalars_workspace_bytes(B, D, H, W, True, C), dtype=torch.uint8, device=dev)
    assert_bitexact(N(ext.advect_scalars(1.0, src, U, f, MAC, 1, False, 0.6, ws)), N(fluid.advectScalars(1.0, src, U, f, MAC, 1, False, 0.6)),
                    "caller's workspace")


# ---- the stage in simulate()
def _sim_state(D, dev, with_scalars):
    st = plume_state(24, D)
    rng = np.random.default_rng(2)
    st["U"] = (st["U"] + rng.standard_normal(st["U"].shape).astype(np.float32) * np.float32(0.5)).astype(np.float32)
    st["density"] = rng.random(st["density"].shape).astype(np.float32)
    if with_scalars:
        extra = rng.random((1, 2) + st["density"].shape[2:]).astype(np.float32)
        st["scalars"] = np.concatenate([st["density"], extra], 1)
        st["scalarsBC"] = np.concatenate([st["densityBC"], np.zeros_like(extra)], 1)
        st["scalarsBCInvMask"] = np.concatenate([st["densityBCInvMask"], np.ones_like(extra)], 1)
    return {k: T(v, dev) for k, v in st.items()}


@pytest.mark.parametrize("correct", [False, True])
@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("D", [1, 8])
def test_simulate_carries_the_scalars(dev, D, fused, correct):
    """channel 0 starts as the density with the density's BC arrays and stays the density, bit for bit; the flow does not see the key"""
    from fluidnet_cxx_amd import _simulate, simulate
    cfg = dict(PLUME_CFG, jacobiIter=9, correctScalar=correct)
    _simulate.release_workspaces()
    a, b = _sim_state(D, dev, True), _sim_state(D, dev, False)
    start = N(a["scalars"])
    for step in range(3):
        simulate(cfg, a, None, "jacobi", fused=fused)
        simulate(cfg, b, None, "jacobi", fused=fused)
        assert a["scalars"].shape == start.shape
        assert_bitexact(N(a["scalars"][:, 0:1]), N(a["density"]), f"D={D} fused={fused} correctScalar={correct} step {step}: channel 0 vs density")
        for k in ("p", "U", "density"):
            assert_bitexact(N(a[k]), N(b[k]), f"D={D} fused={fused} correctScalar={correct} step {step}: {k} with and without the key")
    got = N(a["scalars"])
    assert np.isfinite(got).all() and (got[:, 1:] != start[:, 1:]).mean() > 0.2, "the other channels moved"
    _simulate.release_workspaces()


def test_simulate_without_density_and_with_output_div(dev):
    from fluidnet_cxx_amd import fluid, simulate
    cfg = dict(PLUME_CFG, jacobiIter=9)
    for kw in (dict(), dict(output_div=True)):
        a = _sim_state(1, dev, True)
        for k in ("density", "densityBC", "densityBCInvMask"):
            del a[k]
        s0, U0, f = a["scalars"].clone(), a["U"].clone(), a["flags"]
        simulate(cfg, a, None, "jacobi", **kw)
        want = fluid.advectScalars(cfg["dt"], s0, U0, f, MAC, 1, cfg["sampleOutsideFluid"], cfg["maccormackStrength"])
        want = want * a["scalarsBCInvMask"] + a["scalarsBC"]
        assert_bitexact(N(a["scalars"]), N(want), f"no density key, {kw}")


def test_simulate_refuses_a_view_with_the_key(dev, ext):
    from fluidnet_cxx_amd import simulate
    cfg = dict(PLUME_CFG, jacobiIter=4)
    for geom in (ext.Geom(k_begin=2, k_end=6), ext.Geom(z_offset=2, D_global=40)):
        a = _sim_state(8, dev, True)
        with pytest.raises(ValueError, match="single-domain only"):
            simulate(cfg, a, None, "jacobi", geom=geom)


def test_step_with_scalars_is_graph_capturable(dev):
    """one captured 2D step replayed three times = three eager steps.  The stage is out of place (batch_dict['scalars'] = s), so the
    graph reads the tensor the key held at capture time and writes the one it holds afterwards: the caller copies one into the other
    between replays, as for any out-of-place graph output"""
    from fluidnet_cxx_amd import _simulate, simulate
    _simulate.release_workspaces()
    cfg = dict(PLUME_CFG, jacobiIter=9)
    a, b = _sim_state(1, dev, True), _sim_state(1, dev, True)
    for _ in range(2):
        simulate(cfg, a, None, "jacobi")
        simulate(cfg, b, None, "jacobi", static_flags=0)
    torch.cuda.synchronize()
    s_in = a["scalars"]
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        simulate(cfg, a, None, "jacobi")
    s_out = a["scalars"]
    assert s_out.data_ptr() != s_in.data_ptr()
    for _ in range(3):
        g.replay()
        s_in.copy_(s_out)
        simulate(cfg, b, None, "jacobi", static_flags=0)
    torch.cuda.synchronize()
    for k in ("U", "density", "p", "scalars"):
        assert torch.equal(a[k], b[k]), k
    assert_bitexact(N(a["scalars"][:, 0:1]), N(a["density"]), "channel 0 vs density after the replays")
    _simulate.release_workspaces()


# ---- output files and the driver
def test_save_state_writes_the_scalars(dev, tmp_path):
    from fluidnet_cxx_amd import output
    for D in (1, 8):
        with_key, without = _sim_state(D, dev, True), _sim_state(D, dev, False)
        da, db = tmp_path / f"a{D}", tmp_path / f"b{D}"
        da.mkdir(); db.mkdir()
        fa = output.save_state(str(da), 7, with_key)
        fb = output.save_state(str(db), 7, without)
        assert [os.path.basename(f) for f in fb] == ["output_00007.png", "output_00007.vtr", "restart.pth"]
        assert [os.path.basename(f) for f in fa] == ["output_00007.png", "scalars_00007.png", "output_00007.vtr", "restart.pth"]
        assert open(fa[1], "rb").read(8) == b"\x89PNG\r\n\x1a\n"
        _, cells_a = output.read_vtr(fa[2])
        _, cells_b = output.read_vtr(fb[1])
        assert sorted(set(cells_a) - set(cells_b)) == ["scalar0", "scalar1", "scalar2"]
        for c in range(3):
            assert_bitexact(cells_a[f"scalar{c}"], np.ascontiguousarray(N(with_key["scalars"][0, c]).transpose(2, 1, 0)), f"scalar{c}")
        for k in cells_b:
            assert_bitexact(cells_a[k], cells_b[k], k)
        img = output.scalars_image(with_key)
        s = N(with_key["scalars"])[0, :, D // 2]
        want = (np.clip(np.moveaxis(s, 0, -1), 0, 1) * 255.0 + 0.5).astype(np.uint8)
        want[N(with_key["flags"])[0, 0, D // 2] == 2.0] = 128
        assert img.shape == (24, 24, 3) and (img == want[::-1]).all()


def test_plume_driver_with_two_dyes(dev, tmp_path):
    """examples/plume.py --res 32 --iters 3 --dyes 2: finite channels whose sum over the inlet rows is the density's BC pattern x 10"""
    spec = importlib.util.spec_from_file_location("plume_example", os.path.join(REPO, "examples", "plume.py"))
    plume = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(plume)
    bd, it = plume.main(["--res", "32", "--iters", "3", "--dyes", "2", "--out-iter", "2", "--folder", str(tmp_path)])
    assert it == 3 and tuple(bd["scalars"].shape) == (1, 2, 1, 32, 32)
    s = N(bd["scalars"])
    assert np.isfinite(s).all()
    rows = s[0, :, :, 0:4].sum(0)
    want = N(bd["densityBC"])[0, 0, :, 0:4] * np.float32(10)
    assert (want > 0).any()
    assert_bitexact(rows, want, "the dyes on the inlet rows")
    for c in range(2):
        assert (s[0, c, :, 0:4] > 0).any(), f"dye {c} enters"
    assert (s[0, 0] * s[0, 1])[:, 0:4].max() == 0, "the sectors do not overlap"
    assert os.path.isfile(tmp_path / "scalars_00000.png") and os.path.isfile(tmp_path / "scalars_00002.png")
