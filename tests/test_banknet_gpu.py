"""The reference's 'FluidNet' bank model on the GPU (fnx_banknet.hip): the net against the float64 model of tests/banknet_reference.py
and the whole forward and the 'convnet' step against what the reference computed (tests/golden/banknet.npz), all under weights with
which every level reaches the output (tests/test_banknet_host.py shows that they do); batch independence, repeatability, graph replay,
the operator path of simulate(), 'hybrid', and that the ScaleNet path is left as it was."""
import os

import numpy as np
import pytest
import torch

from banknet_reference import GOLDEN_SHAPES, SHAPES, bank_input, banknet_forward64, propagating_bank_weights
from util import PLUME_CFG, assert_bitexact, assert_close_rel, plume_state

pytestmark = pytest.mark.gpu

MCONF = dict(PLUME_CFG, model="FluidNet", inputChannels=dict(div=True, pDiv=False, UDiv=False), normalizeInput=True,
             normalizeInputChan="UDiv", inputDim=2, is3D=False)
KEYS = ("U", "density", "p")
IDS = ["x".join(map(str, s)) for s in SHAPES]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "banknet.npz"))


@pytest.fixture(scope="module")
def net(dev):
    from fluidnet_cxx_amd import FluidNet
    return FluidNet.from_weights(MCONF, propagating_bank_weights(), dev).eval()


@pytest.fixture(scope="module")
def refs():
    """(x, float64 p) per shape, computed once"""
    w = propagating_bank_weights()
    out = {}
    for s in SHAPES:
        x = bank_input(*s, boxes=s[1] >= 16)
        out[s] = (x, banknet_forward64(w, x).numpy())
    return out


def T(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(dev)


def N(t):
    return t.detach().cpu().numpy()


def forward_input(golden, i):
    U, flags = golden[f"fwd{i}_U"], golden[f"fwd{i}_flags"]
    zero = np.zeros_like(flags)
    return np.concatenate([zero, U, flags, zero], 1)


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_bank_vs_float64_model(dev, net, refs, shape):
    x, ref = refs[shape]
    got = N(net.bank(T(x, dev)))
    print(f"{shape}: {np.abs(got - ref).max() / np.abs(ref).max():.2e} |ref|max")
    assert_close_rel(got, ref, 1e-5, f"net.bank at {shape}")


@pytest.mark.parametrize("i", range(len(GOLDEN_SHAPES)), ids=IDS[:len(GOLDEN_SHAPES)])
def test_forward_vs_reference(dev, net, golden, i):
    """FluidNet.forward (p, U) and the net alone on the reference's own net input, against the reference"""
    p, U = net(T(forward_input(golden, i), dev))
    assert_close_rel(N(p), golden[f"fwd{i}_p"], 1e-5, f"forward p at {GOLDEN_SHAPES[i]}")
    assert_close_rel(N(U), golden[f"fwd{i}_Uout"], 1e-5, f"forward U at {GOLDEN_SHAPES[i]}")
    assert_close_rel(N(net.bank(T(golden[f"fwd{i}_net_x"], dev))), golden[f"fwd{i}_net_p"], 1e-5, f"net at {GOLDEN_SHAPES[i]}")


def test_a_sample_does_not_depend_on_the_batch(dev, net, refs, golden):
    x = T(refs[(3, 36, 68)][0], dev)
    whole = N(net.bank(x))
    inp = T(forward_input(golden, 3), dev)
    p, U = (N(t) for t in net(inp))
    for b in range(3):
        assert_bitexact(N(net.bank(x[b:b + 1].contiguous()))[0], whole[b], f"net, sample {b}")
        pb, Ub = net(inp[b:b + 1].contiguous())
        assert_bitexact(N(pb)[0], p[b], f"forward p, sample {b}")
        assert_bitexact(N(Ub)[0], U[b], f"forward U, sample {b}")


def test_repeatable_and_graph_replay(dev, net, refs, golden):
    x = T(refs[(3, 36, 68)][0], dev)
    inp = T(forward_input(golden, 3), dev)
    eager = [N(net.bank(x))] + [N(t) for t in net(inp)]
    again = [N(net.bank(x))] + [N(t) for t in net(inp)]
    for a, b, what in zip(eager, again, ("net", "p", "U")):
        assert_bitexact(a, b, f"second call, {what}")
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        q = net.bank(x)
        p, U = net(inp)
    for _ in range(2):
        q.zero_(); p.zero_(); U.zero_()
        g.replay()
        torch.cuda.synchronize()
        for a, b, what in zip(eager, (q, p, U), ("net", "p", "U")):
            assert_bitexact(a, N(b), f"graph replay, {what}")


def hand_step(fluid, cfg, bd, net):
    """one 'convnet' step of the plume configuration, operator by operator in the reference's order (simulate.py:28-171)"""
    p, U, flags = bd["p"], bd["U"], bd["flags"]
    dt = cfg["dt"]
    rho = fluid.advectScalar(dt, bd["density"], U, flags, method="maccormackFluidNet", boundary_width=1,
                             sample_outside_fluid=cfg["sampleOutsideFluid"], maccormack_strength=cfg["maccormackStrength"])
    U = fluid.advectVelocity(dt=dt, orig=U, U=U, flags=flags, method="maccormackFluidNet", boundary_width=1,
                             maccormack_strength=cfg["maccormackStrength"])
    fluid.setConstVals(bd, p, U, flags, rho)
    g = cfg["gravityVec"]
    gravity = (torch.tensor([g["x"], g["y"], g["z"]], dtype=torch.float32) * (-cfg["buoyancyScale"])).tolist()
    U = fluid.addBuoyancy(U, flags, rho, gravity, cfg["operatingDensity"], dt)
    fluid.setConstVals(bd, p, U, flags, rho)
    p, U = net(torch.cat((p, U, flags, rho), 1))
    fluid.setConstVals(bd, p, U, flags, rho)
    bd.update(p=p, U=U, density=rho)


def test_convnet_step_vs_hand_composition_and_reference(dev, net, golden):
    """simulate(..., 'convnet') with a bank net takes the operator path whatever `fused` says: the operators composed by hand, bit for
    bit, and the reference's states after 1 and 2 steps"""
    from fluidnet_cxx_amd import fluid, simulate
    assert int(golden["steps"]) == 2
    for k in ("flags", "UBC", "UBCInvMask", "densityBC", "densityBCInvMask"):
        assert np.array_equal(golden[k], plume_state(64)[k]), k
    runs = {}
    for how in (True, False, "hand"):
        bd = {k: T(v, dev) for k, v in plume_state(64).items()}
        runs[how] = []
        for it in (1, 2):
            if how == "hand":
                hand_step(fluid, MCONF, bd, net)
            else:
                simulate(MCONF, bd, net, "convnet", fused=how)
            runs[how].append({k: N(bd[k]) for k in KEYS})
    for it in (1, 2):
        for k in KEYS:
            assert_bitexact(runs[True][it - 1][k], runs["hand"][it - 1][k], f"fused=True vs by hand: {k} after {it}")
            assert_bitexact(runs[False][it - 1][k], runs["hand"][it - 1][k], f"fused=False vs by hand: {k} after {it}")
            assert_close_rel(runs[True][it - 1][k], golden[f"step{it}_{k}"], 1e-5, f"convnet {k} after {it}")


def test_hybrid_with_a_bank_net_converges(dev, net):
    """'hybrid' starts the converged solve from the bank net's pressure: the projection leaves what 'pcg' leaves (pcgTol), the guess
    is used, and fused=True is the operator path"""
    from fluidnet_cxx_amd import _simulate, fluid, simulate
    from test_hybrid_gpu import divergence_norm, remaining_divergence
    cfg = dict(MCONF, pcgTol=1e-5, pcgIter=60)
    bd = {k: T(v, dev) for k, v in plume_state(64).items()}
    for _ in range(3):
        simulate(PLUME_CFG, bd, None, "jacobi")
    U0 = bd["U"].clone()
    fluid.setWallBcs(U0, bd["flags"])
    p0, _ = net(torch.cat((bd["p"], U0, bd["flags"], bd["density"]), 1))
    norm = divergence_norm(bd["flags"], False)
    left, iters, _ = remaining_divergence(fluid, bd, False, norm, p0)
    left_cold, cold, _ = remaining_divergence(fluid, bd, False, norm, None)
    print(f"remaining divergence from the bank net's pressure: {left:.3e} after {iters} iterations (cold: {left_cold:.3e}, {cold})")
    assert left <= 2e-5, left
    runs = []
    for fused in (True, False):
        b2 = {k: v.clone() for k, v in bd.items()}
        for _ in range(2):
            simulate(cfg, b2, net, "hybrid", fused=fused)
        runs.append({k: N(b2[k]) for k in KEYS})
    b3 = {k: v.clone() for k, v in bd.items()}
    for _ in range(2):
        simulate(cfg, b3, None, "pcg")
    for k in KEYS:
        assert_bitexact(runs[0][k], runs[1][k], f"hybrid fused / operator path: {k}")
        assert np.isfinite(runs[0][k]).all()
    assert not np.array_equal(runs[0]["p"].view(np.int32), N(b3["p"]).view(np.int32)), "the guess is used"
    _simulate.release_workspaces()


def test_scalenet_path_is_left_as_it_was(dev, net, refs, golden):
    """A ScaleNet forward (tests/golden/cnn.npz input) and a 'convnet' step of the 64x64 plume give the same bits before and after bank
    forwards on the same stream: the bank path leaves nothing behind"""
    from fluidnet_cxx_amd import FluidNet, _simulate, simulate
    from fluidnet_cxx_amd.weights import make_scalenet_weights
    here = os.path.dirname(os.path.abspath(__file__))
    inp = T(np.load(os.path.join(here, "golden", "cnn.npz"))["fluidnet_in"], dev)
    sconf = dict(MCONF, model="ScaleNet")
    snet = FluidNet.from_weights(sconf, make_scalenet_weights(0), dev)

    def scalenet_run():
        _simulate.release_workspaces()
        p, U = snet(inp)
        bd = {k: T(v, dev) for k, v in plume_state(64).items()}
        simulate(sconf, bd, snet, "convnet")
        return [N(p), N(U)] + [N(bd[k]) for k in KEYS]

    before = scalenet_run()
    net.bank(T(refs[(1, 132, 260)][0], dev))
    net(T(forward_input(golden, 3), dev))
    after = scalenet_run()
    for a, b, what in zip(before, after, ("p", "U", "step U", "step density", "step p")):
        assert_bitexact(a, b, f"ScaleNet {what} after a bank forward")
    _simulate.release_workspaces()


def test_refusals(dev, net):
    from fluidnet_cxx_amd import FluidNet
    from fluidnet_cxx_amd._ext import ext
    with pytest.raises(RuntimeError, match="2D only"):
        ext.banknet_forward(net.bank.packed, torch.zeros(1, 2, 4, 8, 8, device=dev), "fp32")
    with pytest.raises(RuntimeError, match="2D only"):
        ext.fluidnet_bank_forward(net.bank.packed, torch.zeros(1, 6, 4, 8, 8, device=dev), 1e-5, "fp32")
    with pytest.raises(RuntimeError, match="H = 18 must be a positive multiple of 4"):
        net.bank(torch.zeros(1, 2, 18, 24, device=dev))
    with pytest.raises(RuntimeError, match="W = 26 must be a positive multiple of 4"):
        net(torch.zeros(1, 5, 1, 16, 26, device=dev))
    for mode in ("bf16x6", "bf16x3"):
        with pytest.raises(RuntimeError, match="fp32 arithmetic only"):
            ext.banknet_forward(net.bank.packed, torch.zeros(1, 2, 8, 8, device=dev), mode)
        half = FluidNet.from_weights(dict(MCONF, precisionMode=mode), propagating_bank_weights(), dev)
        with pytest.raises(RuntimeError, match="fp32 arithmetic only"):
            half(torch.zeros(1, 5, 1, 8, 8, device=dev))
    with pytest.raises(RuntimeError, match="image from banknet_pack"):
        ext.banknet_forward(torch.zeros(16, dtype=torch.uint8, device=dev), torch.zeros(1, 2, 8, 8, device=dev), "fp32")
    with pytest.raises(RuntimeError, match="bank model"):
        net.packed_for(dev)
    # every fp32 mode runs the one kernel family: the same bits
    x = torch.from_numpy(bank_input(1, 16, 24, boxes=True)).to(dev)
    base = N(net.bank(x))
    for mode in ("fp32_direct", "fp32_f4", "fp32_f2"):
        assert_bitexact(N(ext.banknet_forward(net.bank.packed, x, mode)), base, mode)
