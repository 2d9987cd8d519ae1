"""The Conv3d bank net ('FluidNet3D') on the GPU (fnx_banknet3d.hip): the net and the whole forward against the float64 model of
tests/banknet3d_reference.py under weights with which every level reaches the output (tests/test_banknet3d_host.py shows that they do);
batch independence, repeatability, graph replay, the operator path of simulate() for 'convnet' and 'hybrid', that the 3D ScaleNet path
is left as it was, and the refusals through the binding."""
import numpy as np
import pytest
import torch

from banknet3d_reference import SHAPES3D, bank3d_input, banknet3d_forward64, propagating_bank3d_weights
from test_banknet_gpu import hand_step
from util import PLUME_CFG, assert_bitexact, assert_close_rel, plume_state

pytestmark = pytest.mark.gpu

MCONF = dict(PLUME_CFG, model="FluidNet3D", inputChannels=dict(div=True, pDiv=False, UDiv=False), normalizeInput=True,
             normalizeInputChan="UDiv", inputDim=3, is3D=True)
KEYS = ("U", "density", "p")
IDS = ["x".join(map(str, s)) for s in SHAPES3D]
BATCH = (2, 8, 12, 20)              # the shape of the batch tests: two samples, three y tiles and two z chunks at full resolution


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def net(dev):
    from fluidnet_cxx_amd import FluidNet
    return FluidNet.from_weights(MCONF, propagating_bank3d_weights(), dev).eval()


@pytest.fixture(scope="module")
def refs():
    """(x, float64 p) per shape, computed once"""
    w = propagating_bank3d_weights()
    out = {}
    for s in SHAPES3D:
        x = bank3d_input(*s)
        out[s] = (x, banknet3d_forward64(w, x).numpy())
    return out


def T(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(dev)


def N(t):
    return t.detach().cpu().numpy()


def plume3d(dev, res=24, D=12, obstacle=True):
    """the 3D plume's initial state on a D x res x res grid, with an obstacle box above the inlet"""
    st = plume_state(res, D=D)
    if obstacle:
        st["flags"][0, 0, D // 3:D // 3 + 3, res // 2:res // 2 + 3, res // 3:res // 3 + 5] = 2
    return {k: T(v, dev) for k, v in st.items()}


@pytest.fixture(scope="module")
def forward_input(dev):
    """(2,6,12,24,24) = [p, U, flags, density]: the plume with an obstacle after two and after three 'jacobi' steps"""
    from fluidnet_cxx_amd import _simulate, simulate
    bd = plume3d(dev)
    samples = []
    for it in range(3):
        simulate(PLUME_CFG, bd, None, "jacobi")
        if it >= 1:
            samples.append(torch.cat((bd["p"], bd["U"], bd["flags"], bd["density"]), 1))
    _simulate.release_workspaces()
    return torch.cat(samples, 0).contiguous()


@pytest.mark.parametrize("shape", SHAPES3D, ids=IDS)
def test_bank_vs_float64_model(dev, net, refs, shape):
    """1e-5 |ref|max, the project's CNN tolerance.  Measured on an MI355X: 5.3e-7, 1.5e-6, 1.3e-6, 1.1e-6, 1.2e-6 |ref|max."""
    x, ref = refs[shape]
    got = N(net.bank(T(x, dev)))
    print(f"{shape}: {np.abs(got - ref).max() / np.abs(ref).max():.2e} |ref|max")
    assert_close_rel(got, ref, 1e-5, f"net.bank at {shape}")


def test_forward_vs_float64_composition(dev, net, forward_input):
    """net(input) against the composition around the float64 model: div = fluid.velocityDivergence(U, flags), s = clamp(unbiased std of U
    per sample, thr), p = model([div / s, occupancy]), velocityUpdate(p, U / s), p s and U s, setWallBcs"""
    from fluidnet_cxx_amd import fluid
    inp = forward_input
    p, U = net(inp)
    B = inp.size(0)
    U0, flags = inp[:, 1:4].contiguous(), inp[:, 4:5].contiguous()
    assert set(np.unique(N(flags))) == {1.0, 2.0}
    div = N(fluid.velocityDivergence(U0, flags)).astype(np.float64)
    s = np.maximum(N(U0).astype(np.float64).reshape(B, -1).std(axis=1, ddof=1), MCONF["normalizeInputThreshold"]).reshape(B, 1, 1, 1, 1)
    assert (s > 1e-3).all(), "the state moves"
    x = np.concatenate((div / s, (N(flags) == 2.0).astype(np.float64)), 1)
    p_ref = banknet3d_forward64(propagating_bank3d_weights(), x).numpy()
    U_ref = T(N(U0) / s, dev)
    fluid.velocityUpdate(T(p_ref, dev), U_ref, flags)
    U_ref = T(N(U_ref).astype(np.float64) * s, dev)
    fluid.setWallBcs(U_ref, flags)
    for got, ref, what in ((p, p_ref * s, "p"), (U, N(U_ref), "U")):
        print(f"forward {what}: {np.abs(N(got) - ref).max() / np.abs(ref).max():.2e} |ref|max")
        assert_close_rel(N(got), ref, 1e-5, f"forward {what}")
    assert np.abs(p_ref).max() > 0 and np.abs(N(U) - N(U0)).max() > 1e-3 * np.abs(N(U0)).max(), "the projection moves U"


def test_a_sample_does_not_depend_on_the_batch(dev, net, refs, forward_input):
    x = T(refs[BATCH][0], dev)
    whole = N(net.bank(x))
    p, U = (N(t) for t in net(forward_input))
    for b in range(2):
        assert_bitexact(N(net.bank(x[b:b + 1].contiguous()))[0], whole[b], f"net, sample {b}")
        pb, Ub = net(forward_input[b:b + 1].contiguous())
        assert_bitexact(N(pb)[0], p[b], f"forward p, sample {b}")
        assert_bitexact(N(Ub)[0], U[b], f"forward U, sample {b}")
    # a sample of the batch in another batch position
    swapped = N(net.bank(torch.flip(x, (0,)).contiguous()))
    assert_bitexact(swapped[1], whole[0], "net, sample 0 in position 1")


def test_repeatable_and_graph_replay(dev, net, refs, forward_input):
    x = T(refs[BATCH][0], dev)
    inp = forward_input
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


def test_convnet_step_vs_hand_composition(dev, net):
    """simulate(..., 'convnet') with a 3D bank net takes the operator path whatever `fused` says: the public operators composed by hand
    (test_banknet_gpu.hand_step), bit for bit, over two steps"""
    from fluidnet_cxx_amd import _simulate, fluid, simulate
    runs = {}
    for how in (True, False, "hand"):
        bd = plume3d(dev)
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
            assert np.isfinite(runs[True][it - 1][k]).all()
    assert np.abs(runs[True][1]["p"]).max() > 0
    _simulate.release_workspaces()


def test_hybrid_with_a_3d_bank_net(dev, net):
    """'hybrid' starts the converged solve from the bank net's pressure on a 3D state: fused=True is the operator path, the guess is
    used, and the projection leaves what 'pcg' leaves"""
    from fluidnet_cxx_amd import _simulate, fluid, simulate
    from test_hybrid_gpu import divergence_norm, remaining_divergence
    cfg = dict(MCONF, pcgTol=1e-5, pcgIter=60)
    bd = plume3d(dev)
    for _ in range(3):
        simulate(PLUME_CFG, bd, None, "jacobi")
    U0 = bd["U"].clone()
    fluid.setWallBcs(U0, bd["flags"])
    p0, _ = net(torch.cat((bd["p"], U0, bd["flags"], bd["density"]), 1))
    norm = divergence_norm(bd["flags"], True)
    left, iters, _ = remaining_divergence(fluid, bd, True, norm, p0)
    print(f"remaining divergence from the 3D bank net's pressure: {left:.3e} after {iters} iterations")
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


def test_scalenet_path_is_left_as_it_was(dev, net, refs, forward_input):
    """A 3D ScaleNet forward and a 'convnet' step of the 3D plume give the same bits before and after bank forwards on the same stream"""
    from fluidnet_cxx_amd import FluidNet, _simulate, simulate
    from fluidnet_cxx_amd.weights import make_scalenet_weights
    sconf = dict(MCONF, model="ScaleNet")
    snet = FluidNet.from_weights(sconf, make_scalenet_weights(0, ndim=3), dev)

    def scalenet_run():
        _simulate.release_workspaces()
        p, U = snet(forward_input)
        bd = plume3d(dev)
        simulate(sconf, bd, snet, "convnet")
        return [N(p), N(U)] + [N(bd[k]) for k in KEYS]

    before = scalenet_run()
    net.bank(T(refs[(1, 20, 12, 132)][0], dev))
    net(forward_input)
    after = scalenet_run()
    for a, b, what in zip(before, after, ("p", "U", "step U", "step density", "step p")):
        assert_bitexact(a, b, f"ScaleNet {what} after a bank forward")
    _simulate.release_workspaces()


def test_refusals(dev, net):
    from fluidnet_cxx_amd import FluidNet
    from fluidnet_cxx_amd._ext import ext
    packed = net.bank.packed
    with pytest.raises(RuntimeError, match="3D only"):
        ext.banknet3d_forward(packed, torch.zeros(1, 2, 8, 8, device=dev), "fp32")
    with pytest.raises(RuntimeError, match="3D only"):
        ext.fluidnet_bank3d_forward(packed, torch.zeros(1, 5, 1, 8, 8, device=dev), 1e-5, "fp32")
    for shape, text in (((1, 2, 6, 8, 8), "D = 6"), ((1, 2, 8, 18, 24), "H = 18"), ((1, 2, 8, 16, 26), "W = 26")):
        with pytest.raises(RuntimeError, match=text + " must be a positive multiple of 4"):
            net.bank(torch.zeros(shape, device=dev))
        with pytest.raises(RuntimeError, match=text + " must be a positive multiple of 4"):
            net(torch.zeros((1, 6) + shape[2:], device=dev))
    for mode in ("bf16x6", "bf16x3"):
        with pytest.raises(RuntimeError, match="fp32 arithmetic only"):
            ext.banknet3d_forward(packed, torch.zeros(1, 2, 8, 8, 8, device=dev), mode)
        half = FluidNet.from_weights(dict(MCONF, precisionMode=mode), propagating_bank3d_weights(), dev)
        with pytest.raises(RuntimeError, match="fp32 arithmetic only"):
            half(torch.zeros(1, 6, 8, 8, 8, device=dev))
    with pytest.raises(RuntimeError, match="image from banknet3d_pack"):
        ext.banknet3d_forward(torch.zeros(16, dtype=torch.uint8, device=dev), torch.zeros(1, 2, 8, 8, 8, device=dev), "fp32")
    # the 2D net's image and entry points stay what they were: a 3D tensor is refused there, and neither image passes for the other
    with pytest.raises(RuntimeError, match="image from banknet_pack"):
        ext.banknet_forward(packed, torch.zeros(1, 2, 8, 8, device=dev), "fp32")
    with pytest.raises(RuntimeError, match="bank model"):
        net.packed_for(dev)
    # every fp32 mode runs the one kernel family: the same bits
    x = torch.from_numpy(bank3d_input(1, 8, 12, 20)).to(dev)
    base = N(net.bank(x))
    for mode in ("fp32_direct", "fp32_f4", "fp32_f2"):
        assert_bitexact(N(ext.banknet3d_forward(packed, x, mode)), base, mode)


def test_plume_driver_runs_a_fluidnet3d_checkpoint(dev, tmp_path):
    """examples/plume.py --depth N --method convnet --weights3d CKPT with a checkpoint whose mconf['model'] is 'FluidNet3D': the
    checkpoint's mconf picks the net; a depth that is no multiple of 4 is refused with a sentence, not a traceback"""
    import os
    import subprocess
    import sys
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    ck = str(tmp_path / "bank3d.pth")
    torch.save(dict(state_dict={k: torch.from_numpy(v) for k, v in propagating_bank3d_weights().items()},
                    mconf={k: v for k, v in MCONF.items() if k not in PLUME_CFG or k == "normalizeInputThreshold"}), ck)
    out = tmp_path / "plume3d"
    base = [sys.executable, os.path.join(repo, "examples", "plume.py"), "--res", "24", "--iters", "2", "--out-iter", "1", "--method", "convnet",
            "--weights3d", ck, "--folder", str(out)]
    r = subprocess.run(base + ["--depth", "12"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "It = 0" in r.stdout and any(n.endswith(".png") or n.endswith(".vtk") or n.endswith(".pth") for n in os.listdir(out)), os.listdir(out)
    # in this process: the same driver on a depth the net cannot take ends with its sentence before anything is allocated
    import importlib.util
    spec = importlib.util.spec_from_file_location("plume_driver", base[1])
    plume = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(plume)
    with pytest.raises(SystemExit, match="must be multiples of 4"):
        plume.main(base[2:] + ["--depth", "10"])
