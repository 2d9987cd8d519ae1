"""The 'FluidNet' bank net in the native step (fnx_simulate_step_net) on the GPU: simulate(..., 'convnet' | 'hybrid') with such a net runs
the native step, with the bits of the operator path -- plain, with flags_stick, with the optional 2D stages, on the static path, in a
HIP graph and with the training net -- and leaves the ScaleNet step as it was.  The Conv3d bank net ('FluidNet3D') stays on the operator
path: the step refuses its kind.

Small plumes with an obstacle box and inlet BCs: 2D B = 2, 36 x 68 (partial tiles in both axes), 3D B = 2, 12 x 24 x 36; the weights
are those under which every level of the net reaches the output (propagating_bank_weights / propagating_bank3d_weights)."""
import numpy as np
import pytest
import torch

from banknet3d_reference import propagating_bank3d_weights
from banknet_reference import propagating_bank_weights
from util import PLUME_CFG, assert_bitexact, box_plume_state

pytestmark = pytest.mark.gpu

NET = dict(inputChannels=dict(div=True, pDiv=False, UDiv=False), normalizeInput=True, normalizeInputChan="UDiv")
MCONF = {2: dict(PLUME_CFG, model="FluidNet", inputDim=2, is3D=False, pcgTol=1e-5, pcgIter=40, **NET),
         3: dict(PLUME_CFG, model="FluidNet3D", inputDim=3, is3D=True, pcgTol=1e-5, pcgIter=40, **NET)}
SHAPE = {2: (2, 1, 36, 68), 3: (2, 12, 24, 36)}
WEIGHTS = {2: propagating_bank_weights, 3: propagating_bank3d_weights}
KEYS = ("p", "U", "density")
CASES = [(2, "convnet"), (2, "hybrid")]
CASE_IDS = [f"{nd}d-{m}" for nd, m in CASES]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def nets(dev):
    from fluidnet_cxx_amd import FluidNet
    return {nd: FluidNet.from_weights(MCONF[nd], WEIGHTS[nd](), dev).eval() for nd in (2, 3)}


@pytest.fixture(autouse=True)
def fresh_workspaces():
    from fluidnet_cxx_amd import _simulate
    _simulate.release_workspaces()
    yield
    _simulate.release_workspaces()


def N(t):
    return t.detach().cpu().numpy()


def plume(ndim, dev, stick=False):
    """util.box_plume_state on the (B, D, H, W) grid of SHAPE[ndim], on the device"""
    return {k: torch.from_numpy(v).to(dev) for k, v in box_plume_state(*SHAPE[ndim], stick=stick).items()}


def run(cfg, bd, net, method, steps, **kw):
    """`steps` steps of simulate() on bd; the state after each"""
    from fluidnet_cxx_amd import simulate
    out = []
    for _ in range(steps):
        simulate(cfg, bd, net, method, **kw)
        out.append({k: N(bd[k]) for k in KEYS})
    return out


def same_bits(a, b, what):
    assert len(a) == len(b)
    for it, (x, y) in enumerate(zip(a, b), 1):
        for k in KEYS:
            assert np.isfinite(x[k]).all(), f"{what}: {k} after {it} steps is not finite"
            assert_bitexact(x[k], y[k], f"{what}: {k} after {it} steps")
    assert np.abs(a[-1]["p"]).max() > 0 and np.abs(a[-1]["U"]).max() > 0, what


@pytest.mark.parametrize("ndim,method", CASES, ids=CASE_IDS)
def test_the_native_path_is_taken(dev, nets, monkeypatch, ndim, method):
    """With fluid.advectVelocity replaced by a function that raises, the step of a bank net still runs: it does not go operator by
    operator.  (fused=False does, and raises.)"""
    from fluidnet_cxx_amd import _simulate

    def no_operator_path(*args, **kw):
        raise AssertionError("simulate() took the operator path")

    monkeypatch.setattr(_simulate.fluid, "advectVelocity", no_operator_path)
    bd = plume(ndim, dev)
    out = run(MCONF[ndim], bd, nets[ndim], method, 2)
    assert np.isfinite(out[-1]["U"]).all() and np.abs(out[-1]["p"]).max() > 0
    with pytest.raises(AssertionError, match="operator path"):
        run(MCONF[ndim], plume(ndim, dev), nets[ndim], method, 1, fused=False)


@pytest.mark.parametrize("ndim,method", CASES, ids=CASE_IDS)
def test_same_bits_as_the_operator_path(dev, nets, ndim, method):
    native = run(MCONF[ndim], plume(ndim, dev), nets[ndim], method, 3)
    operators = run(MCONF[ndim], plume(ndim, dev), nets[ndim], method, 3, fused=False)
    same_bits(native, operators, f"{ndim}D {method}, fused=True vs fused=False")


def test_same_bits_with_flags_stick_2d(dev, nets):
    native = run(MCONF[2], plume(2, dev, stick=True), nets[2], "convnet", 3)
    operators = run(MCONF[2], plume(2, dev, stick=True), nets[2], "convnet", 3, fused=False)
    same_bits(native, operators, "2D convnet with flags_stick")
    plain = run(MCONF[2], plume(2, dev), nets[2], "convnet", 3)
    assert not np.array_equal(native[-1]["U"], plain[-1]["U"]), "the no-slip cells act on the flow"


@pytest.mark.parametrize("method", ["convnet", "hybrid"])
def test_same_bits_with_the_optional_stages_2d(dev, nets, method):
    """viscosity (dt = 0.1 with 0.02: a pair whose product the step's two floats give), gravityScale, correctScalar and the vorticity
    confinement together"""
    cfg = dict(MCONF[2], viscosity=0.02, gravityScale=0.5, correctScalar=True, vorticityConfinementAmp=0.3)
    native = run(cfg, plume(2, dev), nets[2], method, 3)
    operators = run(cfg, plume(2, dev), nets[2], method, 3, fused=False)
    same_bits(native, operators, f"2D {method} with the optional stages")
    plain = run(MCONF[2], plume(2, dev), nets[2], method, 3)
    assert not np.array_equal(native[-1]["U"], plain[-1]["U"])


@pytest.mark.parametrize("ndim,method", CASES, ids=CASE_IDS)
def test_static_path(dev, nets, ndim, method):
    """Five steps of the four-argument call (the automatic static mode: from the third step on the class map, in 3D the stage words,
    and the PCG hierarchy are reused) against five steps at static_flags=0 on an explicit workspace, and against the explicit promises
    0, 3, 7, 7, 7 (with 8 for the kept hierarchy) on a workspace of FNX_OP_STEP_STATIC's size"""
    from fluidnet_cxx_amd import simulate
    from fluidnet_cxx_amd._ext import ext
    B, D, H, W = SHAPE[ndim]
    auto = run(MCONF[ndim], plume(ndim, dev), nets[ndim], method, 5)
    ws = torch.empty(ext.step_workspace_bytes(B, D, H, W, ndim == 3), dtype=torch.uint8, device=dev)
    fresh = run(MCONF[ndim], plume(ndim, dev), nets[ndim], method, 5, workspace=ws, static_flags=0)
    same_bits(auto, fresh, f"{ndim}D {method}: automatic static mode vs static_flags=0")
    ws.fill_(0xA5)
    bd, promised = plume(ndim, dev), []
    for it in range(5):
        bits = (0, 3, 7, 7, 7)[it] | (8 if method == "hybrid" and it > 0 else 0)
        simulate(MCONF[ndim], bd, nets[ndim], method, workspace=ws, static_flags=bits)
        promised.append({k: N(bd[k]) for k in KEYS})
    same_bits(promised, fresh, f"{ndim}D {method}: explicit promises vs static_flags=0")


@pytest.mark.parametrize("ndim", [2])
def test_graph_replay(dev, nets, ndim):
    """one native 'convnet' step captured and replayed twice: the states of two eager steps from the same state"""
    from fluidnet_cxx_amd import simulate
    a, b = plume(ndim, dev), plume(ndim, dev)
    run(MCONF[ndim], a, nets[ndim], "convnet", 2)
    run(MCONF[ndim], b, nets[ndim], "convnet", 2)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        simulate(MCONF[ndim], a, nets[ndim], "convnet")
    for it in (1, 2):
        g.replay()
        simulate(MCONF[ndim], b, nets[ndim], "convnet")
        torch.cuda.synchronize()
        for k in KEYS:
            assert_bitexact(N(a[k]), N(b[k]), f"{ndim}D graph replay {it}: {k}")
    assert np.isfinite(N(a["U"])).all() and np.abs(N(a["p"])).max() > 0


@pytest.mark.parametrize("ndim", [2])
def test_training_nets_hand_out_their_current_image(dev, nets, ndim):
    """Under no_grad, simulate() with FluidNetBankTrain gives the bits of FluidNet holding the same weights; after an in-place update of
    a parameter, those of a fresh FluidNet built from the new weights"""
    from fluidnet_cxx_amd import FluidNet, FluidNetBankTrain
    tnet = FluidNetBankTrain(MCONF[ndim])
    tnet.load_state_dict({k: torch.from_numpy(v) for k, v in WEIGHTS[ndim]().items()})
    tnet = tnet.to(dev)
    assert tnet.step_net(dev)[0] == "bank"
    for method in ("convnet", "hybrid"):
        with torch.no_grad():
            got = run(MCONF[ndim], plume(ndim, dev), tnet, method, 2)
        same_bits(got, run(MCONF[ndim], plume(ndim, dev), nets[ndim], method, 2), f"{ndim}D {method}: training net vs FluidNet")
    before = tnet.step_net(dev)[1].clone()
    with torch.no_grad():
        tnet.conv1.weight.mul_(1.25)
        tnet.convOut.bias.add_(0.01)
    assert not torch.equal(before, tnet.step_net(dev)[1]), "a new image after the update"
    fresh = FluidNet.from_weights(MCONF[ndim], {k: v.detach().cpu() for k, v in tnet.state_dict().items()}, dev).eval()
    with torch.no_grad():
        got = run(MCONF[ndim], plume(ndim, dev), tnet, "convnet", 2)
    same_bits(got, run(MCONF[ndim], plume(ndim, dev), fresh, "convnet", 2), f"{ndim}D: the updated training net vs a fresh FluidNet")
    old = run(MCONF[ndim], plume(ndim, dev), nets[ndim], "convnet", 2)
    assert not np.array_equal(got[-1]["p"], old[-1]["p"]), "the update reaches the step"


@pytest.mark.parametrize("ndim", [2, 3])
def test_scalenet_step_is_left_as_it_was(dev, nets, ndim):
    """a ScaleNet 'convnet' step, 2D and 3D, gives the same bits before and after native bank steps (2D: on the same cached workspace)
    and a step of the net of its own dimension"""
    from fluidnet_cxx_amd import FluidNet
    from fluidnet_cxx_amd.weights import make_scalenet_weights
    sconf = dict(MCONF[ndim], model="ScaleNet")
    snet = FluidNet.from_weights(sconf, make_scalenet_weights(0, ndim=ndim), dev).eval()
    assert snet.step_net(dev)[0] == "scalenet" and snet.step_net(dev)[1].data_ptr() == snet.packed_for(dev).data_ptr()
    before = run(sconf, plume(ndim, dev), snet, "convnet", 2)
    run(MCONF[2], plume(2, dev), nets[2], "convnet", 2)
    run(MCONF[2], plume(2, dev), nets[2], "hybrid", 1)
    run(MCONF[ndim], plume(ndim, dev), nets[ndim], "convnet", 1)
    after = run(sconf, plume(ndim, dev), snet, "convnet", 2)
    same_bits(before, after, f"{ndim}D ScaleNet step before and after a bank step")


def test_standalone_cpp_host_runs_a_bank_step(dev, nets, tmp_path):
    """examples/cabi_plume.bin STEPS RES WEIGHTS: a C++ host without torch packs the bank weights and runs the 'convnet' step through
    fnx_simulate_step_net(FNX_NET_BANK); its field hashes are those of simulate() with the same net"""
    import os
    import subprocess
    from fluidnet_cxx_amd import build, fluid, simulate
    from fluidnet_cxx_amd.model import _bank_keys, blob_from_state_dict
    exe = os.path.join(os.path.dirname(build.HERE), "examples", "cabi_plume.bin")
    if not os.path.isfile(exe):                     # normally built by __graft_entry__.build()
        build.build_examples()
    blob = tmp_path / "bank.f32"
    blob_from_state_dict(propagating_bank_weights(), keys=_bank_keys()).astype("<f4").tofile(blob)
    out = subprocess.run([exe, "3", "64", str(blob)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    got = dict(l.split() for l in out.stdout.splitlines()[:3])

    def fnv1a(a):
        h = 1469598103934665603
        for byte in a.tobytes():
            h = ((h ^ byte) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
        return f"{h:016x}"

    bd = dict(p=torch.zeros(1, 1, 1, 64, 64, device=dev), U=torch.zeros(1, 2, 1, 64, 64, device=dev),
              flags=torch.zeros(1, 1, 1, 64, 64, device=dev), density=torch.zeros(1, 1, 1, 64, 64, device=dev))
    fluid.emptyDomain(bd["flags"]); fluid.createPlumeBCs(bd, 0.1, 2, 0.145)
    for _ in range(3):
        simulate(MCONF[2], bd, nets[2], "convnet")
    assert np.abs(N(bd["p"])).max() > 0
    for k in KEYS:
        assert got[k] == fnv1a(N(bd[k])), k
    # a size the net cannot take ends with the C refusal's sentence
    bad = subprocess.run([exe, "1", "66", str(blob)], capture_output=True, text=True, timeout=120)
    assert bad.returncode != 0 and "fnx_simulate_step_net: H = 66 must be a positive multiple of 4" in bad.stderr, bad.stderr


def test_binding_refusals(dev, nets):
    """ext.simulate_step_ checks the image against its kind by size; the kinds the step does not take on a grid raise the C refusals"""
    from fluidnet_cxx_amd import FluidNet, simulate
    from fluidnet_cxx_amd.weights import make_scalenet_weights

    class Mislabelled:
        precision_mode = "fp32"

        def __init__(self, kind, image):
            self.kind, self.image = kind, image

        def step_net(self, device):
            return self.kind, self.image

    snet = FluidNet.from_weights(dict(MCONF[2], model="ScaleNet"), make_scalenet_weights(0, ndim=2), dev).eval()
    kind, image = nets[2].step_net(dev)
    assert kind == "bank"
    image3 = nets[3].bank.packed
    for method in ("convnet", "hybrid"):
        with pytest.raises(RuntimeError, match="image from banknet_pack"):
            simulate(MCONF[2], plume(2, dev), Mislabelled("bank", snet.packed_for(dev)), method)
        with pytest.raises(RuntimeError, match="image from scalenet_pack"):
            simulate(MCONF[2], plume(2, dev), Mislabelled("scalenet", image), method)
    with pytest.raises(RuntimeError, match="net_kind"):
        simulate(MCONF[2], plume(2, dev), Mislabelled("banknet", image), "convnet")
    # the Conv3d net's image under the 2D kind, and the 2D net's under the Conv3d kind
    with pytest.raises(RuntimeError, match="image from banknet_pack"):
        simulate(MCONF[2], plume(2, dev), Mislabelled("bank", image3), "convnet")
    with pytest.raises(RuntimeError, match="image from banknet3d_pack"):
        simulate(MCONF[2], plume(2, dev), Mislabelled("bank3d", image), "convnet")
    # the Conv3d kind with its own image: the C refusal, under the entry point's name, before anything is written
    bd = plume(2, dev)
    U0 = bd["U"].clone()
    with pytest.raises(RuntimeError, match=r"fnx_simulate_step_net: FNX_NET_BANK3D is not built into the step"):
        simulate(MCONF[2], bd, Mislabelled("bank3d", image3), "convnet")
    assert torch.equal(bd["U"], U0)
    # the 2D kind on a 3D grid (simulate() itself keeps a net with is_bank on the operator path in 3D: a net without that mark gets there)
    with pytest.raises(RuntimeError, match=r"fnx_simulate_step_net: .*2D only"):
        simulate(MCONF[3], plume(3, dev), Mislabelled("bank", image), "convnet")
    with pytest.raises(RuntimeError, match="'FluidNet3D' bank model, which the native step does not take"):
        nets[3].step_net(dev)


@pytest.mark.parametrize("method", ["convnet", "hybrid"])
def test_the_conv3d_bank_net_stays_on_the_operator_path(dev, nets, monkeypatch, method):
    """simulate() with a 'FluidNet3D' net gives the same bits whatever `fused` says, and goes operator by operator for both"""
    from fluidnet_cxx_amd import _simulate
    a = run(MCONF[3], plume(3, dev), nets[3], method, 2)
    b = run(MCONF[3], plume(3, dev), nets[3], method, 2, fused=False)
    same_bits(a, b, f"3D {method}")

    def operator_path(*args, **kw):
        raise AssertionError("the operator path")

    monkeypatch.setattr(_simulate.fluid, "advectVelocity", operator_path)
    with pytest.raises(AssertionError, match="the operator path"):
        run(MCONF[3], plume(3, dev), nets[3], method, 1)
