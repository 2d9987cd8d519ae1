"""The automatic mode of the four-argument simulate() call on the GPU, across methods and across what a caller does between calls: mixed
'jacobi' / 'pcg' / 'convnet' / 'hybrid' steps on one set of tensors and one cached workspace, calls that raise, flags at a recycled
address, evicted workspaces and two streams.

Two legs run the same events on tensors of their own.  The automatic leg makes four-argument calls.  The reference leg gives every
call a workspace of its own, filled with 0xA5 before the call, and static_flags=0: it derives everything and trusts nothing.  After
every call p, U and density of the two legs agree bit for bit.  A spy on ext.simulate_step_ sees the bits the automatic leg sends;
static_inputs_model says whether the workspace holds what they trust.

Grids: 3D (2, 6, 9, 67) -- a partial wave in x, two samples with different obstacle boxes, inlet BCs, D >= 4 for the 3D ScaleNet --
and 2D (2, 1, 36, 68), which takes the ScaleNet and the 2D bank net."""
import numpy as np
import pytest
import torch

from banknet_reference import propagating_bank_weights
from static_inputs_model import PINNED, PINNED_BITS, Workspace
from util import PLUME_CFG, assert_bitexact, box_plume_state

pytestmark = pytest.mark.gpu

SHAPE = {2: (2, 1, 36, 68), 3: (2, 6, 9, 67)}
NET = dict(inputChannels=dict(div=True, pDiv=False, UDiv=False), normalizeInput=True, normalizeInputChan="UDiv")
CFG = {nd: dict(PLUME_CFG, jacobiIter=7, pcgTol=1e-5, pcgIter=40, model="ScaleNet", inputDim=nd, is3D=nd == 3, **NET) for nd in (2, 3)}
METHOD = {"J": "jacobi", "P": "pcg", "C": "convnet", "H": "hybrid"}
KEYS = ("p", "U", "density")
REFUSED = "refused by the spy"


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def nets(dev):
    from fluidnet_cxx_amd import FluidNet
    from fluidnet_cxx_amd.weights import make_scalenet_weights
    nets = {(nd, "scalenet"): FluidNet.from_weights(CFG[nd], make_scalenet_weights(0, ndim=nd), dev).eval() for nd in (2, 3)}
    nets[2, "bank"] = FluidNet.from_weights(dict(CFG[2], model="FluidNet"), propagating_bank_weights(), dev).eval()
    return nets


@pytest.fixture(autouse=True)
def fresh_workspaces():
    from fluidnet_cxx_amd import _simulate
    _simulate.release_workspaces()
    yield
    _simulate.release_workspaces()


class Spy:
    """stands in for ext.simulate_step_: notes the static_flags argument, then calls the extension -- or raises instead (refuse)"""

    def __init__(self, real):
        self.real, self.seen, self.refuse = real, [], False

    def __call__(self, *a, **k):
        self.seen.append(a[20])
        if self.refuse:
            raise RuntimeError(REFUSED)
        return self.real(*a, **k)


@pytest.fixture
def spy(monkeypatch):
    from fluidnet_cxx_amd import _simulate
    s = Spy(_simulate.ext.simulate_step_)
    monkeypatch.setattr(_simulate.ext, "simulate_step_", s)
    return s


def box(flags, n):
    """obstacle box number n (0, 1, 2: three places) written into a flags tensor in place, in every sample"""
    D, H = flags.size(2), flags.size(3)
    zs = slice(None) if D == 1 else slice(1, D - 2)
    flags[:, :, zs, H // 2:H // 2 + 2, 40 + 8 * n:45 + 8 * n] = 2.0


class Legs:
    """the automatic and the reference leg of one simulation, and the model of the automatic leg's cached workspace"""

    def __init__(self, dev, spy, shape, net=None, cfg=None):
        from fluidnet_cxx_amd._ext import ext
        B, D, H, W = shape
        self.is3d = D > 1
        self.cfg, self.net, self.spy = cfg or CFG[3 if self.is3d else 2], net, spy
        st = box_plume_state(B, D, H, W)
        self.auto, self.ref = ({k: torch.from_numpy(v).to(dev) for k, v in st.items()} for _ in range(2))
        self.ws = torch.empty(ext.step_workspace_bytes(B, D, H, W, self.is3d), dtype=torch.uint8, device=dev)
        self.model = Workspace(self.is3d)
        self.generations = 2
        self.g_flags, self.g_bc = 1, 2
        self.bits = []

    def generation(self):
        self.generations += 1
        return self.generations

    def call(self, m, fail=None):
        """One call of method m ('J', 'P', 'C', 'H') on both legs.  fail: 'refusal' -- pcgIter = 0, which fnx_simulate_step refuses
        before its first launch -- or 'spy', which raises without calling the extension: an argument error either way, the state
        untouched, and both legs make the same failing call."""
        from fluidnet_cxx_amd import simulate
        method = METHOD[m]
        cfg = dict(self.cfg, pcgIter=0) if fail == "refusal" else self.cfg
        net = self.net if m in "CH" else None
        self.spy.refuse = fail == "spy"

        def step(bd, **kw):
            if fail:
                with pytest.raises(RuntimeError, match=REFUSED if fail == "spy" else "At least 1 iteration"):
                    simulate(cfg, bd, net, method, **kw)
            else:
                simulate(cfg, bd, net, method, **kw)
            return self.spy.seen[-1]

        try:
            n = len(self.spy.seen)
            bits = step(self.auto)
            self.ws.fill_(0xA5)                              # with static_flags = 0 nothing of it may be read before it is written
            assert step(self.ref, workspace=self.ws, static_flags=0) == 0 and len(self.spy.seen) == n + 2
        finally:
            self.spy.refuse = False
        self.bits.append(bits)
        what = f"call {len(self.bits)} ('{method}'{', ' + fail if fail else ''}), bits {self.bits}"
        bad = self.model.check(bits, method, self.g_flags, self.g_bc)
        assert not bad, f"{what}: the bits trust what the workspace does not hold -- " + "; ".join(bad)
        self.model.call(bits, method, self.g_flags, self.g_bc, ok=not fail)
        for k in KEYS:
            a, r = self.auto[k].detach().cpu().numpy(), self.ref[k].detach().cpu().numpy()
            assert np.isfinite(a).all(), f"{what}: {k} is not finite"
            assert_bitexact(a, r, f"{what}: {k}, four-argument call vs static_flags=0 on a workspace of 0xA5")
        return bits

    def write_flags(self, n=0):
        """an obstacle box inserted in place"""
        for bd in (self.auto, self.ref):
            box(bd["flags"], n)
        self.g_flags = self.generation()

    def write_bc(self):
        """a faster inlet, in place"""
        for bd in (self.auto, self.ref):
            bd["UBC"].mul_(1.5)
        self.g_bc = self.generation()

    def set_flags(self, auto_flags, contents):
        """other flags tensors: `auto_flags` for the automatic leg, a copy of `contents` for the reference leg"""
        self.auto["flags"], self.ref["flags"] = auto_flags, contents.clone()
        self.g_flags = self.generation()

    def moved(self):
        for k in ("p", "U", "density"):
            assert np.abs(self.auto[k].detach().cpu().numpy()).max() > 0, k


def play(legs, script):
    for ev in script.split():
        if ev == "wf":
            legs.write_flags()
        elif ev == "wb":
            legs.write_bc()
        else:
            legs.call(ev[0], {"-": "refusal", "!": "spy"}.get(ev[1:]))
    legs.moved()
    return legs.bits


@pytest.mark.parametrize("ndim,kind", [(2, "scalenet"), (3, "scalenet"), (2, "bank")], ids=["2d", "3d", "2d-bank"])
def test_mixed_methods_on_one_workspace(dev, nets, spy, ndim, kind):
    """the pinned sequence: every method on one set of tensors and one cached workspace, an obstacle box inserted in place and
    UBC.mul_(1.5) between them"""
    assert play(Legs(dev, spy, SHAPE[ndim], nets[ndim, kind]), PINNED) == PINNED_BITS


@pytest.mark.parametrize("how", ["P-", "P!"], ids=["refusal", "spy"])
@pytest.mark.parametrize("ndim", [2, 3])
def test_a_failed_call_leaves_no_promise(dev, nets, spy, ndim, how):
    """J+ P- J+: the failed call was about to build the class map; the next call sends 0 and the bits climb again"""
    assert play(Legs(dev, spy, SHAPE[ndim], nets[ndim, "scalenet"]), f"J {how} J J P P") == [0, 3, 0, 3, 7, 15]


@pytest.mark.parametrize("ndim,script,want", [(3, "JPPJ", [0, 2, 6, 6]), (3, "PJJP", [0, 2, 6, 7]), (2, "PJJP", [0, 2, 6, 7])],
                         ids=["3d-mask", "3d-hierarchy", "2d-hierarchy"])
def test_a_recycled_address(dev, nets, spy, ndim, script, want):
    """m0(A) m1(B) m2(A2) m3(A2), where A2 is a new flags tensor with other obstacles at A's address with A's version: flags carved
    out of a pool through `.data`, which gives the same storage with a fresh version counter.  What m0 left in the workspace (the mask
    of A in 'JPPJ', the hierarchy of A in 'PJJP') is not that of A2, whatever A2's identity says."""
    legs = Legs(dev, spy, SHAPE[ndim], nets[ndim, "scalenet"])
    contents = []
    for n in range(3):
        contents.append(legs.ref["flags"].clone())
        box(contents[n], n)
    pool = torch.empty(contents[0].numel(), device=dev)
    pool.copy_(contents[0].flatten())
    A = pool.data.view(contents[0].shape)
    ptr, version = A.data_ptr(), A._version
    legs.set_flags(A, contents[0])
    del A
    legs.call(script[0])
    legs.set_flags(contents[1].clone(), contents[1])         # B: from here on nothing holds A
    legs.call(script[1])
    pool.copy_(contents[2].flatten())
    A2 = pool.data.view(contents[2].shape)
    assert A2.data_ptr() == ptr and A2._version == version, "the recycled flags tensor does not have the identity of the first"
    legs.set_flags(A2, contents[2])
    legs.call(script[2])
    legs.call(script[3])
    legs.moved()
    assert legs.bits == want


def test_an_evicted_workspace_starts_again(dev, spy):
    """five grid shapes where four workspaces are kept: the least recently used goes, and its next call sends 0"""
    from fluidnet_cxx_amd import _simulate
    assert _simulate._AUTO_MAX == 4
    legs = [Legs(dev, spy, (1, 1, 12 + 4 * i, 16), cfg=CFG[2]) for i in range(5)]
    kept, got = [], []
    order, want = [0, 1, 2, 3, 0, 4, 1, 0], [0, 0, 0, 0, 3, 0, 0, 7]     # 4 evicts 1 (0 was used since), 1 evicts 2
    for i in order:
        if i in kept:
            kept.remove(i)
        elif len(kept) == _simulate._AUTO_MAX:
            legs[kept.pop(0)].model = Workspace(False)       # a fresh workspace: nothing in it
        kept.append(i)
        got.append(legs[i].call("J"))
    assert got == want
    assert len(_simulate._AUTO) == 4
    legs[0].moved()


def test_two_streams_keep_a_workspace_each(dev, spy):
    """one shape stepped alternately on two streams: each stream has its own workspace and its bits climb 0, 3, 7"""
    from fluidnet_cxx_amd import _simulate
    streams = [torch.cuda.Stream(dev), torch.cuda.Stream(dev)]
    legs = [Legs(dev, spy, SHAPE[3]) for _ in streams]
    torch.cuda.synchronize()
    for _ in range(3):
        for s, l in zip(streams, legs):
            with torch.cuda.stream(s):
                l.call("J")
    torch.cuda.synchronize()
    assert [l.bits for l in legs] == [[0, 3, 7], [0, 3, 7]]
    assert len(_simulate._AUTO) == 2
    for l in legs:
        l.moved()
