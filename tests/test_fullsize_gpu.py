"""Benchmark-size launch plans against the CPU oracle (not against themselves).

Every configuration `bench.py` times is advanced to a developed state on the GPU (>= 30 steps: a plume exists, the pressure
front crosses the denormal range, traces leave their cells), then ONE more step is taken by the HIP path -- with exactly the
launch plan bench.py uses at that size (workspace, static_flags promises, XCD-renumbered plane chunks, row-quad hand-over,
row-group mask, LDS-tile advection with its fix-up launches, the fused BC stages with their class map) -- and by
`oracle.simulate_step` from the same state on the host.  U, density and p must agree bit for bit.  One oracle step of a
16.8 M-cell Jacobi-100 configuration is a few seconds on the GPU box's host cores.

3D numbers are the DEFAULT 3D semantics (FnxGrid.ref_quirks = 0): the reference's own 3D path raises (velocityUpdate,
setWallBcs) or carries defects Q10-Q15, so for 3D the oracle -- pinned to the reference in 2D and in quirks mode -- is the
definition; the obstacle-adjacent 3D behaviour has no reference-side check beyond tests/test_parity_gpu.py's axis symmetry."""
import os
import sys

import numpy as np
import pytest
import torch

from util import PLUME_CFG, assert_bitexact, make_flags, random_state

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

DEVELOP = 30


def _np_state(bd):
    return {k: v.detach().cpu().numpy().copy() for k, v in bd.items()}


@pytest.mark.parametrize("name", ["plume2d_1024_jacobi", "rt2d_2048_jacobi", "plume3d_256_jacobi", "plume3d_slab_jacobi"])
def test_benchmark_size_step_vs_oracle(oracle, name):
    import bench
    from fluidnet_cxx_amd import simulate
    from fluidnet_cxx_amd._ext import ext
    dev = torch.device("cuda:0")
    w = bench.WORKLOADS[name]
    m = bench.mconf_for(w)
    is3d = w["D"] > 1
    if w.get("slab"):
        # one z-slab of configs[4] the way bench.py runs it at N = 1: the C++ driver (fnx_slab_step), static flags
        from fluidnet_cxx_amd.slab import NativeSlabSimulator, SlabLayout
        layout = SlabLayout(w["D"], 1, 0, halo=6)
        bd = bench.plume_state_torch(w["res"], layout.D_local, dev, layout.z_offset, layout.D_global)
        sim = NativeSlabSimulator(layout, m, comm=None, sweeps_per_exchange=6, static_flags=True, cfl_check_every=8)

        def step():
            sim.step(bd)
    else:
        bd = bench.build_state(w, dev)
        ws = torch.empty(ext.step_workspace_bytes(1, w["D"], w["res"], w["res"], is3d), dtype=torch.uint8, device=dev)
        seen = []

        def step():
            simulate(m, bd, None, "jacobi", workspace=ws, static_flags=(0, 3, 7)[min(len(seen), 2)])
            seen.append(1)
    for _ in range(DEVELOP):
        step()
    torch.cuda.synchronize()
    st = _np_state(bd)
    umax = float(np.abs(st["U"]).max()) * float(m["dt"])
    assert umax > 0.05, f"the state did not develop (max |U| dt = {umax})"
    step()
    torch.cuda.synchronize()
    ref = oracle.simulate_step(st, m, "jacobi")
    for k in ("U", "density", "p"):
        assert_bitexact(bd[k].cpu().numpy(), ref[k], f"{name}: {k} after step {DEVELOP + 1} (max |U| dt = {umax:.3f})")


@pytest.mark.parametrize("schedule", ["deep_first", "deep_beside"])
def test_benchmark_size_middle_rank_vs_oracle(oracle, schedule):
    """The launch plans of a MIDDLE rank at the size they are timed (bench.py's N > 1 slabs: 512 x 512 x 64 per rank, w = 6,
    static flags): three slabs of a 512 x 512 x 192 plume in lock-step on one device -- the C++ driver (fnx_slab_step), one host
    thread and stream per rank, the in-process communicator -- against ONE `oracle.simulate_step` of the whole domain from the
    same developed state (lib/simulate.py:28-171 per owned plane).  Two slab steps are taken: the first builds the solver mask and
    the BC class map and is compared with the single-domain HIP step; the second runs under the static promise (what bench.py
    times) and is the one compared with the oracle.  Rank 1 has two internal faces: its edge / deep plane-range launches (two
    ranges per launch, 2 x 320 tiles, other plane chunks and XCD renumbering than at 20 x 70) are what this pins."""
    import threading
    import bench
    from fluidnet_cxx_amd import simulate
    from fluidnet_cxx_amd._ext import ext
    from fluidnet_cxx_amd.slab import NativeSlabSimulator, SlabLayout
    dev = torch.device("cuda:0")
    w = bench.WORKLOADS["plume3d_slab_jacobi"]
    m = bench.mconf_for(w)
    world, res, own = 3, w["res"], w["D"]
    D = world * own
    halo = 12 if schedule == "lagged" else 6
    bd = bench.plume_state_torch(res, D, dev)
    ws = torch.empty(ext.step_workspace_bytes(1, D, res, res, True), dtype=torch.uint8, device=dev)
    for n in range(DEVELOP - 1):
        simulate(m, bd, None, "jacobi", workspace=ws, static_flags=(0, 3, 7)[min(n, 2)])
    torch.cuda.synchronize()
    gs = {k: v.cpu() for k, v in bd.items()}
    umax = float(gs["U"].abs().max()) * float(m["dt"])
    assert 0.05 < umax <= 1.0, f"the state did not develop, or left the decomposition's CFL range (max |U| dt = {umax})"
    layouts = [SlabLayout(D, world, r, halo) for r in range(world)]
    states = [{k: l.scatter(v).to(dev) for k, v in gs.items()} for l in layouts]
    group = ext.SlabLoopbackGroup(world)
    sims = [NativeSlabSimulator(l, m, comm=ext.slab_comm_loopback(group, l.rank), sweeps_per_exchange=6, static_flags=True,
                                cfl_check_every=8, schedule=schedule) for l in layouts]

    def slab_step():
        errs = []

        def run(r):
            try:
                with torch.cuda.stream(torch.cuda.Stream(device=dev)):
                    sims[r].step(states[r])
                    torch.cuda.current_stream().synchronize()
            except Exception as e:  # noqa: BLE001
                errs.append((r, e))
        ts = [threading.Thread(target=run, args=(r,)) for r in range(world)]
        for t in ts:
            t.start()
        for t in ts:
            t.join(timeout=300)
        assert not any(t.is_alive() for t in ts), "a rank's thread hangs"
        assert not errs, errs
        torch.cuda.synchronize()

    def check(ref, what):
        for l, st in zip(layouts, states):
            for k in ("U", "density", "p"):
                a = st[k][:, :, l.owned_slice].cpu().numpy()
                assert_bitexact(a, ref[k][:, :, l.z_begin:l.z_begin + l.owned], f"{what}: {k}, rank {l.rank} ({schedule})")

    slab_step()                                                   # step DEVELOP: builds mask + class map
    simulate(m, bd, None, "jacobi", workspace=ws, static_flags=7)
    torch.cuda.synchronize()
    st1 = _np_state(bd)
    check(st1, f"slab step {DEVELOP} vs the single-domain HIP step")
    del ws
    slab_step()                                                   # step DEVELOP + 1: the steady state bench.py times
    ref = oracle.simulate_step(st1, m, "jacobi")
    check(ref, f"slab step {DEVELOP + 1} vs oracle.simulate_step of the 512 x 512 x 192 domain")


@pytest.mark.parametrize("cfl", [0.5, 3.0])
def test_tile_advection_vs_oracle_large(oracle, cfl):
    """The 3D LDS-tile advection kernels (fnx_advect_step: z-marching tiles + fix-up launches) DIRECTLY against the oracle on a
    64 x 128 x 200 domain with obstacles and Empty cells: CFL 0.5 (almost every cell on the in-tile path) and 3 (most cells
    leave the tile and go through the fix-up launches)."""
    from fluidnet_cxx_amd._ext import ext
    dev = torch.device("cuda:0")
    B, D, H, W = 1, 64, 128, 200
    dt = 0.13
    s = random_state(B, D, H, W, cfl / (dt * 4.0), seed=33, empties=True)      # ~4 sigma of the velocity is `cfl` cells
    # a few more obstacles than make_flags' one box: bars and plates across tile and plane-chunk boundaries
    f = s["flags"]
    f[:, :, 20:23, 60:70, 55:130] = 2
    f[:, :, 5:60, 30, 100:104] = 2
    f[:, :, 40, 90:120, 10:190] = 2
    tf, tU, trho = (torch.from_numpy(s[k]).to(dev) for k in ("flags", "U", "rho"))
    for so in (False, True):
        r, u = ext.advect_step(dt, trho, tU, tf, so, 0.7)
        want_r = oracle.advect_scalar(dt, s["rho"], s["U"], f, "maccormackFluidNet", 1, so, 0.7)
        want_u = oracle.advect_vel(dt, s["U"], s["U"], f, "maccormackFluidNet", 1, 0.7)
        assert_bitexact(r.cpu().numpy(), want_r, f"density, CFL {cfl}, sample_outside={so}")
        assert_bitexact(u.cpu().numpy(), want_u, f"U, CFL {cfl}, sample_outside={so}")
        # the reference's call pattern, one advection at a time (cpp/advection.py:64,115): the same tile kernels, one part each
        r1 = ext.advect_scalar(dt, trho, tU, tf, "maccormackFluidNet", 1, so, 0.7)
        assert_bitexact(r1.cpu().numpy(), want_r, f"advect_scalar alone, CFL {cfl}, sample_outside={so}")
    u1 = ext.advect_vel(dt, tU, tU, tf, "maccormackFluidNet", 1, 0.7)
    assert_bitexact(u1.cpu().numpy(), want_u, f"advect_vel alone, CFL {cfl}")


@pytest.mark.parametrize("plan", ["cells", "tiles"])
def test_advection_tall_2d_grid_vs_oracle(oracle, plan):
    """A 2D grid with more than 32 767 rows (40 000 x 64; check_grid admits up to 65 535): the traced cell of the MacCormack clamp
    travels between the two advection passes packed as (row << 16) | column, whose sign bit is set for rows >= 32 768 -- decoded
    with an arithmetic shift the row came out negative and the clamp (fluids_init.cpp:224-263, MacCormackClampFluidNet) was
    silently skipped there.  advectScalar on its own (cell kernels) and the fused advection pair with either kernel family."""
    from fluidnet_cxx_amd._ext import ext
    dev = torch.device("cuda:0")
    B, D, H, W = 1, 1, 40000, 64
    dt = 0.2
    s = random_state(B, D, H, W, 1.2, seed=5)                      # ~CFL 1: the correction overshoots and the clamp acts on most cells
    f = s["flags"]
    f[:, :, :, 36000:36003, 20:40] = 2                             # an obstacle bar in the upper rows
    tf, tU, trho = (torch.from_numpy(s[k]).to(dev) for k in ("flags", "U", "rho"))
    want_r = oracle.advect_scalar(dt, s["rho"], s["U"], f, "maccormackFluidNet", 1, False, 0.8)
    want_u = oracle.advect_vel(dt, s["U"], s["U"], f, "maccormackFluidNet", 1, 0.8)
    top = want_r[0, 0, 0, 33000:]                                   # (clamped values stay inside the source's range [0, 1))
    assert top.min() >= 0.0 and top.max() <= 1.0
    r1 = ext.advect_scalar(dt, trho, tU, tf, "maccormackFluidNet", 1, False, 0.8, plan=plan)
    assert_bitexact(r1.cpu().numpy(), want_r, f"advect_scalar, 40000 x 64, plan={plan}")
    u1 = ext.advect_vel(dt, tU, tU, tf, "maccormackFluidNet", 1, 0.8, plan=plan)
    assert_bitexact(u1.cpu().numpy(), want_u, f"advect_vel, 40000 x 64, plan={plan}")
    r, u = ext.advect_step(dt, trho, tU, tf, False, 0.8, plan=plan)
    assert_bitexact(r.cpu().numpy(), want_r, f"density, 40000 x 64, plan={plan}")
    assert_bitexact(u.cpu().numpy(), want_u, f"U, 40000 x 64, plan={plan}")


def _long_state(D, H, W, seed):
    rng = np.random.default_rng(seed)
    nc = 3 if D > 1 else 2
    flags = make_flags(1, D, H, W, boxes=True)
    st = dict(flags=flags, p=np.zeros((1, 1, D, H, W), np.float32), U=np.zeros((1, nc, D, H, W), np.float32),
              density=np.zeros((1, 1, D, H, W), np.float32))
    UBC = np.zeros_like(st["U"]); M = np.ones_like(st["U"])
    UBC[0, 1, :, 0:4, W // 3:2 * W // 3] = 2.0; M[:, :, :, 0:4] = 0
    dBC = np.zeros_like(st["density"]); dM = np.ones_like(st["density"])
    dBC[0, 0, :, 0:4, W // 3:2 * W // 3] = 0.1; dM[0, 0, :, 0:4, W // 3:2 * W // 3] = 0
    st["U"] += (rng.standard_normal(st["U"].shape) * 0.05).astype(np.float32)
    st.update(UBC=UBC, UBCInvMask=M, densityBC=dBC, densityBCInvMask=dM)
    return st


@pytest.mark.parametrize("case", [("2D 160x200", (1, 160, 200), 120, 28, 40), ("3D 40x48x56", (40, 48, 56), 60, 40, 20)])
def test_long_simulation_stays_bit_identical(oracle, case):
    """A shortened tools/long_parity.py: the HIP path and the oracle side by side through 120 (2D) / 60 (3D) steps of a domain
    with obstacles and an inflow, compared bit for bit every 40 / 20 steps -- differences that only show once the flow has
    developed (long traces, the clamp, the pressure front) have nowhere to hide."""
    from fluidnet_cxx_amd import simulate
    name, (D, H, W), steps, iters, every = case
    dev = torch.device("cuda:0")
    cfg = dict(PLUME_CFG, jacobiIter=iters, gravityVec=dict(x=0.0, y=-1.0, z=0.2 if D > 1 else 0.0))
    st = _long_state(D, H, W, 5)
    bd = {k: torch.from_numpy(v).to(dev) for k, v in st.items()}
    for it in range(1, steps + 1):
        simulate(cfg, bd, None, "jacobi")
        st = oracle.simulate_step(st, cfg, "jacobi")
        if it % every == 0:
            for k in ("U", "density", "p"):
                assert_bitexact(bd[k].cpu().numpy(), st[k], f"{name}: {k} after {it} steps")
    assert float(np.abs(st["U"]).max()) > 0.5, "the flow did not develop"


# ---- the convnet step (lib/simulate.py:131-143 + lib/model.py:118-227) against the oracle --------------------------------------
# The fused convnet step is three launches around the net (fnx_fluidnet.hip: pack_div_kernel -- the divergence of U / s straight into
# the net's input --, the net, post_projection_kernel<IS3D, SCALE=true> -- velocityUpdate, un-normalisation, setWallBcs, the step's
# last setConstVals) behind the advection and staging launches.  Tolerances: the net's arithmetic is a tolerance statement
# (1e-5 * |ref|max on p and U, like every CNN test); everything that does not pass through the net is bit for bit.

def _cnn_cfg(is3d):
    return dict(PLUME_CFG, model="ScaleNet", inputChannels=dict(div=True, pDiv=False, UDiv=False), normalizeInput=True,
                normalizeInputChan="UDiv", is3D=is3d, gravityVec=dict(x=0.0, y=-1.0, z=0.2 if is3d else 0.0))


def _cnn_state(B, D, H, W, seed):
    """B samples with obstacles, an inflow (velocity + density BCs), different random velocities and densities per sample"""
    rng = np.random.default_rng(seed)
    nc = 3 if D > 1 else 2
    flags = make_flags(B, D, H, W, boxes=True)
    if D > 1:
        flags[:, :, 2:D - 2, H // 2, W // 2:W // 2 + 9] = 2          # a bar through most planes
    st = dict(flags=flags, p=rng.standard_normal((B, 1, D, H, W)).astype(np.float32),
              U=(rng.standard_normal((B, nc, D, H, W)) * 0.6).astype(np.float32),
              density=rng.random((B, 1, D, H, W)).astype(np.float32))
    UBC = np.zeros_like(st["U"]); M = np.ones_like(st["U"])
    UBC[:, 1, :, 0:4, W // 3:2 * W // 3] = 2.0; M[:, :, :, 0:4] = 0
    dBC = np.zeros_like(st["density"]); dM = np.ones_like(st["density"])
    dBC[:, 0, :, 0:4, W // 3:2 * W // 3] = 0.1; dM[:, 0, :, 0:4, W // 3:2 * W // 3] = 0
    st.update(UBC=UBC, UBCInvMask=M, densityBC=dBC, densityBCInvMask=dM)
    return st


@pytest.mark.parametrize("shape", [(2, 12, 40, 72), (2, 1, 48, 80), (1, 16, 36, 132)])
def test_convnet_step_vs_oracle(oracle, shape):
    """Three consecutive fused convnet steps (workspace; static_flags 0, 3, 7: the BC class map is built, then reused) in 3D and
    2D with obstacles, inflow BCs and a batch of two: each step against oracle.simulate_step(state before it, "convnet")."""
    from fluidnet_cxx_amd import FluidNet, simulate
    from fluidnet_cxx_amd._ext import ext
    from fluidnet_cxx_amd.weights import make_scalenet_weights
    from util import assert_close_rel
    B, D, H, W = shape
    is3d = D > 1
    dev = torch.device("cuda:0")
    cfg = _cnn_cfg(is3d)
    wts = make_scalenet_weights(0, ndim=3 if is3d else 2)
    blob = oracle.pack_weights(wts, 3 if is3d else 2)
    net = FluidNet.from_weights(cfg, wts, dev)
    bd = {k: torch.from_numpy(v).to(dev) for k, v in _cnn_state(B, D, H, W, 21).items()}
    ws = torch.empty(ext.step_workspace_bytes(B, D, H, W, is3d), dtype=torch.uint8, device=dev)
    for it in range(3):
        st = _np_state(bd)
        simulate(cfg, bd, net, "convnet", workspace=ws, static_flags=(0, 3, 7)[it])
        torch.cuda.synchronize()
        ref = oracle.simulate_step(st, cfg, "convnet", blob)
        assert_bitexact(bd["density"].cpu().numpy(), ref["density"], f"density, step {it + 1}")
        for k in ("p", "U"):
            for b in range(B):          # per sample: each has its own scale
                assert_close_rel(bd[k][b].cpu().numpy(), ref[k][b], 1e-5, f"{k}, sample {b}, step {it + 1}")
        # the cells setWallBcs / setConstVals pin do not pass through the net: the inflow rows carry the BC values exactly
        got = bd["U"].cpu().numpy()
        assert_bitexact(got[:, :, :, 0:4], ref["U"][:, :, :, 0:4], f"U on the inflow rows, step {it + 1}")


@pytest.mark.parametrize("name", ["plume2d_1024_cnn", "plume3d_256_cnn", "plume2d_1024_cnn_bf16x6", "plume3d_256_cnn_bf16x6", "plume2d_1024_cnn_bf16x3"])
def test_benchmark_size_convnet_step_vs_oracle(oracle, name):
    """The convnet step bench.py times at 1024^2 (the metric's configs[1]) and 256^3 (configs[3]), from a developed plume, with
    its launch plan (workspace, static_flags, Winograd MFMA layers): every stage AROUND the net bit for bit against the oracle.
    The oracle runs the step with the HIP net standing in for its MultiScaleNet (`net=`: ext.multiscale_forward on the input the
    ORACLE's stages produced -- the divergence of the staged, normalised velocity), so U, density and p of the HIP step must
    equal the oracle's bit for bit: the advection, the staging pass, pack_div_kernel (else the net sees another input), the
    scale, post_projection_kernel<.,SCALE> and the last setConstVals.  The net itself at this size: test_cnn_benchmark_size.
    (`_bf16x6`: the same step with the opt-in precision mode travelling through mconf -> FluidNet -> fnx_simulate_step.)"""
    import bench
    from fluidnet_cxx_amd import FluidNet, simulate
    from fluidnet_cxx_amd._ext import ext
    from fluidnet_cxx_amd.weights import make_scalenet_weights
    dev = torch.device("cuda:0")
    w = bench.WORKLOADS[name]
    m = bench.mconf_for(w)
    is3d = w["D"] > 1
    net = FluidNet.from_weights(m, make_scalenet_weights(0, ndim=3 if is3d else 2), dev)
    bd = bench.build_state(w, dev)
    ws = torch.empty(ext.step_workspace_bytes(1, w["D"], w["res"], w["res"], is3d), dtype=torch.uint8, device=dev)
    seen = []

    def step(method):
        simulate(m, bd, net if method == "convnet" else None, method, workspace=ws, static_flags=(0, 3, 7)[min(len(seen), 2)])
        seen.append(1)
    m["jacobiIter"] = 28 if not is3d else 40          # developed with the Jacobi projection, as bench.py does
    for _ in range(DEVELOP):
        step("jacobi")
    step("convnet")                                    # (and one CNN step, so that p is a net output like in the timed loop)
    torch.cuda.synchronize()
    st = _np_state(bd)
    umax = float(np.abs(st["U"]).max()) * float(m["dt"])
    assert umax > 0.05, f"the state did not develop (max |U| dt = {umax})"
    step("convnet")
    torch.cuda.synchronize()
    packed = net.packed_for(dev)
    calls = []

    def hip_net(x):
        calls.append(1)
        return ext.multiscale_forward(packed, torch.from_numpy(x).to(dev), w.get("precision", "fp32")).cpu().numpy()
    ref = oracle.simulate_step(st, m, "convnet", None, net=hip_net)
    assert calls == [1]
    for k in ("density", "U", "p"):
        assert_bitexact(bd[k].cpu().numpy(), ref[k], f"{name}: {k} after the convnet step (max |U| dt = {umax:.3f})")
