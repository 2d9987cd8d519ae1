"""The pressure solve started from a guess (fnx_pcg_from: ext.solve_linear_system_pcg(p0=)) on the GPU against the float64 model of
its operator (tests/poisson_reference.py): the cold solve's bits where there is no usable guess, the line search's two properties
(scale and, on singular samples, offset of the guess drop out; never worse than the cold start in the energy norm), fewer iterations
from a good guess."""
import functools

import numpy as np
import pytest
import torch

import poisson_reference as PR
from util import make_flags

pytestmark = pytest.mark.gpu

# (D, H, W), open bottom row; the closed grids are singular, the open ones are not
GRIDS = {"2d_closed": ((1, 48, 40), False), "2d_open": ((1, 48, 40), True), "3d_closed": ((12, 16, 20), False),
         "3d_open": ((12, 16, 20), True)}
SINGULAR = {"2d_closed": True, "2d_open": False, "3d_closed": True, "3d_open": False}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ext():
    from fluidnet_cxx_amd._ext import ext
    return ext


def T(a, dev):
    return torch.from_numpy(np.array(a, np.float32)).to(dev)        # (a copy: the cached inputs are read-only)


def bits(t):
    return t.detach().cpu().numpy().view(np.int32)


def grid_flags(name, B=1):
    (D, H, W), opened = GRIDS[name]
    f = make_flags(B, D, H, W, boxes=True, empties=False)
    if opened:
        f[:, 0, :, 0, 1:W - 1] = 1.0
    return f


@functools.lru_cache(maxsize=None)
def case(name):
    """flags, the three inputs (drawn in the order b, noise, g) and the float64 model's matrix / active mask of one grid; read-only"""
    f = grid_flags(name)
    rng = np.random.default_rng(7)
    b, noise, g = (rng.standard_normal(f.shape).astype(np.float32) for _ in range(3))
    is3d = f.shape[2] > 1
    A, act = PR.matrix(f[0, 0], is3d)
    assert PR.is_singular(A, act) == SINGULAR[name]
    for a in (f, b, noise, g):
        a.setflags(write=False)
    return dict(f=f, b=b, noise=noise, g=g, is3d=is3d, A=A, act=act, sing=SINGULAR[name])


def true_residual(c, div, p):
    """float64 ||b - A p|| / ||b|| of the fp32 p, b the projected div (on singular samples with the active mean of r removed), as
    test_solve_accuracy_against_model measures it"""
    bproj = PR.project(c["f"], div, c["is3d"])[0, 0].ravel()
    r = bproj - c["A"] @ np.asarray(p, np.float64).ravel()
    if c["sing"]:
        r = np.where(c["act"], r - r[c["act"]].mean(), 0.0)
    return np.linalg.norm(r) / np.linalg.norm(bproj)


def accuracy_bound(c):
    return 3e-5 if c["is3d"] else 5e-5                    # test_solve_accuracy_against_model's


def solve(ext, dev, c, div, tol, max_iter, p0=None):
    p0 = None if p0 is None else (p0 if torch.is_tensor(p0) else T(p0, dev))
    p, res, iters = ext.solve_linear_system_pcg(T(c["f"], dev), T(div, dev), c["is3d"], tol, max_iter, False, None, p0=p0)
    return p, res, iters


# ---- 1. no usable guess: the cold solve, bit for bit ---------------------------------------------------------------------------------
COLD_SHAPES = [(name, None, False) for name in GRIDS] + [("quirks", (2, 40, 32, 24), True)]


@pytest.mark.parametrize("name,shape,quirks", COLD_SHAPES, ids=[s[0] for s in COLD_SHAPES])
def test_cold_identity(dev, ext, name, shape, quirks):
    if shape is None:
        f = grid_flags(name, B=2)
    else:
        f = make_flags(*shape, boxes=True, empties=False)
    is3d = f.shape[2] > 1
    geom = ext.Geom(ref_quirks=True) if quirks else None
    rng = np.random.default_rng(7)
    b = rng.standard_normal(f.shape).astype(np.float32)
    g = rng.standard_normal(f.shape).astype(np.float32)
    fl, div = T(f, dev), T(b, dev)
    run = lambda fl, div, **kw: ext.solve_linear_system_pcg(fl, div, is3d, 1e-5, 200, False, geom, **kw)
    p, res, iters = run(fl, div)
    assert min(iters) > 0
    for what, p0 in (("None", None), ("zeros", torch.zeros_like(div)), ("NaN", torch.full_like(div, float("nan")))):
        q, qres, qiters = run(fl, div, p0=p0)
        assert np.array_equal(bits(p), bits(q)), what
        assert np.array_equal(bits(res), bits(qres)) and iters == qiters, (what, iters, qiters)
    # a batch whose sample 1 alone holds an Inf: that sample is the cold one, sample 0 is what it is without its neighbour
    p0 = T(g, dev)
    p0[1, 0, f.shape[2] // 2, f.shape[3] // 2 + 3, 2] = float("inf")
    assert f[1, 0, f.shape[2] // 2, f.shape[3] // 2 + 3, 2] == 1.0, "the Inf sits on an active cell"
    q, _, qiters = run(fl, div, p0=p0)
    assert np.array_equal(bits(p[1]), bits(q[1])) and qiters[1] == iters[1]
    alone, _, aiters = run(fl[0:1].contiguous(), div[0:1].contiguous(), p0=p0[0:1].contiguous())
    assert np.array_equal(bits(alone[0]), bits(q[0])) and aiters[0] == qiters[0]
    assert not np.array_equal(bits(p[0]), bits(q[0])), "sample 0's guess was used"
    # the same call again: the same bits
    q2, _, q2iters = run(fl, div, p0=p0)
    assert np.array_equal(bits(q), bits(q2)) and qiters == q2iters


# ---- 2. restart: scale and null-space offset of the guess drop out -------------------------------------------------------------------
@pytest.mark.parametrize("name", list(GRIDS))
def test_restart_from_the_solution(dev, ext, name):
    c = case(name)
    p1, _, it1 = solve(ext, dev, c, c["b"], 1e-5, 200)
    assert 0 < it1[0] < 200
    guesses = [("p1", p1), ("3.7 p1", 3.7 * p1)]
    if c["sing"]:
        guesses.append(("3.7 p1 + 5", 3.7 * p1 + 5.0))
    for what, p0 in guesses:
        p, res, iters = solve(ext, dev, c, c["b"], 1e-3, 200, p0)
        rel = true_residual(c, c["b"], p.cpu().numpy())
        print(f"{name} from {what}: iters {iters}, recurrence residual {float(res):.2e}, float64 residual {rel:.2e}")
        assert iters == [0], (what, iters)
        assert float(res) <= 1e-3
        assert rel <= accuracy_bound(c), (what, rel)
    if not c["sing"]:
        # the offset is no null vector here: the guess is a poor one and the solve has work to do
        p, res, iters = solve(ext, dev, c, c["b"], 1e-3, 200, 3.7 * p1 + 5.0)
        print(f"{name} from 3.7 p1 + 5: iters {iters}, recurrence residual {float(res):.2e}")
        assert 0 < iters[0] < 200 and float(res) <= 1e-3, (iters, float(res))


# ---- 3. a good guess saves iterations ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(GRIDS))
def test_fewer_iterations_from_a_near_solution(dev, ext, name):
    """float64 model of this PCG (PR.vcycle, the line search) on these inputs: warm / cold 3 / 7 (2D closed), 5 / 10 (2D open),
    4 / 9 (3D closed), 5 / 10 (3D open)"""
    c = case(name)
    p1, _, _ = solve(ext, dev, c, c["b"], 1e-5, 200)
    div = c["b"] + np.float32(1e-3) * c["noise"]
    pc, rc, cold = solve(ext, dev, c, div, 1e-5, 200)
    pw, rw, warm = solve(ext, dev, c, div, 1e-5, 200, p1)
    print(f"{name}: iterations warm {warm[0]}, cold {cold[0]}")
    assert warm[0] < cold[0], (warm, cold)
    for p, r in ((pc, rc), (pw, rw)):
        assert float(r) <= 1e-5
        assert true_residual(c, div, p.cpu().numpy()) <= accuracy_bound(c)


# ---- 4. never worse than the cold start ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(GRIDS))
def test_noise_guess_is_never_worse_at_the_start(dev, ext, name):
    c = case(name)
    A, act = c["A"], c["act"]
    pstar = PR.solve(c["f"], c["b"], c["is3d"])[0, 0].ravel()
    x, _, iters = solve(ext, dev, c, c["b"], 1e-5, 0, c["g"])
    assert iters == [0]
    x = x.cpu().numpy().astype(np.float64).ravel()
    assert not np.any(np.where(act, 0.0, x)), "p must be 0 off the active cells"
    assert np.any(x), "the guess was used"
    e = pstar - x
    if c["sing"]:
        e = np.where(act, e - e[act].mean(), 0.0)
    ratio = (e @ (A @ e)) / (pstar @ (A @ pstar))
    print(f"{name}: energy of the error at the start / energy of p* = {ratio:.6f}")
    assert ratio <= 1.0 + 1e-6
    p, res, iters = solve(ext, dev, c, c["b"], 1e-5, 200, c["g"])
    print(f"{name}: from noise {iters[0]} iterations")
    assert float(res) <= 1e-5 and iters[0] < 200
    assert true_residual(c, c["b"], p.cpu().numpy()) <= accuracy_bound(c)


# ---- 5. arguments --------------------------------------------------------------------------------------------------------------------
def test_argument_errors(dev, ext):
    from fluidnet_cxx_amd import fluid
    f = T(make_flags(1, 8, 10, 12), dev)
    div = torch.zeros_like(f)
    with pytest.raises(RuntimeError, match="negative"):
        ext.solve_linear_system_pcg(f, div, True, 1e-5, -1, False, None, p0=div.clone())
    with pytest.raises(RuntimeError, match="mismatch"):
        ext.solve_linear_system_pcg(f, div, True, 1e-5, 10, False, None, p0=torch.zeros(1, 1, 8, 10, 11, device=dev))
    with pytest.raises(RuntimeError, match="compute window|z-slab"):
        ext.solve_linear_system_pcg(f, div, True, 1e-5, 10, False, ext.Geom(k_begin=1, k_end=5), p0=div.clone())
    with pytest.raises(RuntimeError, match="iteration"):
        ext.solve_linear_system_pcg(f, div, True, 1e-5, 0, False, None)
    with pytest.raises(AssertionError):
        fluid.solveLinearSystemPCG(f, div, True, p0=torch.zeros(1, 8, 10, 12, device=dev))
    # max_iter 0 with a guess is a call like any other
    p, res, iters = ext.solve_linear_system_pcg(f, div, True, 1e-5, 0, False, None, p0=torch.ones_like(f))
    assert not p.any() and iters == [0]                    # div = 0: zeros
