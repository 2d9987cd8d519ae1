"""3D default mode (ref_quirks = 0) of the HIP kernels against the float64 model whose axis is a loop variable
(fluid_model_nd.py), on ALL cells -- the obstacle faces, the Empty cells and index 0 that the axis-exchange test has to leave
out included.  States (semantics3d_cases.py): (B, D, H, W) = (1, 10, 11, 67), which crosses an x tile at 64, a row tile at 8 and
a z chunk at 8 planes (3D default MacCormack always takes the z-marching tile kernels), and (2, 5, 9, 13), each at
max|U| dt = 0.6 and 3.1, with a plate one plane thick in z, a bar along z that touches plane k = 1, single obstacle cells and
Empty cells; and each shape once more at max|U| dt = 6.2 with four open faces (k = 0, k = D - 1, i = 0, j = H - 1), the only
states in which rays leave the domain and the trace's ray / border intersection runs (no golden reaches it).  Every operator and option through `fluid.*` with the default plan, `advect_step` with plan='cells', and one
fused simulate(..., 'jacobi') step of 7 sweeps against the model chain (advect, buoyancy, setWallBcs, divergence, 7 sweeps of
p <- p + (div - A p) / 6 with poisson_reference.matrix, velocity update, setWallBcs).

Comparison rule (semantics3d_cases.py): a cell is bad beyond tol x the field's magnitude, at most 1e-3 of the cells of an output
array may be bad (7 cells of the larger state), tol = 4 x the model's own float32-against-float64 figure on that state.
Measured figures on these six states (FIGURE there has them per state): advect_scalar 3.4e-7 .. 4.1e-6, advect_vel
6.0e-7 .. 3.9e-6, step_p / step_U / step_density up to 2.5e-6 / 2.7e-6 / 4.0e-6, divergence 9.3e-8, velocity_update 7.2e-8,
add_buoyancy 3.6e-8, add_gravity 5.2e-8, set_wall_bcs 0 -- so tol is 1.0e-6 .. 1.6e-5 for the advections and the step,
<= 3.7e-7 for the stencils, 0 for setWallBcs.  Observed kernel-against-model errors: see the test output (each comparison
prints tol, the worst error and the number of bad cells) and DESIGN.md section 2."""
import numpy as np
import pytest
import torch

import semantics3d_cases as C

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


def T(x, dev):
    return torch.from_numpy(np.array(x, order="C", copy=True)).to(dev)      # the cases' arrays are read-only


def N(t):
    return t.detach().cpu().numpy()


class KernelBackend:
    """the operators through fluid.* with the default plan and geometry"""

    def __init__(self, dev):
        from fluidnet_cxx_amd import fluid
        self.fl, self.dev = fluid, dev

    def advect_scalar(self, dt, src, U, flags, method, outside, strength):
        return N(self.fl.advectScalar(dt, T(src, self.dev), T(U, self.dev), T(flags, self.dev), method, 1, outside, strength))

    def advect_vel(self, dt, orig, U, flags, method, strength):
        tU = T(U, self.dev)
        to = tU if orig is U else T(orig, self.dev)
        return N(self.fl.advectVelocity(dt, to, tU, T(flags, self.dev), method, 1, strength))

    def add_buoyancy(self, U, flags, rho, g, rho_star, dt):
        return N(self.fl.addBuoyancy(T(U, self.dev), T(flags, self.dev), T(rho, self.dev), g, rho_star, dt))

    def add_gravity(self, U, flags, g, dt):
        return N(self.fl.addGravity(T(U, self.dev), T(flags, self.dev), g, dt))

    def set_wall_bcs(self, U, flags):
        return N(self.fl.setWallBcs(T(U, self.dev), T(flags, self.dev)))

    def divergence(self, U, flags):
        return N(self.fl.velocityDivergence(T(U, self.dev), T(flags, self.dev)))

    def velocity_update(self, p, U, flags):
        tU = T(U, self.dev)
        self.fl.velocityUpdate(T(p, self.dev), tU, T(flags, self.dev))
        return N(tU)


@pytest.mark.parametrize("name", C.GPU_STATES)
def test_operators_vs_model_all_cells(dev, name):
    out = C.run_ops(KernelBackend(dev), C.state(name))
    for op in C.OPS:
        C.check(out[op], name, op, "kernel vs model")


@pytest.mark.parametrize("name", ["tile_lo", "small_hi", "small_open"])
def test_advect_step_cells_plan_vs_model(dev, name):
    from fluidnet_cxx_amd._ext import ext
    s = C.state(name)
    r, u = ext.advect_step(s["dt"], T(s["rho"], dev), T(s["U"], dev), T(s["flags"], dev), False, 0.6, plan="cells")
    C.check(N(r), name, "advect_scalar_maccormackFluidNet_0", "advect_step(cells) vs model")
    C.check(N(u), name, "advect_vel_maccormackFluidNet", "advect_step(cells) vs model")


@pytest.mark.parametrize("name", C.GPU_STATES)
def test_fused_jacobi_step_vs_model_chain(dev, name):
    from fluidnet_cxx_amd import simulate
    s = C.state(name)
    bd = dict(p=torch.zeros_like(T(s["rho"], dev)), U=T(s["U"], dev), flags=T(s["flags"], dev), density=T(s["rho"], dev))
    simulate(C.step_cfg(name), bd, None, "jacobi")
    for op, key in zip(C.STEP_OUT, ("p", "U", "density")):
        C.check(N(bd[key]), name, op, "fused step vs model chain")
