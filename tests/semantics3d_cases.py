"""States, operator lists, tolerances and the comparison rule shared by test_fluid_model_nd.py (CPU) and
test_semantics3d_gpu.py (GPU): the float64 model of fluid_model_nd.py against the goldens, the oracle and the kernels.

The comparison rule.  A cell is BAD when |got - model64| > tol * max|model64|; a comparison passes when at most CAP = 1e-3 of
the cells of an output array are bad (the cap of test_3d_default_semantics_axis_symmetry: it absorbs the few cells where a
rounding difference flips an integer part or a fluid / non-fluid decision; a wrong rule moves every cell beside an obstacle
face or every cell of a component).  tol is not chosen: TOL[state][family] below is 4 x FIGURE[state][family], the largest
scaled difference between the model run in float32 and in float64 on that state over the cells that are not such flips
(a flip is a difference above JUMP = 1e-4 of the field's magnitude -- float32 rounding of positions below 128 and values
of order one cannot reach it, an integer part that flips moves the result by the local gradient); the factor 4 covers
an expression order and FMA contraction that differ from the model's float32 run (headroom the oracle and the kernels do not
use today: their worst errors equal the FIGURE entries, so the float32 model has their expression order almost everywhere --
no reason to widen it).  The guard (test_model_precision_guard)
re-measures this at every run: float32 against float64 leaves at most CAP / 4 of the cells beyond TOL.  Nothing here is
derived from the oracle or the kernels.
"""
import functools
import os

import numpy as np

import fluid_model_nd as M
import hostile2d_cases as HC

CAP = 1e-3
JUMP = 1e-4
GOLDEN_2D = ("ops_2d_a", "ops_2d_b", "ops_2d_c", "ops_2d_d")
GOLDEN_3D = ("ops_3d_a", "ops_3d_b")
# the reference on the geometries of hostile2d_cases.py (open sides, scattered cells, per-sample flags): hostile2d.npz / hostile2d_hi.npz
HOSTILE_2D = tuple("hostile2d_" + n for n in HC.GOLDEN_STATES)
#               B, D,  H,  W, max|U| dt, seed
OWN = {"tile_lo": (1, 10, 11, 67, 0.6, 11),      # crosses an x tile at 64, a row tile at 8 and a z chunk at 8 planes
       "tile_hi": (1, 10, 11, 67, 3.1, 12),
       "small_lo": (2, 5, 9, 13, 0.6, 13),
       "small_hi": (2, 5, 9, 13, 3.1, 14),
       "large_lo": (2, 12, 14, 18, 0.6, 15),     # CPU only
       "large_hi": (2, 12, 14, 18, 3.1, 16),
       # the same obstacles, but the faces k = 0, k = D - 1, i = 0 and j = H - 1 are open (Fluid with a few Empty cells): the only
       # states whose rays leave the domain, i.e. that reach the ray / border intersection of the line trace
       "tile_open": (1, 10, 11, 67, 6.2, 17),
       "small_open": (2, 5, 9, 13, 6.2, 18),
       "large_open": (2, 12, 14, 18, 6.2, 19)}   # CPU only
OPEN = ("tile_open", "small_open", "large_open")
GPU_STATES = ("tile_lo", "tile_hi", "small_lo", "small_hi", "tile_open", "small_open")
STEP_CFG = dict(maccormackStrength=0.6, sampleOutsideFluid=False, buoyancyScale=0.25, gravityScale=0, viscosity=0,
                correctScalar=False, gravityVec=dict(x=0.3, y=-1.0, z=0.5), operatingDensity=0.05, pTol=0.0, jacobiIter=7)

METHODS = ("maccormackFluidNet", "eulerFluidNet")
OPS = tuple(f"advect_scalar_{m}_{so}" for m in METHODS for so in (0, 1)) + tuple(f"advect_vel_{m}" for m in METHODS) + \
    ("advect_vel_orig", "add_buoyancy", "add_gravity", "set_wall_bcs", "divergence", "velocity_update")
STEP_OUT = ("step_p", "step_U", "step_density")


def family(op):
    for f in ("advect_scalar", "advect_vel"):
        if op.startswith(f):
            return f
    return op


def _own_flags(B, D, H, W, open_faces=False):
    f = np.full((B, 1, D, H, W), M.FLUID, np.float32)
    f[:, :, :, 0] = f[:, :, :, -1] = f[..., 0] = f[..., -1] = f[:, :, 0] = f[:, :, -1] = M.OBST
    if open_faces:
        f[:, :, 0, 1:, :-1] = f[:, :, -1, 1:, :-1] = f[:, :, :, 1:, 0] = f[:, :, :, -1, :-1] = M.FLUID
        f[:, :, 0, 2, 3:5] = f[:, :, -1, 4, 2] = f[:, :, 2, 5, 0] = f[:, :, 1, -1, 6] = M.EMPTY
    if (D, H, W) == (10, 11, 67):
        f[:, :, 5, 2:7, 20:40] = M.OBST                    # a plate one plane thick in z
        f[:, :, 1:9, 8, 62:66] = M.OBST                    # a bar along z across the x tile boundary, touching plane k = 1
        for k, j, i in ((3, 4, 10), (7, 2, 50), (8, 8, 30)):
            f[:, :, k, j, i] = M.OBST                      # single cells
        for k, j, i in ((2, 8, 5), (2, 8, 6), (6, 5, 64)):
            f[:, :, k, j, i] = M.EMPTY
    elif (D, H, W) == (5, 9, 13):
        f[:, :, 1:4, 6, 9] = M.OBST                        # a bar along z, wall to wall
        f[:, :, 2, 4, 6] = M.OBST
        f[:, :, 1, 2, 3] = M.EMPTY
        f[1, :, 3, 3, 4] = M.OBST
    else:
        assert (D, H, W) == (12, 14, 18)
        f[:, :, 6, 3:8, 3:9] = M.OBST                      # a plate one plane thick in z
        f[:, :, 2:9, 10, 12] = M.OBST                      # a bar along z
        f[:, :, 1:3, 4:6, 12:15] = M.OBST                  # a block touching plane k = 1
        for k, j, i in ((4, 10, 5), (9, 3, 14), (10, 11, 2)):
            f[:, :, k, j, i] = M.OBST                      # single cells
        for k, j, i in ((3, 11, 3), (3, 11, 4), (8, 6, 15)):
            f[:, :, k, j, i] = M.EMPTY
        f[1, :, 5, 7, 10] = M.OBST                         # the samples of the batch differ
    return f


@functools.lru_cache(maxsize=None)
def state(name):
    """the inputs of a case: float32 arrays and python scalars (never modified)"""
    if name in OWN:
        B, D, H, W, cfl, seed = OWN[name]
        rng = np.random.default_rng(seed)
        U = rng.standard_normal((B, 3, D, H, W)).astype(np.float32)
        s = dict(flags=_own_flags(B, D, H, W, name in OPEN), U=U, orig=rng.standard_normal(U.shape).astype(np.float32),
                 rho=rng.random((B, 1, D, H, W)).astype(np.float32), p=rng.standard_normal((B, 1, D, H, W)).astype(np.float32),
                 dt=float(np.float32(cfl / np.abs(U).max())), gravity=[0.3, 0.25, -0.2], rho_star=0.05)
    else:
        pre = ""
        if name in HOSTILE_2D:
            pre, name = name[len("hostile2d_"):] + "_", HC.golden_file(name)
        z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", name + ".npz"))
        z = HC.Prefixed(z, pre)
        s = dict(flags=z["flags"], U=z["U"], orig=z["orig"], rho=z["rho"], p=z["p"], dt=float(z["dt"]),
                 gravity=z["gravity"].tolist(), rho_star=float(z["rho_star"]))
        s["golden"] = {k: z[k] for k in OPS if k in z.files}
    for v in s.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return s


class ModelBackend:
    def __init__(self, dtype):
        self.dtype = dtype

    def advect_scalar(self, dt, src, U, flags, method, outside, strength):
        return M.advect_scalar(dt, src, U, flags, method, outside, strength, self.dtype)

    def advect_vel(self, dt, orig, U, flags, method, strength):
        return M.advect_velocity(dt, orig, U, flags, method, strength, self.dtype)

    def add_buoyancy(self, U, flags, rho, g, rho_star, dt):
        return M.add_buoyancy(U, flags, rho, g, rho_star, dt, self.dtype)

    def add_gravity(self, U, flags, g, dt):
        return M.add_gravity(U, flags, g, dt, self.dtype)

    def set_wall_bcs(self, U, flags):
        return M.set_wall_bcs(U, flags, self.dtype)

    def divergence(self, U, flags):
        return M.velocity_divergence(U, flags, self.dtype)

    def velocity_update(self, p, U, flags):
        return M.velocity_update(p, U, flags, self.dtype)


class OracleBackend:
    """the CPU oracle in default mode (quirks = False)"""

    def __init__(self, O):
        self.O = O

    def advect_scalar(self, dt, src, U, flags, method, outside, strength):
        return self.O.advect_scalar(dt, src, U, flags, method, 1, outside, strength, False)

    def advect_vel(self, dt, orig, U, flags, method, strength):
        return self.O.advect_vel(dt, orig, U, flags, method, 1, strength, False)

    def add_buoyancy(self, U, flags, rho, g, rho_star, dt):
        return self.O.add_buoyancy(U, flags, rho, g, rho_star, dt, False)

    def add_gravity(self, U, flags, g, dt):
        return self.O.add_gravity(U, flags, g, dt)

    def set_wall_bcs(self, U, flags):
        return self.O.set_wall_bcs(U, flags)

    def divergence(self, U, flags):
        return self.O.velocity_divergence(U, flags)

    def velocity_update(self, p, U, flags):
        return self.O.velocity_update(p, U, flags)


def run_ops(be, s):
    """every operator and option of OPS on the state s through one backend"""
    o = {}
    for m in METHODS:
        for so in (0, 1):
            o[f"advect_scalar_{m}_{so}"] = be.advect_scalar(s["dt"], s["rho"], s["U"], s["flags"], m, bool(so), 0.6)
        o[f"advect_vel_{m}"] = be.advect_vel(s["dt"], s["U"], s["U"], s["flags"], m, 0.6)
    o["advect_vel_orig"] = be.advect_vel(s["dt"], s["orig"], s["U"], s["flags"], "maccormackFluidNet", 0.75)
    o["add_buoyancy"] = be.add_buoyancy(s["U"], s["flags"], s["rho"], s["gravity"], s["rho_star"], s["dt"])
    o["add_gravity"] = be.add_gravity(s["U"], s["flags"], s["gravity"], s["dt"])
    o["set_wall_bcs"] = be.set_wall_bcs(s["U"], s["flags"])
    o["divergence"] = be.divergence(s["U"], s["flags"])
    o["velocity_update"] = be.velocity_update(s["p"], s["U"], s["flags"])
    return o


@functools.lru_cache(maxsize=None)
def model_outputs(name, dtype=np.float64):
    """the model's outputs of a case, computed once per process and never modified"""
    s = state(name)
    o = run_ops(ModelBackend(dtype), s)
    if name in OWN:
        gv = STEP_CFG["gravityVec"]
        p, U, rho = M.jacobi_step(s["U"], s["flags"], s["rho"], s["dt"], STEP_CFG["maccormackStrength"], False,
                                  STEP_CFG["buoyancyScale"], [gv["x"], gv["y"], gv["z"]], STEP_CFG["operatingDensity"],
                                  STEP_CFG["jacobiIter"], dtype)
        o.update(step_p=p, step_U=U, step_density=rho)
    for v in o.values():
        v.setflags(write=False)
    return o


def step_cfg(name):
    return dict(STEP_CFG, dt=state(name)["dt"])


def measure(got, want, tol):
    """(share of bad cells, number of bad cells, worst scaled error over all cells, worst over the cells that are not bad)"""
    want = np.asarray(want, np.float64)
    got = np.asarray(got, np.float64)
    assert got.shape == want.shape, (got.shape, want.shape)
    d = np.abs(got - want) / max(float(np.abs(want).max()), 1e-30)
    bad = ~(d <= tol)                                       # a NaN is bad
    return float(bad.mean()), int(bad.sum()), float(np.nanmax(d)), float(d[~bad].max()) if (~bad).any() else 0.0


def check(got, name, op, what, cap=CAP):
    """assert the comparison rule for one output array; prints the figures (pytest shows them with -s or on failure)"""
    tol = TOL[name][family(op)]
    share, nbad, worst, worst_ok = measure(got, model_outputs(name)[op], tol)
    line = f"{what} {name}:{op}: tol {tol:.2e}, worst {worst:.2e}, worst within tol {worst_ok:.2e}, bad cells {nbad} ({share:.2e})"
    print(line)
    assert share <= cap, line


def figure(name, op):
    """the measured float32-against-float64 figure of the model on one output: largest scaled difference below JUMP"""
    _, _, _, fig = measure(model_outputs(name, np.float32)[op], model_outputs(name)[op], JUMP)
    return fig


# FIGURE[state][family]: max over the family's outputs of figure(), as measured (`python tests/semantics3d_cases.py` prints this table); TOL = 4 x.
FIGURE = {
    "ops_2d_a": {"advect_scalar": 7.12e-07, "advect_vel": 1.43e-06, "add_buoyancy": 3.15e-08, "add_gravity": 2.77e-08, "set_wall_bcs": 0.00e+00, "divergence": 6.62e-08, "velocity_update": 4.16e-08},
    "ops_2d_b": {"advect_scalar": 3.54e-06, "advect_vel": 2.17e-06, "add_buoyancy": 5.04e-08, "add_gravity": 2.56e-08, "set_wall_bcs": 0.00e+00, "divergence": 6.19e-08, "velocity_update": 4.74e-08},
    "ops_2d_c": {"advect_scalar": 3.64e-07, "advect_vel": 9.15e-07, "add_buoyancy": 3.36e-08, "add_gravity": 2.86e-08, "set_wall_bcs": 0.00e+00, "divergence": 3.22e-08, "velocity_update": 4.39e-08},
    "ops_2d_d": {"advect_scalar": 6.16e-06, "advect_vel": 2.77e-06, "add_buoyancy": 3.91e-08, "add_gravity": 3.15e-08, "set_wall_bcs": 0.00e+00, "divergence": 7.72e-08, "velocity_update": 4.00e-08},
    "ops_3d_a": {"advect_scalar": 4.00e-07, "advect_vel": 4.54e-07, "add_buoyancy": 3.23e-08, "add_gravity": 2.98e-08, "set_wall_bcs": 0.00e+00, "divergence": 8.48e-08, "velocity_update": 3.55e-08},
    "ops_3d_b": {"advect_scalar": 1.25e-06, "advect_vel": 6.82e-07, "add_buoyancy": 3.23e-08, "add_gravity": 2.60e-08, "set_wall_bcs": 0.00e+00, "divergence": 6.77e-08, "velocity_update": 3.15e-08},
    "tile_lo": {"advect_scalar": 2.40e-06, "advect_vel": 3.88e-06, "add_buoyancy": 3.16e-08, "add_gravity": 2.77e-08, "set_wall_bcs": 0.00e+00, "divergence": 6.10e-08, "velocity_update": 7.20e-08, "step_p": 1.57e-06, "step_U": 2.49e-06, "step_density": 1.72e-06},
    "tile_hi": {"advect_scalar": 2.78e-06, "advect_vel": 3.58e-06, "add_buoyancy": 3.30e-08, "add_gravity": 2.12e-08, "set_wall_bcs": 0.00e+00, "divergence": 9.26e-08, "velocity_update": 6.91e-08, "step_p": 2.21e-06, "step_U": 2.49e-06, "step_density": 2.50e-06},
    "small_lo": {"advect_scalar": 3.88e-07, "advect_vel": 6.67e-07, "add_buoyancy": 2.94e-08, "add_gravity": 2.23e-08, "set_wall_bcs": 0.00e+00, "divergence": 9.16e-08, "velocity_update": 6.74e-08, "step_p": 2.73e-07, "step_U": 4.79e-07, "step_density": 3.08e-07},
    "small_hi": {"advect_scalar": 3.42e-07, "advect_vel": 7.18e-07, "add_buoyancy": 3.01e-08, "add_gravity": 3.64e-08, "set_wall_bcs": 0.00e+00, "divergence": 4.57e-08, "velocity_update": 5.95e-08, "step_p": 5.24e-07, "step_U": 6.99e-07, "step_density": 2.46e-07},
    "large_lo": {"advect_scalar": 7.68e-07, "advect_vel": 1.12e-06, "add_buoyancy": 5.01e-08, "add_gravity": 4.93e-08, "set_wall_bcs": 0.00e+00, "divergence": 7.01e-08, "velocity_update": 7.14e-08, "step_p": 7.00e-07, "step_U": 6.06e-07, "step_density": 5.90e-07},
    "large_hi": {"advect_scalar": 1.13e-06, "advect_vel": 1.03e-06, "add_buoyancy": 2.77e-08, "add_gravity": 2.06e-08, "set_wall_bcs": 0.00e+00, "divergence": 7.92e-08, "velocity_update": 5.41e-08, "step_p": 8.32e-07, "step_U": 7.88e-07, "step_density": 1.02e-06},
    "tile_open": {"advect_scalar": 4.06e-06, "advect_vel": 3.86e-06, "add_buoyancy": 3.58e-08, "add_gravity": 5.18e-08, "set_wall_bcs": 0.00e+00, "divergence": 7.96e-08, "velocity_update": 6.65e-08, "step_p": 2.49e-06, "step_U": 2.67e-06, "step_density": 3.95e-06},
    "small_open": {"advect_scalar": 1.15e-06, "advect_vel": 5.99e-07, "add_buoyancy": 3.28e-08, "add_gravity": 2.04e-08, "set_wall_bcs": 0.00e+00, "divergence": 6.73e-08, "velocity_update": 5.29e-08, "step_p": 4.28e-07, "step_U": 4.58e-07, "step_density": 1.02e-06},
    "large_open": {"advect_scalar": 2.57e-06, "advect_vel": 1.47e-06, "add_buoyancy": 5.18e-08, "add_gravity": 4.31e-08, "set_wall_bcs": 0.00e+00, "divergence": 8.83e-08, "velocity_update": 6.07e-08, "step_p": 5.88e-07, "step_U": 1.17e-06, "step_density": 2.57e-06},
    "hostile2d_open2_lo": {"advect_scalar": 1.37e-06, "advect_vel": 2.03e-06, "add_buoyancy": 3.05e-08, "add_gravity": 2.66e-08, "set_wall_bcs": 0.00e+00, "divergence": 5.74e-08, "velocity_update": 6.46e-08},
    "hostile2d_open2_hi": {"advect_scalar": 2.54e-06, "advect_vel": 2.28e-06, "add_buoyancy": 3.86e-08, "add_gravity": 2.14e-08, "set_wall_bcs": 0.00e+00, "divergence": 9.55e-08, "velocity_update": 5.96e-08},
    "hostile2d_open4_lo": {"advect_scalar": 1.37e-06, "advect_vel": 2.03e-06, "add_buoyancy": 3.05e-08, "add_gravity": 2.66e-08, "set_wall_bcs": 0.00e+00, "divergence": 5.74e-08, "velocity_update": 6.46e-08},
    "hostile2d_open4_hi": {"advect_scalar": 2.56e-06, "advect_vel": 2.28e-06, "add_buoyancy": 3.86e-08, "add_gravity": 2.14e-08, "set_wall_bcs": 0.00e+00, "divergence": 9.55e-08, "velocity_update": 5.96e-08},
    "hostile2d_salt_lo": {"advect_scalar": 1.37e-06, "advect_vel": 2.03e-06, "add_buoyancy": 3.05e-08, "add_gravity": 2.66e-08, "set_wall_bcs": 0.00e+00, "divergence": 5.74e-08, "velocity_update": 6.46e-08},
    "hostile2d_salt_hi": {"advect_scalar": 2.46e-06, "advect_vel": 2.26e-06, "add_buoyancy": 3.86e-08, "add_gravity": 2.14e-08, "set_wall_bcs": 0.00e+00, "divergence": 9.55e-08, "velocity_update": 5.96e-08},
}

TOL = {n: {f: 4.0 * v for f, v in fam.items()} for n, fam in FIGURE.items()}


def print_figures():
    for n in GOLDEN_2D + GOLDEN_3D + tuple(OWN) + HOSTILE_2D:
        fam = {}
        for op in model_outputs(n):
            fam[family(op)] = max(fam.get(family(op), 0.0), figure(n, op))
        print(f'    "{n}": {{' + ", ".join(f'"{k}": {v:.2e}' for k, v in fam.items()) + "},")


if __name__ == "__main__":
    print_figures()
