"""Hostile 2D geometries (numpy only), shared by tools/make_golden.py (gen_hostile2d), test_hostile2d_reference.py (CPU) and
test_hostile2d_gpu.py: what tests/util.py:make_flags never builds -- Fluid and Empty cells on the domain border (rays that leave the
domain, the MacCormack correction on fluid border cells), scattered Obstacle / Empty cells (every adjacency in both axes, diagonal
contacts, one-cell gaps) and samples of a batch whose flags differ in many cells and in which sides are open.

  open2   column i = 0 (rows 1..) and row j = H-1 (columns ..W-2) are Fluid, two of those cells Empty; sample 1 also opens row j = 0
  open4   all four sides Fluid, the same two Empty cells
  salt    closed ring; interior cells independently 8 % Obstacle, 5 % Empty, drawn per sample
every kind has one 3x4 obstacle box, and every sample b >= 1 draws its own 8 % / 5 % scatter from seed + b.  The only sample of a
batch of one draws it too: with the box alone fewer than 50 rays of an open state would end in a non-fluid cell.

The seeds are not tuned to any code under test: GOLDEN_SEED["hi"] and LARGE_SEED are the smallest seeds (from 3) for which
check_conditions() -- counts on the float64 model -- holds on every state built from them (scan_seeds() prints the search).
"""
import functools

import numpy as np

FLUID, OBST, EMPTY = 1.0, 2.0, 4.0
KINDS = ("open2", "open4", "salt")
CFLS = {"lo": 0.6, "hi": 6.2}
GOLDEN_SHAPE = (2, 19, 37)
GOLDEN_SEED = {"lo": 3, "hi": 6}
# the states of tests/golden/hostile2d.npz (cfl 0.6) and hostile2d_hi.npz (cfl 6.2): name -> (kind, cfl, seed)
GOLDEN_STATES = {f"{k}_{c}": (k, CFLS[c], GOLDEN_SEED[c]) for k in KINDS for c in CFLS}
STICK_SEED = 103
# the states the GPU tests build beyond the golden ones: seed, and the shapes of the Jacobi and of the adjoint / PCG tests
LARGE_SEED = 5
LARGE_SHAPES = ((2, 40, 70), (1, 35, 130), (3, 33, 258))       # one, two and four 64-column tiles, partial tiles in x and y
JACOBI_SHAPE = (2, 96, 150)
ADJOINT_SHAPE = (2, 33, 70)
P_OBST, P_EMPTY = 0.08, 0.05


def _scatter(f, rng):
    """8 % Obstacle, 5 % Empty on the interior cells of one sample's (H, W) flags"""
    r = rng.random(f.shape)
    inner = np.zeros(f.shape, bool)
    inner[1:-1, 1:-1] = True
    f[(r < P_OBST) & inner] = OBST
    f[(r > 1.0 - P_EMPTY) & inner] = EMPTY


def flags(kind, B, H, W, seed):
    assert kind in KINDS and H >= 12 and W >= 12
    f = np.full((B, 1, 1, H, W), FLUID, np.float32)
    f[:, :, :, 0, :] = f[:, :, :, -1, :] = f[:, :, :, :, 0] = f[:, :, :, :, -1] = OBST
    for b in range(B):
        g = f[b, 0, 0]
        if kind == "salt" or b >= 1 or B == 1:
            _scatter(g, np.random.default_rng(seed + b))
        if kind in ("open2", "open4"):
            g[1:, 0] = FLUID
            g[-1, :-1] = FLUID
            if kind == "open4" or b == 1:
                g[0, :-1] = FLUID
            if kind == "open4":
                g[0, :] = FLUID
                g[:, -1] = FLUID
            g[-1, 6] = EMPTY
            g[5, 0] = EMPTY
        g[H // 3:H // 3 + 3, W // 4:W // 4 + 4] = OBST
    return f


def make_state(kind, B, H, W, cfl, seed):
    """like semantics3d_cases.state: U standard normal, rho in [0, 1), p and orig standard normal, dt = float32(cfl / max|U|)"""
    rng = np.random.default_rng(seed)
    U = rng.standard_normal((B, 2, 1, H, W)).astype(np.float32)
    s = dict(kind=kind, cfl=cfl, flags=flags(kind, B, H, W, seed), U=U, orig=rng.standard_normal(U.shape).astype(np.float32),
             rho=rng.random((B, 1, 1, H, W)).astype(np.float32), p=rng.standard_normal((B, 1, 1, H, W)).astype(np.float32),
             dt=float(np.float32(cfl / np.abs(U).max())), gravity=[0.3, 0.25, -0.2], rho_star=0.05)
    for v in s.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return s


@functools.lru_cache(maxsize=None)
def state(kind, B, H, W, cfl, seed):
    """the inputs of a case, built once per process and never modified"""
    return make_state(kind, B, H, W, cfl, seed)


def golden_state(name):
    kind, cfl, seed = GOLDEN_STATES[name]
    return state(kind, *GOLDEN_SHAPE, cfl, seed)


def golden_file(name):
    return "hostile2d_hi" if name.endswith("_hi") else "hostile2d"


def stick_flags(f, seed):
    """flags_stick: about 60 % of the obstacle cells (border ring, box and scatter alike) become TypeStick (128)"""
    fs = f.copy()
    fs[(f == OBST) & (np.random.default_rng(seed).random(f.shape) < 0.6)] = 128
    return fs


def border_mask(shape):
    m = np.zeros(shape, bool)
    m[..., 0, :] = m[..., -1, :] = m[..., :, 0] = m[..., :, -1] = True
    return m


def adjacency(f):
    """number of neighbouring cell pairs of each unordered type pair, in x and in y: {"FO_x": n, "FE_x": n, "EO_x": n, "FO_y": ...}"""
    out = {}
    for ax, tag in ((-1, "x"), (-2, "y")):
        n = f.shape[ax]
        a, b = np.take(f, range(0, n - 1), ax), np.take(f, range(1, n), ax)
        for name, (s, t) in (("FO", (FLUID, OBST)), ("FE", (FLUID, EMPTY)), ("EO", (EMPTY, OBST))):
            out[f"{name}_{tag}"] = int((((a == s) & (b == t)) | ((a == t) & (b == s))).sum())
    return out


def conditions(s):
    """what a state puts in front of the kernels (counts, none of them a measurement of the code under test):
    border_rays / blocked_rays   unit steps of the float64 model's line trace that left the domain / ended in a non-fluid cell over
                                 ONE MacCormack advectScalar: its forward pass and its backward pass, which traces the opposite
                                 way (fluid_model_nd.TRACE_STATS).  The Euler call is that forward pass alone, the two
                                 sample_outside_fluid settings trace the same rays, and advectVelocity has no line trace (it
                                 samples at x - dt u): no operator reaches case 1 with other rays than these
    fluid_border_cells           Fluid cells on the domain border
    adjacency                    see adjacency()
    sample_diff                  smallest share of cells in which two samples of the batch differ (1.0 for B = 1)"""
    import fluid_model_nd as M
    M.TRACE_STATS.update(border=0, blocked=0)
    M.advect_scalar(s["dt"], s["rho"], s["U"], s["flags"], "maccormackFluidNet", False, 0.6)
    f = s["flags"]
    B = f.shape[0]
    diff = [float((f[a] != f[b]).mean()) for a in range(B) for b in range(a + 1, B)]
    return dict(border_rays=M.TRACE_STATS["border"], blocked_rays=M.TRACE_STATS["blocked"],
                fluid_border_cells=int(((f == FLUID) & border_mask(f.shape)).sum()), adjacency=adjacency(f),
                sample_diff=min(diff) if diff else 1.0)


def check_conditions(s, c=None):
    """the conditions every state of this module must meet, by kind and cfl"""
    c = conditions(s) if c is None else c
    kind, hi = s["kind"], s["cfl"] > 1.0
    what = f"{kind} cfl {s['cfl']} {s['flags'].shape}: {c}"
    if kind != "salt" and hi:
        assert c["border_rays"] >= 30, what
    else:
        assert c["border_rays"] == 0, what
    if hi:
        assert c["blocked_rays"] >= 50, what
    if kind != "salt":
        assert c["fluid_border_cells"] >= 100, what
    else:
        assert min(c["adjacency"].values()) >= 5, what
    if s["flags"].shape[0] > 1:
        assert c["sample_diff"] >= 0.05, what
    return c


def one_signed(U, sign):
    """the velocity fields of the tile tests whose every forward trace goes towards one corner (|U| * sign)"""
    return np.ascontiguousarray(np.abs(U) * np.float32(sign))


def one_signed_state(s, sign):
    """the state s with U replaced by one_signed(U, sign): same dt, so max|U| dt stays the state's cfl"""
    return dict(s, U=one_signed(s["U"], sign))


def golden_arrays(golden, name):
    """the arrays of the golden state `name` ("open2_lo", ...): z[k] and z.files as of an .npz that held this state alone.
    `golden` is the suite's fixture (name of a file under tests/golden -> NpzFile)"""
    return Prefixed(golden(golden_file(name)), name + "_")


class Prefixed:
    """the arrays of one state in an .npz that holds several: z[k] is npz[prefix + k]"""

    def __init__(self, npz, prefix):
        self.npz, self.prefix = npz, prefix
        self.files = [f[len(prefix):] for f in npz.files if f.startswith(prefix)]

    def __getitem__(self, k):
        return self.npz[self.prefix + k]


# ---- whole-step states (the sim_* goldens): a 48^2 plume with open sides ---------------------------------------------------
SIM_RES = 48
SIM_KINDS = ("open_top", "open_all")


def sim_flags(kind, closed):
    """`closed` is the plume's closed-ring flags (1, 1, 1, 48, 48); open_top: the top row Fluid with four Empty cells; open_all: also
    both side columns from row 4 up, one Empty cell; one 3x5 obstacle box"""
    assert kind in SIM_KINDS
    f = closed.copy()
    res = f.shape[-1]
    f[:, :, :, -1, 1:-1] = FLUID
    f[:, :, :, -1, 10:14] = EMPTY
    if kind == "open_all":
        f[:, :, :, 4:, 0] = FLUID
        f[:, :, :, 4:, -1] = FLUID
        f[:, :, :, 20, 0] = EMPTY
    f[:, :, :, res // 2:res // 2 + 3, res // 3:res // 3 + 5] = OBST
    return f


def sim_state(kind, plume):
    """`plume` is util.plume_state(SIM_RES): the same BC arrays, hostile flags and start"""
    st = dict(plume)
    st["flags"] = sim_flags(kind, plume["flags"])
    st["U"], st["density"] = sim_fields(plume["U"].shape, plume["density"].shape)
    return st


def sim_fields(shape_U, shape_rho):
    """U = 3 N(0, 1), density in [0, 1).  With dt = 0.1 that is max|U| dt = 1.2: no ray leaves the domain (one from an interior cell
    centre needs more than 1.5); these states bring border Fluid and Empty cells to every stage of the step"""
    rng = np.random.default_rng(1)
    U = (rng.standard_normal(shape_U) * 3.0).astype(np.float32)
    return U, rng.random(shape_rho).astype(np.float32)


def all_states(golden_hi_seed, large_seed):
    """every state of state() that the tests use: the cfl 6.2 goldens, the larger GPU shapes at both cfl, the Jacobi and the adjoint /
    PCG states, and the one-signed variants of the larger shapes at cfl 6.2"""
    out = [make_state(k, *GOLDEN_SHAPE, CFLS["hi"], golden_hi_seed) for k in KINDS]
    for shp in LARGE_SHAPES:
        for k in KINDS:
            for cfl in CFLS.values():
                out.append(make_state(k, *shp, cfl, large_seed))
            out += [one_signed_state(out[-1], sign) for sign in (-1.0, 1.0)]
    out += [make_state(k, *shp, CFLS["lo"], large_seed) for shp in (JACOBI_SHAPE, ADJOINT_SHAPE) for k in ("open4", "salt")]
    return out


def scan_seeds(stop=40):
    """prints, for each seed from 3, whether check_conditions() holds on every state built from it as the golden cfl 6.2 seed and as
    LARGE_SEED"""
    for seed in range(3, stop):
        ok = {}
        for what, states in (("golden hi", all_states(seed, seed)[:len(KINDS)]), ("large", all_states(seed, seed)[len(KINDS):])):
            try:
                for s in states:
                    check_conditions(s)
                ok[what] = True
            except AssertionError as e:
                ok[what] = str(e)[:110]
        print(seed, ok)


if __name__ == "__main__":
    scan_seeds()
