"""3D obstacles from geometry on the GPU: fluid.voxelizeMesh, fluid.createSphere and fluid.createBox3D must give the flags of the numpy
model (tests/voxel_reference.py; tests/test_voxel_reference.py holds the model to exact ray casts) on every cell, and the report's
two counts.  Then a few time steps around a voxelised body."""
import numpy as np
import pytest
import torch

import voxel_reference as VR
from util import PLUME_CFG, plume_state

pytestmark = pytest.mark.gpu

FIXTURES = dict(VR.fixtures(), torus=VR.placed(VR.torus(6.0, 2.5), 1.0, (17.4, 9.7, 5.8), VR.rotation(7)))
_MODEL = {}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


def model(shape, mesh, key=None):
    """voxelize_model, computed once per key"""
    if key is None:
        return VR.voxelize_model(shape, *mesh)
    if key not in _MODEL:
        _MODEL[key] = VR.voxelize_model(shape, *mesh)
    return _MODEL[key]


def fluid_flags(B, shape):
    return np.full((B, 1) + tuple(shape), VR.FLUID, np.float32)


def on_device(mesh, dev):
    v, f = mesh
    return torch.from_numpy(np.ascontiguousarray(v, np.float32)).to(dev), torch.from_numpy(np.ascontiguousarray(f, np.int32)).to(dev)


def voxelize(dev, flags0, mesh, sample=None, check=False):
    """-> (flags after the call as numpy, the report as a list)"""
    from fluidnet_cxx_amd import fluid
    bd = dict(flags=torch.from_numpy(flags0.copy()).to(dev))
    v, f = on_device(mesh, dev)
    report = fluid.voxelizeMesh(bd, v, f, sample=sample, check=check)
    return bd["flags"].cpu().numpy(), (None if report is None else report.tolist())


def assert_cells(got, want, what):
    assert got.shape == want.shape and np.array_equal(got, want), f"{what}: {int((got != want).sum())} of {got.size} cells differ"


def merged(*meshes):
    vs, fs, base = [], [], 0
    for v, f in meshes:
        vs.append(v); fs.append(f + base); base += len(v)
    return np.concatenate(vs).astype(np.float32), np.concatenate(fs).astype(np.int32)


@pytest.mark.parametrize("name", sorted(FIXTURES))
def test_base_fixtures(dev, name):
    inside, open_rows, bad = model(VR.GRID, FIXTURES[name], name)
    assert (open_rows, bad) == (0, 0) and inside.any()
    flags0 = fluid_flags(2, VR.GRID)
    got, report = voxelize(dev, flags0, FIXTURES[name])
    assert_cells(got, VR.apply_model(flags0, inside), name)
    assert report == [0, 0]
    got, report = voxelize(dev, flags0, FIXTURES[name], check=True)          # a closed mesh passes the check
    assert report is None
    assert_cells(got, VR.apply_model(flags0, inside), name + ", check=True")


@pytest.mark.parametrize("W", [31, 32, 33, 64])
def test_word_boundaries(dev, W):
    """the bit of index W is the last of a word (W = 31), the first of the next (32, 64) or the second (33); the ball sticks out of the
    domain at high x, so rows cross at i0 == W: no cell toggles, the row still closes"""
    shape = (4, 6, W)
    mesh = VR.placed(VR.icosphere(1), 2.4, (W - 1.3, 2.9, 1.9))
    inside, open_rows, bad = model(shape, mesh)
    assert inside[:, :, W - 1].any() and (open_rows, bad) == (0, 0)
    flags0 = fluid_flags(1, shape)
    got, report = voxelize(dev, flags0, mesh)
    assert_cells(got, VR.apply_model(flags0, inside), f"W = {W}")
    assert report == [0, 0]


def test_wide_rows(dev):
    """66 words a row: more than a wave's 64 lanes, the carry is handed on; the ellipsoid is clipped at both ends of x"""
    shape = (3, 5, 2100)
    mesh = VR.placed(VR.icosphere(3), (1057.5, 12.0, 8.0), (1052.5, 2.1, 1.1))
    assert mesh[0][:, 0].min() < -4.9 and mesh[0][:, 0].max() > 2109.9
    inside, open_rows, bad = model(shape, mesh)
    assert inside[:, :, 0].any() and inside[:, :, -1].any() and not inside.all() and (open_rows, bad) == (0, 0)
    flags0 = fluid_flags(2, shape)
    got, report = voxelize(dev, flags0, mesh)
    assert_cells(got, VR.apply_model(flags0, inside), "wide rows")
    assert report == [0, 0]


def test_mixed_face_sizes(dev):
    """5 120 faces smaller than a cell (each walked by its own lane) and a box whose faces span 195 rows (walked by a whole wave), in one
    call and in two"""
    shape = (16, 20, 40)
    ball = VR.placed(VR.icosphere(4), 3.0, (8.3, 9.7, 8.1))
    box = VR.placed(VR.box_mesh((14.5, 2.5, 1.5), (36.2, 17.5, 14.5)))
    inside, open_rows, bad = model(shape, merged(ball, box))
    assert (open_rows, bad) == (0, 0)
    flags0 = fluid_flags(1, shape)
    want = VR.apply_model(flags0, inside)
    got, report = voxelize(dev, flags0, merged(ball, box))
    assert_cells(got, want, "one call")
    assert report == [0, 0]
    first, _ = voxelize(dev, flags0, ball)
    both, _ = voxelize(dev, first, box)
    assert_cells(both, want, "two calls")                       # the bodies are disjoint: their union is the even-odd result


def test_bad_input(dev):
    """a face index out of range, a NaN vertex, an Inf vertex and a far vertex: counted and skipped, nothing else changes"""
    from fluidnet_cxx_amd import fluid
    v, f = FIXTURES["icosphere"]
    n = len(v)
    v2 = np.concatenate([v, [[np.nan, 1, 1], [1, np.inf, 1], [1, 1, 3e4], [-2e4, 1, 1]]]).astype(np.float32)
    f2 = f.copy()
    f2[0, 1] = len(v2)                                          # one past the end
    f2[1, 0] = -1
    f2[2] = (n, 0, 1)
    f2 = np.concatenate([f2, [[n + 1, 0, 1], [2, n + 2, 1], [2, 3, n + 3], [2 ** 31 - 1, 0, 1]]]).astype(np.int32)
    inside, open_rows, bad = model(VR.GRID, (v2, f2))
    want = VR.voxelize_model(VR.GRID, v, f[3:])
    assert bad == 7 and open_rows == want[1] > 0 and np.array_equal(inside, want[0])
    flags0 = fluid_flags(2, VR.GRID)
    got, report = voxelize(dev, flags0, (v2, f2), check=False)
    assert_cells(got, VR.apply_model(flags0, inside), "bad faces")
    assert report == [open_rows, bad]
    bd = dict(flags=torch.from_numpy(flags0.copy()).to(dev))
    with pytest.raises(ValueError, match=rf"{open_rows} open rows.*{bad} bad faces"):
        fluid.voxelizeMesh(bd, *on_device((v2, f2), dev))
    # bad faces alone raise too
    closed = (v2, np.concatenate([f, [[n, 0, 1]]]).astype(np.int32))
    with pytest.raises(ValueError, match=r"0 open rows.*1 bad faces"):
        fluid.voxelizeMesh(bd, *on_device(closed, dev))
    # no faces at all: nothing is written
    got, report = voxelize(dev, flags0, (v, f[:0]))
    assert_cells(got, flags0, "no faces")
    assert report == [0, 0]


def test_one_sample(dev):
    from fluidnet_cxx_amd import fluid
    inside = model(VR.GRID, FIXTURES["rotated_box"], "rotated_box")[0]
    flags0 = fluid_flags(3, VR.GRID)
    flags0[2, 0, 3:5] = VR.EMPTY
    got, report = voxelize(dev, flags0, FIXTURES["rotated_box"], sample=1)
    assert_cells(got, VR.apply_model(flags0, inside, sample=1), "sample=1")
    assert report == [0, 0]
    bd = dict(flags=torch.from_numpy(flags0).to(dev))
    for bad in (3, -1):
        with pytest.raises(ValueError, match="out of range"):
            fluid.voxelizeMesh(bd, *on_device(FIXTURES["rotated_box"], dev), sample=bad)


def test_prior_contents(dev):
    """cells outside keep what they held (TypeEmpty, inflow codes, obstacles); cells inside are overwritten whatever they held"""
    inside = model(VR.GRID, FIXTURES["icosphere"], "icosphere")[0]
    rng = np.random.default_rng(5)
    flags0 = rng.choice(np.array([1, 2, 4, 8, 16, 128], np.float32), size=(2, 1) + VR.GRID)
    got, _ = voxelize(dev, flags0, FIXTURES["icosphere"])
    assert_cells(got, VR.apply_model(flags0, inside), "prior contents")
    assert (got[:, 0][:, inside] == VR.OBSTACLE).all() and np.array_equal(got[:, 0][:, ~inside], flags0[:, 0][:, ~inside])
    assert (flags0[:, 0][:, ~inside] == VR.EMPTY).any() and (flags0[:, 0][:, inside] == VR.EMPTY).any()


def test_workspace_reuse_and_graph_replay(dev):
    from fluidnet_cxx_amd import fluid
    from fluidnet_cxx_amd._ext import ext
    a, b = FIXTURES["torus"], FIXTURES["icosphere_clipped"]
    flags0 = fluid_flags(2, VR.GRID)
    want_a = VR.apply_model(flags0, model(VR.GRID, a, "torus")[0])
    want_b = VR.apply_model(flags0, model(VR.GRID, b, "icosphere_clipped")[0])
    fl = torch.from_numpy(flags0).to(dev)
    ws = torch.full((ext.voxelize_mesh_ws_bytes(fl),), 0xA5, dtype=torch.uint8, device=dev)     # whatever the workspace held
    for mesh, want in ((a, want_a), (b, want_b), (a, want_a)):
        fl = torch.from_numpy(flags0).to(dev)
        report = ext.voxelize_mesh_(fl, *on_device(mesh, dev), -1, ws)
        assert_cells(fl.cpu().numpy(), want, "one workspace, call after call")
        assert report.tolist() == [0, 0]
    with pytest.raises(RuntimeError, match="workspace too small"):
        ext.voxelize_mesh_(fl, *on_device(a, dev), -1, ws[:-4])
    # a captured call replayed onto fresh flags
    va, fa = on_device(a, dev)
    bd = dict(flags=torch.from_numpy(flags0).to(dev))
    fluid.voxelizeMesh(bd, va, fa, check=False)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        report = fluid.voxelizeMesh(bd, va, fa, check=False)
    for _ in range(2):
        bd["flags"].fill_(VR.FLUID)
        report.fill_(-1)
        g.replay()
        torch.cuda.synchronize()
        assert_cells(bd["flags"].cpu().numpy(), want_a, "graph replay")
        assert report.tolist() == [0, 0]


def test_primitives(dev):
    from fluidnet_cxx_amd import fluid
    shape = (9, 22, 70)                                          # W = 70: two 64-wide blocks; H = 22: no multiple of the block's 4 rows
    rng = np.random.default_rng(9)
    flags0 = rng.choice(np.array([1, 2, 4], np.float32), size=(3, 1) + shape)
    for args in ((33.4, 10.2, 4.0, 3.7), (66.0, 3.0, 1.0, 6.5), (0.0, 0.0, 0.0, 2.0), (30.0, 11.0, 4.0, 0.0), (35.0, 11.0, 4.0, 40.0)):
        for sample in (None, 2):
            bd = dict(flags=torch.from_numpy(flags0.copy()).to(dev))
            fluid.createSphere(bd, *args, sample=sample)
            assert_cells(bd["flags"].cpu().numpy(), VR.apply_model(flags0, VR.sphere_model(shape, *args), sample), f"sphere {args}, sample={sample}")
    for args in ((2, 7, 3, 8, 1, 6), (60.5, 99, -3, 4.5, 2.2, 2.9), (0, 70, 0, 22, 0, 9), (5, 5, 1, 9, 1, 9)):
        for sample in (None, 0):
            bd = dict(flags=torch.from_numpy(flags0.copy()).to(dev))
            fluid.createBox3D(bd, *args, sample=sample)
            assert_cells(bd["flags"].cpu().numpy(), VR.apply_model(flags0, VR.box_model(shape, *args), sample), f"box {args}, sample={sample}")
    # the sphere's middle slice is createCylinder's disc
    for cx, cy, cz, r in ((33.4, 10.2, 4.0, 3.7), (20.0, 9.5, 6.0, 7.3)):
        one = fluid_flags(1, shape)
        s, c = dict(flags=torch.from_numpy(one.copy()).to(dev)), dict(flags=torch.from_numpy(one.copy()).to(dev))
        fluid.createSphere(s, cx, cy, cz, r)
        fluid.createCylinder(c, cx, cy, r)
        k = int(cz)
        assert torch.equal(s["flags"][0, 0, k], c["flags"][0, 0, k]) and (s["flags"][0, 0, k] == VR.OBSTACLE).any()
    # an integer mesh box is createBox3D's box
    (x0, y0, z0), (x1, y1, z1) = VR.BOX_LO, VR.BOX_HI
    bd = dict(flags=torch.from_numpy(fluid_flags(2, VR.GRID)).to(dev))
    fluid.createBox3D(bd, x0, x1, y0, y1, z0, z1)
    got, _ = voxelize(dev, fluid_flags(2, VR.GRID), FIXTURES["integer_box"])
    assert_cells(got, bd["flags"].cpu().numpy(), "mesh box against createBox3D")


def test_refusals(dev):
    from fluidnet_cxx_amd import fluid
    v, f = on_device(FIXTURES["integer_box"], dev)
    flat = dict(flags=torch.ones(1, 1, 1, 16, 16, device=dev))
    for call in (lambda: fluid.createSphere(flat, 8, 8, 0, 3), lambda: fluid.createBox3D(flat, 1, 4, 1, 4, 0, 1),
                 lambda: fluid.voxelizeMesh(flat, v, f)):
        with pytest.raises(RuntimeError, match="3D grids only"):
            call()
    bd = dict(flags=torch.ones((1, 1) + VR.GRID, device=dev))
    with pytest.raises(RuntimeError, match=r"\(F,3\) int32"):
        fluid.voxelizeMesh(bd, v, f.long())
    with pytest.raises(RuntimeError, match=r"\(V,3\) float32"):
        fluid.voxelizeMesh(bd, v.double(), f)
    with pytest.raises(RuntimeError, match="on the device of flags"):
        fluid.voxelizeMesh(bd, v.cpu(), f)
    assert (bd["flags"] == 1).all()


def test_steps_around_a_voxelised_sphere(dev):
    """three 'jacobi' steps of the 3D plume with a voxelised ball in its way: finite fields, no flow through the faces of the body"""
    from fluidnet_cxx_amd import fluid, simulate
    D, res = 16, 24
    bd = {k: torch.from_numpy(v).to(dev) for k, v in plume_state(res, D).items()}
    mesh = VR.placed(VR.icosphere(2), 3.6, (12.2, 11.7, 8.3))
    inside, open_rows, bad = model((D, res, res), mesh)
    assert inside.sum() > 100 and (open_rows, bad) == (0, 0)
    flags0 = bd["flags"].cpu().numpy()
    fluid.voxelizeMesh(bd, *on_device(mesh, dev))
    assert_cells(bd["flags"].cpu().numpy(), VR.apply_model(flags0, inside), "flags of the step")
    for _ in range(3):
        simulate(PLUME_CFG, bd, None, "jacobi")
    torch.cuda.synchronize()
    for k in ("U", "density", "p"):
        assert torch.isfinite(bd[k]).all(), k
    U = bd["U"][0].cpu().numpy()
    assert np.abs(U).max() > 0.1
    for c, axis in ((0, 2), (1, 1), (2, 0)):
        assert (U[c][inside] == 0).all()                                 # the face below the cell
        assert (np.roll(U[c], -1, axis=axis)[inside] == 0).all()         # and the one above it (the body touches no domain wall)
