"""The 64-column tiling of the 3D two-sweep Jacobi march (fnx_jacobi.hip, X64): a workgroup's waves own 64 columns each and hand each
other their edge columns through LDS.  It must compute the bits of the 60-column kernel and of the CPU oracle.  Both tilings are forced
per call (`ext.Geom(jacobi_x=60 / 64)`, i.e. bits 8-9 of FnxGrid.ref_quirks).

Shapes: W in {64, 67, 128, 130, 192} (one, two and three waves a row; a last tile of 3 and of 2 columns), H in {8, 12}, D in
{3, 5, 24} (one, two and many steps a chunk), B = 2.  Sweeps 2, 4, 7 and 100: an odd count ends in the single-sweep kernel.  Obstacles:
none; a block that straddles the seams between waves (columns 62-65 and 126-129); obstacles that differ in every plane (no "same" bit);
obstacles extruded in z.  From zero and from a random p.  `div` has a band of denormals over the first seam, so that the scaled division
(div6_tiny) runs in the edge lanes, whose x neighbour comes through the mailbox."""
import numpy as np
import pytest
import torch

from util import PLUME_CFG, assert_bitexact, box_plume_state, make_flags

pytestmark = pytest.mark.gpu

KINDS = ("none", "block", "planes", "extruded")
SWEEPS = (2, 4, 7, 100)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ext():
    from fluidnet_cxx_amd._ext import ext
    return ext


@pytest.fixture(scope="module")
def tiling(ext):
    return lambda x: ext.Geom(jacobi_x=x)


def T(x, dev):
    return torch.from_numpy(np.ascontiguousarray(x)).to(dev)


def N(t):
    return t.detach().cpu().numpy()


def seam_flags(kind, B, D, H, W):
    f = make_flags(B, D, H, W, boxes=False)
    cols = [c for c in (62, 63, 64, 65, 126, 127, 128, 129) if c < W - 1]
    rows = [r for r in (3, 4, 5) if r < H - 1]
    if kind == "block":                              # through the middle planes only: the planes next to it differ from it
        k0, k1 = (1, D - 1) if D <= 5 else (D // 3, 2 * D // 3)
        for c in cols:
            f[:, :, k0:k1, 3:6, c] = 2
    elif kind == "extruded":
        for n, c in enumerate(cols):
            f[:, :, 1:D - 1, rows[n % len(rows)], c] = 2
    elif kind == "planes":
        rng = np.random.default_rng(7)
        for b in range(B):
            for k in range(1, D - 1):
                for c in rng.choice(cols, size=min(3, len(cols)), replace=False):
                    f[b, 0, k, rng.choice(rows), c] = 2
                f[b, 0, k, 1 + (k + b) % (H - 2), 1 + (7 * k) % (W - 2)] = 2
    return f


def seam_div(B, D, H, W, seed):
    rng = np.random.default_rng(seed)
    div = rng.standard_normal((B, 1, D, H, W)).astype(np.float32)
    div[..., 60:68] *= np.float32(1e-40)             # denormals on both sides of the seam at column 64 (and at the wall of W = 64, 67)
    div[:, :, :, 2, 61:67] = np.float32(-3e-45)      # quotients that round to -0
    return div


@pytest.mark.parametrize("W", [64, 67, 128, 130, 192])
@pytest.mark.parametrize("H,D", [(8, 3), (8, 5), (8, 24), (12, 3), (12, 5), (12, 24)])
def test_solve_bits(dev, ext, oracle, tiling, W, H, D):
    """ext.solve_linear_system (from zero) and ext.jacobi_sweeps_ (from a random p): forced 64 == forced 60 == the oracle"""
    B = 2
    div = seam_div(B, D, H, W, 100 * D + W)
    p0 = np.random.default_rng(W + H).standard_normal((B, 1, D, H, W)).astype(np.float32)
    td = T(div, dev)
    for kind in KINDS:
        flags = seam_flags(kind, B, D, H, W)
        tf = T(flags, dev)
        for n in SWEEPS:
            got = {}
            for x in (60, 64):
                pz = ext.solve_linear_system(tf, td, True, 0.0, n, False, tiling(x))[0]
                pr = T(p0, dev)
                ext.jacobi_sweeps_(tf, td, pr, True, n, geom=tiling(x))
                got[x] = (pz, pr)
            what = f"{kind} {(B, D, H, W)}: {n} sweeps"
            assert torch.equal(got[64][0], got[60][0]), what + " from zero, 64 vs 60 columns"
            assert torch.equal(got[64][1], got[60][1]), what + " from p, 64 vs 60 columns"
            # the solve's last sweep is the residual's single sweep; its iterate is the oracle's after n sweeps all the same
            assert_bitexact(N(got[64][0]), oracle.jacobi(flags, div, True, 0.0, n)[0], what + " from zero")
            assert_bitexact(N(got[64][1]), oracle.jacobi_sweeps(flags, div, p0, True, n), what + " from p")


@pytest.mark.parametrize("shape", [(2, 5, 12, 130), (2, 24, 8, 192)])
def test_simulate_bits(dev, tiling, shape):
    """two steps of simulate(..., 'jacobi') on a 3D plume with an obstacle box: every field the same under both tilings"""
    from fluidnet_cxx_amd import simulate
    B, D, H, W = shape
    st = box_plume_state(B, D, H, W)
    st["flags"][:, 0, 1:D - 1, H - 4:H - 2, 62:66] = 2   # a block over the seam at column 64
    st["density"][st["flags"] != 1] = 0
    out = {}
    for x in (60, 64):
        bd = {k: T(v, dev) for k, v in st.items()}
        for cfg in (dict(PLUME_CFG, jacobiIter=7), dict(PLUME_CFG, jacobiIter=100)):
            simulate(cfg, bd, None, "jacobi", geom=tiling(x))
        torch.cuda.synchronize()
        out[x] = bd
    for k in ("p", "U", "density"):
        assert torch.equal(out[64][k], out[60][k]), f"{shape}: {k} differs between the tilings"
    assert torch.isfinite(out[64]["p"]).all() and float(out[64]["p"].abs().max()) > 0
