"""The 3D two-sweep Jacobi march keeps the mask registers of a plane whose mask equals the plane below over the wave's whole
footprint (one "same" bit per sample, tile and plane, built with the mask; fnx_jacobi.hip) instead of loading them again.  The
solve keeps the bits of the CPU oracle: obstacles that differ from plane to plane and sit on the seams of the 60-column x 4-row
tiles (a wave loads columns bx*60-2 .. bx*60+61 and rows j0-1 .. j0+4, so columns 58-62 and rows 3/4/5 belong to two or three
footprints), obstacles extruded in z (every interior bit set), an empty box, 1 to 7 sweeps and 100, H % 4 != 0 (row layout),
plane ranges and two ranges per launch, B = 2, and flags edited between two solves without the static promise."""
import numpy as np
import pytest
import torch

from util import assert_bitexact, make_flags

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def fl():
    from fluidnet_cxx_amd import fluid
    return fluid


@pytest.fixture(scope="module")
def ext():
    from fluidnet_cxx_amd._ext import ext
    return ext


def T(x, dev):
    return torch.from_numpy(np.ascontiguousarray(x)).to(dev)


def N(t):
    return t.detach().cpu().numpy()


def seam_flags(B, D, H, W, kind):
    """kind 'empty': walls only; 'extruded': obstacles through every interior plane; 'planes': obstacles that differ from plane
    to plane.  Obstacles sit on tile seams: columns 58-62 (and 118-122 where the grid has them), rows 3, 4, 5."""
    f = make_flags(B, D, H, W, boxes=False)
    if kind == "empty":
        return f
    cols = [c for c in (58, 59, 60, 61, 62, 118, 119, 120, 121, 122) if c < W - 1]
    rows = [r for r in (3, 4, 5) if r < H - 1]
    if kind == "extruded":
        for n, c in enumerate(cols):
            f[:, :, 1:D - 1, rows[n % len(rows)], c] = 2
        if H > 9:
            f[:, :, 1:D - 1, 7:9, 2:4] = 2
        return f
    rng = np.random.default_rng(5)
    for b in range(B):
        for k in range(1, D - 1):
            if k % 5 == 4:                     # every fifth plane repeats the one below: set and cleared bits alternate
                f[b, :, k] = f[b, :, k - 1]
                continue
            for c in rng.choice(cols, size=min(3, len(cols)), replace=False):
                f[b, 0, k, rng.choice(rows), c] = 2
            if k % 3 == 0 and H > 9:
                f[b, 0, k, 8, (5 * k) % (W - 2) + 1] = 2
    return f


@pytest.mark.parametrize("kind", ["planes", "extruded", "empty"])
@pytest.mark.parametrize("shape", [(1, 12, 12, 70), (2, 9, 16, 130), (1, 40, 10, 64), (1, 70, 8, 63)])
def test_solve_bits_of_the_oracle(dev, fl, oracle, kind, shape):
    """1 to 7 sweeps and 100 (H % 4 == 0: the passes hand each other p in the row-quad layout; 10: in rows; D = 40 and 70: bits from
    two and three 32-plane words).  Grids this small are cut into chunks of a few planes; test_segment_longer_than_its_bits has the
    long segments."""
    B, D, H, W = shape
    flags = seam_flags(B, D, H, W, kind)
    rng = np.random.default_rng(D + W)
    div = rng.standard_normal((B, 1, D, H, W)).astype(np.float32)
    tf, td = T(flags, dev), T(div, dev)
    for n in (1, 2, 3, 4, 5, 6, 7, 100):
        pg, _ = fl.solveLinearSystemJacobi(tf, td, True, 0.0, n)
        po, _, _ = oracle.jacobi(flags, div, True, 0.0, n)
        assert_bitexact(N(pg), po, f"{kind} {shape}: {n} sweeps")


@pytest.mark.parametrize("kind", ["planes", "extruded"])
@pytest.mark.parametrize("shape", [(1, 40, 12, 70), (2, 40, 10, 130)])
def test_plane_ranges_and_two_ranges_per_launch(dev, ext, oracle, kind, shape):
    """fnx_jacobi_pass on a plane range and fnx_jacobi_pass2 on two: each range's planes are the oracle's two sweeps of the full
    field there (ranges that start and end at any phase of the 32-plane words), the other planes stay untouched."""
    B, D, H, W = shape
    flags = seam_flags(B, D, H, W, kind)
    rng = np.random.default_rng(17)
    div = rng.standard_normal((B, 1, D, H, W)).astype(np.float32)
    p = rng.standard_normal((B, 1, D, H, W)).astype(np.float32)
    tf, td, tp = T(flags, dev), T(div, dev), T(p, dev)
    ws = torch.empty(ext.jacobi_workspace_bytes(B, D, H, W, True), dtype=torch.uint8, device=dev)
    first = True
    for n in (2, 1):
        full = oracle.jacobi_sweeps(flags, div, p, True, n)
        for (a, b, a2) in ((3, 17, -1), (0, 40, -1), (30, 36, -1), (31, 34, -1), (1, 2, -1), (2, 8, 30), (0, 5, 35), (3, 17, 20)):
            out = torch.full((B, 1, D, H, W), 7.0, device=dev)
            ext.jacobi_pass_(tf, td, tp, out, n, a, b, ws, not first, a2); first = False
            want = np.full((B, 1, D, H, W), 7.0, np.float32)
            want[:, :, a:b] = full[:, :, a:b]
            if a2 >= 0:
                want[:, :, a2:a2 + b - a] = full[:, :, a2:a2 + b - a]
            assert_bitexact(N(out), want, f"{kind} {shape}: n={n} planes [{a},{b}) + {a2}")


def test_segment_longer_than_its_bits(dev, fl, oracle):
    """704 x 700 x 67: 12 x 175 = 2100 tiles, more than half the 4096 wave slots of a 256-CU device, so every tile is ONE chunk of 67
    planes: longer than the 64 planes the two words of bits read at segment start cover; the planes past them load their mask (the
    `sq < 64` guard).  Obstacles extruded in z (every bit set up to there), with more obstacles from plane 65 on."""
    B, D, H, W = 1, 67, 700, 704
    flags = seam_flags(B, D, H, W, "extruded")
    flags[0, 0, 65:D - 1, 4, 61] = 2; flags[0, 0, 65:D - 1, 300, 359:362] = 2
    rng = np.random.default_rng(41)
    div = rng.standard_normal((B, 1, D, H, W)).astype(np.float32)
    tf, td = T(flags, dev), T(div, dev)
    for n in (2, 5):
        pg, _ = fl.solveLinearSystemJacobi(tf, td, True, 0.0, n)
        po, _, _ = oracle.jacobi(flags, div, True, 0.0, n)
        assert_bitexact(N(pg), po, f"{D}x{H}x{W}: {n} sweeps")


def test_flags_edited_between_two_solves(dev, fl, ext, oracle):
    """No static promise: the second solve sees the edited flags (an obstacle added in one plane clears that plane's bit and the
    next one's; one removed sets them), through the operator and through fnx_jacobi_pass with reuse_mask = False."""
    B, D, H, W = 2, 14, 12, 70
    rng = np.random.default_rng(23)
    div = rng.standard_normal((B, 1, D, H, W)).astype(np.float32)
    td = T(div, dev)
    f0 = seam_flags(B, D, H, W, "extruded")
    f1 = f0.copy(); f1[0, 0, 6, 4, 60] = 2; f1[1, 0, 9, 3, 59] = 1; f1[1, 0, 3, 5, 61] = 2
    f2 = seam_flags(B, D, H, W, "empty")
    tf = T(f0, dev)
    ws = torch.empty(ext.jacobi_workspace_bytes(B, D, H, W, True), dtype=torch.uint8, device=dev)
    for f in (f0, f1, f2, f0):
        tf.copy_(T(f, dev))                    # the same tensor, edited in place
        for n in (6, 7):
            pg, _ = fl.solveLinearSystemJacobi(tf, td, True, 0.0, n)
            po, _, _ = oracle.jacobi(f, div, True, 0.0, n)
            assert_bitexact(N(pg), po, f"operator, {n} sweeps after an edit")
        out = torch.empty(B, 1, D, H, W, device=dev)
        ext.jacobi_pass_(tf, td, None, out, 2, 0, 0, ws, False)
        assert_bitexact(N(out), oracle.jacobi_sweeps(f, div, np.zeros_like(div), True, 2), "pass, mask rebuilt after an edit")
