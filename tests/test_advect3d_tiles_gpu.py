"""The 3D z-marching advection tile kernels (fnx_advect_march.h) against one thread per cell (plan='cells'), bit for bit, on the
cases their per-plane bookkeeping has to get right: partial x / y tiles, few planes and z-chunk boundaries, batch 2, obstacles on
the tile edges, CFL just below and above 1 (the fix-up bitmaps fire), and a z-slab view (z_offset != 0).  Every plan that runs
tile kernels is covered: the fused backward march ('auto' / 'tiles'), the two separate marches ('tiles_split') and the stand-alone
density / velocity advections, each with both sample_outside_fluid settings."""
import numpy as np
import pytest
import torch

from util import make_flags

pytestmark = pytest.mark.gpu

DT = 0.13
M = "maccormackFluidNet"


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ext():
    from fluidnet_cxx_amd._ext import ext
    return ext


@pytest.fixture(scope="module")
def fl():
    from fluidnet_cxx_amd import fluid
    return fluid


def same_bits(got, want, what):
    g, w = got.detach().cpu().numpy(), want.detach().cpu().numpy()
    assert g.shape == w.shape, what
    bad = g.view(np.int32) != w.view(np.int32)
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} cells differ, first at {np.argwhere(bad)[0].tolist()}"


def state(B, D, H, W, cfl, seed):
    """Flags with obstacles on the tile edges (x = 63 / 64, rows 7 / 8, the z planes around a chunk boundary) and Empty cells; U
    uniform in +-cfl / DT per component, so a trace's length reaches sqrt(3) cfl cells: cfl 0.55 keeps every trace below one cell,
    0.62 puts a share of them above it (fix-up lanes)."""
    rng = np.random.default_rng(seed)
    f = make_flags(B, D, H, W, boxes=True, empties=True)
    z = slice(1, D - 1)
    for x in (63, 64, 127, 128):
        if x < W - 1:
            f[:, :, z, 2:H - 2:3, x] = 2
    for y in (7, 8, 15, 16):
        if y < H - 1:
            f[:, :, z, y, 5:W - 2:4] = 2
    for k in (8, 9):
        if k < D - 1:
            f[:, :, k, 3:H - 3:5, 2:W - 2:5] = 2
    U = rng.uniform(-cfl / DT, cfl / DT, (B, 3, D, H, W)).astype(np.float32)
    rho = rng.random((B, 1, D, H, W)).astype(np.float32)
    return f, U, rho


SHAPES = [  # B, D, H, W: partial x tiles (W not a multiple of 64), partial row tiles (H not a multiple of 8), 4 / 5 / 7 planes,
            # planes across a z-chunk boundary (chunks of >= 8 planes), batch 2
    (1, 4, 13, 70),
    (2, 5, 21, 130),
    (1, 7, 9, 67),
    (2, 20, 17, 129),
    (1, 26, 30, 200),
]


@pytest.mark.parametrize("cfl", [0.55, 0.62])
@pytest.mark.parametrize("shape", SHAPES)
def test_tile_plans_equal_cells(ext, fl, dev, shape, cfl):
    B, D, H, W = shape
    f, U, rho = state(B, D, H, W, cfl, seed=D * 131 + W)
    tf, tU, trho = (torch.from_numpy(a).to(dev) for a in (f, U, rho))
    uc = fl.advectVelocity(DT, tU, tU, tf, M, 1, 0.7, plan="cells")
    for so in (False, True):
        rc, uc2 = ext.advect_step(DT, trho, tU, tf, so, 0.7, None, None, None, "cells")
        same_bits(uc2, uc, f"advect_step cells vs advectVelocity cells so={so}")
        for plan in ("auto", "tiles", "tiles_split"):
            r, u = ext.advect_step(DT, trho, tU, tf, so, 0.7, None, None, None, plan)
            same_bits(r, rc, f"density so={so} plan={plan}")
            same_bits(u, uc, f"U so={so} plan={plan}")
        same_bits(fl.advectScalar(DT, trho, tU, tf, M, 1, so, 0.7, plan="tiles"), rc, f"advectScalar tiles so={so}")
    same_bits(fl.advectVelocity(DT, tU, tU, tf, M, 1, 0.7, plan="tiles"), uc, "advectVelocity tiles")


@pytest.mark.parametrize("plan", ["auto", "tiles_split"])
def test_tile_plans_equal_cells_in_a_slab(ext, dev, plan):
    """A z-slab of a deeper domain (z_offset 5 of D_global 40): the marches' global plane numbers, border planes and traced cells
    are offset; the compute window [1, D-1) is what a slab step advects."""
    B, D, H, W = 2, 14, 19, 97
    f, U, rho = state(B, D, H, W, 0.6, seed=7)
    tf, tU, trho = (torch.from_numpy(a).to(dev) for a in (f, U, rho))
    g = ext.Geom(z_offset=5, D_global=40, k_begin=1, k_end=D - 1)
    for so in (False, True):
        rc, ucl = torch.zeros_like(trho), torch.zeros_like(tU)
        ext.advect_step(DT, trho, tU, tf, so, 0.7, rc, ucl, g, "cells")
        r, u = torch.zeros_like(trho), torch.zeros_like(tU)
        ext.advect_step(DT, trho, tU, tf, so, 0.7, r, u, g, plan)
        same_bits(r, rc, f"slab density so={so}")
        same_bits(u, ucl, f"slab U so={so}")
