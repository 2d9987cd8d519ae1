"""The scene kernels (fnx_scene_obstacles, fnx_scene_turbulence) on the GPU against their numpy statement (tests/scene_reference.py):
the same bits, at every shape and at each end of every parameter's range, and independent of the batch slot."""
import numpy as np
import pytest
import torch

import scene_reference as SR
from util import assert_bitexact

pytestmark = pytest.mark.gpu

SHAPES = [(1, 64, 64), (5, 37, 53), (3, 128, 96)]                       # (B, H, W)
IDS = {1: [7], 5: [0, 3, 1000003, 12, 2 ** 31 - 1], 3: [41, 5, 90000]}   # non-consecutive scene ids
SEED = 20240
# each parameter at both ends of what the entry points accept (and the sampler's own set)
PARAMS = {
    "defaults": {},
    "no_primitives": dict(n_min=0, n_max=0),
    "cap_primitives": dict(n_min=SR.MAX_PRIMITIVES, n_max=SR.MAX_PRIMITIVES, size_min=0.0, size_max=0.05),
    "point_ranges": dict(n_min=3, n_max=3, centre_min=0.1, centre_max=0.1, size_min=0.2, size_max=0.2),
    "wide_ranges": dict(n_min=1, n_max=9, centre_min=-0.6, centre_max=0.6, size_min=0.0, size_max=0.5),
    "one_octave": dict(octaves=1, wavelength=1.0, amplitude=-3.0, density_scale=0.0),
    "eight_octaves": dict(octaves=SR.MAX_OCTAVES, wavelength=128.0, amplitude=100.0, density_scale=-2.5),
    "odd_wavelength": dict(octaves=3, wavelength=11.3, amplitude=0.0, density_scale=7.0),
}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ext():
    from fluidnet_cxx_amd._ext import ext
    return ext


def _gpu(ext, dev, ids, H, W, prm, seed=SEED, with_density=True):
    t = torch.tensor(ids, dtype=torch.int64).to(torch.int32).to(dev)
    flags = ext.scene_obstacles(t, H, W, seed, prm["n_min"], prm["n_max"], prm["centre_min"], prm["centre_max"], prm["size_min"], prm["size_max"])
    U, rho = ext.scene_turbulence(t, H, W, seed, prm["octaves"], prm["wavelength"], prm["amplitude"], prm["density_scale"], with_density)
    return flags.cpu().numpy(), U.cpu().numpy(), None if rho is None else rho.cpu().numpy()


@pytest.mark.parametrize("name", list(PARAMS))
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_kernels_have_the_bits_of_the_numpy_model(ext, dev, shape, name):
    B, H, W = shape
    prm = dict(SR.DEFAULTS[2], **PARAMS[name])
    flags, U, rho = _gpu(ext, dev, IDS[B], H, W, prm)
    assert flags.shape == (B, 1, 1, H, W) and U.shape == (B, 2, 1, H, W) and rho.shape == (B, 1, 1, H, W)
    assert_bitexact(flags, SR.obstacles(SEED, IDS[B], (H, W), **prm), f"flags {shape} {name}")
    wantU, wantrho = SR.turbulence(SEED, IDS[B], (H, W), **prm)
    assert_bitexact(U, wantU, f"U {shape} {name}")
    assert_bitexact(rho, wantrho, f"density {shape} {name}")


def test_a_scene_does_not_depend_on_its_slot(ext, dev):
    k, (H, W) = 1000003, (37, 53)
    prm = dict(SR.DEFAULTS[2])
    one = _gpu(ext, dev, [k], H, W, prm)
    five = _gpu(ext, dev, [4, 9, 2, k, 77], H, W, prm)
    for a, b, what in zip(one, five, ("flags", "U", "density")):
        assert_bitexact(a[0], b[3], what)
    other = _gpu(ext, dev, [k], H, W, prm, seed=SEED + 1)
    assert not np.array_equal(other[1], one[1])
    assert _gpu(ext, dev, [k], H, W, prm, with_density=False)[2] is None


def test_refusals_reach_python(ext, dev):
    t = torch.zeros(2, dtype=torch.int32, device=dev)
    d = SR.DEFAULTS[2]
    with pytest.raises(RuntimeError, match="2D only"):
        ext.scene_obstacles(t, 16, 16, 0, 0, 4, -0.3, 0.3, 0.03, 0.12, depth=8)
    with pytest.raises(RuntimeError, match="2D only"):
        ext.scene_turbulence(t, 16, 16, 0, d["octaves"], d["wavelength"], 1.0, 1.0, True, depth=8)
    with pytest.raises(RuntimeError, match="cap of"):
        ext.scene_obstacles(t, 16, 16, 0, 0, SR.MAX_PRIMITIVES + 1, -0.3, 0.3, 0.03, 0.12)
    with pytest.raises(RuntimeError, match="at least 4 cells"):
        ext.scene_obstacles(t, 3, 16, 0, 0, 4, -0.3, 0.3, 0.03, 0.12)
