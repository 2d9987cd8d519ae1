"""The 3D scene kernels (fnx_scene_obstacles3d, fnx_scene_turbulence3d) on the GPU against their numpy statement
(tests/scene_reference.py): the same bits, at shapes that cross a workgroup edge in every direction (the block is 64 x 4 cells of
one plane, z comes from the grid) and at each end of every parameter's range, and independent of the batch slot."""
import numpy as np
import pytest
import torch

import scene_reference as S3
from util import assert_bitexact

pytestmark = pytest.mark.gpu

SHAPES = [(5, 6, 70), (9, 7, 33), (16, 16, 16)]                          # (D, H, W)
IDS = [1000003, 5, 2 ** 31 - 1]                                          # B = 3: neither consecutive nor ordered
SEED = 20263
# each parameter at both ends of what the entry points accept (and the sampler's own set)
PARAMS = {
    "defaults": {},
    "no_primitives": dict(n_min=0, n_max=0),
    "cap_primitives": dict(n_min=S3.MAX_PRIMITIVES, n_max=S3.MAX_PRIMITIVES, size_min=0.0, size_max=0.08),
    "point_ranges": dict(n_min=3, n_max=3, centre_min=0.1, centre_max=0.1, size_min=0.2, size_max=0.2),
    "wide_ranges": dict(n_min=1, n_max=9, centre_min=-0.6, centre_max=0.6, size_min=0.0, size_max=0.5),
    "one_octave_smallest_wavelength": dict(octaves=1, wavelength=1.0, amplitude=-3.0, density_scale=0.0),
    "cap_octaves_smallest_wavelength": dict(octaves=S3.MAX_OCTAVES, wavelength=128.0, amplitude=100.0, density_scale=-2.5),
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


def _gpu(ext, dev, ids, D, H, W, prm, seed=SEED, with_density=True):
    t = torch.tensor(ids, dtype=torch.int64).to(torch.int32).to(dev)
    flags = ext.scene_obstacles3d(t, D, H, W, seed, prm["n_min"], prm["n_max"], prm["centre_min"], prm["centre_max"], prm["size_min"],
                                  prm["size_max"])
    U, rho = ext.scene_turbulence3d(t, D, H, W, seed, prm["octaves"], prm["wavelength"], prm["amplitude"], prm["density_scale"], with_density)
    return flags.cpu().numpy(), U.cpu().numpy(), None if rho is None else rho.cpu().numpy()


@pytest.mark.parametrize("name", list(PARAMS))
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_kernels_have_the_bits_of_the_numpy_model(ext, dev, shape, name):
    D, H, W = shape
    B = len(IDS)
    prm = dict(S3.DEFAULTS[3], **PARAMS[name])
    flags, U, rho = _gpu(ext, dev, IDS, D, H, W, prm)
    assert flags.shape == (B, 1, D, H, W) and U.shape == (B, 3, D, H, W) and rho.shape == (B, 1, D, H, W)
    assert_bitexact(flags, S3.obstacles(SEED, IDS, shape, **prm), f"flags {shape} {name}")
    wantU, wantrho = S3.turbulence(SEED, IDS, shape, **prm)
    assert_bitexact(U, wantU, f"U {shape} {name}")
    assert_bitexact(rho, wantrho, f"density {shape} {name}")


def test_a_scene_does_not_depend_on_its_slot(ext, dev):
    k, (D, H, W) = 1000003, (9, 7, 33)
    prm = dict(S3.DEFAULTS[3])
    one = _gpu(ext, dev, [k], D, H, W, prm)
    five = _gpu(ext, dev, [4, 9, 2, k, 77], D, H, W, prm)
    for a, b, what in zip(one, five, ("flags", "U", "density")):
        assert_bitexact(a[0], b[3], what)
    other = _gpu(ext, dev, [k], D, H, W, prm, seed=SEED + 1)
    assert not np.array_equal(other[1], one[1])
    assert _gpu(ext, dev, [k], D, H, W, prm, with_density=False)[2] is None


def test_refusals_reach_python(ext, dev):
    t = torch.zeros(2, dtype=torch.int32, device=dev)
    d = S3.DEFAULTS[3]
    with pytest.raises(RuntimeError, match="3D only"):
        ext.scene_obstacles3d(t, 1, 16, 16, 0, 0, 4, -0.3, 0.3, 0.03, 0.12)
    with pytest.raises(RuntimeError, match="3D only"):
        ext.scene_turbulence3d(t, 3, 16, 16, 0, d["octaves"], d["wavelength"], 1.0, 1.0, True)
    with pytest.raises(RuntimeError, match="cap of"):
        ext.scene_obstacles3d(t, 8, 16, 16, 0, 0, S3.MAX_PRIMITIVES + 1, -0.3, 0.3, 0.03, 0.12)
    with pytest.raises(RuntimeError, match="at least 4 cells per axis"):
        ext.scene_obstacles3d(t, 8, 3, 16, 0, 0, 4, -0.3, 0.3, 0.03, 0.12)
    with pytest.raises(RuntimeError, match="wavelength"):
        ext.scene_turbulence3d(t, 8, 16, 16, 0, 4, 4.0, 1.0, 1.0, True)
