"""Volume rendering on the device (fluid.renderVolume -> fnx_render_volume, fnx_render.hip) against its numpy statement
(tests/render_reference.py), bit for bit: the arithmetic is fp32 add / subtract / multiply / compare in a fixed order, so no tolerance.

Inputs of every case: density uniform in [-0.2, 1.3] (both clamps act) and zeroed in half the volume, flags from emptyDomain plus a few
random obstacle boxes, absorptions of 1.5 and 2.5 per cell (min(k rho, 1) saturates from rho = 0.67 / 0.4).  A saturated cell takes T or
the light to exactly 0, after which nothing further along the ray shows in the result, so every comparison is also made with thin smoke
(0.04 and 0.03 per cell), where a ray's values stay non-zero through the whole volume unless it meets an obstacle.  The kernels' tiles are 64
rows x 64 x (x march), 256 columns per block and batches of 16 cells along the march (y / z march): the shapes below have partial and
several tiles / blocks / batches on every axis, so none is added."""
import itertools
import os
import struct
import subprocess
import sys
import zlib

import numpy as np
import pytest
import torch

import render_reference as rr

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
KV, KL = 1.5, 2.5
ABSORPTIONS = {"saturating": (KV, KL), "thin": (0.04, 0.03)}
# every view direction with a perpendicular light on each remaining axis, the headlight and the backlight
PAIRS8 = (("+x", "-y"), ("-x", "+z"), ("+y", "-x"), ("-y", "+z"), ("+z", "+x"), ("-z", "-y"), ("-x", "-x"), ("+y", "-y"))
ALL36 = tuple(itertools.product(rr.DIRECTIONS, rr.DIRECTIONS))


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def fluid():
    from fluidnet_cxx_amd import fluid
    return fluid


def T(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(dev)


def make_case(shape, seed=0):
    """(density, flags) as (B, D, H, W) numpy arrays"""
    B, D, H, W = shape
    rng = np.random.default_rng(seed)
    density = rng.uniform(-0.2, 1.3, shape).astype(f32)
    half = rng.integers(0, 2, (B, (D + 3) // 4, (H + 3) // 4, (W + 3) // 4)).astype(bool)       # zeroed in 4^3 blocks: half the volume
    density[np.repeat(np.repeat(np.repeat(half, 4, 1), 4, 2), 4, 3)[:, :D, :H, :W]] = 0
    flags = np.ones(shape, f32)
    flags[:, :, 0] = flags[:, :, -1] = flags[:, :, :, 0] = flags[:, :, :, -1] = rr.TYPE_OBSTACLE
    if D > 1:
        flags[:, 0] = flags[:, -1] = rr.TYPE_OBSTACLE
    for _ in range(4):
        z, y, x = (int(rng.integers(0, n)) for n in (D, H, W))
        dz, dy, dx = (int(rng.integers(1, max(2, n // 4))) for n in (D, H, W))
        flags[:, z:z + dz, y:y + dy, x:x + dx] = rr.TYPE_OBSTACLE
    return density, flags


_cases = {}


def case(shape, dev):
    """the inputs of a shape on the host and on the device, made once"""
    if shape not in _cases:
        d, f = make_case(shape)
        _cases[shape] = (d, f, T(d[:, None], dev), T(f[:, None], dev))
    return _cases[shape]


def device_render(fluid, dt, ft, view, light, **kw):
    kw = dict(dict(absorption=KV, light_absorption=KL), **kw)
    return fluid.renderVolume(dt, ft, view, light, **kw).cpu().numpy()


def model_render(d, f, view, light, **kw):
    kw = dict(dict(k_view=KV, k_light=KL), **kw)
    return rr.render(d, f, view, light, **kw)


def assert_same_bits(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape)
    bad = got.view(np.uint32) != want.view(np.uint32)
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} values differ, first at {tuple(np.argwhere(bad)[0])}: " \
                          f"{got[bad][0]!r} != {want[bad][0]!r}"


@pytest.mark.parametrize("shape,pairs", [((2, 5, 7, 9), ALL36), ((1, 33, 70, 65), PAIRS8), ((1, 70, 13, 130), PAIRS8),
                                         ((1, 130, 128, 192), PAIRS8), ((2, 1, 37, 53), PAIRS8)],
                         ids=["2x5x7x9-all36", "33x70x65", "70x13x130", "130x128x192", "2d-2x37x53"])
@pytest.mark.parametrize("smoke", list(ABSORPTIONS))
def test_bit_identical_to_the_model(dev, fluid, shape, pairs, smoke):
    d, f, dt, ft = case(shape, dev)
    kv, kl = ABSORPTIONS[smoke]
    sat = np.minimum(np.maximum(d, 0), 1)
    assert (d < 0).any() and (d > 1).any() and (sat * f32(KV) > 1).any() and (sat * f32(KL) < 1).any()     # the inputs do what they are for
    lit = 0
    for view, light in pairs:
        got = device_render(fluid, dt, ft, view, light, absorption=kv, light_absorption=kl)
        assert got.shape == (shape[0], 2) + rr.image_shape(shape, view)
        assert_same_bits(got, model_render(d, f, view, light, k_view=kv, k_light=kl), f"{shape} view {view} light {light} {smoke} smoke")
        lit += int((got[:, 1] > 0).sum())
    assert smoke != "thin" or lit > 0, "no ray of thin smoke got through the volume"


def _permuted_direction(direction, perm):
    old = {"z": 0, "y": 1, "x": 2}[direction[1]]
    return direction[0] + "zyx"[perm.index(old)]


@pytest.mark.parametrize("perm", [p for p in itertools.permutations(range(3)) if p != (0, 1, 2)])
def test_axis_symmetry_on_the_device(dev, fluid, perm):
    """the render of the permuted volume with the permuted directions is the permuted render: the LDS-tiled x march against the y / z
    march, in all three modes (light and view passes, and the headlight's single march)"""
    shape = (1, 20, 35, 70)
    d, f, dt, ft = case(shape, dev)
    tp = (0, 1) + tuple(p + 2 for p in perm)
    dp, fp = dt.permute(tp).contiguous(), ft.permute(tp).contiguous()
    pairs = (("+x", "+x"), ("-y", "-y"), ("-z", "-z"), ("+x", "-y"), ("-y", "+z"), ("+z", "-x"), ("-x", "+x"))
    for (view, light), (kv, kl) in itertools.product(pairs, ABSORPTIONS.values()):
        kw = dict(absorption=kv, light_absorption=kl)
        want = device_render(fluid, dt, ft, view, light, **kw)
        got = device_render(fluid, dp, fp, _permuted_direction(view, perm), _permuted_direction(light, perm), **kw)
        rest = [a for a in range(3) if "zyx"[a] != view[1]]
        new_rest = sorted(perm.index(a) for a in rest)
        order = [rest.index(perm[a]) for a in new_rest]
        assert_same_bits(got, np.ascontiguousarray(want.transpose([0, 1] + [2 + o for o in order])), f"perm {perm} view {view} light {light}")


@pytest.mark.parametrize("bnd", [0, 2])
def test_bnd_values(dev, fluid, bnd):
    for shape in ((1, 33, 70, 65), (2, 1, 37, 53)):
        d, f, dt, ft = case(shape, dev)
        for (view, light), (kv, kl) in itertools.product((("-z", "-y"), ("+x", "-z"), ("+y", "+y")), ABSORPTIONS.values()):
            assert_same_bits(device_render(fluid, dt, ft, view, light, bnd=bnd, absorption=kv, light_absorption=kl),
                             model_render(d, f, view, light, bnd=bnd, k_view=kv, k_light=kl),
                             f"bnd {bnd} {shape} view {view} light {light} k {kv} {kl}")


def test_exact_cases_on_the_device(dev, fluid):
    """what tests/test_render_host.py asks of the model, asked of the kernels"""
    # a uniform column under a headlight: T is n fp32 multiplications by (1 - a) (also on a shape of two x tiles and more than one
    # batch along z and y); C the float64 closed form to 1e-6 relative, on the shape of the host test, whose sums of 6 to 11 terms
    # the model keeps within that bound
    rho, k = f32(0.4), f32(0.3)
    a = f32(k * rho)
    for shape, closed_form in (((1, 6, 9, 11), True), ((1, 18, 21, 70), False)):
        ones = T(np.ones((1, 1) + shape[1:], f32), dev)
        dens = T(np.full((1, 1) + shape[1:], rho, f32), dev)
        for view in rr.DIRECTIONS:
            n = shape[rr._axis(view)[0]]
            img = fluid.renderVolume(dens, ones, view, view, absorption=float(k), light_absorption=float(k), ambient=0.25, bnd=0).cpu().numpy()
            Tn = f32(1)
            for _ in range(n):
                Tn = f32(Tn * f32(f32(1) - a))
            assert (img[:, 1] == Tn).all(), (shape, view)
            if closed_form:
                Ti = (1.0 - float(a)) ** np.arange(n)
                C64 = float(np.sum(Ti * float(a) * (0.25 + 0.75 * Ti)))
                assert np.abs(img[:, 0].astype(np.float64) - C64).max() <= 1e-6 * C64, (shape, view)
    # an obstacle plane: T == 0 exactly behind it, C the hand-computed expression
    shape = (1, 6, 5, 4)
    fl = np.ones(shape, f32)
    fl[:, 3] = rr.TYPE_OBSTACLE
    kv, kl, rho = f32(0.25), f32(0.5), f32(0.5)
    img = fluid.renderVolume(T(np.full((1, 1) + shape[1:], rho, f32), dev), T(fl[:, None], dev), "+z", "-y", absorption=float(kv),
                             light_absorption=float(kl), ambient=0.25, albedo_smoke=1.0, albedo_obstacle=0.5, bnd=0).cpu().numpy()
    assert (img[:, 1] == 0).all()
    amb, oma, av, al, H = f32(0.25), f32(1) - f32(0.25), f32(kv * rho), f32(kl * rho), shape[2]
    for y in range(H):
        Ls = f32(1)
        for _ in range(H - 1 - y):
            Ls = f32(Ls * f32(f32(1) - al))
        Lo = f32(1) if y == H - 1 else f32(0)
        Tv, C = f32(1), f32(0)
        for _ in range(3):
            C = f32(C + f32(f32(Tv * av) * f32(f32(1) * f32(amb + f32(oma * Ls)))))
            Tv = f32(Tv * f32(f32(1) - av))
        C = f32(C + f32(Tv * f32(f32(0.5) * f32(amb + f32(oma * Lo)))))
        assert (img[0, 0, y] == C).all(), y
    # nothing there: C == 0 and T == 1 exactly; emptyDomain's wall is invisible with bnd = 1 and opaque with bnd = 0
    shape = (1, 6, 7, 8)
    flags = torch.zeros((1, 1) + shape[1:], device=dev)
    fluid.emptyDomain(flags)
    zero = torch.zeros_like(flags)
    for view, light in (("-z", "-y"), ("+x", "+x"), ("-y", "+y"), ("-x", "+z"), ("+y", "-x"), ("+z", "-z")):
        img = fluid.renderVolume(zero, torch.ones_like(flags), view, light, bnd=0).cpu().numpy()
        assert (img[:, 0] == 0).all() and (img[:, 1] == 1).all(), view
        seen = fluid.renderVolume(zero, flags, view, light, bnd=1).cpu().numpy()
        assert (seen[:, 0] == 0).all() and (seen[:, 1] == 1).all(), view
        wall = fluid.renderVolume(zero, flags, view, light, bnd=0).cpu().numpy()
        assert (wall[:, 1] == 0).all() and (wall[:, 0] > 0).all(), view


def test_inputs_untouched_repeatable_and_capturable(dev, fluid):
    shape = (1, 33, 70, 65)
    d, f, dt, ft = case(shape, dev)
    for view, light in (("-z", "-y"), ("+x", "-y"), ("-x", "-x")):
        first = device_render(fluid, dt, ft, view, light)
        again = device_render(fluid, dt, ft, view, light)
        assert_same_bits(again, first, f"second call, view {view} light {light}")
        assert_same_bits(dt.cpu().numpy()[:, 0], d, "density after the calls")
        assert_same_bits(ft.cpu().numpy()[:, 0], f, "flags after the calls")
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            out = fluid.renderVolume(dt, ft, view, light, absorption=KV, light_absorption=KL)
        out.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert_same_bits(out.cpu().numpy(), first, f"graph replay, view {view} light {light}")


def test_python_surface(dev, fluid):
    shape = (1, 12, 20, 28)
    d, f, dt, ft = case(shape, dev)
    # defaults: view -z, light -y, absorption 16 / cells along the axis, ambient 0.25, albedos 1 and 0.5, bnd 1
    assert_same_bits(fluid.renderVolume(dt, ft).cpu().numpy(), rr.render(d, f), "defaults")
    assert_same_bits(fluid.renderVolume(dt, ft, "+x", "+z").cpu().numpy(),
                     rr.render(d, f, "+x", "+z", k_view=f32(16.0 / 28), k_light=f32(16.0 / 12)), "default absorptions")
    assert_same_bits(fluid.renderVolume(dt, ft, ambient=0.1, albedo_smoke=0.8, albedo_obstacle=0.3).cpu().numpy(),
                     rr.render(d, f, ambient=0.1, albedo_smoke=0.8, albedo_obstacle=0.3), "keywords")
    with pytest.raises(AssertionError, match="Dimension mismatch"):
        fluid.renderVolume(dt[0], ft[0])
    with pytest.raises(AssertionError, match="size mismatch"):
        fluid.renderVolume(dt[:, :, 1:].contiguous(), ft)
    with pytest.raises(AssertionError, match="not contiguous"):
        fluid.renderVolume(dt.transpose(3, 4), ft.transpose(3, 4))
    with pytest.raises(AssertionError, match="on the GPU"):
        fluid.renderVolume(dt.cpu(), ft.cpu())
    with pytest.raises(AssertionError, match="float32"):
        fluid.renderVolume(dt.double(), ft.double())
    with pytest.raises(AssertionError, match="view / light"):
        fluid.renderVolume(dt, ft, "z", "-y")
    with pytest.raises(RuntimeError, match="finite and not negative"):
        fluid.renderVolume(dt, ft, absorption=-1.0)


def _png_pixels(fname):
    raw = open(fname, "rb").read()
    assert raw[:8] == b"\x89PNG\r\n\x1a\n"
    pos, chunks = 8, {}
    while pos < len(raw):
        n = struct.unpack(">I", raw[pos:pos + 4])[0]
        tag, payload = raw[pos + 4:pos + 8], raw[pos + 8:pos + 8 + n]
        assert struct.unpack(">I", raw[pos + 8 + n:pos + 12 + n])[0] == zlib.crc32(tag + payload) & 0xFFFFFFFF
        chunks[tag] = payload
        pos += 12 + n
    w, h, depth, colour = struct.unpack(">IIBBBBB", chunks[b"IHDR"])[:4]
    assert (depth, colour) == (8, 2)
    px = np.frombuffer(zlib.decompress(chunks[b"IDAT"]), np.uint8).reshape(h, 1 + w * 3)
    assert (px[:, 0] == 0).all()
    return px[:, 1:].reshape(h, w, 3)


def test_output_functions(dev, fluid, tmp_path):
    from fluidnet_cxx_amd import output
    from util import plume_state
    shape = (1, 12, 20, 28)
    d, f, dt, ft = case(shape, dev)
    bd = dict(density=dt, flags=ft)
    img = output.render_image(bd, "+x", "-y", background=0.5)
    assert img.shape == (12, 20, 3) and img.dtype == np.uint8
    m = rr.render(d, f, "+x", "-y")[0]
    grey = (np.clip(m[0] + m[1] * f32(0.5), 0, 1) * 255.0 + 0.5).astype(np.uint8)
    assert np.array_equal(img, np.repeat(grey[::-1, :, None], 3, 2))
    views = (("-z", "-y"), ("+x", "-y"), ("-y", "-y"))
    files = output.save_render(str(tmp_path), 7, bd, views)
    assert [os.path.basename(n) for n in files] == ["render_-z_00007.png", "render_+x_00007.png", "render_-y_00007.png"]
    for (view, light), name in zip(views, files):
        px = _png_pixels(name)
        assert px.shape == rr.image_shape(shape, view) + (3,)
        assert np.array_equal(px, output.render_image(bd, view, light))
    assert [os.path.basename(n) for n in output.save_render(str(tmp_path), 8, bd)] == ["render_-z_00008.png"]
    # save_state: without render= the list it always returned; with it, the renders between the VTK file and the restart file
    st = {k: T(v, dev) for k, v in plume_state(16).items()}
    a, b = tmp_path / "a", tmp_path / "b"
    a.mkdir(); b.mkdir()
    plain = output.save_state(str(a), 3, st)
    assert [os.path.basename(n) for n in plain] == ["output_00003.png", "output_00003.vtr", "restart.pth"]
    assert sorted(os.listdir(a)) == ["output_00003.png", "output_00003.vtr", "restart.pth"]
    with_r = output.save_state(str(b), 3, st, render=(("-z", "-y"),))
    assert [os.path.basename(n) for n in with_r] == ["output_00003.png", "output_00003.vtr", "render_-z_00003.png", "restart.pth"]
    assert _png_pixels(with_r[2]).shape == (16, 16, 3)                       # a 2D state renders too


def test_driver(dev, tmp_path):
    """examples/plume.py --depth 24 --render: two renders per output event, not uniform (the inlet's density is there from the first
    step), a restart file that reloads; without --depth and --render the file list of the 2D driver"""
    from fluidnet_cxx_amd import load_restart
    out3, out2 = tmp_path / "d3", tmp_path / "d2"
    common = [sys.executable, os.path.join(REPO, "examples", "plume.py"), "--res", "32", "--iters", "4", "--out-iter", "2", "--method", "jacobi"]
    r = subprocess.run(common + ["--depth", "24", "--render", "--folder", str(out3)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    want = ["plumeConfig.yaml", "restart.pth"]
    for it in (0, 2):
        want += [f"output_{it:05}.png", f"output_{it:05}.vtr", f"render_-z_{it:05}.png", f"render_+x_{it:05}.png"]
    assert sorted(os.listdir(out3)) == sorted(want)
    for it in (0, 2):
        front, side = _png_pixels(str(out3 / f"render_-z_{it:05}.png")), _png_pixels(str(out3 / f"render_+x_{it:05}.png"))
        assert front.shape == (32, 32, 3) and side.shape == (24, 32, 3)
        assert front.min() < front.max() and side.min() < side.max(), "a uniform render"
    bd, it = load_restart(str(out3 / "restart.pth"), dev)
    assert it == 2 and tuple(bd["density"].shape) == (1, 1, 24, 32, 32) and tuple(bd["U"].shape) == (1, 3, 24, 32, 32)
    assert float(bd["density"].max()) > 0
    r = subprocess.run(common + ["--folder", str(out2)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert sorted(os.listdir(out2)) == sorted(["plumeConfig.yaml", "restart.pth", "output_00000.png", "output_00000.vtr",
                                              "output_00002.png", "output_00002.vtr"])
