"""The HIP MultiScale net in every precision mode against the float64 model of the reference net (tests/cnn_reference.py), on
weights under which every layer shows in the output (propagating_weights: He-uniform scaling of the benchmark's hashed weights).

The shapes come from the launchers' own thresholds (fluidnet_cxx_amd/csrc/fnx_cnn.hip, fnx_cnn_wino4.h, fnx_cnn_bf16x6.h; 256 CUs),
so that between them every conv kernel instantiation the launchers can choose runs at least once, in 2D and in 3D.  Each case
names what it is there for; per layer, the choice is
  bf16x6 / bf16x3, 64/128-output-channel 3x3 layers: conv3_wbf_kernel<IS3D, 6 / 3>   if ceil(W/32) ceil(H/8) B D Cout/64 >= 512
  fp32, the same layers:                conv3_wino4_kernel<IS3D, W % 4 == 0>        if ceil(W/32) ceil(H/16) B D Cout/64 >= #CUs
  fp32 / fp32_f2 / bf16, 3x3 MFMA layers: conv3_wino3_kernel<2,2> (Cout 64/128)    if ceil(W/32) ceil(H/8) B D Cout/64 >= 512,
                                        conv3_wino3_kernel<1,2> (Cout 32)           if ceil(W/32) ceil(H/8) B D >= 1024
  otherwise (and everything in fp32_direct): conv3_mfma_kernel<CB = Cout % 64 ? 1 : 2, PR>, PR = 4 / 2 / 1 where
                                        ceil(W/32) ceil(H/16 / 8) B D Cout/(32 CB) >= 512 / else
  2->32 3x3: conv_direct_kernel; 32->1 3x3: conv3_to1_kernel; 5x5 3->32: conv5_mfma16_kernel KPACK; 5x5 32->8 + 1x1: PAIR.
conv3_wino3_kernel<2,1> is unreachable: it would need ceil(W/32) ceil(H/4) X >= 1024 with ceil(W/32) ceil(H/8) X < 512, and
ceil(H/4) <= 2 ceil(H/8).  Each float64 reference is computed once per shape (on the CPU) and shared by the modes.

Measured (fraction of |ref|max; the error is spread evenly over tile positions, boundary planes and batch entries): fp32 (F(4x4))
2.5e-6 (2D) .. 4.8e-6 (3D), 2x under its 1e-5; fp32_f2, fp32_direct and bf16x6 0.8e-6 .. 2.5e-6, 4x under; bf16x3 8.0e-5 .. 9.2e-5,
within its 1e-4 by 8 % -- under the benchmark's weights that mode measures 2-3e-5, so these are the cases that pin it."""
import numpy as np
import pytest
import torch

from cnn_reference import multiscale_fp64, net_input, propagating_weights
from util import assert_close_rel, random_state

pytestmark = pytest.mark.gpu

RTOL = {"fp32": 1e-5, "fp32_f2": 1e-5, "fp32_direct": 1e-5, "bf16x6": 1e-5, "bf16x3": 1e-4}
MODES = list(RTOL)

# (B, D, H, W): D == 1 is the 2D net.  What each shape adds to the coverage (resolutions: full, half = int(0.5 n), quarter = int(0.25 n)).
SHAPES = {
    (2, 1, 255, 508): "2D: wino4<2D, v16> at full resolution (W % 4 == 0), wino4<2D, !v16> at half (127x254, the 64->128 layer), "
                      "wino3<2,2> and <1,2> (fp32_f2), wbf<2D, 6 / 3>, fp32_direct: mfma CB1 / CB2 PR4 (full), CB2 PR2 (half)",
    (3, 1, 199, 215): "2D: mfma<CB1, PR2> for the 64->32 layer at full resolution in every mode (below wino3<1,2>'s 1024 tiles), "
                      "partial tiles in x and y, odd sizes, B = 3",
    (2, 1, 37, 53): "2D, small and odd: every 3x3 MFMA layer on mfma PR1; conv_direct, conv3_to1, conv5_mfma16 PAIR / KPACK",
    (3, 11, 70, 100): "3D: wino4<3D, v16>, wino3<2,2> (fp32_f2) and <1,2>, wbf<3D, 6 / 3>, fp32_direct: mfma CB1 / CB2 PR4; D = 11",
    (1, 19, 66, 90): "3D: wino4<3D, !v16> (W % 4 == 2), mfma<CB1, PR2> in every mode, fp32_direct: mfma CB2 PR2; D = 19",
    (2, 4, 13, 18): "3D, the minimum 4 planes (one quarter-resolution plane), B = 2: mfma PR1, conv_direct, conv3_to1, PAIR / KPACK",
    (1, 9, 14, 22): "3D, no axis a multiple of 4: mfma PR1, conv_direct, conv3_to1, PAIR / KPACK",
}


def _id(s):
    return "x".join(str(v) for v in s)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def reference():
    """(shape) -> (weights, x, float64 p), computed once per shape."""
    cache = {}

    def get(shape):
        if shape not in cache:
            B, D, H, W = shape
            nd = 3 if D > 1 else 2
            w = propagating_weights(nd)
            x = net_input(B, D, H, W, seed=sum(shape))
            cache[shape] = (w, x, multiscale_fp64(w, x, nd))
        return cache[shape]
    return get


def _mconf(is3d, mode):
    return dict(model="ScaleNet", inputChannels=dict(div=True, pDiv=False, UDiv=False), normalizeInput=True,
                normalizeInputChan="UDiv", normalizeInputThreshold=1e-5, is3D=is3d, precisionMode=mode)


def _net(w, is3d, mode, dev):
    from fluidnet_cxx_amd import FluidNet
    return FluidNet.from_weights(_mconf(is3d, mode), w, dev)


def _forward(net, x, dev):
    is3d = x.shape[2] > 1
    t = torch.from_numpy(np.ascontiguousarray(x if is3d else x[:, :, 0])).to(dev)
    p = net.multiScale(t)
    return p.cpu().numpy().reshape(x.shape[0], 1, *x.shape[2:])


def _rel(got, want):
    return float(np.abs(got.astype(np.float64) - want).max() / np.abs(want).max())


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("shape", list(SHAPES), ids=_id)
def test_multiscale_vs_fp64(dev, reference, shape, mode):
    w, x, want = reference(shape)
    got = _forward(_net(w, shape[1] > 1, mode, dev), x, dev)
    print(f"\nCNN_ERR {_id(shape)} {mode} {_rel(got, want):.3e}")
    assert_close_rel(got, want, RTOL[mode], f"MultiScaleNet {_id(shape)} ({mode}; {SHAPES[shape]})")


@pytest.mark.parametrize("shape", [(2, 1, 45, 70), (2, 7, 22, 30)], ids=_id)
def test_fluidnet_forward_vs_fp64(dev, oracle, shape):
    """FluidNet.forward (the std normalisation, the net, the unscaling, the velocity update and the wall conditions) against the
    oracle's stages around the float64 net (oracle.fluidnet_forward's net hook)."""
    B, D, H, W = shape
    is3d = D > 1
    nd = 3 if is3d else 2
    w = propagating_weights(nd)
    s = random_state(B, D, H, W, 0.5, seed=13)
    inp = np.concatenate([np.zeros_like(s["p"]), s["U"], s["flags"], s["rho"]], 1)
    po, Uo = oracle.fluidnet_forward(oracle.pack_weights(w, nd), inp, 1e-5, net=lambda x: multiscale_fp64(w, x, nd))
    p, U = _net(w, is3d, "fp32", dev)(torch.from_numpy(inp).to(dev))
    p, U = p.cpu().numpy(), U.cpu().numpy()
    print(f"\nCNN_ERR fluidnet {_id(shape)} p {_rel(p, po):.3e} U {_rel(U, Uo):.3e}")
    assert_close_rel(p, po, 1e-5, "FluidNet p"); assert_close_rel(U, Uo, 1e-5, "FluidNet U")


@pytest.fixture(scope="module")
def slab_reference():
    w = propagating_weights(3)
    x = net_input(2, 104, 13, 18, seed=21)
    return w, x, multiscale_fp64(w, x, 3)


@pytest.mark.parametrize("case,mode", [("bottom", "fp32"), ("middle", "fp32"), ("top", "fp32"), ("middle", "bf16x6")])
def test_nested_crops_vs_fp64(dev, slab_reference, case, mode):
    """net.multiScale(x, trim) (fnx_multiscale_forward_crop) on a z-slab rank's window -- quarter-resolution tower on owned +- NET_MARGIN
    planes, half- / full-resolution towers on owned +- NET_MARGIN_HALF / _FULL, untrimmed at a domain face -- against the float64
    forward over the whole 104-plane domain, on the 8 owned planes; B = 2."""
    from fluidnet_cxx_amd.slab import SlabSimulator as S
    G, MF, MH = S.NET_MARGIN, S.NET_MARGIN_FULL, S.NET_MARGIN_HALF
    w, x, full = slab_reference
    Dg = x.shape[2]
    own = dict(bottom=(0, 8), middle=(48, 56), top=(96, 104))[case]
    e0, e1 = max(own[0] - G, 0), min(own[1] + G, Dg)
    cut_lo, cut_hi = own[0] - e0 == G, e1 - own[1] == G
    trim = [G - MF if cut_lo else 0, G - MF if cut_hi else 0, G - MH if cut_lo else 0, G - MH if cut_hi else 0]
    net = _net(w, True, mode, dev)
    got = net.multiScale(torch.from_numpy(np.ascontiguousarray(x[:, :, e0:e1])).to(dev), trim).cpu().numpy()
    lo = e0 + trim[0]
    got, want = got[:, :, own[0] - lo:own[1] - lo], full[:, :, own[0]:own[1]]
    print(f"\nCNN_ERR crop {case} {mode} {_rel(got, want):.3e}")
    assert_close_rel(got, want, RTOL[mode], f"nested crops ({case}, {mode}): owned planes vs the float64 whole domain")
