"""A float64 torch model of the Conv3d bank net (mconf['model'] = 'FluidNet3D'), written from the statement of the net and sharing no
code with the kernels.  The reference has no 3D form of this net (its lib/model.py asserts 2D), so this model is the yardstick:

    x  = [div / s, occupancy]                             (B,2,D,H,W)
    a  = relu(conv1(x))                                   Conv3d 2 -> 16, 3x3x3, zero padding 1
    a2 = avgpool3d(a, 2); a4 = avgpool3d(a, 4)
    bank(t) = relu(cB2(relu(cB0(t))))                     Conv3d 16 -> 16 -> 16, 3x3x3, zero padding 1 at that level's border, one set of weights
    t  = (bank(a) + up2(bank(a2))) + up4(bank(a4))        nearest in z, y and x
    t  = relu(conv2(t)); t = relu(conv2(t)); t = relu(conv3(t)); p = convOut(t)       1x1x1

`drop` leaves one level (0: full, 1: half, 2: quarter resolution) out of the sum: the host tests use it to show that every level
reaches the output under the weights the tests use.  propagating_bank3d_weights are those weights; with default-scale weights the
output is its bias to within 1.6 %, which would hide almost any error of the kernels.

SHAPES3D (B, D, H, W) and the launch plan of fnx_banknet3d.hip (conv1: 4 x 8 x 64-cell workgroups; the 16 -> 16 convolution: 4 x 30-cell
tiles of (y, x), z split into chunks of at least four planes while fewer than 4096 workgroups are in flight):
  (1,4,4,4)      the quarter level is one cell (all padding), the half level 2^3; every tile is partial
  (2,8,12,20)    a batch, non-cubic; full resolution: three y tiles, two z chunks of four planes; conv1: two y tiles (8 + 4 rows)
  (1,12,20,36)   D/4 = 3; full resolution: two x tiles (30 + 6 columns), five y tiles, three z chunks; an obstacle box
  (2,4,36,68)    D/4 = 1 (the quarter level has one plane, the half level two); three x tiles (30 + 30 + 8); conv1: two x tiles (64 + 4)
  (1,20,12,132)  long rows: five x tiles at full resolution, three at the half level (66 = 30 + 30 + 6), two at the quarter level
                 (33 = 30 + 3); five z chunks; conv1: three x tiles (64 + 64 + 4)
tests/test_banknet3d_host.py checks on the plan itself that tiles and chunks cover every one of these grids (and larger ones) once.
"""
import numpy as np

from banknet_reference import banknet_forward64, propagating_bank_weights
from fluidnet_cxx_amd.weights import hash_uniform

SHAPES3D = [(1, 4, 4, 4), (2, 8, 12, 20), (1, 12, 20, 36), (2, 4, 36, 68), (1, 20, 12, 132)]     # (B, D, H, W)


def propagating_bank3d_weights(seed=0):
    return propagating_bank_weights(seed, ndim=3)


def bank3d_input(B, D, H, W, boxes=True, seed=0):
    """x (B,2,D,H,W) float32 = [a normalised-divergence-like field in [-1, 1), occupancy]: a wall shell of one cell and, with `boxes` on
    a grid of at least 8 cells a side, an obstacle box inside; the first channel is zero in occupied cells, as the divergence is."""
    x = np.zeros((B, 2, D, H, W), np.float32)
    x[:, 0] = hash_uniform(B * D * H * W, 2100 + seed).reshape(B, D, H, W)
    occ = np.zeros((D, H, W), np.float32)
    occ[0] = occ[-1] = 1
    occ[:, 0] = occ[:, -1] = 1
    occ[:, :, 0] = occ[:, :, -1] = 1
    if boxes and min(D, H, W) >= 8:
        occ[D // 4:D // 4 + 2, H // 4:H // 4 + 3, W // 3:W // 3 + 5] = 1
    x[:, 1] = occ
    x[:, 0] *= 1 - occ
    return x


def banknet3d_forward64(weights, x, drop=None):
    """p (B,1,D,H,W) float64 of the net above for x (B,2,D,H,W): banknet_reference's one statement of the net, on five dimensions"""
    assert np.ndim(x) == 5
    return banknet_forward64(weights, x, drop)
