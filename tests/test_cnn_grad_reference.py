"""The differentiable float64 model (tests/cnn_grad_reference.py) is the yardstick of the native backward pass, so it is pinned here,
on the CPU: its forward is the float64 forward model's, imposing its own ReLU decisions changes nothing, its gradient agrees with a
central difference, and the test weights leave no dead entries in any gradient tensor."""
import numpy as np
import pytest
import torch

import cnn_grad_reference as G
from cnn_reference import multiscale_fp64, net_input, propagating_weights

SHAPES = [(2, 37, 53), (1, 48, 64)]


def _case(shape):
    B, H, W = shape
    w = propagating_weights(2)
    x = net_input(B, 1, H, W, seed=sum(shape))[:, :, 0]
    gp = np.random.default_rng(5).standard_normal((B, 1, H, W))
    return w, x, gp


@pytest.mark.parametrize("shape", SHAPES)
def test_forward_is_the_fp64_forward_model(shape):
    w, x, _ = _case(shape)
    with torch.no_grad():
        p = G.forward(G.as_params(w, requires_grad=False), torch.from_numpy(x.astype(np.float64))).numpy()
    assert np.array_equal(p, multiscale_fp64(w, x, 2))


@pytest.mark.parametrize("shape", SHAPES)
def test_own_masks_imposed_change_nothing(shape):
    w, x, gp = _case(shape)
    free, p0, own = G.gradients(w, x, gp)
    masked, p1, _ = G.gradients(w, x, gp, masks=own)
    assert (p0 == p1).all()
    for k in G.PARAM_NAMES:                 # values, not bits: a masked negative is -0.0 where ReLU gives +0.0
        assert (free[k] == masked[k]).all(), k


def test_gradient_matches_a_central_difference():
    """Directional derivative along a random direction of parameter space (each tensor's direction scaled to the tensor's own rms),
    central difference with step 1e-7 in float64.  The loss is piecewise polynomial in the parameters, so the difference is exact up
    to its rounding (1e-16 |f| / h) unless a pre-activation changes sign inside +-h.  Measured at (2, 37, 53): relative disagreement
    1.0e-9 at h = 1e-7, 9.6e-8 at 1e-8 and 4.2e-7 at 1e-9 (rounding), 2.7e-4 at 1e-6 and 4.8e-3 at 1e-5 (sign changes: 1.3 M
    pre-activations of O(1) move by O(h)).  Asserted: 1e-6, a thousand times the measured figure and far below one sign change."""
    w, x, gp = _case(SHAPES[0])
    g, _, _ = G.gradients(w, x, gp)
    rng = np.random.default_rng(11)
    d = {k: rng.standard_normal(g[k].shape) * np.sqrt(np.mean(np.square(w[k], dtype=np.float64))) for k in G.PARAM_NAMES}
    xt, gpt = torch.from_numpy(x.astype(np.float64)), torch.from_numpy(gp)

    def f(h):
        params = {k: torch.from_numpy(np.asarray(w[k], np.float64) + h * d[k]) for k in G.PARAM_NAMES}
        with torch.no_grad():
            return float((G.forward(params, xt) * gpt).sum())
    h = 1e-7
    fd = (f(h) - f(-h)) / (2 * h)
    an = sum(float((g[k] * d[k]).sum()) for k in G.PARAM_NAMES)
    print(f"\nCNN_GRAD_FD step {h:g} finite difference {fd:.12e} autograd {an:.12e} rel {abs(fd - an) / abs(an):.2e}")
    assert abs(fd - an) <= 1e-6 * abs(an)


# An exact zero in a weight gradient is a channel that is dead over the whole batch (its ReLU never fires, or its input is dead), so
# the fraction falls with the pixel count.  At the two large shapes of the GPU tests the bound is 1 % of any tensor.  At (2, 37, 53) the
# half-resolution grid is 18 x 26: there the widest layer (64 -> 128) loses whole channels, 1 / 128 = 0.78 % of the tensor each, and
# the bound is fewer than four of them, 3 %.  Measured, worst of the 34 tensors (that layer each time): 0.0011, 0.0008 and 0.021.
# Under default-init weights the figure is up to 0.12, which is why those are not used.
DEAD_BOUND = {(2, 255, 508): 0.01, (3, 199, 215): 0.01, (2, 37, 53): 0.03}


@pytest.mark.parametrize("shape", G.GPU_SHAPES[2])
def test_propagating_weights_leave_no_dead_gradient_entries(shape):
    """at the shapes and with the inputs of the GPU gradient tests (tests/test_cnn_train_gpu.py)"""
    x, wp = G.case_inputs(shape)
    g, _, _ = G.gradients(propagating_weights(2), x, wp)
    frac = {k: float((g[k] == 0).mean()) for k in G.PARAM_NAMES}
    k = max(frac, key=frac.get)
    print(f"\nCNN_GRAD_ZEROS {shape} {k} {frac[k]:.4f}")
    assert frac[k] < DEAD_BOUND[shape], (k, frac[k])


def test_e32_is_the_rounding_of_a_float32_backward():
    """torch float32 against the float64 model under the float32 run's own masks: 1e-6-ish, not the 2e-3 of free ReLU decisions."""
    w, x, gp = _case(SHAPES[0])
    e = G.e32(w, x, gp)
    print(f"\nCNN_GRAD_E32 {SHAPES[0]} {e:.2e}")
    assert 1e-8 < e < 2e-5


def test_split_blob_is_the_state_dict_layout():
    from fluidnet_cxx_amd.model import blob_from_state_dict
    w = propagating_weights(2)
    parts = G.split_blob(blob_from_state_dict(w), 2)
    assert list(parts) == G.PARAM_NAMES and all(np.array_equal(parts[k], w[k]) for k in parts)
