"""The float64 model of the PCG operator (tests/poisson_reference.py) against the CPU oracle's Jacobi, through the identity
A p = div - denom (sweep(p) - p) on the active cells for any p that is zero elsewhere (one sweep of the Jacobi whose fixed point
the PCG solves for).  CPU only."""
import numpy as np
import pytest

import poisson_reference as PR
from util import make_flags


def case_flags(B, D, H, W, seed):
    """border wall, the util boxes, Empty cells, random interior obstacles that differ per sample, one non-obstacle border cell"""
    f = make_flags(B, D, H, W, boxes=True, empties=True)
    rng = np.random.default_rng(seed)
    is3d = D > 1
    inner = ~PR._border((D, H, W), is3d)
    for b in range(B):
        f[b, 0][(rng.random((D, H, W)) < 0.08) & inner] = 2.0
    f[0, 0, D // 2, 0, W // 2] = 1.0                       # Dirichlet contact
    return f


CASES = [((2, 1, 13, 17), False), ((2, 1, 24, 20), False), ((2, 9, 11, 7), False), ((2, 10, 12, 14), False),
         ((2, 9, 11, 7), True), ((2, 10, 12, 14), True)]


@pytest.mark.parametrize("shape,quirks", CASES)
def test_model_matches_oracle_jacobi_sweep(oracle, shape, quirks):
    B, D, H, W = shape
    is3d = D > 1
    f = case_flags(B, D, H, W, seed=D * 100 + H)
    rng = np.random.default_rng(7)
    act = np.stack([PR.matrix(f[b, 0], is3d, quirks)[1].reshape(D, H, W) for b in range(B)])[:, None]
    p = np.where(act, rng.standard_normal(f.shape), 0.0).astype(np.float32)
    div = np.where(act, rng.standard_normal(f.shape), 0.0).astype(np.float32)
    denom = 6.0 if is3d else 4.0
    swept = oracle.jacobi_sweeps(f, div, p, is3d, 1, quirks=quirks).astype(np.float64)
    want = div.astype(np.float64) - denom * (swept - p.astype(np.float64))
    got = PR.apply(f, p, is3d, quirks)
    scale = max(1.0, float(np.abs(got).max()))
    d = np.abs(np.where(act, got - want, 0.0)).max()
    assert d <= 1e-5 * scale, f"max |A p - identity| = {d:.3e} (scale {scale:.3e})"
    # off the active set the model's A p is 0 and the Jacobi leaves p at 0
    assert not np.any(np.where(act, 0.0, got)), "A p must vanish off the active cells"
    assert not np.any(np.where(act, 0.0, swept)), "the Jacobi keeps inactive cells at 0"


@pytest.mark.parametrize("shape,quirks", CASES)
def test_model_is_symmetric(shape, quirks):
    B, D, H, W = shape
    f = case_flags(B, D, H, W, seed=3)
    for b in range(B):
        A, _ = PR.matrix(f[b, 0], D > 1, quirks)
        assert abs(A - A.T).max() == 0.0


@pytest.mark.parametrize("is3d,quirks", [(False, False), (True, False), (True, True)])
@pytest.mark.parametrize("dirichlet", [False, True])
def test_singularity_detection_matches_rank(is3d, quirks, dirichlet):
    D, H, W = (5, 6, 7) if is3d else (1, 7, 9)
    f = make_flags(1, D, H, W, boxes=False)
    f[0, 0, D // 2, H // 2, W // 2] = 2.0
    if dirichlet:
        f[0, 0, D // 2, 0, W // 2] = 1.0
    A, act = PR.matrix(f[0, 0], is3d, quirks)
    Aa = A.toarray()[np.ix_(act, act)]
    rank = np.linalg.matrix_rank(Aa)
    assert PR.is_singular(A, act) == (rank < act.sum()), (rank, int(act.sum()))
    # a closed box is singular, except in 3D quirks mode: there its z walls count 0 (Q13), like Dirichlet cells
    assert PR.is_singular(A, act) == (not dirichlet and not quirks)
