"""The arithmetic of fnx_render_volume (fluidnet_cxx_amd/csrc/fnx_render.hip, include/fluidnet_hip.h) in numpy: fp32 add, subtract,
multiply, min, max and compare, one operation per line and in the kernels' order, so the device result can be compared bit for bit.

Axes x = W, y = H, z = D.  A direction ('+x' '-x' '+y' '-y' '+z' '-z', codes 0..5) is the way rays or light travel."""
import numpy as np

DIRECTIONS = ("+x", "-x", "+y", "-y", "+z", "-z")
TYPE_OBSTACLE = 2.0
f32 = np.float32


def _axis(direction):
    """numpy axis of a (B, D, H, W) array the direction travels along, and whether it travels towards index 0"""
    code = DIRECTIONS.index(direction)
    return 3 - (code >> 1), bool(code & 1)


def default_absorption(shape, direction):
    """what fluid.renderVolume takes for absorption=None: 16 / (cells along the axis), rounded to fp32 once"""
    return f32(16.0 / shape[_axis(direction)[0]])


def cells(density, flags, bnd):
    """(rho, obs) per cell: the clamped density and the obstacle mask, both emptied within bnd cells of a domain face (a 2D grid,
    D == 1, has no z faces)"""
    density = np.asarray(density, f32)
    rho = np.minimum(np.maximum(density, f32(0)), f32(1))
    obs = np.asarray(flags, f32) == f32(TYPE_OBSTACLE)
    border = np.zeros(density.shape, bool)
    for ax in (1, 2, 3):
        n = density.shape[ax]
        if ax == 1 and n == 1:
            continue
        idx = np.arange(n)
        sh = [1, 1, 1, 1]
        sh[ax] = n
        border |= ((idx < bnd) | (idx >= n - bnd)).reshape(sh)
    return np.where(border, f32(0), rho).astype(f32), obs & ~border


def _marched(a, direction):
    """view of `a` with the march axis first, in travel order"""
    ax, neg = _axis(direction)
    v = np.moveaxis(a, ax, 0)
    return v[::-1] if neg else v


def light_field(rho, obs, light, k_light):
    """L per cell: the light that arrives at it"""
    k = f32(k_light)
    L = np.empty(rho.shape, f32)
    r, o, Lv = _marched(rho, light), _marched(obs, light), _marched(L, light)
    Lin = np.ones(r.shape[1:], f32)
    for s in range(r.shape[0]):
        Lv[s] = Lin
        a = np.minimum(k * r[s], f32(1))
        Lin = np.where(o[s], f32(0), Lin * (f32(1) - a)).astype(f32)
    return L


def render(density, flags, view="-z", light="-y", k_view=None, k_light=None, ambient=0.25, albedo_smoke=1.0, albedo_obstacle=0.5, bnd=1):
    """density, flags: (B, D, H, W).  Returns (B, 2, R, Cc) float32: radiance C and transmittance T; rows and columns are the two axes
    the view does not travel along, in (z, y, x) order."""
    density = np.asarray(density, f32)
    kv = default_absorption(density.shape, view) if k_view is None else f32(k_view)
    kl = default_absorption(density.shape, light) if k_light is None else f32(k_light)
    amb = f32(ambient)
    oma = f32(1) - amb                       # formed once, in fp32
    alb_s, alb_o = f32(albedo_smoke), f32(albedo_obstacle)
    rho, obs = cells(density, flags, bnd)
    L = light_field(rho, obs, light, kl)
    r, o, Lv = _marched(rho, view), _marched(obs, view), _marched(L, view)
    T = np.ones(r.shape[1:], f32)
    C = np.zeros(r.shape[1:], f32)
    for s in range(r.shape[0]):
        sh = amb + oma * Lv[s]
        a = np.minimum(kv * r[s], f32(1))
        C_obs = C + T * (alb_o * sh)
        C_smk = C + (T * a) * (alb_s * sh)
        T_smk = T * (f32(1) - a)
        C = np.where(o[s], C_obs, C_smk).astype(f32)
        T = np.where(o[s], f32(0), T_smk).astype(f32)
    # moveaxis kept the other three axes in (B, z, y, x) order: (B, R, Cc)
    return np.ascontiguousarray(np.stack([C, T], axis=1))


def image_shape(shape, view):
    """(R, Cc) of the image of a (B, D, H, W) volume"""
    ax, _ = _axis(view)
    return tuple(n for i, n in enumerate(shape) if i not in (0, ax))
