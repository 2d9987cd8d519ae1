"""Obstacle geometry written into batch_dict['flags'] in place -- the surface of the reference's
`lib/fluid/geometry_utils.py` (createCylinder :4-34, createBox2D :36-63) as native kernels (fnx_create_cylinder,
fnx_create_box2d): no host round trip, flags bit-exact with the reference's tensor expression.

3D obstacles from geometry (no reference counterpart): createSphere, createBox3D and voxelizeMesh work on
(B,1,D,H,W) flags with B >= 1 and D >= 3.  Cell (i, j, k) sits at the point (x, y, z) = (i, j, k), as for createCylinder; every
function writes TypeObstacle into the cells it finds inside, whatever they held, and touches no other cell."""
from .._ext import ext


def _flags(batch_dict):
    assert "flags" in batch_dict, "Error: flags key is not in batch dict"
    flags = batch_dict["flags"]
    assert flags.dim() == 5, "Input flags must have 5 dimensions"
    assert flags.size(0) == 1, "Only batches of size 1 allowed (inference)"
    return flags


def createCylinder(batch_dict, centerX, centerY, radius):
    """Marks every cell with (x-centerX)^2 + (y-centerY)^2 <= radius^2 as an obstacle, on all z planes
    (geometry_utils.py:26-33: integer cell indices against the float centre)."""
    flags = _flags(batch_dict)
    ext.create_cylinder_(flags, float(centerX), float(centerY), float(radius))
    batch_dict["flags"] = flags


def createBox2D(batch_dict, x0, x1, y0, y1):
    """Marks the cells x0 <= x < x1, y0 <= y < y1 as obstacles.  The reference's version cannot run (it tests
    `Y >= y1 and Y < y1` and then names an undefined mask, geometry_utils.py:59-62); this is the box its docstring
    describes."""
    flags = _flags(batch_dict)
    ext.create_box2d_(flags, float(x0), float(x1), float(y0), float(y1))
    batch_dict["flags"] = flags


def _flags3d(batch_dict, sample):
    assert "flags" in batch_dict, "Error: flags key is not in batch dict"
    flags = batch_dict["flags"]
    assert flags.dim() == 5, "Input flags must have 5 dimensions"
    if sample is None:
        return flags, -1
    sample = int(sample)
    if not 0 <= sample < flags.size(0):
        raise ValueError(f"sample {sample} out of range for a batch of {flags.size(0)}")
    return flags, sample


def createSphere(batch_dict, centerX, centerY, centerZ, radius, sample=None):
    """Marks every cell with dx*dx + dy*dy + dz*dz <= radius*radius (fp32, summed in that order: createCylinder's arithmetic with a
    third term, so the slice k == centerZ is the cylinder's disc bit for bit) as an obstacle.  sample=None: every sample of the
    batch; sample=b: that one alone.  3D grids only."""
    flags, s = _flags3d(batch_dict, sample)
    ext.create_sphere_(flags, float(centerX), float(centerY), float(centerZ), float(radius), s)
    batch_dict["flags"] = flags


def createBox3D(batch_dict, x0, x1, y0, y1, z0, z1, sample=None):
    """Marks the cells x0 <= i < x1, y0 <= j < y1, z0 <= k < z1 (half open, as createBox2D) as obstacles.  3D grids only."""
    flags, s = _flags3d(batch_dict, sample)
    ext.create_box3d_(flags, float(x0), float(x1), float(y0), float(y1), float(z0), float(z1), s)
    batch_dict["flags"] = flags


def voxelizeMesh(batch_dict, vertices, faces, sample=None, check=True):
    """Marks the cells whose point lies inside the closed triangle surface as obstacles, by the even-odd rule along x.

    vertices: (V,3) float32 xyz, faces: (F,3) int32, both on the device of flags.  Two overlapping closed components cancel where
    they overlap; for a union call once per component (the function only ever adds obstacles).  A mesh box with integer corners
    gives exactly createBox3D's half-open box.  Faces with an index outside [0, V), a NaN or Inf coordinate or a vertex farther
    than 2^14 cells from the origin are skipped and counted.

    The call produces a report [open_rows, bad_faces] on the device: an x row crossed an odd number of times is open (the surface
    is not closed there).  check=True reads it -- this synchronises with the device, which a setup call can afford -- and raises
    ValueError naming both counts if either is not zero; the cells found inside have been written by then.  check=False returns
    the report tensor (int32[2]) and never synchronises: the call can be captured into a graph."""
    flags, s = _flags3d(batch_dict, sample)
    report = ext.voxelize_mesh_(flags, vertices, faces, s)
    batch_dict["flags"] = flags
    if not check:
        return report
    open_rows, bad_faces = report.tolist()
    if open_rows or bad_faces:
        raise ValueError(f"voxelizeMesh: {open_rows} open rows (the surface is not closed there), {bad_faces} bad faces (skipped)")
    return None


def load_obj(path):
    """A small host reader of Wavefront OBJ files: the `v x y z` and `f a b c ...` lines, nothing else.  Polygons are triangulated
    as fans; indices may carry /vt/vn suffixes and may be negative (relative to the vertices read so far).
    Returns (vertices (V,3) float32, faces (F,3) int32) as numpy arrays."""
    import numpy as np
    verts, faces = [], []
    with open(path) as fh:
        for line in fh:
            tok = line.split()
            if not tok:
                continue
            if tok[0] == "v" and len(tok) >= 4:
                verts.append([float(tok[1]), float(tok[2]), float(tok[3])])
            elif tok[0] == "f" and len(tok) >= 4:
                idx = []
                for t in tok[1:]:
                    i = int(t.split("/")[0])
                    idx.append(i - 1 if i > 0 else len(verts) + i)
                for n in range(1, len(idx) - 1):
                    faces.append([idx[0], idx[n], idx[n + 1]])
    return (np.asarray(verts, dtype=np.float32).reshape(-1, 3), np.asarray(faces, dtype=np.int32).reshape(-1, 3))
