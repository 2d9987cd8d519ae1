#!/usr/bin/env python3
"""Print every size and layout the training entry points report, from the host-side functions of the C ABI alone (no GPU needed):

    python tools/cnn_train_sizes.py [path/to/libfluidnet_hip.so] > sizes.txt

the two packed_t sizes and, per grid, the tape layout (every entry), fnx_multiscale*_backward_ws_bytes and fnx_fluidnet*_train_ws_bytes.
Two builds report the same sizes exactly when their outputs are equal."""
import ctypes as C
import os
import sys

GRIDS2D = [(2, 37, 53), (1, 4, 4)]
GRIDS3D = [(2, 6, 10, 37), (1, 9, 14, 70), (1, 4, 4, 4)]


class Grid(C.Structure):
    _fields_ = [(n, C.c_int) for n in "B D H W is3D ref_quirks z_offset D_global k_begin k_end".split()]


class Entry2(C.Structure):
    _fields_ = [("name", C.c_char * 8), ("offset", C.c_size_t), ("C", C.c_int), ("H", C.c_int), ("W", C.c_int)]


class Entry3(C.Structure):
    _fields_ = [("name", C.c_char * 8), ("offset", C.c_size_t), ("C", C.c_int), ("D", C.c_int), ("H", C.c_int), ("W", C.c_int)]


def main():
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    lib = C.CDLL(sys.argv[1] if len(sys.argv) > 1 else os.path.join(here, "fluidnet_cxx_amd", "libfluidnet_hip.so"))
    for fn in ("fnx_scalenet_packed_t_bytes", "fnx_scalenet3d_packed_t_bytes", "fnx_multiscale_tape_layout", "fnx_multiscale3d_tape_layout",
               "fnx_multiscale_backward_ws_bytes", "fnx_multiscale3d_backward_ws_bytes", "fnx_fluidnet_train_ws_bytes",
               "fnx_fluidnet3d_train_ws_bytes"):
        getattr(lib, fn).restype = C.c_size_t
    n = lib.fnx_multiscale_tape_entries()
    print("fnx_scalenet_packed_t_bytes", lib.fnx_scalenet_packed_t_bytes())
    print("fnx_scalenet3d_packed_t_bytes", lib.fnx_scalenet3d_packed_t_bytes())
    for dims in GRIDS2D + GRIDS3D:
        is3d = len(dims) == 4
        B, D, H, W = dims if is3d else (dims[0], 1, dims[1], dims[2])
        g = Grid(B=B, D=D, H=H, W=W, is3D=int(is3d))
        sfx = "3d" if is3d else ""
        entries = ((Entry3 if is3d else Entry2) * n)()
        floats = getattr(lib, f"fnx_multiscale{sfx}_tape_layout")(C.byref(g), entries)
        print(f"grid {dims}: tape floats {floats}")
        for e in entries:
            shape = (e.C, e.D, e.H, e.W) if is3d else (e.C, e.H, e.W)
            print(f"  {e.name.decode():<4} offset {e.offset} shape {shape}")
        print(f"  fnx_multiscale{sfx}_backward_ws_bytes", getattr(lib, f"fnx_multiscale{sfx}_backward_ws_bytes")(C.byref(g)))
        print(f"  fnx_fluidnet{sfx}_train_ws_bytes", getattr(lib, f"fnx_fluidnet{sfx}_train_ws_bytes")(C.byref(g)))


if __name__ == "__main__":
    main()
