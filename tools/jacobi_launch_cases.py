#!/usr/bin/env python3
"""The Jacobi calls whose launch sequence the host side decides, once each, through the C ABI of a library given by path -- to compare
two builds launch by launch:

    rocprofv3 --kernel-trace --output-format csv -d OUT -o t -- python tools/jacobi_launch_cases.py --lib A/libfluidnet_hip.so
    python tools/jacobi_launch_cases.py --reduce OUT/.../t_kernel_trace.csv > a.txt       # (kernel, grid, workgroup) per launch, in order

and the same for B: the two reduced files must be identical.  The cases: fnx_jacobi with and without the residual and
fnx_jacobi_sweeps_ex with and without the start from zero, in 2D at 1, 2, 7, 8, 9, 16, 28, 37 and 100 sweeps and in 3D at 1, 2, 3, 7 and 10
(H a multiple of 4 and not); two-sweep passes of one plane range on a small grid, of two ranges that share the resident set, on more tiles
than wave slots, of two ranges that do not fit at once, from zero in each layout, and the mirrored launches.  `--time` instead measures
three solves (mean of 5 rounds of 20 after warm-up)."""
import argparse
import csv
import ctypes
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
vp, ci, cf, sz = ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_size_t


class FnxGrid(ctypes.Structure):
    _fields_ = [(n, ci) for n in ("B", "D", "H", "W", "is3D", "ref_quirks", "z_offset", "D_global", "k_begin", "k_end")]


class FnxPlaneMirror(ctypes.Structure):
    _fields_ = [("out", vp * 2 * 2), ("slot_select", vp * 2), ("k_first", ci * 2), ("planes", ci), ("sample_stride", sz), ("start_clock", vp)]


def reduce(path):
    rows = list(csv.DictReader(open(path)))
    rows.sort(key=lambda r: int(r.get("Dispatch_Id") or r["Start_Timestamp"]))
    for r in rows:
        if "jacobi" in r["Kernel_Name"] or "residual_" in r["Kernel_Name"]:
            print(r["Kernel_Name"].replace("(anonymous namespace)::", "").replace("void ", "").split("(")[0],
                  "grid", "x".join(r["Grid_Size_" + a] for a in "XYZ"), "wg", "x".join(r["Workgroup_Size_" + a] for a in "XYZ"))


class Case:
    """one grid: fluid inside an obstacle shell with a few obstacle cells, a random divergence, p and a second pressure array, the workspace"""

    def __init__(self, lib, shape):
        import torch
        self.lib, self.shape = lib, shape
        B, D, H, W = shape
        self.g = FnxGrid(B=B, D=D, H=H, W=W, is3D=int(D > 1))
        dev = torch.device("cuda:0")
        gen = torch.Generator(device=dev).manual_seed(B + 3 * D + 5 * H + 7 * W)
        f = torch.full(shape, 2.0, device=dev)
        inner = f[:, 1:-1, 1:-1, 1:-1] if D > 1 else f[:, :, 1:-1, 1:-1]
        inner.fill_(1.0)
        inner[torch.rand(inner.shape, device=dev, generator=gen) < 0.02] = 2.0
        self.flags, self.div = f, torch.rand(shape, device=dev, generator=gen) - 0.5
        self.p, self.q, self.res = torch.zeros(shape, device=dev), torch.zeros(shape, device=dev), torch.zeros(1, device=dev)
        self.ws_bytes = lib.fnx_workspace_bytes(ctypes.byref(self.g), 2)
        self.ws = torch.zeros(self.ws_bytes, dtype=torch.uint8, device=dev)
        self.keep = []

    def check(self, rc, what):
        if rc != 0:
            sys.exit(f"{what} on {self.shape}: {rc} {self.lib.fnx_last_error().decode()}")

    def solve(self, n, residual):
        self.check(self.lib.fnx_jacobi(ctypes.byref(self.g), self.flags.data_ptr(), self.div.data_ptr(), self.p.data_ptr(),
                                       self.res.data_ptr() if residual else None, 0.0, n, None, self.ws.data_ptr(), self.ws_bytes, None), "fnx_jacobi")

    def sweeps(self, n, from_zero):
        self.check(self.lib.fnx_jacobi_sweeps_ex(ctypes.byref(self.g), self.flags.data_ptr(), self.div.data_ptr(), self.p.data_ptr(), n,
                                                 self.ws.data_ptr(), self.ws_bytes, 2 if from_zero else 0, None), "fnx_jacobi_sweeps_ex")

    def pass_(self, n=2, kb=0, ke=0, kb2=-1, layout=0, from_zero=False, reuse=1):
        self.check(self.lib.fnx_jacobi_pass_layout(ctypes.byref(self.g), self.flags.data_ptr(), self.div.data_ptr(), None if from_zero else self.p.data_ptr(),
                                                   self.q.data_ptr(), n, kb, ke, kb2, layout, self.ws.data_ptr(), self.ws_bytes, reuse, None), "fnx_jacobi_pass_layout")

    def mirror(self, kb, ke, kb2, layout):
        import torch
        B, D, H, W = self.shape
        n = ke - kb - 1                                    # all but the first plane of each range
        m = FnxPlaneMirror(planes=n, sample_stride=n * H * W)
        for r in range(2):
            buf = torch.zeros((B, n, H, W), device=self.p.device)
            self.keep.append(buf)
            m.out[r][0] = buf.data_ptr()
        m.k_first[0], m.k_first[1] = kb + 1, max(kb2, 0) + 1
        if not self.lib.fnx_jacobi_pass_mirror_ok(ctypes.byref(self.g), ke - kb, int(kb2 >= 0), layout):
            sys.exit(f"mirror_ok refuses {self.shape} {kb} {ke} {kb2} {layout}")
        self.check(self.lib.fnx_jacobi_pass_mirror(ctypes.byref(self.g), self.flags.data_ptr(), self.div.data_ptr(), self.p.data_ptr(), self.q.data_ptr(),
                                                   kb, ke, kb2, layout, ctypes.byref(m), self.ws.data_ptr(), self.ws_bytes, 1, None), "fnx_jacobi_pass_mirror")


def load(path):
    import torch  # noqa: F401  (first: the library resolves libamdhip64 through it)
    lib = ctypes.CDLL(path)
    lib.fnx_last_error.restype = ctypes.c_char_p
    lib.fnx_workspace_bytes.restype = sz
    G = ctypes.POINTER(FnxGrid)
    lib.fnx_workspace_bytes.argtypes = [G, ci]
    lib.fnx_jacobi.argtypes = [G, vp, vp, vp, vp, cf, ci, vp, vp, sz, vp]
    lib.fnx_jacobi_sweeps_ex.argtypes = [G, vp, vp, vp, ci, vp, sz, ci, vp]
    lib.fnx_jacobi_pass_layout.argtypes = [G, vp, vp, vp, vp, ci, ci, ci, ci, ci, vp, sz, ci, vp]
    lib.fnx_jacobi_pass_mirror.argtypes = [G, vp, vp, vp, vp, ci, ci, ci, ci, ctypes.POINTER(FnxPlaneMirror), vp, sz, ci, vp]
    lib.fnx_jacobi_pass_mirror_ok.argtypes = [G, ci, ci, ci]
    return lib


def launch_cases(lib):
    import torch
    for shape, counts in (((2, 1, 40, 70), (1, 2, 7, 8, 9, 16, 28, 37, 100)), ((1, 1, 515, 509), (1, 2, 7, 8, 9, 16, 28, 37, 100)),
                          ((1, 12, 24, 66), (1, 2, 3, 7, 10)), ((1, 6, 21, 66), (1, 2, 3, 7, 10))):
        c = Case(lib, shape)
        for n in counts:
            for flag in (False, True):
                c.solve(n, residual=flag)
                c.sweeps(n, from_zero=flag)
        torch.cuda.synchronize()
        print("schedule cases", shape, "done", flush=True)
    c = Case(lib, (1, 12, 24, 66))                         # 12 tiles: chunks of two planes
    c.pass_(reuse=0)
    for layout in (0, 1, 2, 3):
        c.pass_(layout=layout)
        c.pass_(kb=3, ke=6, layout=layout)
        c.pass_(kb=2, ke=5, kb2=7, layout=layout)
    for layout in (0, 1, 2, 3):
        c.pass_(layout=layout, from_zero=True)
    c.pass_(n=1, kb=2, ke=5, kb2=7)
    c.pass_(n=1, from_zero=True)
    for layout in (0, 3):
        c.mirror(2, 5, -1, layout)
        c.mirror(2, 5, 7, layout)
    torch.cuda.synchronize()
    c = Case(lib, (1, 40, 70, 130))                        # 54 tiles: two ranges share the resident set
    c.pass_(reuse=0)
    c.pass_(kb=2, ke=8, kb2=30)
    c.pass_(kb=1, ke=20, kb2=20)
    c.mirror(2, 8, 30, 0)
    c.mirror(1, 39, -1, 0)
    torch.cuda.synchronize()
    print("resident-set cases done", flush=True)
    c = Case(lib, (1, 40, 700, 1030))                      # 3150 tiles: one range is resident, two are launched one after the other
    c.pass_(reuse=0, layout=3)
    c.pass_(kb=2, ke=11, layout=3)
    c.pass_(kb=2, ke=11, kb2=20, layout=3)
    c.mirror(2, 11, -1, 3)
    torch.cuda.synchronize()
    del c
    c = Case(lib, (1, 40, 1040, 1030))                     # 4680 tiles, more than the wave slots: the split launch
    c.pass_(reuse=0, layout=3)
    for layout in (0, 1, 2):
        c.pass_(kb=2, ke=9, layout=layout)
    c.pass_(kb=2, ke=9, kb2=20)
    c.pass_(layout=2, from_zero=True)
    c.pass_(layout=0, from_zero=True)
    c.solve(4, residual=False)
    torch.cuda.synchronize()
    print("split cases done", flush=True)


def time_cases(lib):
    import torch
    cases = {}
    for name, shape, n in (("3D 256^3 x 100", (1, 256, 256, 256), 100), ("2D 2048^2 x 100", (1, 1, 2048, 2048), 100), ("2D 128^2 x 28", (1, 1, 128, 128), 28)):
        c = Case(lib, shape)
        cases[name] = (lambda c=c, n=n: c.solve(n, residual=False))
    for fn in cases.values():
        for _ in range(20):
            fn()
    torch.cuda.synchronize()
    ROUNDS, REPS = 5, 20
    times = {k: [] for k in cases}
    for _ in range(ROUNDS):
        for k, fn in cases.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(REPS):
                fn()
            e1.record()
            torch.cuda.synchronize()
            times[k].append(e0.elapsed_time(e1) / REPS * 1e3)
    for k, v in times.items():
        print(f"{k:18s} mean {sum(v) / len(v):9.2f} us   min {min(v):9.2f} max {max(v):9.2f}   rounds " + " ".join(f"{x:.2f}" for x in v))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default=os.path.join(REPO, "fluidnet_cxx_amd", "libfluidnet_hip.so"))
    ap.add_argument("--reduce", metavar="KERNEL_TRACE_CSV")
    ap.add_argument("--time", action="store_true")
    a = ap.parse_args()
    if a.reduce:
        return reduce(a.reduce)
    lib = load(a.lib)
    (time_cases if a.time else launch_cases)(lib)


if __name__ == "__main__":
    main()
