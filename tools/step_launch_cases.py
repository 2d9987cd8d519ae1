#!/usr/bin/env python3
"""The time steps whose launch sequence the host side decides (fnx_step_plan.h), once each, through the C ABI of a library given by path --
to compare two builds launch by launch and bit by bit:

    rocprofv3 --kernel-trace --output-format csv -d OUT -o t -- python tools/step_launch_cases.py --lib A/libfluidnet_hip.so
    python tools/step_launch_cases.py --reduce OUT/.../t_kernel_trace.csv > a.txt     # the (kernel, grid, workgroup) launched, in order
    python tools/step_launch_cases.py --lib A/libfluidnet_hip.so --digest > da.txt    # sha256 of p, U, density after two steps of each case,
                                                                                      # then of fnx_advect_scalars' output (scalars_digest)

and the same for B: the reduced files must be identical, and the digests equal line for line.  The grids: 2D (2,1,40,70), 3D (1,9,20,66),
and (2,6,21,66) with BC arrays that are the identity almost everywhere and the class map on (whole waves of identity cells, B > 1).  The
cases, in 2D and in 3D where the stage exists there: methods 0 to 4 (untrained packed weights where a net is needed), with and without
density, with and without BC arrays, static_flags 0 then 15 on a second call, periodic 3, 5 and 7, viscosity, flags_stick, vorticity
confinement, gravity_scale, correct_scalar, the reference's 3D quirks; then fnx_pre_projection on a plane range with the divergence (with
and without wall BCs, with the quirks) and on the whole grid with the confinement, each followed by fnx_post_projection.  Together the
cases launch each of the sixteen stage-kernel instances.  The workspace is FNX_OP_STEP_STATIC's where the library has that op (a build
from before it: FNX_OP_STEP's), so in 3D the calls that go by the class map also build the stage word map (stage_word_kernel) and run the
WORD twins of the stage and post-projection kernels; the class-map grid adds a second call that promises the BC arrays but not the flags
(static_flags 6: the word is built again, the class map is not).  Every input comes from a seeded generator on the host."""
import argparse
import csv
import ctypes
import hashlib
import os
import sys
import textwrap

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
vp, ci, cf, sz = ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_size_t


class FnxGrid(ctypes.Structure):
    _fields_ = [(n, ci) for n in ("B", "D", "H", "W", "is3D", "ref_quirks", "z_offset", "D_global", "k_begin", "k_end")]


class FnxStepParams(ctypes.Structure):
    _fields_ = [("dt", cf), ("maccormack_strength", cf), ("sample_outside_fluid", ci), ("buoyancy_scale", cf), ("gravity_vec", cf * 3),
                ("operating_density", cf), ("p_tol", cf), ("jacobi_iter", ci), ("method", ci), ("normalize_threshold", cf),
                ("precision_mode", ci), ("static_flags", ci), ("viscosity", cf), ("gravity_scale", cf), ("correct_scalar", ci),
                ("periodic", ci), ("pcg_tol", cf), ("pcg_iter", ci), ("vorticity_confinement", cf)]


class FnxState(ctypes.Structure):
    _fields_ = [(n, vp) for n in ("p", "U", "density", "flags", "UBC", "UBCInvMask", "densityBC", "densityBCInvMask", "net", "bc_class",
                                  "flags_stick")] + [("density_bc_applied", ci)]


def fold(seq, longest=64):
    """the sequence with every block that is launched n >= 2 times running written once, as n*(block)"""
    out, i = [], 0
    while i < len(seq):
        saved, p, n = 0, 1, 1
        for q in range(1, min(longest, (len(seq) - i) // 2) + 1):
            m = 1
            while seq[i + m * q:i + (m + 1) * q] == seq[i:i + q]:
                m += 1
            if (m - 1) * q > saved:
                saved, p, n = (m - 1) * q, q, m
        body = fold(seq[i:i + p], longest) if n > 1 and p > 1 else seq[i:i + p]
        out.append(body[0] if n == 1 else f"{n}*{body[0]}" if len(body) == 1 and "*" not in body[0] else f"{n}*({' '.join(body)})")
        i += p * n
    return out


def write_launches(launches):
    """the distinct launches, numbered in order of first appearance, then the folded sequence of their numbers: the same text for the
    same sequence, so two traces are compared by comparing their files"""
    names = {}
    seq = [names.setdefault(launch, f"k{len(names)}") for launch in launches]
    print(f"# {len(launches)} launches of {len(names)} kinds: (kernel, grid, workgroup)")
    for launch, k in names.items():
        print(k, launch)
    print("# in dispatch order; n*(...) is a block launched n times running")
    print(textwrap.fill(" ".join(fold(seq)), 150, break_long_words=False, break_on_hyphens=False))


def reduce(path):
    rows = list(csv.DictReader(open(path)))
    rows.sort(key=lambda r: int(r.get("Dispatch_Id") or r["Start_Timestamp"]))
    write_launches([" ".join((r["Kernel_Name"].replace("(anonymous namespace)::", "").replace("void ", "").split("(")[0],
                              "grid", "x".join(r["Grid_Size_" + a] for a in "XYZ"), "wg", "x".join(r["Workgroup_Size_" + a] for a in "XYZ")))
                    for r in rows if not r["Kernel_Name"].startswith(("void at::", "at::"))])  # not the framework's own fills and copies


def load(path):
    import torch  # noqa: F401  (first: the library resolves libamdhip64 through it)
    lib = ctypes.CDLL(path)
    lib.fnx_last_error.restype = ctypes.c_char_p
    lib.fnx_workspace_bytes.restype = lib.fnx_scalenet_weight_floats.restype = lib.fnx_scalenet_packed_bytes.restype = sz
    G, P, S = ctypes.POINTER(FnxGrid), ctypes.POINTER(FnxStepParams), ctypes.POINTER(FnxState)
    lib.fnx_workspace_bytes.argtypes = [G, ci]
    lib.fnx_scalenet_weight_floats.argtypes = lib.fnx_scalenet_packed_bytes.argtypes = [ci]
    lib.fnx_scalenet_pack.argtypes = [ci, vp, vp, vp]
    lib.fnx_simulate_step.argtypes = [G, P, S, vp, sz, vp]
    lib.fnx_pre_projection.argtypes = [G, P, S, vp, vp, vp, vp]
    lib.fnx_post_projection.argtypes = [G, S, vp]
    return lib


class Fields:
    """one grid's inputs, made on the host: fluid inside an obstacle shell with a few obstacle cells, U, density, p, BC arrays (`sparse`:
    the identity on all but a block in a corner, else on half of the cells), flags_stick, the packed weights of an untrained net"""

    def __init__(self, lib, shape, sparse_bc=False):
        import torch
        self.lib, self.shape = lib, shape
        B, D, H, W = shape
        self.is3d, self.nc = D > 1, 3 if D > 1 else 2
        rng = np.random.default_rng(B + 3 * D + 5 * H + 7 * W)
        f = np.full((B, 1, D, H, W), 2.0, np.float32)
        inner = f[:, :, 1:-1, 1:-1, 1:-1] if self.is3d else f[:, :, :, 1:-1, 1:-1]
        inner[...] = np.where(rng.random(inner.shape) < 0.02, 2.0, 1.0)
        stick = f.copy()
        stick[(f == 2.0) & (rng.random(f.shape) < 0.5)] = 128.0
        vel = (B, self.nc, D, H, W)

        def bc(shape):
            where = np.zeros(shape, bool)
            if sparse_bc:
                where[..., 2:5, 3:9] = True
            else:
                where[...] = rng.random(shape) < 0.5
            return np.where(where, rng.standard_normal(shape), 0.0).astype(np.float32), np.where(where, 0.0, 1.0).astype(np.float32)

        UBC, UBCInvMask = bc(vel)
        rhoBC, rhoBCInvMask = bc(f.shape)
        self.host = dict(flags=f, flags_stick=stick, U=(rng.standard_normal(vel) * 0.5).astype(np.float32), density=rng.random(f.shape).astype(np.float32),
                         p=(rng.standard_normal(f.shape) * 0.1).astype(np.float32), UBC=UBC, UBCInvMask=UBCInvMask, densityBC=rhoBC,
                         densityBCInvMask=rhoBCInvMask, U_adv=(rng.standard_normal(vel) * 0.5).astype(np.float32),
                         rho_adv=rng.random(f.shape).astype(np.float32))
        self.dev = torch.device("cuda:0")
        weights = torch.from_numpy((rng.standard_normal(lib.fnx_scalenet_weight_floats(int(self.is3d))) * 0.05).astype(np.float32)).to(self.dev)
        self.net = torch.zeros(lib.fnx_scalenet_packed_bytes(int(self.is3d)), dtype=torch.uint8, device=self.dev)
        self.check(lib.fnx_scalenet_pack(int(self.is3d), weights.data_ptr(), self.net.data_ptr(), None), "fnx_scalenet_pack")
        torch.cuda.synchronize()

    def check(self, rc, what):
        if rc != 0:
            sys.exit(f"{what} on {self.shape}: {rc} {self.lib.fnx_last_error().decode()}")

    def grid(self, **kw):
        B, D, H, W = self.shape
        return FnxGrid(B=B, D=D, H=H, W=W, is3D=int(self.is3d), **kw)

    def fresh(self, density=True, bcs=True, stick=False, net=False):
        """device copies of the inputs and the state that points at them"""
        import torch
        t = {k: torch.from_numpy(v).to(self.dev) for k, v in self.host.items()}
        st = FnxState(p=t["p"].data_ptr(), U=t["U"].data_ptr(), flags=t["flags"].data_ptr())
        if density:
            st.density = t["density"].data_ptr()
        if bcs:
            st.UBC, st.UBCInvMask = t["UBC"].data_ptr(), t["UBCInvMask"].data_ptr()
            if density:
                st.densityBC, st.densityBCInvMask = t["densityBC"].data_ptr(), t["densityBCInvMask"].data_ptr()
        if stick:
            st.flags_stick = t["flags_stick"].data_ptr()
        if net:
            st.net = self.net.data_ptr()
        return t, st


def params(**kw):
    prm = FnxStepParams(dt=0.1, maccormack_strength=1.0, buoyancy_scale=1.0, gravity_vec=(0.3, -0.7, 1.1), operating_density=0.1,
                        jacobi_iter=9, normalize_threshold=1e-5, pcg_iter=3)
    for k, v in kw.items():
        setattr(prm, k, v)
    return prm


def step_cases(is3d):
    """(name, parameters, state options, static_flags of the first and of the second call, grid options)"""
    both = (0, 0)
    cases = [(f"method{m}", dict(method=m), {}, both, {}) for m in range(5)]
    cases += [(f"method{m}_no_density", dict(method=m), dict(density=False), both, {}) for m in (0, 1, 3)]
    cases += [(f"method{m}_no_bcs", dict(method=m), dict(bcs=False), both, {}) for m in (0, 1, 2)]
    cases += [(f"method{m}_static", dict(method=m), {}, (0, 15), {}) for m in (0, 2, 4)]
    cases += [(f"periodic{p}", dict(periodic=p), {}, both, {}) for p in (3, 5, 7)]
    cases += [("periodic7_pcg", dict(periodic=7, method=2), {}, both, {}), ("periodic7_convnet", dict(periodic=7, method=1), {}, both, {})]
    cases += [(f"confinement_method{m}", dict(method=m, vorticity_confinement=0.4), {}, both, {}) for m in (0, 1)]
    cases += [("confinement_periodic7", dict(vorticity_confinement=0.4, periodic=7), {}, both, {}),
              ("confinement_no_density", dict(vorticity_confinement=0.4), dict(density=False), both, {}),
              ("gravity_scale", dict(gravity_scale=1.3), {}, both, {}), ("gravity_scale_convnet", dict(gravity_scale=1.3, method=1), {}, both, {}),
              ("correct_scalar", dict(correct_scalar=1), {}, both, {}), ("no_buoyancy", dict(buoyancy_scale=0.0), {}, both, {})]
    if is3d:
        cases += [(f"quirks_method{m}", dict(method=m), {}, both, dict(ref_quirks=1)) for m in (0, 1)]
        cases += [("quirks_confinement", dict(vorticity_confinement=0.4), {}, both, dict(ref_quirks=1)),
                  ("quirks_periodic7", dict(periodic=7), {}, both, dict(ref_quirks=1))]
    else:
        cases += [("viscosity", dict(viscosity=0.05), {}, both, {}), ("viscosity_no_density", dict(viscosity=0.05), dict(density=False), both, {}),
                  ("viscosity_convnet", dict(viscosity=0.05, method=1), {}, both, {}),
                  ("stick_convnet", dict(method=1), dict(stick=True), both, {}), ("stick_ignored", dict(method=0), dict(stick=True), both, {}),
                  ("stick_convnet_static", dict(method=1), dict(stick=True), (2, 15), {})]
    return cases


def sha(t):
    return hashlib.sha256(t.cpu().numpy().tobytes()).hexdigest()[:32]


def run(lib, digest):
    import torch
    for shape, sparse in (((2, 1, 40, 70), False), ((1, 9, 20, 66), False), ((2, 6, 21, 66), True)):
        F = Fields(lib, shape, sparse_bc=sparse)
        cases = step_cases(F.is3d) if not sparse else ([(f"class_map_method{m}", dict(method=m), {}, (2, 15), {}) for m in range(5)] +
                                                       [("class_map_flags_not_promised", dict(method=0), {}, (2, 6), {})])
        for name, prm_kw, st_kw, static, grid_kw in cases:
            g, prm = F.grid(**grid_kw), params(**prm_kw)
            t, st = F.fresh(net=prm.method in (1, 3), **st_kw)
            ws_bytes = lib.fnx_workspace_bytes(ctypes.byref(g), 6) or lib.fnx_workspace_bytes(ctypes.byref(g), 3)   # FNX_OP_STEP_STATIC, _STEP
            ws = torch.zeros(ws_bytes, dtype=torch.uint8, device=F.dev)
            # a second call only where it differs from the first (its promises) or where the bits of two steps are wanted
            for flags in static if digest or static[1] != static[0] else static[:1]:
                prm.static_flags = flags
                F.check(lib.fnx_simulate_step(ctypes.byref(g), ctypes.byref(prm), ctypes.byref(st), ws.data_ptr(), ws_bytes, None),
                        f"fnx_simulate_step {name}")
            torch.cuda.synchronize()
            if digest:
                print("x".join(map(str, shape)), name, "p", sha(t["p"]), "U", sha(t["U"]), "density", sha(t["density"]), flush=True)
        # the stages alone: a plane range with the divergence (one plane more is staged than divergences are written) -- with the wall BCs,
        # without them (the convnet's stage, which the step never asks a divergence of) and with the 3D quirks --, the stage cut around the
        # confinement on the whole grid, and after each the whole post-projection pass
        for method, quirks, confine in ((0, 0, 0.0), (1, 0, 0.0), (1, 1, 0.0), (1, 0, 0.4)) if F.is3d and not sparse else ():
            window = dict(k_begin=2, k_end=5) if confine == 0.0 else {}
            g, prm = F.grid(ref_quirks=quirks, **window), params(method=method, vorticity_confinement=confine)
            t, st = F.fresh()
            div = torch.zeros_like(t["p"])
            F.check(lib.fnx_pre_projection(ctypes.byref(g), ctypes.byref(prm), ctypes.byref(st), t["U_adv"].data_ptr(), t["rho_adv"].data_ptr(),
                                           div.data_ptr(), None), "fnx_pre_projection")
            whole = F.grid(ref_quirks=quirks)
            F.check(lib.fnx_post_projection(ctypes.byref(whole), ctypes.byref(st), None), "fnx_post_projection")
            torch.cuda.synchronize()
            if digest:
                print("x".join(map(str, shape)), f"stages_alone_method{method}_quirks{quirks}_confinement{confine}", "div", sha(div), "U", sha(t["U"]),
                      "density", sha(t["density"]), flush=True)
        print("x".join(map(str, shape)), "done", file=sys.stderr, flush=True)


def scalars_digest(lib):
    """fnx_advect_scalars on the shapes (B, C, D, H, W) of tests/test_scalars_gpu.py, MacCormack and Euler: sha256 of the output"""
    import torch
    lib.fnx_advect_scalars_workspace_bytes.restype = sz
    lib.fnx_advect_scalars.argtypes = [ctypes.POINTER(FnxGrid), cf, ci, vp, vp, vp, vp, ci, ci, ci, cf, vp, sz, vp]
    for B, C, D, H, W in ((2, 5, 1, 20, 33), (2, 5, 9, 12, 70), (2, 1, 1, 20, 33), (2, 1, 9, 12, 70), (2, 3, 19, 35, 70)):
        F = Fields(lib, (B, D, H, W))
        rng = np.random.default_rng(C + 11 * D)
        t = {k: torch.from_numpy(v).to(F.dev) for k, v in dict(F.host, src=rng.random((B, C, D, H, W)).astype(np.float32),
                                                               U=(rng.standard_normal(F.host["U"].shape) * 3).astype(np.float32)).items()}
        g, out = F.grid(), torch.zeros((B, C, D, H, W), device=F.dev)
        ws_bytes = lib.fnx_advect_scalars_workspace_bytes(ctypes.byref(g), C)
        ws = torch.zeros(ws_bytes, dtype=torch.uint8, device=F.dev)
        for method in (1, 0):
            F.check(lib.fnx_advect_scalars(ctypes.byref(g), 1.0, C, t["src"].data_ptr(), t["U"].data_ptr(), t["flags"].data_ptr(),
                                           out.data_ptr(), method, 1, 0, 0.6, ws.data_ptr(), ws_bytes, None), "fnx_advect_scalars")
            torch.cuda.synchronize()
            print("x".join(map(str, (B, C, D, H, W))), f"advect_scalars_method{method}", "out", sha(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default=os.path.join(REPO, "fluidnet_cxx_amd", "libfluidnet_hip.so"))
    ap.add_argument("--reduce", metavar="KERNEL_TRACE_CSV")
    ap.add_argument("--digest", action="store_true")
    a = ap.parse_args()
    if a.reduce:
        return reduce(a.reduce)
    lib = load(a.lib)
    run(lib, a.digest)
    if a.digest:
        scalars_digest(lib)


if __name__ == "__main__":
    main()
