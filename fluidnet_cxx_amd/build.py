"""In-tree build of the native pieces (gfx950 only).

  libfluidnet_hip.so   HIP kernels + the C ABI of include/fluidnet_hip.h      (hipcc, cross-compiles without a GPU)
  fluidnet_cpp.so      torch cpp-extension with the reference's pybind entry points, linked against the above

Both land next to this file so they travel with the repo snapshot to the GPU box.
"""
import os
import subprocess
import sys
import sysconfig

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
LIB = os.path.join(HERE, "libfluidnet_hip.so")
EXT = os.path.join(HERE, "fluidnet_cpp.so")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")

# file -> extra flags.  Stencil/advection/Jacobi units must not contract a*b+c into FMA: bit-parity with the
# reference's ATen arithmetic depends on it.  The CNN unit is tolerance-checked and may fuse.
HIP_UNITS = {
    "fnx_stencils.hip": ["-ffp-contract=off"],
    "fnx_advect.hip": ["-ffp-contract=off", "-Rpass-analysis=kernel-resource-usage"],
    "fnx_scalars.hip": ["-ffp-contract=off", "-Rpass-analysis=kernel-resource-usage"],
    "fnx_jacobi.hip": ["-ffp-contract=off"],
    "fnx_pcg.hip": ["-Rpass-analysis=kernel-resource-usage"],
    "fnx_step.hip": ["-ffp-contract=off"],
    "fnx_vorticity.hip": ["-ffp-contract=off", "-Rpass-analysis=kernel-resource-usage"],
    "fnx_viscous.hip": ["-ffp-contract=off", "-Rpass-analysis=kernel-resource-usage"],
    "fnx_scenes.hip": ["-ffp-contract=off", "-Rpass-analysis=kernel-resource-usage"],
    "fnx_render.hip": ["-ffp-contract=off", "-Rpass-analysis=kernel-resource-usage"],
    "fnx_voxelize.hip": ["-ffp-contract=off", "-Rpass-analysis=kernel-resource-usage"],
    "fnx_api.hip": ["-ffp-contract=off"],
    # (resource-usage remarks: build_lib checks the kernels of SCRATCH_FREE)
    "fnx_cnn.hip": ["-Rpass-analysis=kernel-resource-usage"],
    # FluidNet.forward around a net: the flags of fnx_cnn.hip, which held it (its fp64 sums of squares contract)
    "fnx_fluidnet.hip": ["-Rpass-analysis=kernel-resource-usage"],
    "fnx_cnn_train.hip": ["-Rpass-analysis=kernel-resource-usage"],
    "fnx_banknet.hip": ["-Rpass-analysis=kernel-resource-usage"],
    "fnx_banknet_train.hip": ["-Rpass-analysis=kernel-resource-usage"],
    "fnx_banknet3d.hip": ["-Rpass-analysis=kernel-resource-usage"],
    "fnx_banknet3d_train.hip": ["-Rpass-analysis=kernel-resource-usage"],
    "fnx_slab.hip": [],
    "fnx_peer.hip": [],
}
# unit -> (kernels that must use no scratch and spill no VGPR, why).  hipcc's resource-usage remarks are checked after each compile.
SCRATCH_FREE = {
    "fnx_cnn.hip": (["conv3_wbf_kernel"], "fnx_cnn_bf16x6.h: the results of its inline-asm LDS reads are only valid behind an explicit "
                                          "wait; a spill copies them before it"),
    "fnx_cnn_train.hip": (["wgrad_mfma_kernel", "wgrad_small_kernel"],
                          "the MFMA kernel's nine 32x32 accumulators (144 VGPRs) live across the whole pixel march at two workgroups per "
                          "CU; a spill puts scratch traffic between the MFMAs.  The plain kernel slices a 5x5x5 layer by dz so that its "
                          "25 fp64 accumulators stay in registers"),
    "fnx_banknet.hip": (["banknet_level_kernel"],
                        "a lane keeps the 36 MFMA weight operands of a bank convolution (and, at full resolution, the tail's 12) in "
                        "registers for the whole tile, and the 6x6x2 input patch of a 4x4 pooling window while it recomputes conv1; a "
                        "spill puts a scratch reload in front of every MFMA"),
    "fnx_banknet_train.hip": (["banknet_level_tape_kernel", "bank_tail_bwd_kernel", "bank_level_bwd_kernel", "bank_conv1_bwd_kernel"],
                              "the level kernels keep a convolution's 36 MFMA weight operands and, in the backward, the 72 accumulator "
                              "registers of the two weight gradients across the workgroup's tiles at two workgroups per CU; the tail "
                              "and conv1 kernels keep their accumulators across the cell march; a spill puts scratch traffic between "
                              "the MFMAs"),
    "fnx_banknet3d.hip": (["bank3d_conv1_kernel", "bank3d_conv_kernel"],
                          "a lane of the convolution keeps its 108 MFMA weight operands, the twelve values of the plane in flight and "
                          "(full resolution) the tail's 24 in registers for the whole z-march at two waves a SIMD; a spill puts a scratch "
                          "reload in front of every MFMA.  conv1 keeps the 32 accumulators of a pair of cells and reads its weights "
                          "from LDS; scratch there would mean the 880 weights were hoisted into registers"),
    "fnx_banknet3d_train.hip": (["bank3d_tail_tape_kernel", "bank3d_conv_bwd_kernel", "bank3d_wgrad_kernel", "bank3d_conv1_bwd_kernel"],
                                "the convolution body keeps its 108 MFMA weight operands in registers for the whole z-march, and the "
                                "weight-gradient kernel its 27 accumulators (108 registers) across all the items of a workgroup, both at "
                                "two waves a SIMD; the tail and conv1 kernels keep their accumulators across the cell march; a spill puts "
                                "scratch traffic between the MFMAs"),
    "fnx_advect.hip": (["advect3d_fwd_tile_kernel", "advect3d_bwd_tile_kernel", "advect3d_bwd_scalar_tile_kernel",
                        "advect3d_bwd_vel_tile_kernel", "box_minmax_kernel"],
                       "fnx_advect_march.h: the 3D advection marches run at 2-3 waves per SIMD with every VGPR in use; a reload from "
                       "scratch is an s_waitcnt vmcnt(0) that also waits for the plane in flight and the stores.  The clamp-bounds "
                       "reduction keeps three xy-reduced planes of eight rows in registers along its z-march; scratch there would mean "
                       "a row array was indexed at run time"),
    "fnx_scalars.hip": (["advect_scalars_fwd_kernel", "advect_scalars_bwd_kernel"],
                        "one thread per cell with one channel's eight interpolation corners in registers at a time; scratch there would "
                        "mean the corner array was indexed at run time, or the line trace's state was pushed out by the channel loop"),
    "fnx_pcg.hip": (["pcg_guess_kernel"],
                    "a streaming kernel like pcg_dir_apply_kernel: a cell's stencil, seven loads and three fp64 partial sums; scratch there "
                    "would mean the partial sums or the stencil were turned into arrays in memory"),
    "fnx_vorticity.hip": (["vorticity_confinement_kernel"],
                          "its z-march keeps three planes of c and n, two of the curl and three of F_z in registers between the barriers; "
                          "a spill puts a scratch round trip into every step of the march"),
    "fnx_viscous.hip": (["add_viscosity3d_kernel"],
                        "its z-march keeps three planes of the three components and of flags, and the halo cell of two planes, in "
                        "registers between the barriers; a spill puts a scratch round trip into every step of a bandwidth-bound march"),
    "fnx_scenes.hip": (["scene_obstacles_kernel", "scene_turbulence_kernel", "train_loss_kernel", "train_loss_finish_kernel"],
                       "they are streaming kernels with a handful of live values per thread in either dimension (the 3D turbulence "
                       "thread's nine potential values, the loss's fp64 partial sums); scratch there would mean the octave loop, the "
                       "per-axis arrays or the partial sums were turned into arrays in memory"),
    "fnx_voxelize.hip": (["geometry3d_kernel", "voxel_faces_kernel", "voxel_fill_kernel"],
                         "a face lane holds nine snapped coordinates and the box of its rows, a fill lane one word and a carry; scratch "
                         "there would mean the face record handed between lanes was turned into an array in memory"),
    "fnx_render.hip": (["render_march_kernel", "render_march_x_kernel"],
                       "a column's running light, transmittance and radiance live in registers for the whole march; scratch there "
                       "would put a memory round trip between every two cells of a serial chain"),
}
# -fno-slp-vectorize: hipcc otherwise packs adjacent scalar f32 adds into v_pk_add_f32 + v_pk_mov shuffles, measured
# 1.6x slower per op than plain VALU on gfx950 (tools/ubench/dpp_bench.hip).
COMMON = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-fno-fast-math", "-fno-slp-vectorize", "-Wall",
          "-Wno-unused-function"]


def _newer(target, deps):
    if not os.path.exists(target):
        return True
    t = os.path.getmtime(target)
    return any(os.path.getmtime(d) > t for d in deps if os.path.exists(d))


def _scratch_users(remarks, kernel):
    """[(function, scratch bytes per lane, VGPR spills)] of the instantiations of `kernel` that use scratch, from hipcc's
    -Rpass-analysis=kernel-resource-usage remarks"""
    import re
    bad, seen = [], 0
    for m in re.finditer(r"Function Name: (\S*" + re.escape(kernel) + r"\S*).*?ScratchSize \[bytes/lane\]: (\d+).*?VGPRs Spill: (\d+)", remarks, re.S):
        seen += 1
        if int(m.group(2)) or int(m.group(3)):
            bad.append((m.group(1), int(m.group(2)), int(m.group(3))))
    return bad, seen


def build_lib(force=False, verbose=False):
    hdrs = [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".h")]
    hdrs.append(os.path.join(HERE, "..", "include", "fluidnet_hip.h"))
    objs = []
    procs = []
    os.makedirs(os.path.join(HERE, "build"), exist_ok=True)
    for unit, extra in HIP_UNITS.items():
        src = os.path.join(CSRC, unit)
        if not os.path.exists(src):
            continue
        obj = os.path.join(HERE, "build", unit.replace(".hip", ".o"))
        objs.append(obj)
        if force or _newer(obj, [src] + hdrs + [__file__]):
            cmd = [HIPCC] + COMMON + extra + os.environ.get("FNX_EXTRA_HIPCC_FLAGS", "").split() + ["-c", src, "-o", obj]
            if verbose:
                print(" ".join(cmd))
            procs.append((unit, subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)))
    failed = False
    for unit, p in procs:
        out, _ = p.communicate()
        if p.returncode != 0:
            failed = True
            sys.stderr.write(f"--- {unit} ---\n{out.decode()}\n")
        elif unit in SCRATCH_FREE:
            kernels, why = SCRATCH_FREE[unit]
            spills = False
            for kernel in kernels:
                bad, seen = _scratch_users(out.decode(), kernel)
                if seen == 0:  # no remark matched (renamed kernel, another hipcc's remark format): the check must not pass unseen
                    msg = (f"no kernel-resource-usage remark for {kernel} was found in hipcc's output -- the no-scratch check could "
                           "not run (fluidnet_cxx_amd/build.py:_scratch_users)")
                elif bad:
                    msg = f"{kernel} must not spill ({why}): {bad}"
                else:
                    continue
                spills = True
                sys.stderr.write(f"{unit}: {msg}\n")
            if spills:
                failed = True
                os.remove(os.path.join(HERE, "build", unit.replace(".hip", ".o")))
        elif verbose and out:
            print(out.decode())
    if failed:
        raise RuntimeError("hipcc failed")
    if force or procs or _newer(LIB, objs):
        cmd = [HIPCC, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", LIB] + objs
        subprocess.check_call(cmd)
    return LIB


def build_ext(force=False, verbose=False):
    """fluidnet_cpp: pybind11 module over the C ABI (g++; needs torch headers, not a GPU)."""
    src = os.path.join(CSRC, "fluidnet_cpp.cpp")
    if not (force or _newer(EXT, [src, LIB, os.path.join(HERE, "..", "include", "fluidnet_hip.h"), __file__])):
        return EXT
    import torch
    from torch.utils import cpp_extension as ce
    tdir = os.path.dirname(torch.__file__)
    inc = ce.include_paths() + [sysconfig.get_paths()["include"], "/opt/rocm/include"]
    cmd = ["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-fvisibility=hidden", "-D__HIP_PLATFORM_AMD__=1", "-DUSE_ROCM=1",
           "-DTORCH_EXTENSION_NAME=fluidnet_cpp", "-DTORCH_API_INCLUDE_EXTENSION_H",
           f"-D_GLIBCXX_USE_CXX11_ABI={int(torch._C._GLIBCXX_USE_CXX11_ABI)}"]
    cmd += [f"-isystem{i}" for i in inc]
    cmd += [src, "-o", EXT, f"-L{HERE}", "-lfluidnet_hip", f"-L{tdir}/lib", "-lc10", "-ltorch_cpu", "-ltorch", "-ltorch_python",
            "-lc10_hip", "-ltorch_hip", "-L/opt/rocm/lib", "-lamdhip64",
            "-Wl,-rpath,$ORIGIN", f"-Wl,-rpath,{tdir}/lib", "-Wl,-rpath,/opt/rocm/lib"]
    if verbose:
        print(" ".join(cmd))
    subprocess.check_call(cmd)
    return EXT


def build_examples(force=False, verbose=False):
    """examples/cabi_plume.bin: a C++ host on the C ABI alone (no torch); run by tests/test_abi.py on the GPU box."""
    repo = os.path.dirname(HERE)
    src = os.path.join(repo, "examples", "cabi_plume.cpp")
    out = os.path.join(repo, "examples", "cabi_plume.bin")
    if not os.path.exists(src) or not (force or _newer(out, [src, LIB, os.path.join(repo, "include", "fluidnet_hip.h")])):
        return out
    cmd = [HIPCC, "--offload-arch=gfx950", "-O2", "-I", os.path.join(repo, "include"), src, "-L", HERE, "-lfluidnet_hip",
           "-Wl,-rpath,$ORIGIN/../fluidnet_cxx_amd", "-Wl,-rpath,/opt/rocm/lib", "-o", out]
    if verbose:
        print(" ".join(cmd))
    subprocess.check_call(cmd)
    return out


def build_all(force=False, verbose=False):
    build_lib(force, verbose)
    build_ext(force, verbose)
    build_examples(force, verbose)


if __name__ == "__main__":
    build_all(force="--force" in sys.argv, verbose=True)
