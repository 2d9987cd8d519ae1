#!/bin/bash
# A/B of two builds of libfluidnet_hip.so on ONE box (boxes differ by a few per cent, so do runs minutes apart):
#   here:     [UNIT=fnx_jacobi] [ABFLAGS=-DX=1] tools/ab_libs.sh build <name> [git-rev]   -> variants/libfluidnet_hip_<name>.so from the working
#             tree's (or the revision's) csrc/$UNIT.hip (default fnx_cnn) and the other objects of the current build
#             tools/ab_libs.sh keep <name>        -> the current build whole, for a change that spans units or the binding: libfluidnet_hip.so
#             as variants/libfluidnet_hip_<name>.so and fluidnet_cpp.so as variants/fluidnet_cpp_<name>.so
#   GPU box:  tools/ab_libs.sh run <rounds> <name>... -- <command>     (round-robin over the builds; prints the command's output; a
#             build kept with its binding runs with its binding)
set -u
cd "$(dirname "$0")/.."
V=variants
if [ "$1" = build ]; then
  mkdir -p $V
  U=${UNIT:-fnx_cnn}
  extra=""; [ $U != fnx_cnn ] && [ $U != fnx_fluidnet ] && [ $U != fnx_slab ] && [ $U != fnx_peer ] && extra="-ffp-contract=off"    # (build.py's per-unit flags)
  src=fluidnet_cxx_amd/csrc/$U.hip
  if [ $# -ge 3 ]; then git show $3:$src > fluidnet_cxx_amd/csrc/.ab_$2.hip; src=fluidnet_cxx_amd/csrc/.ab_$2.hip; fi
  /opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -fno-fast-math -fno-slp-vectorize -Wno-unused-value $extra ${ABFLAGS:-} \
      -c $src -o $V/${U}_$2.o 2>/dev/null &&
  objs=$(ls fluidnet_cxx_amd/build/*.o | grep -v "/$U.o" | grep -v "hip-amdgcn\|host-x86") &&
  /opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o $V/libfluidnet_hip_$2.so $objs $V/${U}_$2.o && echo built $2
  rm -f $V/${U}_$2.o fluidnet_cxx_amd/csrc/.ab_$2.hip
elif [ "$1" = keep ]; then
  mkdir -p $V
  cp fluidnet_cxx_amd/libfluidnet_hip.so $V/libfluidnet_hip_$2.so && cp fluidnet_cxx_amd/fluidnet_cpp.so $V/fluidnet_cpp_$2.so && echo kept $2
else
  n=$2; shift 2
  names=()
  while [ "$1" != "--" ]; do names+=("$1"); shift; done
  shift
  cp fluidnet_cxx_amd/libfluidnet_hip.so /tmp/libfluidnet_hip.keep
  cp fluidnet_cxx_amd/fluidnet_cpp.so /tmp/fluidnet_cpp.keep
  for i in $(seq $n); do
    for v in "${names[@]}"; do
      cp $V/libfluidnet_hip_$v.so fluidnet_cxx_amd/libfluidnet_hip.so
      if [ -f $V/fluidnet_cpp_$v.so ]; then cp $V/fluidnet_cpp_$v.so fluidnet_cxx_amd/fluidnet_cpp.so; else cp /tmp/fluidnet_cpp.keep fluidnet_cxx_amd/fluidnet_cpp.so; fi
      echo -n "$v: "; "$@" 2>&1 | tail -n +1
      rc=${PIPESTATUS[0]}
      # a command that failed (a fault, a time limit) ends the run: nothing more is started on that GPU
      if [ $rc -ne 0 ]; then echo "$v: exit status $rc, stopping"; break 2; fi
    done
  done
  cp /tmp/libfluidnet_hip.keep fluidnet_cxx_amd/libfluidnet_hip.so
  cp /tmp/fluidnet_cpp.keep fluidnet_cxx_amd/fluidnet_cpp.so
  exit ${rc:-0}
fi
