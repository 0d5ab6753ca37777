#!/bin/bash
# Build exp/ab/librsp_<name>.so from the frame-chain units (K1, K2, K3, the auxiliary kernels, their two
# shared headers) and plan sources of git revision REV (default HEAD), against the current other
# headers and the other objects of the shipped build: the "before" side of an A/B (tools/ab.sh).
# REV must be a revision that has the per-stage units and the plan units (rsp_plan.h, rsp_plan_cfar.cpp,
# rsp_plan_calls.cpp); an older one is built whole from an export of it (git archive, make).
# usage: tools/ab/build_head_variant.sh NAME [REV]
set -e
name=$1; rev=${2:-HEAD}
C=radar-signal-simulation-and-target-detection_amd/csrc
d=/tmp/rsp_variant_$name
units="rsp_k1.hip rsp_k2.hip rsp_k3.hip rsp_frame_aux.hip rsp_plan.cpp rsp_plan_cfar.cpp rsp_plan_calls.cpp"
rm -rf $d && mkdir -p $d exp/ab
for f in $units rsp_plan.h rsp_internal.h rsp_device.h rsp_fft_passes.h; do git show $rev:$C/$f > $d/$f; done
F="-O3 -std=c++17 -fPIC --offload-arch=gfx950 -Iinclude -I$d -I$C -Wall -Wno-unused-function"
objs=""
for u in $units; do
  /opt/rocm/bin/hipcc $F -x hip -c $d/$u -o $d/$u.o &
  objs="$objs $d/$u.o"
done
wait
rest=""
for o in $C/build/*.o; do
  case " $units " in *" $(basename $o .o) "*) ;; *) rest="$rest $o" ;; esac
done
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -o exp/ab/librsp_$name.so $objs $rest -lz -lpthread
echo built exp/ab/librsp_$name.so from $rev
