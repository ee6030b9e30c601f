#!/bin/bash
# What the `.count()` kernel does outside its step loop (round 14): the library with tools/variants/gram4_edges.patch applied to a copy of
# gram4_kernels.hip and compiled with -DG4_EDGES — every wave stamps wall_clock64 at entry, when its first step's text has arrived, when its
# last region is done and at exit, and its lane 0 writes the stamps to a buffer (a measuring build: counts are right, a step costs one branch more).
#   build (no GPU needed):   bash tools/gram4_edges.sh build      -> abtmp/g4edges/libdaachorse_amd.so   (needs daachorse_amd/build/)
#   on the GPU:              bash tools/gram4_edges.sh run [mib] [launches] [name=value ...]
R=$(cd "$(dirname "$0")/.." && pwd); V=$R/abtmp/g4edges
if [ "$1" = build ]; then
  set -e
  mkdir -p $V/s && cp $R/daachorse_amd/csrc/gram4_kernels.hip $V/s/
  (cd $V/s && patch -s -p0 gram4_kernels.hip < $R/tools/variants/gram4_edges.patch)
  /opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -DG4_EDGES -I$R/daachorse_amd/csrc -I$R/include -c $V/s/gram4_kernels.hip -o $V/g4.o
  /opt/rocm/bin/hipcc --offload-arch=gfx950 -fPIC -shared -o $V/libdaachorse_amd.so $(ls $R/daachorse_amd/build/*.o | grep -v "/gram4_kernels.hip.o") $V/g4.o
  ls -la $V/libdaachorse_amd.so
else
  shift
  python $R/tools/gram4_edges.py "$@" 2>&1 | grep -v amdgpu.ids
fi
