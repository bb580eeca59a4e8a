#!/bin/bash
# diagnostic build (-DVS_STAMPS: clock stamps by one thread of a workgroup or one lane of a wave) of the library into
# scratch/stamps/ of this tree (git-ignored; never the product library).  The stamp readers in this directory load it
# through pkg.LIB_PATH.  "build_stamps.sh ends" builds the light mode of the prefilter sweep instead (-DVS_F32F_ENDS: a wave's
# start, loop end and end, nothing inside its loop) into scratch/ends/, for f32fstamps.py --ends.
set -e
ROOT=$(cd "$(dirname "$0")/../.." && pwd)
cd "$ROOT/hai-25-rag-on-edge_amd/csrc"
HIPCC=${HIPCC:-/opt/rocm/bin/hipcc}
if [ "$1" = ends ]; then O=$ROOT/scratch/ends; DEF=-DVS_F32F_ENDS; else O=$ROOT/scratch/stamps; DEF=-DVS_STAMPS; fi
mkdir -p $O
F="--offload-arch=gfx950 -O3 -std=c++17 -fPIC -fvisibility=hidden -Wno-unused-function $DEF"
for f in *.hip; do $HIPCC $F -c $f -o $O/${f%.hip}.o & done
$HIPCC -O3 -std=c++17 -fPIC -fvisibility=hidden -x c++ -c vs_host.cpp -o $O/vs_host.o &
wait
$HIPCC --offload-arch=gfx950 -shared -o $O/libvsearch_hip.so $O/*.o -lpthread
ls -la $O/libvsearch_hip.so
