#!/bin/bash
# usage: tools/experiments/build_variant.sh NAME "-DFLAG=1 ..." object1 [object2 ...]   -> easykv_amd/csrc/variants/lib_NAME.so
# (A/B builds for the experiment drivers in this directory: select one with EASYKV_HIP_LIB=...; *.so is git-ignored but travels with gpurun;
#  an object is named as the library's build names it: an instance of easykv_amd/csrc/ekv_instances.def, e.g. ekv_attn_decode_d128_plain,
#  or a .hip file's base name; objects of the untouched sources are reused from csrc/obj)
set -e
ROOT=$(cd "$(dirname "$0")/../.." && pwd)
cd $ROOT/easykv_amd/csrc
NAME=$1; FLAGS=$2; shift 2
mkdir -p /tmp/ekv_var/obj_$NAME $ROOT/easykv_amd/csrc/variants
OBJS=""
for o in obj/*.o; do
  b=$(basename $o .o); use=$o
  for f in "$@"; do if [ "$b" == "$(basename $f .hip)" ]; then use=/tmp/ekv_var/obj_$NAME/$b.o; fi; done
  OBJS="$OBJS $use"
done
for f in "$@"; do
  b=$(basename $f .hip)
  # the source and switches of the object, as easykv_amd/_build.py derives them
  SRC=$(cd $ROOT && python3 -c "import sys; from easykv_amd import _build; print(' '.join(dict(_build.objects())[sys.argv[1]]))" $b)
  /opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -fPIC -Wall -Wno-unused-function $FLAGS -c $SRC -o /tmp/ekv_var/obj_$NAME/$b.o &
done
wait
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC $OBJS -o $ROOT/easykv_amd/csrc/variants/lib_$NAME.so
echo built easykv_amd/csrc/variants/lib_$NAME.so
