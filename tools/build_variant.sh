#!/bin/bash
# build_variant.sh NAME "extra flags": a tools-build variant library robust-dynrf_amd/abl_NAME.so (all translation units of the
# Makefile's SRCS recompiled with the extra flags, e.g. -DRDRF_APP_F32)
cd "$(dirname "$(readlink -f "$0")")/../robust-dynrf_amd/csrc" || exit 1
CX="-O3 -std=c++17 -fPIC -munsafe-fp-atomics -mllvm -disable-promote-alloca-to-lds=1 --offload-arch=gfx950 -I../../include -I. -Wno-unused-result -DRDRF_TOOLS $2"
SRCS=$(sed -n 's/^SRCS *= *//p' Makefile)
[ -n "$SRCS" ] || { echo "no SRCS in the Makefile"; exit 1; }
mkdir -p /tmp/var_$1
for f in $SRCS; do
  /opt/rocm/bin/hipcc $CX -c $f -o /tmp/var_$1/${f%.hip}.o 2>/dev/null &
done
wait
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC /tmp/var_$1/*.o -o ../abl_$1.so && echo built abl_$1.so
