#!/bin/bash
# Builds the C-ABI shared library of HIP kernels for gfx950 (MI355X).  No GPU needed to compile.
set -e
cd "$(dirname "$0")"
HIPCC=${HIPCC:-/opt/rocm/bin/hipcc}
FLAGS="--offload-arch=gfx950 -O3 -std=c++17 -fPIC -Wno-unused-value -munsafe-fp-atomics $CS_EXTRA_FLAGS"
# An object is rebuilt when its source, any header here or any public header is newer: every source includes the header it implements.
stale() {
  [ ! -f "$2" ] && return 0
  for d in "$1" *.h ../../include/*.h; do
    [ "$d" -nt "$2" ] && return 0
  done
  return 1
}
OBJS=""
PIDS=""
for f in gemm gemm_stream thin attention norm elementwise roialign_loss adamw preprocess det_post roi_extract det_assign det_loss det_mask det_proposal conv3x3 batchnorm runtime; do
  if stale "$f.hip" "_obj_$f.o"; then
    $HIPCC $FLAGS -c "$f.hip" -o "_obj_$f.o" &
    PIDS="$PIDS $!"
  fi
  OBJS="$OBJS _obj_$f.o"
done
FAILED=0
for p in $PIDS; do
  wait "$p" || FAILED=1
done
if [ "$FAILED" != 0 ]; then
  echo "build.sh: a compile failed, nothing is linked" >&2
  exit 1
fi
g++ -O2 -fPIC -std=c++17 -c errors.cpp -o _obj_errors.o
$HIPCC --offload-arch=gfx950 -shared -fPIC $OBJS _obj_errors.o -o libclipself_hip.so
echo "built $(pwd)/libclipself_hip.so"
