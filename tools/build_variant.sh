#!/bin/bash
# builds a variant of libingvio_hip.so into build_var/<name>/ with extra hipcc flags (e.g. -DINGVIO_DBG_STAMPS for the
# shader-clock probes); select it at run time with INGVIO_HIP_LIB=<repository>/build_var/<name>/libingvio_hip.so
NAME=$1; shift
ROOT=$(cd "$(dirname "$0")/.." && pwd)
OUT=$ROOT/build_var/$NAME
mkdir -p "$OUT"
cd "$ROOT/ingvio_amd/csrc"
OBJS=""
# the sources and their per-file flags are build.py's (HIP_SOURCES, EXTRA_FLAGS): one "<file> <flags>" line each
while read -r f EXTRA; do
  /opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -Wno-unused-value $EXTRA "$@" -c $f -o "$OUT/${f%.hip}.o" &
  OBJS="$OBJS $OUT/${f%.hip}.o"
done < <(cd "$ROOT" && python3 -c 'from ingvio_amd import build
for s in build.HIP_SOURCES: print(s, *build.EXTRA_FLAGS.get(s, []))')
wait
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o "$OUT/libingvio_hip.so" $OBJS "$ROOT/ingvio_amd/lib/build_id.o"      # the regular build's id object (ingvio_build_id): run python ingvio_amd/build.py first
ls -la "$OUT/libingvio_hip.so"
