#!/bin/bash
# Build a variant of the library with extra flags for some translation units:
#   scripts/dev/build_variant.sh NAME "-DPGP_ORDER=1 ..." [pair|expander]   -> scripts/dev/ab/NAME.so
# (the other objects come from the in-tree build; run python -m safeopt_amd.build first;
# no third argument: sweep.hip and sweep_pair.hip are rebuilt; "pair": only sweep_pair.hip;
# "expander": only expander.hip, e.g. stats "-DEXPM_STATS" expander for scripts/dev/expm_stats.py)
set -e
cd "$(dirname "$0")/../.."
NAME=$1; FLAGS=$2; ONLY=$3
C=safeopt_amd/csrc; O=/tmp/variant_$NAME; mkdir -p $O scripts/dev/ab
BASE="--offload-arch=gfx950 -O3 -std=c++17 -fPIC -I include -I $C -Wall -Wno-unused-function -Wno-inline-asm"
case "$ONLY" in
  expander) REBUILT="expander" ;;
  pair) REBUILT="sweep_pair" ;;
  *) REBUILT="sweep sweep_pair" ;;
esac
for u in $REBUILT; do
  EXTRA=""; [ $u = sweep ] && EXTRA="-mllvm -amdgpu-spill-vgpr-to-agpr=0"
  /opt/rocm/bin/hipcc $BASE $FLAGS $EXTRA -c $C/$u.hip -o $O/$u.o &
done
wait
OBJS=""
for o in $C/*.o; do
  u=$(basename $o .o)
  case " $REBUILT " in *" $u "*) OBJS="$OBJS $O/$u.o" ;; *) OBJS="$OBJS $o" ;; esac
done
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o scripts/dev/ab/$NAME.so $OBJS -ldl
echo built scripts/dev/ab/$NAME.so
