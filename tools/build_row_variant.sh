#!/bin/bash
# tools/build_row_variant.sh <mlpw|qkvw|qkv640w|gegluw> <name> [VAR=value ...] [-- extra hipcc flags]: a library
# tools/ubench/v_<name>/libidf_gfx950.so whose row kernel of that family is built on a stream generated with the given options of its
# tools/gen_<kernel>_stream.py (<PREFIX>_LA, _PRE_DMA, _MAXV, _NO_EPI / _NO_DMA = 1 ...; prefixes MW, QW, QM, GW); the other objects
# are the shipped ones (build.sh first).
#   LD_LIBRARY_PATH=tools/ubench/v_<name> tools/ubench/mlp_harness 5
#   IDF_LIB_PATH=tools/ubench/v_<name>/libidf_gfx950.so python tools/geglu_ab.py
set -e
kern=$1; name=$2; shift 2
case $kern in
  mlpw) file=mlp_fused; macro=MLPW_STREAM_INC ;;
  qkvw) file=qkv_fused; macro=QKVW_STREAM_INC ;;
  qkv640w) file=qkv640_fused; macro=QKV640W_STREAM_INC ;;
  gegluw) file=geglu_fused; macro=GEGLUW_STREAM_INC ;;
  *) echo "unknown kernel family $kern" >&2; exit 2 ;;
esac
envs=""; while [ $# -gt 0 ] && [ "$1" != "--" ]; do envs="$envs $1"; shift; done
[ "$1" = "--" ] && shift
root="$(cd "$(dirname "$0")/.." && pwd)"
cd "$root/instancediffusion_amd/csrc"
mkdir -p build "$root/tools/ubench/v_$name"
env $envs python "$root/tools/gen_${kern}_stream.py" -o build/${kern}_$name.inc
FLAGS="--offload-arch=gfx950 -O3 -std=c++17 -fPIC -fno-gpu-rdc -Wno-unused-result -mllvm -amdgpu-mfma-vgpr-form"
hipcc $FLAGS -D$macro="\"build/${kern}_$name.inc\"" "$@" -c $file.hip -o build/${file}_$name.o
OBJS=""
for f in gemm_conv gemm_big mlp_fused qkv_fused qkv640_fused geglu_fused attention attention4 attention4w attention8 norms scaleu misc convnext; do
  [ $f = $file ] || OBJS="$OBJS build/$f.o"
done
hipcc --offload-arch=gfx950 -shared -fPIC $OBJS build/${file}_$name.o -o "$root/tools/ubench/v_$name/libidf_gfx950.so"
echo built v_$name
