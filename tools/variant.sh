#!/bin/bash
# usage: tools/variant.sh <name> <tu> [-DFLAG ...] -- a variant of the library that differs in ONE instance translation unit
# (e.g. kmr_inst_skc1) compiled with extra flags: kmernator_amd/csrc/build/v/<name>.so (development aid for tools/ab.sh).
# An instance unit kmr_inst_<group><w> is kmr_inst.hip with -DKMR_INST_<GROUP> -DKMR_INST_W=<w>, as in the Makefile (without its
# SKC_FLAGS: pass them as extra flags to have them); any other unit is <tu>.hip.
name=$1; tu=$2; shift 2
cd $(dirname $0)/../kmernator_amd/csrc && mkdir -p build/v
FLAGS="-O3 -std=c++17 -fPIC --offload-arch=gfx950 -munsafe-fp-atomics -w"
src=$tu.hip; defs=
if [[ $tu =~ ^kmr_inst_([a-z]+)([1-4])$ ]]; then src=kmr_inst.hip; defs="-DKMR_INST_${BASH_REMATCH[1]^^} -DKMR_INST_W=${BASH_REMATCH[2]}"; fi
/opt/rocm/bin/hipcc $FLAGS $defs "$@" -c -o build/v/${name}_$tu.o $src || exit 1
OBJS=$(ls build/*.o | grep -v "/$tu.o")
/opt/rocm/bin/hipcc $FLAGS -shared -Wl,-z,defs -o build/v/$name.so $OBJS build/v/${name}_$tu.o -ldl && echo built build/v/$name.so
