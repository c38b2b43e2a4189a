#!/bin/bash
# build the library with the kernel resource remarks and print those of one kernel, by default the C2 extract kernel (development aid).
# The build goes through the Makefile (every instance object) in a scratch copy of csrc/, so the product library is left alone.
src=$(cd $(dirname $0)/../kmernator_amd/csrc && pwd) || exit 1
out=${BUILD_RES_DIR:-$(mktemp -d)}
mkdir -p $out/kmernator_amd/csrc $out/include && cp $src/Makefile $src/*.hip $src/*.hpp $out/kmernator_amd/csrc && cp $src/../../include/kmernator_amd.h $out/include || exit 1
flags=$(make -s -C $src --eval 'print-flags: ; @echo $(HIPFLAGS)' print-flags)
make -C $out/kmernator_amd/csrc HIPFLAGS="$flags -Rpass-analysis=kernel-resource-usage" > $out/build_res.log 2>&1 || { grep -m3 "error" -A5 $out/build_res.log; exit 1; }
pat=${1:-_ZN3kmr14extract_kernelILi1ELb0ENS_8LinearOpILi1ELb0ELb0EEELb0E}
grep -A9 "Function Name: $pat" $out/build_res.log | grep -E "Name|SGPRs|VGPRs|Scratch" | sed 's/.*remark: *//'
echo "(log and library: $out)"
