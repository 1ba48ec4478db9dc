#!/bin/bash
# Build an A/B variant of libonepose_hip.so:  tools/build_variant.sh <name> <git rev> <csrc file> [<csrc file> ...]
# = the working tree's csrc with the listed files taken from <git rev>; result: onepose_st_amd/lib/variants/libonepose_hip_<name>.so
# EXTRA="-D..." in the environment adds compiler flags; <git rev> may be "-" with no files (working tree + EXTRA only).
# (load it with OPHIP_LIB=<path>; `tools/box.sh <name> ab:R:S:variants` runs variants interleaved on one box).  Variants are scratch: git-ignored like every .so.
# A first <csrc file> that is the <name> of any `satellite` line of csrc/Makefile is a goal, not a file: the variant is then that satellite
# library, libonepose_<goal>.so (load it with its OP*_LIB variable, onepose_st_amd/cabi.py LIBRARIES), e.g. the seeded faults of tests/test_gpu_sfm_tracks.py:
#   EXTRA=-DOPSFT_FAULT_TIE_INITIAL_ORDER tools/build_variant.sh tie - sfm_tracks   -> lib/variants/libonepose_sfm_tracks_tie.so
set -e
name=$1; rev=$2; shift 2
root=$(cd $(dirname $0)/.. && pwd)
lib=libonepose_hip; var=OUT
# a goal is the <name> of a `satellite` line of csrc/Makefile; its tag names the variable that takes the output path
tag=$(sed -n "s/^\$(eval \$(call satellite,\([A-Z]*\),[a-z]*,$1))\$/\1/p" $root/onepose_st_amd/csrc/Makefile)
if [ -n "$tag" ]; then lib=libonepose_$1; var=${tag}_OUT; shift; fi
tmp=$(mktemp -d)
mkdir -p $tmp/onepose_st_amd $root/onepose_st_amd/lib/variants
cp -r $root/onepose_st_amd/csrc $tmp/onepose_st_amd/csrc
cp -r $root/include $tmp/include
rm -rf $tmp/onepose_st_amd/csrc/build
[ "$rev" = "-" ] || for f in "$@"; do git -C $root show $rev:onepose_st_amd/csrc/$f > $tmp/onepose_st_amd/csrc/$f; done
out=$root/onepose_st_amd/lib/variants/${lib}_$name.so
make -C $tmp/onepose_st_amd/csrc -j8 EXTRA="$EXTRA" $var=$out $out > $tmp/build.log 2>&1 || { tail -20 $tmp/build.log; exit 1; }
rm -rf $tmp
echo built $out
