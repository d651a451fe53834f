#!/bin/bash
# Build a variant of the library with extra -D flags on ONE translation unit (a unit of fateavatar_amd/csrc/Makefile):
#   tools/diag/build_variant_file.sh <name> <fr_preprocess|fr_blend_bwd|...> -DFR_DIAG_... ->  .ab/libfr_<name>.so
# A full build of its own through that Makefile (objects under /tmp).  fr_diag.hpp lists the switches.
set -e
name=$1; unit=$2; shift; shift
cd "$(dirname "$0")/../.."
mkdir -p .ab
make -C fateavatar_amd/csrc -B -s -j8 OBJ=/tmp/fr_$name OUT=../../.ab/libfr_$name.so EXTRA_$unit="$*"
echo built .ab/libfr_$name.so
