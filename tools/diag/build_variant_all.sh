#!/bin/bash
# Build a variant of the WHOLE library with extra -D flags on every translation unit (switches that live in fr_common.hpp):
#   tools/diag/build_variant_all.sh <name> -DFR_PRE_WG=64 ...   ->  .ab/libfr_<name>.so
set -e
name=$1; shift
cd "$(dirname "$0")/../.."
mkdir -p .ab
make -C fateavatar_amd/csrc -B -s -j8 OBJ=/tmp/fr_$name OUT=../../.ab/libfr_$name.so EXTRA="$*"
echo built .ab/libfr_$name.so
