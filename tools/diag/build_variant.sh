#!/bin/bash
# Build a variant of the library with extra -D flags on the three per-tile units (fr_tile_sort, fr_blend_fwd, fr_blend_bwd):
#   tools/diag/build_variant.sh <name> -DFR_DIAG_TRACE ...   ->  .ab/libfr_<name>.so     (fr_diag.hpp lists the switches)
# A full build of its own through the library's Makefile (objects under /tmp), which alone knows the units and their flags.
set -e
name=$1; shift
cd "$(dirname "$0")/../.."
mkdir -p .ab
make -C fateavatar_amd/csrc -B -s -j8 OBJ=/tmp/fr_$name OUT=../../.ab/libfr_$name.so \
    EXTRA_fr_tile_sort="$*" EXTRA_fr_blend_fwd="$*" EXTRA_fr_blend_bwd="$*"
echo built .ab/libfr_$name.so
