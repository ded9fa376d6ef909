#!/bin/bash
# tools/build_variant.sh NAME "-DFLAG=1 ..." [SOURCE] : an A/B build of the multiply kernel -> build/variants/NAME.so (tools only).
# Lab switches (EFFORT_CUT_FINE, EFFORT_LEAN_STAMPS, EFFORT_ABLATE_*) need -DEFFORT_LAB among the flags; without it the variant is a
# product build (no stamps), linked against the tree's product objects -- with it, against the lab ones.  SOURCE: another
# bucket_mul.hip to compile in place of the tree's (say, an earlier commit's, for an A/B of two versions of the kernel).
# The objects it links are the Makefile's own list (effort_amd/csrc/Makefile, target `variant`).
set -e
SRC=${3:+$(realpath "$3")}
cd "$(dirname "$0")/../effort_amd/csrc"
make -s variant VARIANT="$1" VARIANT_FLAGS="$2" ${SRC:+VARIANT_SRC="$SRC"}
