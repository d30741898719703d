#!/bin/bash
# An experimental build of the library with extra compiler flags (the product sources hold no experiment switch any more -- tests/test_build_properties.py --: a
# variant is a patch to the sources plus, maybe, generic flags such as -mllvm options): stenos_amd/lib/exp/libstenos_<name>.so (git-ignored, travels
# to the GPU box; tools/exp_variants.sh and STENOS_LIB_PATH select it).  usage: tools/build_variant.sh <name> [-DSTENOS_...=.. ...]
# The product's Makefile does the work (ENCODE_FLAGS and DECODE_FLAGS in the environment replace its per-file flags); a variant
# keeps its objects, so building it again after a change compiles the changed files only.
set -e
name="$1"; shift
here="$(cd "$(dirname "$0")/.." && pwd)"
make -s -j8 -C "$here/stenos_amd/csrc" LIB="$here/stenos_amd/lib/exp/libstenos_$name.so" EXTRA="$*"
echo "built libstenos_$name.so"
