#!/bin/bash
# Dev tool: build A/B variants of liblincheck.so with -D switches into
# gpurun-shipped build dirs: tools/variants/<name>/liblincheck.so
#   tools/build_variants.sh <name> [-DSWITCH=value ...]
# (then tools/ab_bench.sh benches every directory under tools/variants)
# Built by the library's own Makefile (its source list, its flags plus the
# switches), with the build id "variant".
set -e
cd "$(dirname "$0")/.."
name=$1; shift
out=$PWD/tools/variants/$name
mkdir -p "$out"
make -C jepsen/etcd_amd/csrc BUILD="$out/obj" OUT="$out/liblincheck.so" EXTRA="$*" BUILD_ID=variant
rm -rf "$out/obj"
