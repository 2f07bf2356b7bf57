#!/bin/bash
# Build a variant of the library next to the default one, for A/B runs on one GPU box (tools/ab.py):
#   tools/build_variant.sh <name> [extra hipcc flags, e.g. -DSIPX_F64_VEC=4]   ->  setintersectionprojection.jl_amd/libsipx_<name>.so
# Select it with SIPX_LIBRARY=<path> (host.py) or pass <name> to tools/ab.py.  `git stash; tools/build_variant.sh prev; git stash pop`
# gives the committed state as the baseline of an uncommitted change.
# The build is the Makefile's own, with another output name and an object directory of its own.
set -e
name=$1; shift
root=$(cd "$(dirname "$0")/.." && pwd)
out=$(mktemp -d)
make -j"${MAX_JOBS:-8}" -C "$root/setintersectionprojection.jl_amd/csrc" OUT="../libsipx_$name.so" OBJDIR="$out" EXTRA="$*"
rm -rf "$out"
echo "built libsipx_$name.so"
