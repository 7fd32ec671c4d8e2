#!/bin/bash
# Builds libepx.so and variants/libepx_fence.so for gfx950 (cross-compiles without a GPU): runs the Makefile beside it,
# which states what the library is made of.  EPX_STAMPS=1 adds the diagnostic variants/libepx_stamps.so.
# Arguments, if any, go to make in place of the default goal (the scripts/ helpers: build.sh variant NAME=... TUS=... EXTRA=...).
set -e
cd "$(dirname "$0")"
jobs=${MAX_JOBS:-12}          # a default build has 11 compiles; never sized by the machine's core count
[ "$jobs" -le 16 ] || jobs=16
[ $# -gt 0 ] || set -- all
[ "$EPX_STAMPS" = "1" ] && set -- "$@" stamps
exec make -j"$jobs" "$@"
