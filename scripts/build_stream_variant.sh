#!/bin/bash
# A/B helper: variants/libepx_<name>.so = the library with nuts_stream.hip recompiled under extra flags, the C5 shape only
# (-DEPX_STREAM_MIN: NV = 7, DPB = 128; seconds instead of minutes).  The other objects come from csrc/build, up to date.
# usage: scripts/build_stream_variant.sh <name> <extra hipcc flags...>
name=$1; shift
exec "$(dirname "$0")/../ep-stan_amd/csrc/build.sh" variant NAME="$name" TUS=nuts_stream EXTRA="-DEPX_STREAM_MIN $*"
