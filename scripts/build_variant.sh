#!/bin/bash
# A/B helper: variants/libepx_<name>.so = the library with nuts_duo.hip recompiled under extra flags.
# usage: scripts/build_variant.sh <name> <extra hipcc flags...>      (the other objects come from csrc/build, up to date)
name=$1; shift
exec "$(dirname "$0")/../ep-stan_amd/csrc/build.sh" variant NAME="$name" TUS=nuts_duo EXTRA="$*"
