#!/bin/bash
# Robustness check of the kernels' hand-written assembly against the compiler's schedule (round 5: this is how the missing
# wait states in front of logistic_pair_lean's inline assembly were found): build EVERY kernel translation unit under another
# machine scheduler into variants/libepx_sched_<name>.so, then run the parity tests against that library on a GPU box:
#   scripts/schedule_robustness.sh minreg -mllvm -amdgpu-sched-strategy=iterative-minreg          (here: builds)
#   EPX_LIB=$PWD/variants/libepx_sched_minreg.so python -m pytest tests -m gpu -q \
#       --deselect tests/test_gpu_parity.py::test_native_library_is_loaded                          (on the box)
# Results must not depend on the schedule: every draw-by-draw test passes under iterative-minreg and max-ilp.
name=$1; shift
# (TUS reaches make unexpanded: the Makefile's own list of the kernel translation units)
exec "$(dirname "$0")/../ep-stan_amd/csrc/build.sh" variant NAME="sched_$name" 'TUS=$(KERNEL_TUS)' EXTRA="$*"
