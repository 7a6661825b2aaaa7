// TEST HARNESS ONLY: the host-side API file, floating.hip and floating_exact.hip (the exact body sums of floating bodies), compiled
// for the host through the stand-in tests/hostemu/hip/hip_runtime.h (read its header).  Built by tests/test_floating_exact_hostemu.py
// into tests/hostemu/_build/ with -DFLOAT_MAX_BLOCKS=4, so that the grid-stride loop runs several rounds at a small row count, and
// with the launches of both files rewritten into _build/floating_exact_emu_*.inc: the kernels meet in shuffles and barriers, so
// their blocks run as teams of fibres (SPHX_LAUNCH_WAVES).  LDS atomics are the plain operation: one fibre runs at a time.
#include <hip/hip_runtime.h>
thread_local dim3 blockIdx, threadIdx, blockDim, gridDim;
#include "../../gpusph_amd/csrc/sphx_api.hip"
#include "floating_exact_emu_step.inc"
#include "floating_exact_emu_sums.inc"
