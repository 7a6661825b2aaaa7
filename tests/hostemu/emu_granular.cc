// TEST HARNESS ONLY: the host-side API file and granular.hip (the effective-pressure Jacobi solver of the GRANULAR rheology),
// compiled for the host through the stand-in tests/hostemu/hip/hip_runtime.h (read its header).  Built by
// tests/test_granular_hostemu.py into tests/hostemu/_build/, with the launches of granular.hip rewritten into
// _build/granular_emu.inc: its kernels reduce and compact by wave operations, so every block runs as a team of fibres
// (SPHX_LAUNCH_WAVES), the one-thread stop test as it is.
#include <hip/hip_runtime.h>
thread_local dim3 blockIdx, threadIdx, blockDim, gridDim;
#define __ballot(b) __builtin_amdgcn_ballot_w64(b)
#define __popcll(x) __builtin_popcountll(x)
#include "../../gpusph_amd/csrc/sphx_api.hip"
#include "granular_emu.inc"
