// TEST HARNESS ONLY: the host-side API file and diagnostics.hip (the save-time diagnostics), compiled for the host through the
// stand-in tests/hostemu/hip/hip_runtime.h (read its header).  Built by tests/test_diagnostics_hostemu.py into
// tests/hostemu/_build/ with -DDIAG_MAX_BLOCKS=8, so that the grid-stride loop runs several rounds at a small particle count,
// and with the launches rewritten into _build/diagnostics_emu.inc: both kernels meet in shuffles (and the first in a barrier),
// so their blocks run as teams of fibres (SPHX_LAUNCH_WAVES).
#include <hip/hip_runtime.h>
thread_local dim3 blockIdx, threadIdx, blockDim, gridDim;
#include "../../gpusph_amd/csrc/sphx_api.hip"
#include "diagnostics_emu.inc"
