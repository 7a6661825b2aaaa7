// TEST HARNESS ONLY: the host-side API file, filters.hip (density filters and the post-processing engines) and gages.hip (the wave
// gages), compiled for the host through the stand-in tests/hostemu/hip/hip_runtime.h (read its header).  Built by
// tests/test_sa_postprocess_hostemu.py into tests/hostemu/_build/, with the launches of the two files rewritten into
// _build/filters_emu.inc and _build/gages_emu.inc: the post-processing kernels are one thread per particle (serial launches), the
// two reducing kernels of the gages meet in ballots and shuffles, so their blocks run as teams of fibres (SPHX_LAUNCH_WAVES).
#include <hip/hip_runtime.h>
thread_local dim3 blockIdx, threadIdx, blockDim, gridDim;
#include "../../gpusph_amd/csrc/sphx_api.hip"
#include "filters_emu.inc"
#include "gages_emu.inc"
