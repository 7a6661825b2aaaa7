// TEST HARNESS ONLY: the host-side API file and floating.hip (the rigid-body dynamics of floating bodies), compiled for the host
// through the stand-in tests/hostemu/hip/hip_runtime.h (read its header).  Built by tests/test_floating_hostemu.py into
// tests/hostemu/_build/ with -DFLOAT_MAX_BLOCKS=4, so that the grid-stride loop runs several rounds at a small row count, and with
// the launches rewritten into _build/floating_emu.inc: the kernels meet in shuffles (and the first in a barrier), so their blocks
// run as teams of fibres (SPHX_LAUNCH_WAVES).
#include <hip/hip_runtime.h>
thread_local dim3 blockIdx, threadIdx, blockDim, gridDim;
#include "../../gpusph_amd/csrc/sphx_api.hip"
#include "floating_emu.inc"

// "device" memory is host memory here: both images of the rigid-body table, for the tests of what sphx_rb_flush leaves on the device
extern "C" unsigned emu_rb_tables(sphx_ctx *ctx, void *dev_out, void *host_out, void *stream)
{
	if (sphx_rb_flush(ctx, (hipStream_t)stream) != SPHX_OK) return 0u;
	if (dev_out) memcpy(dev_out, ctx->rb_dev, sizeof(RbParams));
	if (host_out) memcpy(host_out, &ctx->rb_host, sizeof(RbParams));
	return (unsigned)sizeof(RbParams);
}
