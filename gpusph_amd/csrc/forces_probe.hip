// forces_probe.hip -- not part of the library: two instantiations of the tiled kernel alone, for reading their ISA (scripts/probe_plain_isa.sh): the plain forces pass of the bench workload
// (gravity along z) and its form for any gravity
#include "forces_tile.h"

void sphx_probe_plain(const sphx_ctx *ctx, hipStream_t stream, const ForcesArgs &a)
{
	if (plain_gravity_z(ctx))
		forces_tile_kernel<SPHX_WENDLAND, SPHX_ARTIFICIAL, DIFF_COLAGROSSI_GZ, false><<<ctx->tile_grid, TILE_THREADS, 0, stream>>>(ctx->dev, a,
			ctx->tiles, ctx->tile_ctl, ctx->cell_end_copy);
	else
		forces_tile_kernel<SPHX_WENDLAND, SPHX_ARTIFICIAL, DIFF_COLAGROSSI, false><<<ctx->tile_grid, TILE_THREADS, 0, stream>>>(ctx->dev, a,
			ctx->tiles, ctx->tile_ctl, ctx->cell_end_copy);
}
