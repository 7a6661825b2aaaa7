// forces_sa.hip -- the SA_BOUNDARY modes of the tiled kernel (Wendland) and their launcher.
#include "forces_tile.h"

void sphx_part_sa_tile(const sphx_ctx *ctx, hipStream_t stream, const ForcesArgs &fa, int mode, bool newtonian)
{
#define SPHX_SA_TILE_D(T, DIFF) forces_tile_kernel<SPHX_WENDLAND, (T), DIFF, false><<<ctx->tile_grid, TILE_THREADS, 0, stream>>>(ctx->dev, fa, \
		ctx->tiles, ctx->tile_ctl, ctx->cell_end_copy)
#define SPHX_SA_TILE(T) SPHX_SA_TILE_D(T, DIFF_NONE)
	// Ferrari diffusion in the continuity equation (Spheric2SA's set; sa_forces_check admits it for that form only): instantiations of
	// their own, so that the code of the runs without it stays what it was.  The fluid section carries the term; the vertex section
	// (walked in the place of the boundary section) runs with the diffusion switched off (walk_runs: diffuse = false), and the
	// boundary elements' share is sa_forces_wall_kernel's or the walker's
	const bool ferrari = mode == SPHX_SA_TILE_FORCES && ctx->dev.densitydiff == SPHX_FERRARI;
	if (mode == SPHX_SA_TILE_DSUM) SPHX_SA_TILE(SPHX_LAMINAR_FLOW | SPHX_TURB_SA_DSUM);
	else if (mode == SPHX_SA_TILE_DIFF) SPHX_SA_TILE(SPHX_LAMINAR_FLOW | SPHX_TURB_SA_DIFF);
	else if (ferrari && newtonian) SPHX_SA_TILE_D(SPHX_LAMINAR_FLOW | SPHX_TURB_NEWT | SPHX_TURB_SA, DIFF_FERRARI);
	else if (ferrari) SPHX_SA_TILE_D(SPHX_LAMINAR_FLOW | SPHX_TURB_SA, DIFF_FERRARI);
	else if (newtonian) SPHX_SA_TILE(SPHX_LAMINAR_FLOW | SPHX_TURB_NEWT | SPHX_TURB_SA);
	else SPHX_SA_TILE(SPHX_LAMINAR_FLOW | SPHX_TURB_SA);
#undef SPHX_SA_TILE
#undef SPHX_SA_TILE_D
}
