// forces_part.hip -- the forces, stress and SPS kernels of ONE SPH kernel type, SPHX_FORCES_PART, and their launchers
// (sphx_part_*_k<type>, forces_args.h).  Compiled once per type (see the Makefile): the macro is a template argument, nothing more.
#include "forces_generic.h"
#include "forces_tile.h"

#ifndef SPHX_FORCES_PART
#error "forces_part.hip: compile with -DSPHX_FORCES_PART=<SPH kernel type, 1..4>"
#endif

template<int KERNEL, int TURB, int COLA>
static void launch_forces_mf(bool multifluid, dim3 grid, hipStream_t stream, const DevParams &p, const ForcesArgs &a,
	const uint32_t *guard)
{
	if (guard) grid.x = grid.x < 2048u ? grid.x : 2048u;   // stand-by launch (see forces_kernel)
	if (multifluid)
		forces_kernel<KERNEL, TURB, COLA, true><<<grid, SPHX_BLOCK_FORCES, 0, stream>>>(p, a, guard);
	else
		forces_kernel<KERNEL, TURB, COLA, false><<<grid, SPHX_BLOCK_FORCES, 0, stream>>>(p, a, guard);
}

template<int KERNEL, int TURB, int COLA>
static void launch_tile(const sphx_ctx *ctx, hipStream_t stream, const ForcesArgs &a)
{
	ForcesTimer t(ctx, stream, true);
	if (ctx->dev.boundarytype == SPHX_LJ_BOUNDARY)
		forces_tile_kernel<KERNEL, TURB, COLA, true><<<ctx->tile_grid, TILE_THREADS, 0, stream>>>(ctx->dev, a,
			ctx->tiles, ctx->tile_ctl, ctx->cell_end_copy);
	else
		forces_tile_kernel<KERNEL, TURB, COLA, false><<<ctx->tile_grid, TILE_THREADS, 0, stream>>>(ctx->dev, a,
			ctx->tiles, ctx->tile_ctl, ctx->cell_end_copy);
}

// launches the tiled kernel when the tiling of this neighbour list is available, plus the generic
// kernel guarded by the device-side overflow flag (it returns at once when the tiles were used)
template<int KERNEL>
static int launch_forces_k(const sphx_ctx *ctx, dim3 grid, hipStream_t stream, const ForcesArgs &a, bool use_tiles)
{
	const DevParams &p = ctx->dev;
	const bool mf = p.numfluids > 1;
	const int diff = (p.densitydiff == SPHX_COLAGROSSI) ? DIFF_COLAGROSSI : (p.densitydiff == SPHX_FERRARI) ? DIFF_FERRARI : DIFF_NONE;
	const bool newt = p.rheology == SPHX_NEWTONIAN;
	const uint32_t *guard = use_tiles ? sphx_tiles_standby_guard(ctx) : nullptr;
	const bool standby = !use_tiles || guard;   // the host saw the tiling succeed: no stand-by launch
	ForcesTimer t(ctx, stream, !use_tiles);   // without tiles the generic kernel is the dominant one
	// tiled kernel, then the generic one, guarded by the overflow flag
	// more than one fluid or Ferrari diffusion: tiled only for the Wendland kernel (every such problem of the reference uses
	// it), to bound the number of kernel instantiations; use_tiles is false for the other kernels then
#define SPHX_LAUNCH_TILE(T) do { if (use_tiles) { \
		if (mf) { if (KERNEL == SPHX_WENDLAND) { \
			if (diff == DIFF_COLAGROSSI) launch_tile<SPHX_WENDLAND, (T) | SPHX_TURB_MF, DIFF_COLAGROSSI>(ctx, stream, a); \
			else if (diff == DIFF_FERRARI) launch_tile<SPHX_WENDLAND, (T) | SPHX_TURB_MF, DIFF_FERRARI>(ctx, stream, a); \
			else launch_tile<SPHX_WENDLAND, (T) | SPHX_TURB_MF, DIFF_NONE>(ctx, stream, a); } } \
		else if (diff == DIFF_COLAGROSSI) launch_tile<KERNEL, T, DIFF_COLAGROSSI>(ctx, stream, a); \
		else if (diff == DIFF_FERRARI) { if (KERNEL == SPHX_WENDLAND) launch_tile<SPHX_WENDLAND, T, DIFF_FERRARI>(ctx, stream, a); } \
		else launch_tile<KERNEL, T, DIFF_NONE>(ctx, stream, a); } } while (0)
#define SPHX_LAUNCH_GENERIC(T, G) do { if (!standby) break; \
		if (diff == DIFF_COLAGROSSI) launch_forces_mf<KERNEL, T, DIFF_COLAGROSSI>(mf, grid, stream, p, a, G); \
		else if (diff == DIFF_FERRARI) launch_forces_mf<KERNEL, T, DIFF_FERRARI>(mf, grid, stream, p, a, G); \
		else launch_forces_mf<KERNEL, T, DIFF_NONE>(mf, grid, stream, p, a, G); } while (0)
	switch (p.turbmodel) {
	case SPHX_ARTIFICIAL:
		if constexpr (KERNEL == SPHX_WENDLAND) {      // (this part alone holds the second instantiation)
			if (use_tiles && plain_gravity_z(ctx)) {
				ForcesTimer tt(ctx, stream, true);
				forces_tile_kernel<SPHX_WENDLAND, SPHX_ARTIFICIAL, DIFF_COLAGROSSI_GZ, false><<<ctx->tile_grid, TILE_THREADS, 0, stream>>>(ctx->dev, a,
					ctx->tiles, ctx->tile_ctl, ctx->cell_end_copy);
			} else
				SPHX_LAUNCH_TILE(SPHX_ARTIFICIAL);
		} else {
			SPHX_LAUNCH_TILE(SPHX_ARTIFICIAL);
		}
		SPHX_LAUNCH_GENERIC(SPHX_ARTIFICIAL, guard);
		break;
	case SPHX_SPS:
		if (newt) {
			SPHX_LAUNCH_TILE(SPHX_SPS | SPHX_TURB_NEWT);
			SPHX_LAUNCH_GENERIC(SPHX_SPS | SPHX_TURB_NEWT, guard);
		} else {
			SPHX_LAUNCH_TILE(SPHX_SPS);
			SPHX_LAUNCH_GENERIC(SPHX_SPS, guard);
		}
		break;
	case SPHX_LAMINAR_FLOW:
		if (newt) {
			SPHX_LAUNCH_TILE(SPHX_LAMINAR_FLOW | SPHX_TURB_NEWT);
			SPHX_LAUNCH_GENERIC(SPHX_LAMINAR_FLOW | SPHX_TURB_NEWT, guard);
		} else {
			SPHX_LAUNCH_TILE(SPHX_LAMINAR_FLOW);
			SPHX_LAUNCH_GENERIC(SPHX_LAMINAR_FLOW, guard);
		}
		break;
	default:
		return sphx_set_error(SPHX_ERR_UNSUPPORTED, "sphx_forces_basicstep: turbulence model not built");
	}
#undef SPHX_LAUNCH_TILE
#undef SPHX_LAUNCH_GENERIC
	return SPHX_OK;
}

#define SPHX_PASTE2(a, b) a##b
#define SPHX_PASTE(a, b) SPHX_PASTE2(a, b)
int SPHX_PASTE(sphx_part_forces_k, SPHX_FORCES_PART)(const sphx_ctx *ctx, dim3 grid, hipStream_t stream, const ForcesArgs &a, bool use_tiles)
{
	return launch_forces_k<SPHX_FORCES_PART>(ctx, grid, stream, a, use_tiles);
}
void SPHX_PASTE(sphx_part_stress_k, SPHX_FORCES_PART)(const sphx_ctx *ctx, hipStream_t stream, const ForcesArgs &fa)
{
	forces_tile_kernel<SPHX_FORCES_PART, SPHX_ARTIFICIAL | SPHX_TURB_STRESS, DIFF_NONE, false>
		<<<ctx->tile_grid, TILE_THREADS, 0, stream>>>(ctx->dev, fa, ctx->tiles, ctx->tile_ctl, ctx->cell_end_copy);
}
void SPHX_PASTE(sphx_part_sps_k, SPHX_FORCES_PART)(const sphx_ctx *ctx, dim3 grid, hipStream_t stream, const SpsArgs &a, const uint32_t *guard)
{
	if (ctx->dev.numfluids > 1) sps_kernel<SPHX_FORCES_PART, true><<<grid, 128, 0, stream>>>(ctx->dev, a, guard);
	else sps_kernel<SPHX_FORCES_PART, false><<<grid, 128, 0, stream>>>(ctx->dev, a, guard);
}
