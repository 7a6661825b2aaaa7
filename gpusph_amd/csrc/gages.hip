// gages.hip -- wave gages on the device for gfx950: the water level at given (x, y) from the particles that the surface
// detection flagged.  The reference computes them in GPUSPH::doWrite on a full host copy of the state (src/GPUSPH.cc:1565-1571
// Wendland2D, :1649-1668 the loop over the particles, :1688-1694 the division); here the state stays where it is and a dozen
// numbers come back.
//
//   smoothing length h > 0   z = sum z_i W(r_i, h) / sum W(r_i, h) over the surface particles with r_i < 2 h, r the horizontal
//                            distance, W the 2D Wendland kernel ("a standard average, not an SPH smoothing")
//   smoothing length 0       z of the surface particle with the smallest r, the lowest row among equals (strict < in row order)
//
// in double precision on the global position (cell size)*(cell + 1/2) + local position + world origin, as calcGlobalPosOffset
// (src/GlobalData.h:378-384) forms it.  The cell size and the world origin are the uploaded constants (float).
//
// Same state in, same bits out: no floating-point atomics.  One grid-stride pass reads INFO (8 B per particle: what bounds the
// kernel), and a wave that holds no surface row goes on at once.  A wave has 64 lanes and there are at most SPHX_MAX_GAGES = 64
// gages: the wave reduces a gage's terms by a butterfly (every lane ends with the same sum) and lane g keeps the running value of
// gage g in its registers, chunk after chunk in index order.  The waves of a block are folded in wave order into
// [block][gage], and a second kernel folds the blocks, one wave per gage, in a fixed order.  The grid depends on the particle count alone.
// Compiled without FMA contraction, so that the terms are the host's.
#include "gages.h"
#include <cmath>

#define GAGE_BLOCK      256
#define GAGE_WAVES      (GAGE_BLOCK/64)
#define GAGE_NO_ROW     4294967296.0      // row of "nothing found": behind every uint32 row, exact in a double

struct GageArgs {
	const float4 *pos;
	const particleinfo *info;
	const uint32_t *hash;
	const double *gages;       // [numGages][4]: x, y, unused, smoothing length
	uint32_t numGages, numParticles;
	double cs[3], wo[3];
};

// the running value of one gage: Wendland mode (a, b) = (sum z W, sum W); nearest mode (a, b, row) = (z, r, row)
struct GageAcc { double a, b, row; };

__device__ __forceinline__ bool gage_nearer(double r, double row, double r2, double row2)
{ return r < r2 || (r == r2 && row < row2); }

__device__ __forceinline__ void gage_fold(bool nearest, GageAcc &into, const GageAcc &v)
{
	if (!nearest) { into.a += v.a; into.b += v.b; }
	else if (gage_nearer(v.b, v.row, into.b, into.row)) into = v;
}

__device__ __forceinline__ GageAcc gage_empty(bool nearest)
{ GageAcc e; e.a = 0.0; e.b = nearest ? (double)INFINITY : 0.0; e.row = GAGE_NO_ROW; return e; }

__device__ __forceinline__ double gage_wendland2d(double r, double h)
{
	const double q = r/h;
	double temp = 1 - q/2.;
	temp *= temp;
	temp *= temp;
	return 7/(4*M_PI*h*h)*temp*(2*q + 1);
}

__global__ void __launch_bounds__(GAGE_BLOCK)
gage_partials_kernel(DevParams p, GageArgs a, double *__restrict__ blockPartials)
{
	__shared__ double sAcc[GAGE_WAVES][SPHX_MAX_GAGES][3];
	const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
	const bool mine = lane < a.numGages;
	const bool myNearest = mine && !(a.gages[4u*lane + 3u] > 0.0);
	GageAcc acc = gage_empty(myNearest);
	// (base is the same for the 64 lanes of a wave: every ballot and shuffle below is reached by the whole wave)
	for (uint32_t base = blockIdx.x*GAGE_BLOCK + wave*64u; base < a.numParticles; base += gridDim.x*GAGE_BLOCK) {
		const uint32_t index = base + lane;
		bool surf = false;
		if (index < a.numParticles) surf = (a.info[index].x & FG_SURFACE) != 0;
		if (!__builtin_amdgcn_ballot_w64(surf)) continue;
		double x = 0.0, y = 0.0, z = 0.0;
		if (surf) {
			const float4 pos = a.pos[index];
			surf = is_active_w(pos.w);
			const int3 g = grid_pos_from_hash(p, a.hash[index] & CELLTYPE_BITMASK);
			x = a.cs[0]*(g.x + 0.5) + (double)pos.x + a.wo[0];
			y = a.cs[1]*(g.y + 0.5) + (double)pos.y + a.wo[1];
			z = a.cs[2]*(g.z + 0.5) + (double)pos.z + a.wo[2];
		}
		for (uint32_t k = 0; k < a.numGages; ++k) {
			const double gx = a.gages[4u*k], gy = a.gages[4u*k + 1u], h = a.gages[4u*k + 3u];
			const double r = sqrt((x - gx)*(x - gx) + (y - gy)*(y - gy));
			const bool nearest = !(h > 0.0);
			const bool in = surf && (nearest || r < 2*h);
			if (!__builtin_amdgcn_ballot_w64(in)) continue;
			GageAcc v = gage_empty(nearest);
			if (in) {
				if (nearest) { v.a = z; v.b = r; v.row = (double)index; }
				else { const double W = gage_wendland2d(r, h); v.a = z*W; v.b = W; }
			}
#pragma unroll
			for (int d = 1; d < 64; d <<= 1) {
				GageAcc o;
				o.a = __shfl_xor(v.a, d); o.b = __shfl_xor(v.b, d); o.row = __shfl_xor(v.row, d);
				gage_fold(nearest, v, o);
			}
			if (lane == k) gage_fold(nearest, acc, v);
		}
	}
	if (mine) { sAcc[wave][lane][0] = acc.a; sAcc[wave][lane][1] = acc.b; sAcc[wave][lane][2] = acc.row; }
	__syncthreads();
	if (threadIdx.x < a.numGages) {
		GageAcc tot = gage_empty(myNearest);
		for (uint32_t w = 0; w < GAGE_WAVES; ++w) {
			GageAcc v; v.a = sAcc[w][threadIdx.x][0]; v.b = sAcc[w][threadIdx.x][1]; v.row = sAcc[w][threadIdx.x][2];
			gage_fold(myNearest, tot, v);
		}
		double *out = blockPartials + ((size_t)blockIdx.x*SPHX_MAX_GAGES + threadIdx.x)*3u;
		out[0] = tot.a; out[1] = tot.b; out[2] = tot.row;
	}
}

// the blocks' partials -> partials[gage][4]: (sum z W, sum W, 0, 0), or (z, r, found, row) in nearest mode.  One wave per gage: lane l
// folds the blocks l, l + 64, ... in that order, the lanes are folded by the butterfly -- a fixed order for a given number of blocks
__global__ void __launch_bounds__(64)
gage_fold_kernel(const double *__restrict__ blockPartials, const double *__restrict__ gages, uint32_t numGages, uint32_t numBlocks,
	double *__restrict__ partials)
{
	const uint32_t g = blockIdx.x, lane = threadIdx.x;
	const bool nearest = !(gages[4u*g + 3u] > 0.0);
	GageAcc tot = gage_empty(nearest);
	for (uint32_t b = lane; b < numBlocks; b += 64u) {
		const double *in = blockPartials + ((size_t)b*SPHX_MAX_GAGES + g)*3u;
		GageAcc v; v.a = in[0]; v.b = in[1]; v.row = in[2];
		gage_fold(nearest, tot, v);
	}
#pragma unroll
	for (int d = 1; d < 64; d <<= 1) {
		GageAcc o;
		o.a = __shfl_xor(tot.a, d); o.b = __shfl_xor(tot.b, d); o.row = __shfl_xor(tot.row, d);
		gage_fold(nearest, tot, o);
	}
	if (lane) return;
	double *out = partials + 4u*g;
	const bool found = tot.row < GAGE_NO_ROW;
	out[0] = tot.a; out[1] = tot.b;
	out[2] = nearest ? (found ? 1.0 : 0.0) : 0.0;
	out[3] = nearest ? tot.row : 0.0;
}

// GPUSPH.cc:1688-1694: z /= sum W with a smoothing length (0/0 = NaN over dry ground); the nearest particle's z, or the 0 the
// gage was reset to when no surface particle exists
__global__ void __launch_bounds__(64)
gage_finish_kernel(const double *__restrict__ partials, const double *__restrict__ gages, uint32_t numGages, double *__restrict__ z)
{
	const uint32_t g = threadIdx.x;
	if (g >= numGages) return;
	const double *in = partials + 4u*g;
	if (gages[4u*g + 3u] > 0.0) z[g] = in[0]/in[1];
	else z[g] = in[2] != 0.0 ? in[0] : 0.0;
}

extern "C" int sphx_wave_gages(sphx_ctx *ctx, double *d_partials, const double *gages, uint32_t numGages,
	const void *pos, const void *info, const uint32_t *hash, uint32_t numParticles, void *stream)
{
	SPHX_REQUIRE(ctx && ctx->have_params, "sphx_wave_gages: constants not set");
	SPHX_REQUIRE(numGages <= SPHX_MAX_GAGES, "sphx_wave_gages: more than SPHX_MAX_GAGES (64) gages in one call");
	if (!numGages) return SPHX_OK;
	SPHX_REQUIRE(d_partials && gages, "sphx_wave_gages: missing buffer (partials, gages)");
	SPHX_REQUIRE(!numParticles || (pos && info && hash), "sphx_wave_gages: missing buffer (POS, INFO, HASH)");
	hipStream_t st = (hipStream_t)stream;
	double *scratch = sphx_gage_scratch(ctx);
	if (!scratch) return sphx_set_error(SPHX_ERR_RUNTIME, "sphx_wave_gages: no device memory for the partials of the blocks");
	GageArgs a;
	a.pos = (const float4*)pos; a.info = (const particleinfo*)info; a.hash = hash; a.gages = gages;
	a.numGages = numGages; a.numParticles = numParticles;
	for (int k = 0; k < 3; ++k) { a.cs[k] = (double)ctx->params.cellSize[k]; a.wo[k] = (double)ctx->params.worldOrigin[k]; }
	uint32_t blocks = div_up_u(numParticles, GAGE_BLOCK);
	blocks = blocks < 1u ? 1u : blocks > GAGE_MAX_BLOCKS ? (uint32_t)GAGE_MAX_BLOCKS : blocks;
	gage_partials_kernel<<<blocks, GAGE_BLOCK, 0, st>>>(ctx->dev, a, scratch);
	SPHX_LAUNCH_CHECK("gage_partials_kernel");
	gage_fold_kernel<<<numGages, 64, 0, st>>>(scratch, gages, numGages, blocks, d_partials);
	SPHX_LAUNCH_CHECK("gage_fold_kernel");
	return SPHX_OK;
}

extern "C" int sphx_wave_gages_finish(sphx_ctx *ctx, double *d_z, const double *d_partials, const double *gages, uint32_t numGages,
	void *stream)
{
	SPHX_REQUIRE(ctx != nullptr, "sphx_wave_gages_finish: NULL ctx");
	SPHX_REQUIRE(numGages <= SPHX_MAX_GAGES, "sphx_wave_gages_finish: more than SPHX_MAX_GAGES (64) gages in one call");
	if (!numGages) return SPHX_OK;
	SPHX_REQUIRE(d_z && d_partials && gages, "sphx_wave_gages_finish: missing buffer");
	gage_finish_kernel<<<1, 64, 0, (hipStream_t)stream>>>(d_partials, gages, numGages, d_z);
	SPHX_LAUNCH_CHECK("gage_finish_kernel");
	return SPHX_OK;
}
