// diagnostics.hip -- what GPUSPH::doWrite takes from a full host copy of the state at every save besides the wave gages
// (gages.hip), for gfx950: the kinetic, potential and internal energy per fluid that CommonWriter keeps in energy.txt
// (src/GPUSPH.cc:1597-1647, src/writers/CommonWriter.cc:226-241), the largest particle speed behind the "Peak particle speed"
// line of a run's end (:1672-1684, :775-776) and the first particle without a finite position (:1627-1635).  Here the state
// stays where it is and two dozen numbers come back.
//
// Every ACTIVE row (finite pos.w) adds m (|v|^2/2, -gp.g, e_int) and 1 to its class, fluid_num for a fluid particle and
// SPHX_MAX_FLUIDS for everybody else; gp is the global position (cell size)*(cell + 1/2) + local position + world origin in
// double, as calcGlobalPosOffset (src/GlobalData.h:378-384) forms it, from the uploaded (float) cell size, world origin and
// gravity.  |v|^2 = vx vx + vy vy + vz vz is a float; its largest value over the active rows is kept (NaN ignored, as fmax does)
// and the caller takes ONE float square root of it: sqrt is monotone, so that is the largest length(vel) whatever the order.
// Where this leaves the reference (include/sphx.h): inactive rows count for nothing (the reference's sums would be NaN);
// kinetic and potential energy are formed without an energy buffer as well, internal = 0 (the reference writes zeros then); a
// non-finite position of an active row poisons the potential energy of its class as in the reference, and the lowest such row is
// reported where the reference prints a warning.
//
// One grid-stride pass reads POS, VEL (16 B each), INFO (8 B), HASH (4 B) and the energy (4 B) of every row: 44 or 48 B per
// particle, which is what bounds the kernel.  Same state in, same bits out: no floating-point atomics.  A lane sums its rows in
// index order into (SPHX_MAX_FLUIDS + 1) x 4 doubles it holds in registers -- the class is data, so every class is added to
// through a select and the array is never indexed with it --, the lanes of a wave meet in a butterfly, the waves of a block are
// folded in wave order into [block][...], and a second kernel of one wave folds the blocks in a fixed order.  The grid depends
// on the particle count alone.  Compiled without FMA contraction, so that the terms are the host's.
#include "diagnostics.h"
#include <cmath>

#define DIAG_BLOCK      256
#define DIAG_WAVES      (DIAG_BLOCK/64)
#define DIAG_CLASSES    (SPHX_MAX_FLUIDS + 1)
#define DIAG_VALUES     (SPHX_DIAG_NANROW + 1)      // what is reduced: the sums, the largest |v|^2, the lowest row
#define DIAG_NO_ROW32   0xFFFFFFFFu

struct DiagArgs {
	const float4 *pos, *vel;
	const particleinfo *info;
	const uint32_t *hash;
	const float *energy;       // may be NULL
	uint32_t numParticles;
	double cs[3], wo[3], g[3];
};

// value q of the result: a sum, the largest |v|^2 (never NaN) or the lowest row (as a double, SPHX_DIAG_NO_ROW for none)
__device__ __forceinline__ double diag_fold(uint32_t q, double a, double b)
{ return q < SPHX_DIAG_MAXSQ ? a + b : q == SPHX_DIAG_MAXSQ ? fmax(a, b) : fmin(a, b); }

__device__ __forceinline__ double diag_empty(uint32_t q) { return q == SPHX_DIAG_NANROW ? SPHX_DIAG_NO_ROW : 0.0; }

__device__ __forceinline__ bool diag_finite(double v) { return fabs(v) < (double)INFINITY; }

__global__ void __launch_bounds__(DIAG_BLOCK)
diag_partials_kernel(DevParams p, DiagArgs a, double *__restrict__ blockPartials)
{
	__shared__ double sAcc[DIAG_WAVES][DIAG_VALUES];
	const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
	double acc[DIAG_CLASSES][4];
#pragma unroll
	for (int c = 0; c < DIAG_CLASSES; ++c) { acc[c][0] = 0.0; acc[c][1] = 0.0; acc[c][2] = 0.0; acc[c][3] = 0.0; }
	float maxsq = 0.0f;
	uint32_t nanrow = DIAG_NO_ROW32;
	// (64-bit row counter: the stride of the last round may pass 2^32)
	for (uint64_t row = (uint64_t)blockIdx.x*DIAG_BLOCK + threadIdx.x; row < a.numParticles; row += (uint64_t)gridDim.x*DIAG_BLOCK) {
		const uint32_t index = (uint32_t)row;
		const float4 pos = a.pos[index];
		const float4 vel = a.vel[index];
		const particleinfo info = a.info[index];
		const uint32_t hash = a.hash[index];
		const float e = a.energy ? a.energy[index] : 0.0f;
		if (!is_active_w(pos.w)) continue;
		const int3 g = grid_pos_from_hash(p, hash & CELLTYPE_BITMASK);
		const double x = a.cs[0]*(g.x + 0.5) + (double)pos.x + a.wo[0];
		const double y = a.cs[1]*(g.y + 0.5) + (double)pos.y + a.wo[1];
		const double z = a.cs[2]*(g.z + 0.5) + (double)pos.z + a.wo[2];
		if (nanrow == DIAG_NO_ROW32 && !(diag_finite(x) && diag_finite(y) && diag_finite(z))) nanrow = index;      // (rows come in rising order)
		const double m = (double)pos.w;
		const float sq = vel.x*vel.x + vel.y*vel.y + vel.z*vel.z;
		maxsq = fmaxf(maxsq, sq);
		const double kinetic = m*(double)(sq/2);
		const double potential = -m*(x*a.g[0] + y*a.g[1] + z*a.g[2]);
		const double internal = m*(double)e;
		const int cls = IS_FLUID(info) ? (int)FLUID_NUM(info) : SPHX_MAX_FLUIDS;
#pragma unroll
		for (int c = 0; c < DIAG_CLASSES; ++c) {
			const bool in = cls == c;
			acc[c][0] += in ? kinetic : 0.0;
			acc[c][1] += in ? potential : 0.0;
			acc[c][2] += in ? internal : 0.0;
			acc[c][3] += in ? 1.0 : 0.0;
		}
	}
	// the lanes of the wave: after the butterfly every lane holds the same values (a + b and b + a are the same bits)
	double mx = (double)maxsq, nr = nanrow == DIAG_NO_ROW32 ? SPHX_DIAG_NO_ROW : (double)nanrow;
#pragma unroll
	for (int d = 1; d < 64; d <<= 1) {
#pragma unroll
		for (int c = 0; c < DIAG_CLASSES; ++c) {
#pragma unroll
			for (int k = 0; k < 4; ++k) acc[c][k] += __shfl_xor(acc[c][k], d);
		}
		mx = fmax(mx, __shfl_xor(mx, d));
		nr = fmin(nr, __shfl_xor(nr, d));
	}
	if (lane == 0) {
#pragma unroll
		for (int c = 0; c < DIAG_CLASSES; ++c) {
#pragma unroll
			for (int k = 0; k < 4; ++k) sAcc[wave][4*c + k] = acc[c][k];
		}
		sAcc[wave][SPHX_DIAG_MAXSQ] = mx;
		sAcc[wave][SPHX_DIAG_NANROW] = nr;
	}
	__syncthreads();
	if (threadIdx.x < DIAG_VALUES) {
		double tot = diag_empty(threadIdx.x);
		for (uint32_t w = 0; w < DIAG_WAVES; ++w) tot = diag_fold(threadIdx.x, tot, sAcc[w][threadIdx.x]);
		blockPartials[(size_t)blockIdx.x*SPHX_DIAG_DOUBLES + threadIdx.x] = tot;
	}
}

// the blocks' partials -> out[SPHX_DIAG_DOUBLES].  One wave: for every value in turn lane l folds the blocks l, l + 64, ... in that
// order and the lanes are folded by the butterfly -- a fixed order for a given number of blocks
__global__ void __launch_bounds__(64)
diag_fold_kernel(const double *__restrict__ blockPartials, uint32_t numBlocks, double *__restrict__ out)
{
	const uint32_t lane = threadIdx.x;
	for (uint32_t q = 0; q < DIAG_VALUES; ++q) {
		double tot = diag_empty(q);
		for (uint32_t b = lane; b < numBlocks; b += 64u) tot = diag_fold(q, tot, blockPartials[(size_t)b*SPHX_DIAG_DOUBLES + q]);
#pragma unroll
		for (int d = 1; d < 64; d <<= 1) tot = diag_fold(q, tot, __shfl_xor(tot, d));
		if (lane == 0) out[q] = tot;
	}
	if (lane >= DIAG_VALUES && lane < SPHX_DIAG_DOUBLES) out[lane] = 0.0;
}

extern "C" int sphx_save_diagnostics(sphx_ctx *ctx, double *d_out, const void *pos, const void *vel, const void *info,
	const uint32_t *hash, const float *intEnergy, uint32_t numParticles, void *stream)
{
	SPHX_REQUIRE(ctx && ctx->have_params, "sphx_save_diagnostics: constants not set");
	SPHX_REQUIRE(d_out != nullptr, "sphx_save_diagnostics: missing buffer (the result)");
	SPHX_REQUIRE(!numParticles || (pos && vel && info && hash), "sphx_save_diagnostics: missing buffer (POS, VEL, INFO, HASH)");
	hipStream_t st = (hipStream_t)stream;
	double *scratch = sphx_diag_scratch(ctx);
	if (!scratch) return sphx_set_error(SPHX_ERR_RUNTIME, "sphx_save_diagnostics: no device memory for the partials of the blocks");
	DiagArgs a;
	a.pos = (const float4*)pos; a.vel = (const float4*)vel; a.info = (const particleinfo*)info; a.hash = hash; a.energy = intEnergy;
	a.numParticles = numParticles;
	for (int k = 0; k < 3; ++k) {
		a.cs[k] = (double)ctx->params.cellSize[k]; a.wo[k] = (double)ctx->params.worldOrigin[k]; a.g[k] = (double)ctx->params.gravity[k];
	}
	uint32_t blocks = div_up_u(numParticles, DIAG_BLOCK);
	blocks = blocks < 1u ? 1u : blocks > DIAG_MAX_BLOCKS ? (uint32_t)DIAG_MAX_BLOCKS : blocks;
	diag_partials_kernel<<<blocks, DIAG_BLOCK, 0, st>>>(ctx->dev, a, scratch);
	SPHX_LAUNCH_CHECK("diag_partials_kernel");
	diag_fold_kernel<<<1, 64, 0, st>>>(scratch, blocks, d_out);
	SPHX_LAUNCH_CHECK("diag_fold_kernel");
	return SPHX_OK;
}
