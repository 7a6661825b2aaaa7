// granular.hip -- the effective pressure of the GRANULAR rheology (src/cuda/visc_kernel.cu:813-1101, src/cuda/visc.cu:257-660) for
// gfx950: a Jacobi solve of a Laplace-like system over the sediment, three times per step.
//   sphx_jacobi_fs_boundary_conditions     jacobiFSBoundaryConditionsDevice: Dirichlet value on surface / interface sediment
//   sphx_jacobi_wall_boundary_conditions   jacobiWallBoundaryConditionsDevice: Shepard interpolation onto the wall particles
//   sphx_jacobi_build_vectors              jacobiBuildVectorsDevice: (D, Rx, B, NaN) of every row
//   sphx_jacobi_update_effpres             jacobiUpdateEffPresDevice: p = (B - Rx)/D
// These four are the reference's passes, one thread per particle walking its own u16 list (neib_iter.h); a caller drives them as
// the reference's integrator does (PredictorCorrectorIntegrator.cc:1046-1182) with two host reads per iteration.
//   sphx_jacobi_solve                      the whole solve.  Within a solve nothing moves but the pressure, so the list walk, the
// distances, the kernel values and the volumes are evaluated ONCE: the rows that iterate are compacted and each of their list
// entries is stored as {neighbour, coefficient}, column-major over the compact rows.  An iteration then streams those entries
// (one coalesced 8- or 12-byte load and one gathered 4-byte load per entry instead of a list walk with position, velocity and
// info rows and a kernel evaluation), and the stop test runs on the device.
// Every pair term has ONE form, shared by both paths through jc_walk_interior / jc_walk_wall and jc_update / jc_wall_value: the
// fused solve gives the bits of the entry-point loop (tests/test_gpu_granular.py).
// Built for DYN_BOUNDARY (wall rows are PT_BOUNDARY particles; the boundary-element terms of SA_BOUNDARY are not built).
#include "neib_iter.h"
#include <cstring>

// ctx->gr.ctl: device words of a solve
enum { JC_FLAG = 0,          // the stop test has fired: kernels of later iterations return at once
       JC_COUNTER,           // h_jacobiCounter
       JC_BACKERR,           // float bits: largest backward error of the iteration in flight (atomicMax)
       JC_RESIDUAL,          // ... largest residual
       JC_LAST_BACKERR,      // the maxima the last stop test saw
       JC_LAST_RESIDUAL,
       JC_EXEC,              // iterations executed
       JC_NINT = 8,          // compact rows: sediment-interior ...
       JC_NWALL,             // ... and wall
       JC_MAXINT,            // longest stored row of each kind
       JC_MAXWALL,
       JC_WORDS = 16 };
#define JE_RHS 0x80000000u   // entry of an interior row that feeds B (the others feed Rx)

struct JcArgs {
	const float4 *pos, *vel;
	const particleinfo *info;
	const uint32_t *hash, *cellStart;
	const neibdata *neibsList;
};

// Delta rho of the boundary conditions: rho0[0] with one fluid, |rho0[0] - rho0[1]| otherwise (:844-846)
__device__ __forceinline__ float jc_delta_rho(const DevParams &p)
{
	return p.numfluids > 1 ? fabsf(p.rho0[0] - p.rho0[1]) : p.rho0[0];
}

__device__ __forceinline__ bool jc_is_interior(const particleinfo &info)
{
	return IS_FLUID(info) && IS_SEDIMENT(info) && !IS_INTERFACE(info) && !IS_SURFACE(info);
}

__device__ __forceinline__ float jc_volume(const DevParams &p, const JcArgs &a, uint32_t j, float mass, const particleinfo &ninfo)
{
	return mass/((a.vel[j].w + 1.0f)*p.rho0[FLUID_NUM(ninfo)]);
}

// the entries of a sediment-interior row, in list order (fluid section, then boundary section: for_every_neib without SA):
// f(j, c, rhs) with c = V_j F_ij; D sums every c, Rx the c p_j of interior sediment neighbours, B those of the others (:1015-1050)
template<class F>
__device__ __forceinline__ void jc_walk_interior(const DevParams &p, const JcArgs &a, uint32_t index, const float4 &pos, F &&f)
{
	const int3 gridPos = grid_pos_from_hash(p, a.hash[index] & CELLTYPE_BITMASK);
	auto pair = [&](uint32_t j, const float4 &npos, float rx, float ry, float rz) {
		const float r = sqrtf(fmaf(rz, rz, fmaf(ry, ry, rx*rx)));
		if (!is_active_w(npos.w) || r >= p.influenceradius) return;
		const particleinfo ninfo = a.info[j];
		const bool nfluid = IS_FLUID(ninfo);
		if (!((nfluid && IS_SEDIMENT(ninfo)) || IS_BOUNDARY(ninfo))) return;
		const float c = jc_volume(p, a, j, npos.w, ninfo)*gn_F(p, r);
		f(j, c, !(nfluid && !IS_INTERFACE(ninfo) && !IS_SURFACE(ninfo)));
	};
	for_each_neib<PT_FLUID>(p, a, index, pos, gridPos, pair);
	for_each_neib<PT_BOUNDARY>(p, a, index, pos, gridPos, pair);
}

// the entries of a wall row: its sediment FLUID neighbours (no reach test, as the reference: :916-953), f(j, a, b) with
// a = V_j W_ij and b = Delta rho g . r_ij
template<class F>
__device__ __forceinline__ void jc_walk_wall(const DevParams &p, const JcArgs &a, uint32_t index, const float4 &pos, F &&f)
{
	const int3 gridPos = grid_pos_from_hash(p, a.hash[index] & CELLTYPE_BITMASK);
	const float delta_rho = jc_delta_rho(p);
	for_each_neib<PT_FLUID>(p, a, index, pos, gridPos, [&](uint32_t j, const float4 &npos, float rx, float ry, float rz) {
		if (!is_active_w(npos.w)) return;
		const particleinfo ninfo = a.info[j];
		if (!IS_SEDIMENT(ninfo)) return;
		const float r = sqrtf(fmaf(rz, rz, fmaf(ry, ry, rx*rx)));
		const float av = jc_volume(p, a, j, npos.w, ninfo)*gn_W(p, r);
		f(j, av, delta_rho*(p.gravity[0]*rx + p.gravity[1]*ry + p.gravity[2]*rz));
	});
}

__device__ __forceinline__ float jc_wall_term(float av, float b, float pj) { return fmaxf(av*(pj + b), 0.0f); }

// value and backward error of a wall row from its sums (:954-962); the reference pressure is delta_rho (c0/10)^2 in double
__device__ __forceinline__ float jc_wall_value(const DevParams &p, float sum, float alpha, float old, float &backErr)
{
	backErr = 0.0f;
	if (!(alpha > 0.0f)) return 0.0f;
	const float v = sum/alpha;
	const double refpres = (double)jc_delta_rho(p)*((double)p.sscoeff[0]/10.)*((double)p.sscoeff[0]/10.);
	backErr = (float)((double)fabsf(v - old)/refpres);
	return v;
}

// reference pressure of the residual: rho0 c0^2/100 of the row's fluid (:1080)
__device__ __forceinline__ float jc_refpres(const DevParams &p, uint32_t fl) { return p.rho0[fl]*(p.sscoeff[fl]*p.sscoeff[fl])/100; }

// p = (B - Rx)/D, NaN -> 0; the signed residual (:1088-1095)
__device__ __forceinline__ float jc_update(float D, float Rx, float B, float refpres, float &residual)
{
	const float v = (B - Rx)/D;
	residual = (fmaf(D, v, Rx) - B)/refpres;
	return v == v ? v : 0.0f;
}

// largest value of a wave -> one atomic maximum on the float's bits (non-negative floats order like their bits; NaN and negative
// values lose against the baseline 0, so the signed residual is reduced as max(residual, 0))
__device__ __forceinline__ void jc_reduce_max(uint32_t *dst, float v)
{
	v = fmaxf(v, 0.0f);
#pragma unroll
	for (int d = 32; d > 0; d >>= 1) v = fmaxf(v, __shfl_down(v, d));
	if ((threadIdx.x & 63u) == 0u && v > 0.0f) atomicMax(dst, __float_as_uint(v));
}

// ---- the reference-shaped passes ------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(128)
jacobi_fs_kernel(DevParams p, float *__restrict__ effpres, const float4 *__restrict__ pos, const particleinfo *__restrict__ info,
	uint32_t n, float deltap)
{
	const uint32_t index = blockIdx.x*128 + threadIdx.x;
	if (index >= n || !is_active_w(pos[index].w)) return;
	const particleinfo pinfo = info[index];
	if (IS_FLUID(pinfo) && IS_SEDIMENT(pinfo) && (IS_SURFACE(pinfo) || IS_INTERFACE(pinfo)))
		effpres[index] = deltap*jc_delta_rho(p)*sqrtf(p.gravity[0]*p.gravity[0] + p.gravity[1]*p.gravity[1] + p.gravity[2]*p.gravity[2]);
}

__global__ void __launch_bounds__(128)
jacobi_wall_kernel(DevParams p, JcArgs a, float *effpres, uint32_t *maxBackErr, uint32_t n)
{
	const uint32_t index = blockIdx.x*128 + threadIdx.x;
	float backErr = 0.0f;
	if (index < n) {
		const float4 pos = a.pos[index];
		if (is_active_w(pos.w) && IS_BOUNDARY(a.info[index])) {
			float sum = 0.0f, alpha = 0.0f;
			jc_walk_wall(p, a, index, pos, [&](uint32_t j, float av, float b) { sum += jc_wall_term(av, b, effpres[j]); alpha += av; });
			effpres[index] = jc_wall_value(p, sum, alpha, effpres[index], backErr);      // wall rows are written, sediment fluid rows read
		}
	}
	jc_reduce_max(maxBackErr, backErr);
}

__global__ void __launch_bounds__(128)
jacobi_build_kernel(DevParams p, JcArgs a, const float *__restrict__ effpres, float4 *__restrict__ jacobi, uint32_t n)
{
	const uint32_t index = blockIdx.x*128 + threadIdx.x;
	if (index >= n) return;
	const float4 pos = a.pos[index];
	// a disabled particle: the reference leaves its row as it was; here it is marked (w = 0 where a built row has NaN), so that
	// the update pass, which sees no positions, leaves the particle's pressure alone instead of reading a stale row
	if (!is_active_w(pos.w)) { jacobi[index] = make_float4(0.0f, 0.0f, 0.0f, 0.0f); return; }
	float D = 0.0f, Rx = 0.0f, B = 0.0f;
	if (jc_is_interior(a.info[index]))
		jc_walk_interior(p, a, index, pos, [&](uint32_t j, float c, bool rhs) {
			D += c;
			if (rhs) B = fmaf(c, effpres[j], B); else Rx = fmaf(-c, effpres[j], Rx);
		});
	jacobi[index] = make_float4(D, Rx, B, __builtin_nanf(""));
}

__global__ void __launch_bounds__(128)
jacobi_update_kernel(DevParams p, float *__restrict__ effpres, const float4 *__restrict__ jacobi,
	const particleinfo *__restrict__ info, uint32_t *maxResidual, uint32_t n)
{
	const uint32_t index = blockIdx.x*128 + threadIdx.x;
	float residual = 0.0f;
	if (index < n) {
		const particleinfo pinfo = info[index];
		if (jc_is_interior(pinfo)) {
			const float4 jb = jacobi[index];
			if (jb.w != jb.w)      // a built row (see jacobi_build_kernel)
				effpres[index] = jc_update(jb.x, jb.y, jb.z, jc_refpres(p, FLUID_NUM(pinfo)), residual);
		}
	}
	jc_reduce_max(maxResidual, residual);
}

// ---- the fused solve: assembly ------------------------------------------------------------------------------------------------
// one thread per particle: is it a row that iterates, and how many entries will it store?  Rows are compacted a wave at a time
// (one atomic per wave and kind), so the rows of a wave stay consecutive and the order of the waves does not matter: every row is
// summed by its own thread and the maxima are exact
__global__ void __launch_bounds__(128)
jacobi_classify_kernel(DevParams p, JcArgs a, uint32_t *ctl, uint32_t *__restrict__ rowsInt, uint32_t *__restrict__ cntInt,
	uint32_t *__restrict__ rowsWall, uint32_t *__restrict__ cntWall, uint32_t n)
{
	const uint32_t index = blockIdx.x*128 + threadIdx.x;
	const uint32_t lane = threadIdx.x & 63u;
	bool interior = false, wall = false;
	uint32_t count = 0;
	if (index < n) {
		const float4 pos = a.pos[index];
		if (is_active_w(pos.w)) {
			const particleinfo pinfo = a.info[index];
			interior = jc_is_interior(pinfo);
			wall = IS_BOUNDARY(pinfo);
			if (interior) jc_walk_interior(p, a, index, pos, [&](uint32_t, float, bool) { ++count; });
			if (wall) jc_walk_wall(p, a, index, pos, [&](uint32_t, float, float) { ++count; });
		}
	}
	const unsigned long long below = (1ull << lane) - 1ull;
	const unsigned long long mi = __ballot(interior), mw = __ballot(wall);
	uint32_t baseI = 0, baseW = 0;
	if (lane == 0) {
		if (mi) baseI = atomicAdd(ctl + JC_NINT, (uint32_t)__popcll(mi));
		if (mw) baseW = atomicAdd(ctl + JC_NWALL, (uint32_t)__popcll(mw));
	}
	baseI = __shfl(baseI, 0); baseW = __shfl(baseW, 0);
	if (interior) { const uint32_t r = baseI + (uint32_t)__popcll(mi & below); rowsInt[r] = index; cntInt[r] = count; }      // r < n: rows of distinct particles
	if (wall) { const uint32_t r = baseW + (uint32_t)__popcll(mw & below); rowsWall[r] = index; cntWall[r] = count; }
	uint32_t ci = interior ? count : 0u, cw = wall ? count : 0u;
#pragma unroll
	for (int d = 32; d > 0; d >>= 1) { ci = max(ci, (uint32_t)__shfl_down(ci, d)); cw = max(cw, (uint32_t)__shfl_down(cw, d)); }
	if (lane == 0) { if (ci) atomicMax(ctl + JC_MAXINT, ci); if (cw) atomicMax(ctl + JC_MAXWALL, cw); }
}

// one thread per compact row: entry e of row r goes to [e*rows + r]
__global__ void __launch_bounds__(128)
jacobi_fill_interior_kernel(DevParams p, JcArgs a, const uint32_t *__restrict__ rows, uint2 *__restrict__ ent, float2 *__restrict__ diag,
	uint32_t nrows, uint32_t maxEntries)
{
	const uint32_t r = blockIdx.x*128 + threadIdx.x;
	if (r >= nrows) return;
	const uint32_t index = rows[r];
	float D = 0.0f;
	uint32_t e = 0;
	jc_walk_interior(p, a, index, a.pos[index], [&](uint32_t j, float c, bool rhs) {
		D += c;
		if (e < maxEntries) ent[(size_t)e*nrows + r] = make_uint2(j | (rhs ? JE_RHS : 0u), __float_as_uint(c));
		++e;
	});
	diag[r] = make_float2(D, jc_refpres(p, FLUID_NUM(a.info[index])));
}

__global__ void __launch_bounds__(128)
jacobi_fill_wall_kernel(DevParams p, JcArgs a, const uint32_t *__restrict__ rows, uint32_t *__restrict__ entJ, float2 *__restrict__ entAB,
	uint32_t nrows, uint32_t maxEntries)
{
	const uint32_t r = blockIdx.x*128 + threadIdx.x;
	if (r >= nrows) return;
	const uint32_t index = rows[r];
	uint32_t e = 0;
	jc_walk_wall(p, a, index, a.pos[index], [&](uint32_t j, float av, float b) {
		if (e < maxEntries) { entJ[(size_t)e*nrows + r] = j; entAB[(size_t)e*nrows + r] = make_float2(av, b); }
		++e;
	});
}

// ---- the fused solve: iteration -----------------------------------------------------------------------------------------------
// A Jacobi sweep reads the pressures of the previous sweep only, so it writes to the other of two pressure arrays (src -> dst).
// The arrays agree on every row that does not iterate (they start as copies of each other); a sweep writes every interior row,
// the wall pass behind it every wall row.
__global__ void __launch_bounds__(128)
jacobi_sweep_interior_kernel(const uint32_t *ctl_flag, uint32_t *maxResidual, const float *__restrict__ src, float *__restrict__ dst,
	const uint32_t *__restrict__ rows, const uint32_t *__restrict__ cnt, const uint2 *__restrict__ ent, const float2 *__restrict__ diag,
	uint32_t nrows)
{
	if (*ctl_flag) return;
	const uint32_t r = blockIdx.x*128 + threadIdx.x;
	float residual = 0.0f;
	if (r < nrows) {
		const uint32_t count = cnt[r];
		float Rx = 0.0f, B = 0.0f;
#pragma unroll 4
		for (uint32_t e = 0; e < count; ++e) {
			const uint2 en = ent[(size_t)e*nrows + r];
			const float c = __uint_as_float(en.y), pj = src[en.x & ~JE_RHS];
			if (en.x & JE_RHS) B = fmaf(c, pj, B); else Rx = fmaf(-c, pj, Rx);
		}
		const float2 d = diag[r];
		dst[rows[r]] = jc_update(d.x, Rx, B, d.y, residual);
	}
	jc_reduce_max(maxResidual, residual);
}

// wall rows from the sweep's result: reads sediment fluid rows of dst, writes wall rows of dst; the old value is the row in src
__global__ void __launch_bounds__(128)
jacobi_sweep_wall_kernel(DevParams p, const uint32_t *ctl_flag, uint32_t *maxBackErr, const float *__restrict__ src, float *dst,
	const uint32_t *__restrict__ rows, const uint32_t *__restrict__ cnt, const uint32_t *__restrict__ entJ, const float2 *__restrict__ entAB,
	uint32_t nrows)
{
	if (*ctl_flag) return;
	const uint32_t r = blockIdx.x*128 + threadIdx.x;
	float backErr = 0.0f;
	if (r < nrows) {
		const uint32_t count = cnt[r];
		float sum = 0.0f, alpha = 0.0f;
#pragma unroll 4
		for (uint32_t e = 0; e < count; ++e) {
			const float2 ab = entAB[(size_t)e*nrows + r];
			sum += jc_wall_term(ab.x, ab.y, dst[entJ[(size_t)e*nrows + r]]);
			alpha += ab.x;
		}
		const uint32_t index = rows[r];
		dst[index] = jc_wall_value(p, sum, alpha, src[index], backErr);
	}
	jc_reduce_max(maxBackErr, backErr);
}

// JACOBI_STOP_CRITERION (src/GPUSPH.cc:2300-2321) on the device: stop when both maxima are under their thresholds or the counter
// has passed maxiter, count otherwise; the maxima start the next iteration from zero
__global__ void jacobi_stop_kernel(uint32_t *ctl, uint32_t maxiter, float backerr, float residual)
{
	if (ctl[JC_FLAG]) return;
	const float be = __uint_as_float(ctl[JC_BACKERR]), rs = __uint_as_float(ctl[JC_RESIDUAL]);
	ctl[JC_LAST_BACKERR] = ctl[JC_BACKERR]; ctl[JC_LAST_RESIDUAL] = ctl[JC_RESIDUAL];
	ctl[JC_BACKERR] = 0u; ctl[JC_RESIDUAL] = 0u;
	ctl[JC_EXEC] += 1u;
	if ((be < backerr && rs < residual) || ctl[JC_COUNTER] > maxiter) ctl[JC_FLAG] = 1u;
	else ctl[JC_COUNTER] += 1u;
}

// ---- host side ----------------------------------------------------------------------------------------------------------------
extern "C" int sphx_set_granular(sphx_ctx *ctx, const float *sinpsi, uint32_t maxiter, float backerr, float residual)
{
	SPHX_REQUIRE(ctx && sinpsi, "sphx_set_granular: NULL argument");
	SPHX_REQUIRE(backerr == backerr && residual == residual, "sphx_set_granular: the stop thresholds must be numbers");
	for (int f = 0; f < SPHX_MAX_FLUIDS; ++f) ctx->gr.sinpsi[f] = ctx->dev.sinpsi[f] = sinpsi[f];
	ctx->gr.maxiter = maxiter; ctx->gr.backerr = backerr; ctx->gr.residual = residual;
	ctx->gr.set = true;
	return SPHX_OK;
}

static int jc_check(sphx_ctx *ctx, const char *who)
{
	SPHX_REQUIRE(ctx && ctx->have_params, "sphx (granular): constants not set");
	if (ctx->params.rheologytype != SPHX_GRANULAR)
		return sphx_set_error(SPHX_ERR_INVALID, std::string(who) + ": the effective pressure belongs to the GRANULAR rheology");
	SPHX_REQUIRE(ctx->gr.set, "sphx (granular): sphx_set_granular has not been called");
	if (!ctx->gr.ctl) {
		SPHX_HIP(hipMalloc((void**)&ctx->gr.ctl, JC_WORDS*sizeof(uint32_t)));
		SPHX_HIP(hipHostMalloc((void**)&ctx->gr.ctl_host, JC_WORDS*sizeof(uint32_t), hipHostMallocDefault));
	}
	return SPHX_OK;
}

static JcArgs jc_args(const void *pos, const void *vel, const void *info, const uint32_t *hash, const uint32_t *cellStart, const uint16_t *neibsList)
{
	JcArgs a = {};
	a.pos = (const float4*)pos; a.vel = (const float4*)vel; a.info = (const particleinfo*)info;
	a.hash = hash; a.cellStart = cellStart; a.neibsList = neibsList;
	return a;
}

// one float maximum from its device word to the caller (one host synchronisation, as the reference's cflmax)
static int jc_read_max(sphx_ctx *ctx, uint32_t word, float *h_out, hipStream_t st)
{
	if (!h_out) return SPHX_OK;
	SPHX_HIP(hipMemcpyAsync(ctx->gr.ctl_host + word, ctx->gr.ctl + word, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
	SPHX_HIP(hipStreamSynchronize(st));
	memcpy(h_out, ctx->gr.ctl_host + word, sizeof(float));
	return SPHX_OK;
}

extern "C" int sphx_jacobi_fs_boundary_conditions(sphx_ctx *ctx, float *effpres, const void *pos, const void *info,
	uint32_t numParticles, uint32_t particleRangeEnd, float deltap, void *stream)
{
	int rc = jc_check(ctx, "sphx_jacobi_fs_boundary_conditions");
	if (rc != SPHX_OK) return rc;
	SPHX_REQUIRE(effpres && pos && info, "sphx_jacobi_fs_boundary_conditions: missing buffer");
	SPHX_REQUIRE(particleRangeEnd <= numParticles, "sphx_jacobi_fs_boundary_conditions: range beyond the particles");
	if (!particleRangeEnd) return SPHX_OK;
	jacobi_fs_kernel<<<div_up_u(particleRangeEnd, 128), 128, 0, (hipStream_t)stream>>>(ctx->dev, effpres, (const float4*)pos,
		(const particleinfo*)info, particleRangeEnd, deltap);
	SPHX_LAUNCH_CHECK("jacobi_fs_kernel");
	return SPHX_OK;
}

static int jc_wall_launch(sphx_ctx *ctx, float *effpres, const JcArgs &a, uint32_t particleRangeEnd, hipStream_t st)
{
	SPHX_HIP(hipMemsetAsync(ctx->gr.ctl + JC_BACKERR, 0, sizeof(uint32_t), st));
	if (!particleRangeEnd) return SPHX_OK;
	jacobi_wall_kernel<<<div_up_u(particleRangeEnd, 128), 128, 0, st>>>(ctx->dev, a, effpres, ctx->gr.ctl + JC_BACKERR, particleRangeEnd);
	SPHX_LAUNCH_CHECK("jacobi_wall_kernel");
	return SPHX_OK;
}

extern "C" int sphx_jacobi_wall_boundary_conditions(sphx_ctx *ctx, float *effpres, float *h_backerr,
	const void *pos, const void *vel, const void *info, const uint32_t *hash, const uint32_t *cellStart, const uint16_t *neibsList,
	uint32_t numParticles, uint32_t particleRangeEnd, float deltap, void *stream)
{
	(void)deltap;
	int rc = jc_check(ctx, "sphx_jacobi_wall_boundary_conditions");
	if (rc != SPHX_OK) return rc;
	SPHX_REQUIRE(effpres && pos && vel && info && hash && cellStart && neibsList, "sphx_jacobi_wall_boundary_conditions: missing buffer");
	SPHX_REQUIRE(particleRangeEnd <= numParticles, "sphx_jacobi_wall_boundary_conditions: range beyond the particles");
	hipStream_t st = (hipStream_t)stream;
	rc = jc_wall_launch(ctx, effpres, jc_args(pos, vel, info, hash, cellStart, neibsList), particleRangeEnd, st);
	if (rc != SPHX_OK) return rc;
	return jc_read_max(ctx, JC_BACKERR, h_backerr, st);
}

extern "C" int sphx_jacobi_build_vectors(sphx_ctx *ctx, void *jacobi, const float *effpres,
	const void *pos, const void *vel, const void *info, const uint32_t *hash, const uint32_t *cellStart, const uint16_t *neibsList,
	uint32_t numParticles, uint32_t particleRangeEnd, void *stream)
{
	int rc = jc_check(ctx, "sphx_jacobi_build_vectors");
	if (rc != SPHX_OK) return rc;
	SPHX_REQUIRE(jacobi && effpres && pos && vel && info && hash && cellStart && neibsList, "sphx_jacobi_build_vectors: missing buffer");
	SPHX_REQUIRE(particleRangeEnd <= numParticles, "sphx_jacobi_build_vectors: range beyond the particles");
	if (!particleRangeEnd) return SPHX_OK;
	jacobi_build_kernel<<<div_up_u(particleRangeEnd, 128), 128, 0, (hipStream_t)stream>>>(ctx->dev,
		jc_args(pos, vel, info, hash, cellStart, neibsList), effpres, (float4*)jacobi, particleRangeEnd);
	SPHX_LAUNCH_CHECK("jacobi_build_kernel");
	return SPHX_OK;
}

extern "C" int sphx_jacobi_update_effpres(sphx_ctx *ctx, float *effpres, float *h_residual, const void *jacobi,
	const void *info, uint32_t numParticles, uint32_t particleRangeEnd, void *stream)
{
	int rc = jc_check(ctx, "sphx_jacobi_update_effpres");
	if (rc != SPHX_OK) return rc;
	SPHX_REQUIRE(effpres && jacobi && info, "sphx_jacobi_update_effpres: missing buffer");
	SPHX_REQUIRE(particleRangeEnd <= numParticles, "sphx_jacobi_update_effpres: range beyond the particles");
	hipStream_t st = (hipStream_t)stream;
	SPHX_HIP(hipMemsetAsync(ctx->gr.ctl + JC_RESIDUAL, 0, sizeof(uint32_t), st));
	if (particleRangeEnd) {
		jacobi_update_kernel<<<div_up_u(particleRangeEnd, 128), 128, 0, st>>>(ctx->dev, effpres, (const float4*)jacobi,
			(const particleinfo*)info, ctx->gr.ctl + JC_RESIDUAL, particleRangeEnd);
		SPHX_LAUNCH_CHECK("jacobi_update_kernel");
	}
	return jc_read_max(ctx, JC_RESIDUAL, h_residual, st);
}

// grow-only scratch of the solve: arrays that share one capacity.  Nothing of a solve outlives it, so growing drops the old arrays
template<class C, class... T> static int jc_reserve(C &cap, size_t need, T *&... ptr)
{
	if (need <= cap && (... && (ptr != nullptr))) return SPHX_OK;
	((ptr ? (void)hipFree(ptr) : (void)0, ptr = nullptr), ...);
	cap = 0;
	hipError_t e = hipSuccess;
	((e = (e == hipSuccess) ? hipMalloc((void**)&ptr, sizeof(T)*(need ? need : 1)) : e), ...);
	if (e != hipSuccess) return sphx_set_error(SPHX_ERR_RUNTIME, std::string("sphx_jacobi_solve: scratch: ") + hipGetErrorString(e));
	cap = (C)need;
	return SPHX_OK;
}

// The whole solve on `stream`: preparation (Dirichlet rows, wall rows, counter reset), assembly, then iterations of {sweep, wall
// pass, stop test} until the device-side test fires.  One solve at a time per context (the scratch and the control words are the
// context's).  Two host synchronisations for the assembly (row counts) and one per batch of iterations.
extern "C" int sphx_jacobi_solve(sphx_ctx *ctx, float *effpres,
	const void *pos, const void *vel, const void *info, const uint32_t *hash, const uint32_t *cellStart, const uint16_t *neibsList,
	uint32_t numParticles, uint32_t particleRangeEnd, float deltap, uint32_t *iterations, float *backerr, float *residual, void *stream)
{
	int rc = jc_check(ctx, "sphx_jacobi_solve");
	if (rc != SPHX_OK) return rc;
	SPHX_REQUIRE(effpres && pos && vel && info && hash && cellStart && neibsList, "sphx_jacobi_solve: missing buffer");
	SPHX_REQUIRE(particleRangeEnd <= numParticles, "sphx_jacobi_solve: range beyond the particles");
	SPHX_REQUIRE(numParticles < JE_RHS, "sphx_jacobi_solve: more than 2^31 particles");      // bit 31 of an entry is JE_RHS
	hipStream_t st = (hipStream_t)stream;
	GranularState &g = ctx->gr;
	const JcArgs a = jc_args(pos, vel, info, hash, cellStart, neibsList);
	const uint32_t n = particleRangeEnd;
	// preparation (initializeEffPresSolverPrepSequence): the passes of the entry points themselves
	if (n) {
		jacobi_fs_kernel<<<div_up_u(n, 128), 128, 0, st>>>(ctx->dev, effpres, a.pos, a.info, n, deltap);
		SPHX_LAUNCH_CHECK("jacobi_fs_kernel");
	}
	if ((rc = jc_wall_launch(ctx, effpres, a, n, st)) != SPHX_OK) return rc;
	SPHX_HIP(hipMemsetAsync(g.ctl, 0, JC_WORDS*sizeof(uint32_t), st));      // JACOBI_RESET_STOP_CRITERION, and the row counters
	// assembly
	if ((rc = jc_reserve(g.rows_cap, numParticles, g.rows_int, g.rows_wall, g.cnt_int, g.cnt_wall, g.pres2, g.diag)) != SPHX_OK) return rc;
	if (n) {
		jacobi_classify_kernel<<<div_up_u(n, 128), 128, 0, st>>>(ctx->dev, a, g.ctl, g.rows_int, g.cnt_int, g.rows_wall, g.cnt_wall, n);
		SPHX_LAUNCH_CHECK("jacobi_classify_kernel");
	}
	SPHX_HIP(hipMemcpyAsync(g.ctl_host, g.ctl, JC_WORDS*sizeof(uint32_t), hipMemcpyDeviceToHost, st));
	SPHX_HIP(hipStreamSynchronize(st));
	const uint32_t nInt = g.ctl_host[JC_NINT], nWall = g.ctl_host[JC_NWALL], maxInt = g.ctl_host[JC_MAXINT], maxWall = g.ctl_host[JC_MAXWALL];
	SPHX_REQUIRE(nInt <= n && nWall <= n, "sphx_jacobi_solve: row count beyond the particles");
	if ((rc = jc_reserve(g.ent_int_cap, (size_t)nInt*maxInt, g.ent_int)) != SPHX_OK ||
		(rc = jc_reserve(g.ent_wall_cap, (size_t)nWall*maxWall, g.ent_wall_j, g.ent_wall_ab)) != SPHX_OK) return rc;
	if (nInt) {
		jacobi_fill_interior_kernel<<<div_up_u(nInt, 128), 128, 0, st>>>(ctx->dev, a, g.rows_int, g.ent_int, g.diag, nInt, maxInt);
		SPHX_LAUNCH_CHECK("jacobi_fill_interior_kernel");
	}
	if (nWall) {
		jacobi_fill_wall_kernel<<<div_up_u(nWall, 128), 128, 0, st>>>(ctx->dev, a, g.rows_wall, g.ent_wall_j, g.ent_wall_ab, nWall, maxWall);
		SPHX_LAUNCH_CHECK("jacobi_fill_wall_kernel");
	}
	if (numParticles) SPHX_HIP(hipMemcpyAsync(g.pres2, effpres, sizeof(float)*(size_t)numParticles, hipMemcpyDeviceToDevice, st));
	// iterations.  The host cannot know when the test will fire, so it enqueues a batch and then reads flag and counter once.
	// Iterations enqueued behind the one that fired cost three empty launches each; a read costs a drained queue.  Batches start
	// at 8 iterations and double up to 256: the empty launches stay below the number of iterations that did run (plus the first
	// batch), the reads grow with its logarithm, and no batch goes past the maxiter + 2 iterations a solve can have at most.
	const uint64_t most = (uint64_t)g.maxiter + 2u;
	uint64_t enqueued = 0;
	uint32_t batch = 8;
	for (;;) {
		const uint64_t upto = enqueued + batch < most ? enqueued + batch : most;
		for (; enqueued < upto; ++enqueued) {
			const float *src = (enqueued & 1u) ? g.pres2 : effpres;
			float *dst = (enqueued & 1u) ? effpres : g.pres2;
			if (nInt) {
				jacobi_sweep_interior_kernel<<<div_up_u(nInt, 128), 128, 0, st>>>(g.ctl + JC_FLAG, g.ctl + JC_RESIDUAL, src, dst,
					g.rows_int, g.cnt_int, g.ent_int, g.diag, nInt);
				SPHX_LAUNCH_CHECK("jacobi_sweep_interior_kernel");
			}
			if (nWall) {
				jacobi_sweep_wall_kernel<<<div_up_u(nWall, 128), 128, 0, st>>>(ctx->dev, g.ctl + JC_FLAG, g.ctl + JC_BACKERR, src, dst,
					g.rows_wall, g.cnt_wall, g.ent_wall_j, g.ent_wall_ab, nWall);
				SPHX_LAUNCH_CHECK("jacobi_sweep_wall_kernel");
			}
			jacobi_stop_kernel<<<1, 1, 0, st>>>(g.ctl, g.maxiter, g.backerr, g.residual);
			SPHX_LAUNCH_CHECK("jacobi_stop_kernel");
		}
		SPHX_HIP(hipMemcpyAsync(g.ctl_host, g.ctl, 8*sizeof(uint32_t), hipMemcpyDeviceToHost, st));
		SPHX_HIP(hipStreamSynchronize(st));
		if (g.ctl_host[JC_FLAG]) break;
		if (enqueued >= most) return sphx_set_error(SPHX_ERR_RUNTIME, "sphx_jacobi_solve: the stop test has not fired after maxiter + 2 iterations");
		if (batch < 256) batch *= 2;
	}
	// iteration k (from 0) wrote pres2 when k is even: bring the last one home
	if (((g.ctl_host[JC_EXEC] - 1u) & 1u) == 0u && numParticles)
		SPHX_HIP(hipMemcpyAsync(effpres, g.pres2, sizeof(float)*(size_t)numParticles, hipMemcpyDeviceToDevice, st));
	if (iterations) *iterations = g.ctl_host[JC_COUNTER];
	if (backerr) memcpy(backerr, g.ctl_host + JC_LAST_BACKERR, sizeof(float));
	if (residual) memcpy(residual, g.ctl_host + JC_LAST_RESIDUAL, sizeof(float));
	return SPHX_OK;
}
