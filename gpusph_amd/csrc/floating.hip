// floating.hip -- the rigid-body dynamics of floating bodies (GT_FLOATING_BODY of the reference's problems) for gfx950: the step
// between the RB_FORCES / RB_TORQUES rows the forces passes write and the rigid-body table the Euler kernel moves the bodies'
// particles from.  The reference sums the rows on the device, reads the totals to the host, hands them to Chrono
// (ProblemCore::bodies_timestep, src/ProblemCore.cc:484-618) and uploads translation, step rotation, velocities and centres of
// gravity again, in every substep.  Here the table never leaves the device: two small launches per substep, no host read.
//
// The rule is this project's own (DESIGN.md "Floating bodies", tests/floating_ref.py): semi-implicit Euler on an unconstrained
// body, everything in double, dt1 = dt/2 in the predictor and dt in the corrector, formed in double from the float dt on the device.
// State: centre of rotation x, orientation q (unit quaternion w, x, y, z; R(q) turns body axes into world axes), linear velocity v,
// angular velocity w in the world frame; constants mass m and principal inertia I.  One substep:
//   1. step 1 saves (x, q, v, w) as the state of step n, step 2 starts from what was saved
//   2. v' = v + dt1 (F/m + g)                               gravity belongs here: the rows of body particles carry none
//   3. wb = R(q)^T w, Tb = R(q)^T T, wb' = wb + dt1 I^-1 (Tb - wb x (I wb)), w' = R(q) wb'
//   4. x' = x + dt1 v'
//   5. q' = normalize(q * exp(dt1 wb'/2)), the exact exponential of the constant body rate (sin(h)/h by its series below 1e-4)
//   6. the body's slot of RbParams, rounded to float: trans = x' - x, steprot = R(q' * q^-1), linearvel = v', angularvel = w',
//      the forces engine's centre = grid cell and cell-local position of x', the integration engine's = those of x (step n)
// Contact between bodies and with walls (Chrono's in the reference) is not built.
//
// Same state in, same bits out: no floating-point atomics.  floating_partials_kernel gives every body the same number of blocks
// (a function of the row counts, at most FLOAT_MAX_BLOCKS); a lane sums its rows in index order in double, the lanes of a wave meet
// in a butterfly, the waves of a block are folded in wave order into [body][block][6].  floating_step_kernel, one wave per body,
// folds the blocks in block order and lane 0 applies the rule.  Compiled without FMA contraction, so that the terms are the host's.
#include "floating.h"
#include <cmath>

struct FloatingGrid {      // cell size, world origin and gravity as uploaded (floats, widened), the grid size
	double cs[3], wo[3], g[3];
	int    gs[3];
};

__global__ void __launch_bounds__(FLOAT_BLOCK)
floating_partials_kernel(FloatingDev *__restrict__ d, const float4 *__restrict__ rbforces, const float4 *__restrict__ rbtorques,
	uint32_t blocksPerBody)
{
	__shared__ double sAcc[FLOAT_WAVES][6];
	const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
	const uint32_t body = blockIdx.x/blocksPerBody, blk = blockIdx.x%blocksPerBody;
	const uint32_t first = d->rowstart[body], last = d->rowstart[body + 1];
	double acc[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
	// (64-bit row counter: the stride of the last round may pass 2^32)
	for (uint64_t row = (uint64_t)first + (uint64_t)blk*FLOAT_BLOCK + threadIdx.x; row < last; row += (uint64_t)blocksPerBody*FLOAT_BLOCK) {
		const float4 f = rbforces[row];
		const float4 t = rbtorques[row];
		acc[0] += (double)f.x; acc[1] += (double)f.y; acc[2] += (double)f.z;
		acc[3] += (double)t.x; acc[4] += (double)t.y; acc[5] += (double)t.z;
	}
	// the lanes of the wave: after the butterfly every lane holds the same values (a + b and b + a are the same bits)
#pragma unroll
	for (int s = 1; s < 64; s <<= 1) {
#pragma unroll
		for (int k = 0; k < 6; ++k) acc[k] += __shfl_xor(acc[k], s);
	}
	if (lane == 0) {
#pragma unroll
		for (int k = 0; k < 6; ++k) sAcc[wave][k] = acc[k];
	}
	__syncthreads();
	if (threadIdx.x < 6) {
		double tot = 0.0;
		for (uint32_t w = 0; w < FLOAT_WAVES; ++w) tot += sAcc[w][threadIdx.x];
		d->partials[body][blk][threadIdx.x] = tot;
	}
}

// R(q), row-major
__device__ __forceinline__ void floating_rotmat(const double q[4], double R[9])
{
	const double w = q[0], x = q[1], y = q[2], z = q[3];
	R[0] = 1.0 - 2.0*(y*y + z*z); R[1] = 2.0*(x*y - w*z);       R[2] = 2.0*(x*z + w*y);
	R[3] = 2.0*(x*y + w*z);       R[4] = 1.0 - 2.0*(x*x + z*z); R[5] = 2.0*(y*z - w*x);
	R[6] = 2.0*(x*z - w*y);       R[7] = 2.0*(y*z + w*x);       R[8] = 1.0 - 2.0*(x*x + y*y);
}

// a * b (Hamilton product)
__device__ __forceinline__ void floating_qmul(const double a[4], const double b[4], double o[4])
{
	o[0] = a[0]*b[0] - a[1]*b[1] - a[2]*b[2] - a[3]*b[3];
	o[1] = a[0]*b[1] + a[1]*b[0] + a[2]*b[3] - a[3]*b[2];
	o[2] = a[0]*b[2] - a[1]*b[3] + a[2]*b[0] + a[3]*b[1];
	o[3] = a[0]*b[3] + a[1]*b[2] - a[2]*b[1] + a[3]*b[0];
}

// grid cell and cell-local position of x, as MovingBodies.grid_and_local (bodies.py) forms them; a non-finite x lands in cell 0
__device__ __forceinline__ void floating_grid_and_local(const FloatingGrid &G, const double x[3], int cell[3], float local[3])
{
	for (int a = 0; a < 3; ++a) {
		const double rel = x[a] - G.wo[a];
		const double c = fmin(fmax(floor(rel/G.cs[a]), 0.0), (double)(G.gs[a] - 1));
		cell[a] = (int)c;
		local[a] = (float)(rel - (c + 0.5)*G.cs[a]);
	}
}

__global__ void __launch_bounds__(64)
floating_step_kernel(FloatingDev *__restrict__ d, RbParams *__restrict__ rb, FloatingGrid G, uint32_t blocksPerBody, int step,
	const float *__restrict__ d_dt)
{
	const uint32_t lane = threadIdx.x, body = blockIdx.x;
	// lane k < 6 folds value k of the body's blocks in block order; lane 0 collects the six totals
	double tot = 0.0;
	if (lane < 6u)
		for (uint32_t b = 0; b < blocksPerBody; ++b) tot += d->partials[body][b][lane];
	double FT[6];
#pragma unroll
	for (int k = 0; k < 6; ++k) FT[k] = __shfl(tot, k);
	if (lane != 0) return;
	double *S = d->state[body], *K = d->saved[body];
	if (step == 1) { for (int k = 0; k < FLOAT_KEPT; ++k) K[k] = S[k]; }
	double x[3], q[4], v[3], w[3];
	for (int a = 0; a < 3; ++a) { x[a] = K[a]; v[a] = K[7 + a]; w[a] = K[10 + a]; }
	for (int a = 0; a < 4; ++a) q[a] = K[3 + a];
	const double m = d->consts[body][0];
	const double I[3] = {d->consts[body][1], d->consts[body][2], d->consts[body][3]};
	const double dt = (double)d_dt[0];
	const double dt1 = step == 1 ? 0.5*dt : dt;
	double R[9];
	floating_rotmat(q, R);
	double v1[3], x1[3], wb[3], Tb[3], wb1[3], w1[3];
	for (int a = 0; a < 3; ++a) v1[a] = v[a] + dt1*(FT[a]/m + G.g[a]);
	for (int a = 0; a < 3; ++a) {
		wb[a] = R[a]*w[0] + R[3 + a]*w[1] + R[6 + a]*w[2];
		Tb[a] = R[a]*FT[3] + R[3 + a]*FT[4] + R[6 + a]*FT[5];
	}
	const double Iw[3] = {I[0]*wb[0], I[1]*wb[1], I[2]*wb[2]};
	const double gy[3] = {wb[1]*Iw[2] - wb[2]*Iw[1], wb[2]*Iw[0] - wb[0]*Iw[2], wb[0]*Iw[1] - wb[1]*Iw[0]};
	for (int a = 0; a < 3; ++a) wb1[a] = wb[a] + dt1*((Tb[a] - gy[a])/I[a]);
	for (int a = 0; a < 3; ++a) w1[a] = R[3*a]*wb1[0] + R[3*a + 1]*wb1[1] + R[3*a + 2]*wb1[2];
	for (int a = 0; a < 3; ++a) x1[a] = x[a] + dt1*v1[a];
	const double rate = sqrt(wb1[0]*wb1[0] + wb1[1]*wb1[1] + wb1[2]*wb1[2]);
	const double h = 0.5*dt1*rate;
	const double sinc = fabs(h) < 1.0e-4 ? 1.0 - h*h/6.0 : sin(h)/h;
	const double e[4] = {cos(h), 0.5*dt1*sinc*wb1[0], 0.5*dt1*sinc*wb1[1], 0.5*dt1*sinc*wb1[2]};
	double q1[4], dq[4], dR[9];
	floating_qmul(q, e, q1);
	const double nq = sqrt(q1[0]*q1[0] + q1[1]*q1[1] + q1[2]*q1[2] + q1[3]*q1[3]);
	for (int a = 0; a < 4; ++a) q1[a] = q1[a]/nq;
	const double qc[4] = {q[0], -q[1], -q[2], -q[3]};
	floating_qmul(q1, qc, dq);
	floating_rotmat(dq, dR);
	// the device state and the totals it was made from
	for (int a = 0; a < 3; ++a) { S[a] = x1[a]; S[7 + a] = v1[a]; S[10 + a] = w1[a]; S[13 + a] = FT[a]; S[16 + a] = FT[3 + a]; }
	for (int a = 0; a < 4; ++a) S[3 + a] = q1[a];
	// the body's slot of the rigid-body table
	int cell[3], cellE[3];
	float local[3], localE[3];
	floating_grid_and_local(G, x1, cell, local);
	floating_grid_and_local(G, x, cellE, localE);
	for (int a = 0; a < 3; ++a) {
		rb->trans[body][a] = (float)(x1[a] - x[a]);
		rb->linearvel[body][a] = (float)v1[a];
		rb->angularvel[body][a] = (float)w1[a];
		rb->cgGridPos[body][a] = cell[a]; rb->cgPos[body][a] = local[a];
		rb->cgGridPosE[body][a] = cellE[a]; rb->cgPosE[body][a] = localE[a];
	}
	for (int a = 0; a < 9; ++a) rb->steprot[body][a] = (float)dR[a];
}

// the host's table (image) -> rb, the slots of bodies numfloating .. SPHX_MAX_BODIES-1 only; rbstart is the host's for every body
__global__ void __launch_bounds__(64)
floating_merge_kernel(RbParams *__restrict__ rb, const RbParams *__restrict__ image, int numfloating)
{
	const int lane = (int)threadIdx.x;
	auto take = [&](auto *dst, const auto *src, int per) {
		for (int i = lane; i < SPHX_MAX_BODIES*per; i += 64)
			if (i/per >= numfloating) dst[i] = src[i];
	};
	take(&rb->cgGridPos[0][0], &image->cgGridPos[0][0], 3);
	take(&rb->cgPos[0][0], &image->cgPos[0][0], 3);
	take(&rb->cgGridPosE[0][0], &image->cgGridPosE[0][0], 3);
	take(&rb->cgPosE[0][0], &image->cgPosE[0][0], 3);
	take(&rb->trans[0][0], &image->trans[0][0], 3);
	take(&rb->steprot[0][0], &image->steprot[0][0], 9);
	take(&rb->linearvel[0][0], &image->linearvel[0][0], 3);
	take(&rb->angularvel[0][0], &image->angularvel[0][0], 3);
	if (lane < SPHX_MAX_BODIES) rb->rbstart[lane] = image->rbstart[lane];
}

static int floating_merge(sphx_ctx *ctx, const FloatingEntry *e, hipStream_t st)
{
	floating_merge_kernel<<<1, 64, 0, st>>>(ctx->rb_dev, e->rb_image, e->numfloating);
	SPHX_LAUNCH_CHECK("floating_merge_kernel");
	return SPHX_OK;
}

// the rule over the first blocksPerBody rows of every body's partials (floating_exact.hip reaches it through FloatingEntry::step)
static int floating_step(sphx_ctx *ctx, const FloatingEntry *e, uint32_t blocksPerBody, int step, const float *d_dt, hipStream_t st)
{
	FloatingGrid G;
	for (int a = 0; a < 3; ++a) {
		G.cs[a] = (double)ctx->params.cellSize[a]; G.wo[a] = (double)ctx->params.worldOrigin[a]; G.g[a] = (double)ctx->params.gravity[a];
		G.gs[a] = (int)ctx->params.gridSize[a];
	}
	const uint32_t bodies = (uint32_t)e->numfloating;
	floating_step_kernel<<<bodies, 64, 0, st>>>(e->dev, ctx->rb_dev, G, blocksPerBody, step, d_dt);
	SPHX_LAUNCH_CHECK("floating_step_kernel");
	return SPHX_OK;
}

extern "C" int sphx_floating_setup(sphx_ctx *ctx, int numfloating, const double *h_mass, const double *h_inertia3,
	const double *h_crot3, const double *h_orientation4, const double *h_lvel3, const double *h_avel3, const uint32_t *h_rowstart)
{
	SPHX_REQUIRE(ctx && ctx->have_params, "sphx_floating_setup: constants not set");
	SPHX_REQUIRE(numfloating >= 0, "sphx_floating_setup: negative number of bodies");
	SPHX_REQUIRE(numfloating <= SPHX_MAX_BODIES, "sphx_floating_setup: too many bodies");
	if (numfloating == 0) {      // the feature is dropped: the host owns every slot again
		FloatingEntry *e = sphx_floating_entry(ctx);
		if (e) e->numfloating = 0;
		return SPHX_OK;
	}
	SPHX_REQUIRE(h_mass && h_inertia3 && h_crot3 && h_orientation4 && h_lvel3 && h_avel3 && h_rowstart, "sphx_floating_setup: missing array");
	for (int b = 0; b < numfloating; ++b) {
		SPHX_REQUIRE(h_mass[b] > 0.0 && std::isfinite(h_mass[b]), "sphx_floating_setup: the mass of a body must be positive");
		for (int a = 0; a < 3; ++a)
			SPHX_REQUIRE(h_inertia3[3*b + a] > 0.0 && std::isfinite(h_inertia3[3*b + a]), "sphx_floating_setup: the principal inertia of a body must be positive");
		const double *q = h_orientation4 + 4*b;
		const double n2 = q[0]*q[0] + q[1]*q[1] + q[2]*q[2] + q[3]*q[3];
		SPHX_REQUIRE(n2 > 0.0 && std::isfinite(n2), "sphx_floating_setup: the orientation of a body is a zero quaternion");
		SPHX_REQUIRE(h_rowstart[b] <= h_rowstart[b + 1], "sphx_floating_setup: rowstart decreases");
	}
	FloatingEntry *e = sphx_floating_entry(ctx, true);
	if (!e->dev) SPHX_HIP(hipMalloc((void**)&e->dev, sizeof(FloatingDev)));
	if (!e->rb_image) SPHX_HIP(hipMalloc((void**)&e->rb_image, sizeof(RbParams)));
	if (!e->exact) SPHX_HIP(hipMalloc(&e->exact, FLOAT_EXACT_BYTES));      // so that no substep allocates (floating_exact.hip)
	e->merge = floating_merge;
	e->step = floating_step;
	// the host side of the state: staged here and copied in one piece behind everything the device still runs
	std::vector<double> state((size_t)SPHX_MAX_BODIES*FLOAT_STATE, 0.0), saved((size_t)SPHX_MAX_BODIES*FLOAT_KEPT, 0.0), consts((size_t)SPHX_MAX_BODIES*4, 1.0);
	uint32_t rowstart[SPHX_MAX_BODIES + 1], maxrows = 0;
	for (int b = 0; b <= SPHX_MAX_BODIES; ++b) rowstart[b] = h_rowstart[b < numfloating ? b : numfloating];
	for (int b = 0; b < numfloating; ++b) {
		double *S = &state[(size_t)b*FLOAT_STATE];
		const double *q = h_orientation4 + 4*b;
		// a quaternion that is a unit one to rounding (what floating_step_kernel leaves, what a HotFile holds) is taken bit for bit,
		// so that a resumed run continues with the bits it saved; anything else is normalised
		const double n2 = q[0]*q[0] + q[1]*q[1] + q[2]*q[2] + q[3]*q[3];
		const double nq = std::fabs(n2 - 1.0) <= 1.0e-12 ? 1.0 : std::sqrt(n2);
		for (int a = 0; a < 3; ++a) { S[a] = h_crot3[3*b + a]; S[7 + a] = h_lvel3[3*b + a]; S[10 + a] = h_avel3[3*b + a]; }
		for (int a = 0; a < 4; ++a) S[3 + a] = q[a]/nq;
		for (int k = 0; k < FLOAT_KEPT; ++k) saved[(size_t)b*FLOAT_KEPT + k] = S[k];
		consts[4*b] = h_mass[b];
		for (int a = 0; a < 3; ++a) consts[4*b + 1 + a] = h_inertia3[3*b + a];
		maxrows = std::max(maxrows, rowstart[b + 1] - rowstart[b]);
		// the body's first slot, through the host mirror: at rest relative to itself, both engines' centres at x
		for (int a = 0; a < 3; ++a) {
			const double rel = S[a] - (double)ctx->params.worldOrigin[a], cs = (double)ctx->params.cellSize[a];
			const double c = std::fmin(std::fmax(std::floor(rel/cs), 0.0), (double)((int)ctx->params.gridSize[a] - 1));
			ctx->rb_host.cgGridPos[b][a] = ctx->rb_host.cgGridPosE[b][a] = (int)c;
			ctx->rb_host.cgPos[b][a] = ctx->rb_host.cgPosE[b][a] = (float)(rel - (c + 0.5)*cs);
			ctx->rb_host.trans[b][a] = 0.0f;
			ctx->rb_host.linearvel[b][a] = (float)S[7 + a];
			ctx->rb_host.angularvel[b][a] = (float)S[10 + a];
		}
		for (int a = 0; a < 9; ++a) ctx->rb_host.steprot[b][a] = (a%4 == 0) ? 1.0f : 0.0f;
	}
	SPHX_HIP(hipDeviceSynchronize());
	SPHX_HIP(hipMemcpy(&e->dev->state[0][0], state.data(), sizeof(double)*state.size(), hipMemcpyHostToDevice));
	SPHX_HIP(hipMemcpy(&e->dev->saved[0][0], saved.data(), sizeof(double)*saved.size(), hipMemcpyHostToDevice));
	SPHX_HIP(hipMemcpy(&e->dev->consts[0][0], consts.data(), sizeof(double)*consts.size(), hipMemcpyHostToDevice));
	SPHX_HIP(hipMemcpy(&e->dev->rowstart[0], rowstart, sizeof(rowstart), hipMemcpyHostToDevice));
	const uint32_t blocks = div_up_u(maxrows, FLOAT_BLOCK);
	e->blocks = blocks < 1u ? 1u : blocks > (uint32_t)FLOAT_MAX_BLOCKS ? (uint32_t)FLOAT_MAX_BLOCKS : blocks;
	e->numfloating = numfloating;
	e->whole_upload = true;
	ctx->rb_dirty = true;
	return SPHX_OK;
}

extern "C" int sphx_floating_move(sphx_ctx *ctx, const void *rbforces, const void *rbtorques, int step, const float *d_dt, void *stream)
{
	SPHX_REQUIRE(ctx && ctx->have_params, "sphx_floating_move: constants not set");
	FloatingEntry *e = sphx_floating_entry(ctx);
	SPHX_REQUIRE(e && e->numfloating > 0, "sphx_floating_move: no floating bodies (sphx_floating_setup)");
	SPHX_REQUIRE(step == 1 || step == 2, "sphx_floating_move: step is 1 (predictor) or 2 (corrector)");
	SPHX_REQUIRE(rbforces && rbtorques && d_dt, "sphx_floating_move: missing buffer (RB_FORCES, RB_TORQUES, dt)");
	hipStream_t st = (hipStream_t)stream;
	// pending host uploads first, so that this call's writes come last
	if (int rc = sphx_rb_flush(ctx, st)) return rc;
	const uint32_t grid = (uint32_t)e->numfloating*e->blocks;
	floating_partials_kernel<<<grid, FLOAT_BLOCK, 0, st>>>(e->dev, (const float4*)rbforces, (const float4*)rbtorques, e->blocks);
	SPHX_LAUNCH_CHECK("floating_partials_kernel");
	return floating_step(ctx, e, e->blocks, step, d_dt, st);
}

extern "C" int sphx_floating_state(sphx_ctx *ctx, double *h_state, float *h_slots, void *stream)
{
	SPHX_REQUIRE(ctx != nullptr, "sphx_floating_state: NULL ctx");
	FloatingEntry *e = sphx_floating_entry(ctx);
	SPHX_REQUIRE(e && e->numfloating > 0, "sphx_floating_state: no floating bodies (sphx_floating_setup)");
	hipStream_t st = (hipStream_t)stream;
	if (int rc = sphx_rb_flush(ctx, st)) return rc;
	SPHX_HIP(hipStreamSynchronize(st));
	if (h_state)
		SPHX_HIP(hipMemcpy(h_state, &e->dev->state[0][0], sizeof(double)*FLOAT_STATE*(size_t)e->numfloating, hipMemcpyDeviceToHost));
	if (h_slots) {
		RbParams rb;
		SPHX_HIP(hipMemcpy(&rb, ctx->rb_dev, sizeof(RbParams), hipMemcpyDeviceToHost));
		for (int b = 0; b < e->numfloating; ++b) {
			float *o = h_slots + (size_t)SPHX_FLOATING_SLOT_WORDS*b;
			int32_t *oi = (int32_t*)(o + 24);
			for (int a = 0; a < 3; ++a) {
				o[a] = rb.trans[b][a]; o[12 + a] = rb.linearvel[b][a]; o[15 + a] = rb.angularvel[b][a];
				o[18 + a] = rb.cgPos[b][a]; o[21 + a] = rb.cgPosE[b][a];
				oi[a] = rb.cgGridPos[b][a]; oi[3 + a] = rb.cgGridPosE[b][a];
			}
			for (int a = 0; a < 9; ++a) o[3 + a] = rb.steprot[b][a];
		}
	}
	return SPHX_OK;
}
