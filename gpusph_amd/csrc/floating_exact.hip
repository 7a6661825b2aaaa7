// floating_exact.hip -- the total force and torque on a floating body as the EXACTLY ROUNDED sum of its RB_FORCES / RB_TORQUES rows,
// whatever the order of the rows and however they are split among ranks, for gfx950.  floating.hip sums in double: good to
// n 2^-52 sum|term|, but the bits depend on the order, so slabs of a run would drift from the single domain at rounding level, and
// the total feeds back into every particle of the body.  Here every rank sums its rows into a long fixed-point accumulator in
// integer arithmetic (floating_exact.h has the format), the accumulators travel as integer-valued doubles through the sum
// all-reduce that is there already, and the sum is rounded to double once.  One slab or three: the same bits.
//
//   floating_limbs_kernel         the grid of floating_partials_kernel (the same number of 256-thread blocks per body).  A lane splits
//                                 a float into sign, 24-bit significand and bit position p = e + 149; the significand shifted by p % 32
//                                 spans at most two 32-bit limbs, p / 32 and the next, and is added there, negated for a negative
//                                 row, with 64-bit integer LDS atomics into the accumulator of the lane's wave: integers, so the
//                                 order is immaterial, and one accumulator per wave so that the four waves of a block do not queue
//                                 on the same few addresses.  (Sixty limbs per lane in registers would have to be indexed by p:
//                                 scratch; or be visited all sixty per row with a select: about 300 VALU operations per row against
//                                 twelve LDS atomics.)  A limb takes at most one term below 2^32 per row: 2^31 rows before a signed
//                                 64-bit limb could overflow, and a block sees 2^26 of a body's 2^32 at the most.  The waves are folded
//                                 into [body][block][6][13] signed 64-bit, no zeroing needed, no global atomics.
//   floating_limbs_finish_kernel  one wave per body, a lane per limb: the blocks' sums split into their low 32 bits and the signed
//                                 rest (so that 64 blocks cannot overflow), limb k takes the low halves of its own and the high
//                                 halves of limb k-1's, and six lanes propagate the carries: the canonical limbs, as doubles.
//   floating_round_kernel         after the all-reduce (limbs up to world 2^32): carries in int64, sign and magnitude, the leading
//                                 bit, round to nearest even at 53 bits in integer arithmetic, scaled by 2^-149 with ldexp (exact:
//                                 the result is a normal double).  The six totals go where floating_step_kernel reads its first
//                                 block of partials, and the rule runs unchanged over one block (0.0 + x is x).
// Compiled without FMA contraction like floating.hip; there is no floating-point addition in this file.
#include "floating_exact.h"
#include <cmath>

// one float into the accumulator acc[FLOAT_SLOTS] of its component
__device__ __forceinline__ void floating_limbs_add(unsigned long long *acc, float v)
{
	const uint32_t u = __float_as_uint(v);
	const uint32_t E = (u >> 23) & 0xFFu, M = u & 0x7FFFFFu;
	const bool neg = (u >> 31) != 0u;
	if (E == 0xFFu) {      // not finite: counted, never summed
		atomicAdd(&acc[FLOAT_LIMBS + (M ? 0 : neg ? 2 : 1)], 1ull);
		return;
	}
	const uint32_t sig = E ? (M | 0x800000u) : M;      // v = sig 2^(p - 149)
	if (sig == 0u) return;
	const uint32_t p = E ? E - 1u : 0u;                // 0 .. 253: limbs 0 .. 8
	const unsigned long long w = (unsigned long long)sig << (p & 31u);
	unsigned long long lo = w & 0xFFFFFFFFull, hi = w >> 32;
	if (neg) { lo = 0ull - lo; hi = 0ull - hi; }      // two's complement: the limbs are signed sums
	atomicAdd(&acc[p >> 5], lo);
	if (hi) atomicAdd(&acc[(p >> 5) + 1u], hi);
}

__global__ void __launch_bounds__(FLOAT_BLOCK)
floating_limbs_kernel(const FloatingDev *__restrict__ d, FloatingExactDev *__restrict__ x, const float4 *__restrict__ rbforces,
	const float4 *__restrict__ rbtorques, uint32_t blocksPerBody)
{
	__shared__ unsigned long long sAcc[FLOAT_LIMB_WAVES][6][FLOAT_SLOTS];
	const uint32_t wave = threadIdx.x >> 6;
	const uint32_t body = blockIdx.x/blocksPerBody, blk = blockIdx.x%blocksPerBody;
	const uint32_t first = d->rowstart[body], last = d->rowstart[body + 1];
	for (uint32_t i = threadIdx.x; i < FLOAT_LIMB_WAVES*6u*FLOAT_SLOTS; i += FLOAT_BLOCK) (&sAcc[0][0][0])[i] = 0ull;
	__syncthreads();
	// (64-bit row counter: the stride of the last round may pass 2^32)
	for (uint64_t row = (uint64_t)first + (uint64_t)blk*FLOAT_BLOCK + threadIdx.x; row < last; row += (uint64_t)blocksPerBody*FLOAT_BLOCK) {
		const float4 f = rbforces[row];
		const float4 t = rbtorques[row];
		floating_limbs_add(sAcc[wave][0], f.x); floating_limbs_add(sAcc[wave][1], f.y); floating_limbs_add(sAcc[wave][2], f.z);
		floating_limbs_add(sAcc[wave][3], t.x); floating_limbs_add(sAcc[wave][4], t.y); floating_limbs_add(sAcc[wave][5], t.z);
	}
	__syncthreads();
	if (threadIdx.x < 6u*FLOAT_SLOTS) {
		unsigned long long tot = 0ull;
		for (uint32_t w = 0; w < FLOAT_LIMB_WAVES; ++w) tot += (&sAcc[w][0][0])[threadIdx.x];
		(&x->part[body][blk][0][0])[threadIdx.x] = (long long)tot;
	}
}

__global__ void __launch_bounds__(64)
floating_limbs_finish_kernel(const FloatingExactDev *__restrict__ x, double *__restrict__ limbs, uint32_t blocksPerBody)
{
	__shared__ long long sLo[6][FLOAT_LIMBS], sHi[6][FLOAT_LIMBS];
	const uint32_t lane = threadIdx.x, body = blockIdx.x;
	if (lane < 6u*FLOAT_LIMBS) {
		const uint32_t c = lane/FLOAT_LIMBS, k = lane%FLOAT_LIMBS;
		long long lo = 0, hi = 0;      // v = hi 2^32 + lo with 0 <= lo < 2^32: 64 blocks stay below 2^38 in either
		for (uint32_t b = 0; b < blocksPerBody; ++b) {
			const long long v = x->part[body][b][c][k];
			lo += v & 0xFFFFFFFFll; hi += v >> 32;
		}
		sLo[c][k] = lo; sHi[c][k] = hi;
	}
	__syncthreads();
	double *out = limbs + (size_t)body*6u*FLOAT_SLOTS;
	if (lane < 6u) {      // the carries of one component
		long long carry = 0;
		for (uint32_t k = 0; k + 1u < FLOAT_LIMBS; ++k) {
			const long long s = sLo[lane][k] + (k ? sHi[lane][k - 1u] : 0ll) + carry;
			out[lane*FLOAT_SLOTS + k] = (double)(s & 0xFFFFFFFFll);
			carry = s >> 32;
		}
		const long long top = sLo[lane][FLOAT_LIMBS - 1] + sHi[lane][FLOAT_LIMBS - 1]*4294967296ll + sHi[lane][FLOAT_LIMBS - 2] + carry;
		out[lane*FLOAT_SLOTS + FLOAT_LIMBS - 1] = (double)top;
	} else if (lane >= 32u && lane < 32u + 18u) {      // the counts of the rows that are not finite
		const uint32_t c = (lane - 32u)/3u, j = FLOAT_LIMBS + (lane - 32u)%3u;
		long long n = 0;
		for (uint32_t b = 0; b < blocksPerBody; ++b) n += x->part[body][b][c][j];
		out[c*FLOAT_SLOTS + j] = (double)n;
	}
}

__global__ void __launch_bounds__(64)
floating_round_kernel(FloatingDev *__restrict__ d, const double *__restrict__ limbs)
{
	__shared__ uint32_t sM[6][FLOAT_LIMBS + 2];      // the magnitude: limb 9 may need two words, and one of zeros behind them
	const uint32_t c = threadIdx.x, body = blockIdx.x;
	if (c >= 6u) return;
	const double *L = limbs + ((size_t)body*6u + c)*FLOAT_SLOTS;
	uint32_t *m = sM[c];
	long long carry = 0;
	for (int k = 0; k + 1 < FLOAT_LIMBS; ++k) {
		const long long s = (long long)L[k] + carry;
		m[k] = (uint32_t)(s & 0xFFFFFFFFll);
		carry = s >> 32;
	}
	long long top = (long long)L[FLOAT_LIMBS - 1] + carry;
	const bool neg = top < 0;
	if (neg) {      // N = top 2^288 + R, 0 <= R < 2^288: -N = (-top - 1) 2^288 + (2^288 - R), or -top 2^288 when R = 0
		unsigned long long cy = 1ull;
		for (int k = 0; k + 1 < FLOAT_LIMBS; ++k) {
			const unsigned long long s = (unsigned long long)(uint32_t)~m[k] + cy;
			m[k] = (uint32_t)s;
			cy = s >> 32;
		}
		top = -top - 1 + (long long)cy;
	}
	m[FLOAT_LIMBS - 1] = (uint32_t)((unsigned long long)top & 0xFFFFFFFFull);
	m[FLOAT_LIMBS] = (uint32_t)((unsigned long long)top >> 32);
	m[FLOAT_LIMBS + 1] = 0u;
	int lead = -1;
	for (int k = 0; k <= FLOAT_LIMBS; ++k) if (m[k]) lead = k;
	double r = 0.0;
	if (lead >= 0) {
		const int bits = 32*lead + 32 - __builtin_clz(m[lead]);
		const int shift = bits > 53 ? bits - 53 : 0;      // the 53 leading bits start here
		const int i = shift >> 5, s = shift & 31;
		unsigned long long sig = ((((unsigned long long)m[i + 1]) << 32) | m[i]) >> s;
		if (s) sig |= ((unsigned long long)m[i + 2]) << (64 - s);
		sig &= (1ull << 53) - 1ull;
		if (shift) {      // to nearest, ties to even: the bit below, and whether anything lies below that
			const int rb = shift - 1;
			const bool half = ((m[rb >> 5] >> (rb & 31)) & 1u) != 0u;
			bool rest = (m[rb >> 5] & ((1u << (rb & 31)) - 1u)) != 0u;
			for (int k = 0; k < (rb >> 5); ++k) rest = rest || m[k] != 0u;
			if (half && (rest || (sig & 1ull))) sig += 1ull;      // 2^53 is a double too
		}
		r = ldexp((double)sig, shift - 149);
		if (neg) r = -r;
	}
	const double nans = L[FLOAT_LIMBS], pinf = L[FLOAT_LIMBS + 1], ninf = L[FLOAT_LIMBS + 2];
	if (nans > 0.0 || (pinf > 0.0 && ninf > 0.0)) r = __builtin_nan("");
	else if (pinf > 0.0) r = __builtin_inf();
	else if (ninf > 0.0) r = -__builtin_inf();
	d->partials[body][0][c] = r;
}

extern "C" int sphx_floating_limbs(sphx_ctx *ctx, const void *rbforces, const void *rbtorques, double *d_limbs, void *stream)
{
	SPHX_REQUIRE(ctx && ctx->have_params, "sphx_floating_limbs: constants not set");
	FloatingEntry *e = sphx_floating_entry(ctx);
	SPHX_REQUIRE(e && e->numfloating > 0 && e->exact, "sphx_floating_limbs: no floating bodies (sphx_floating_setup)");
	SPHX_REQUIRE(rbforces && rbtorques, "sphx_floating_limbs: missing buffer (RB_FORCES, RB_TORQUES)");
	SPHX_REQUIRE(d_limbs != nullptr, "sphx_floating_limbs: NULL d_limbs");
	hipStream_t st = (hipStream_t)stream;
	if (int rc = sphx_rb_flush(ctx, st)) return rc;
	FloatingExactDev *x = (FloatingExactDev*)e->exact;
	const uint32_t bodies = (uint32_t)e->numfloating, grid = bodies*e->blocks;
	floating_limbs_kernel<<<grid, FLOAT_BLOCK, 0, st>>>(e->dev, x, (const float4*)rbforces, (const float4*)rbtorques, e->blocks);
	SPHX_LAUNCH_CHECK("floating_limbs_kernel");
	floating_limbs_finish_kernel<<<bodies, 64, 0, st>>>(x, d_limbs, e->blocks);
	SPHX_LAUNCH_CHECK("floating_limbs_finish_kernel");
	return SPHX_OK;
}

extern "C" int sphx_floating_move_limbs(sphx_ctx *ctx, const double *d_limbs, int step, const float *d_dt, void *stream)
{
	SPHX_REQUIRE(ctx && ctx->have_params, "sphx_floating_move_limbs: constants not set");
	FloatingEntry *e = sphx_floating_entry(ctx);
	SPHX_REQUIRE(e && e->numfloating > 0 && e->step, "sphx_floating_move_limbs: no floating bodies (sphx_floating_setup)");
	SPHX_REQUIRE(step == 1 || step == 2, "sphx_floating_move_limbs: step is 1 (predictor) or 2 (corrector)");
	SPHX_REQUIRE(d_dt != nullptr, "sphx_floating_move_limbs: missing buffer (dt)");
	SPHX_REQUIRE(d_limbs != nullptr, "sphx_floating_move_limbs: NULL d_limbs");
	hipStream_t st = (hipStream_t)stream;
	// pending host uploads first, so that this call's writes come last
	if (int rc = sphx_rb_flush(ctx, st)) return rc;
	const uint32_t bodies = (uint32_t)e->numfloating;
	floating_round_kernel<<<bodies, 64, 0, st>>>(e->dev, d_limbs);
	SPHX_LAUNCH_CHECK("floating_round_kernel");
	return e->step(ctx, e, 1u, step, d_dt, st);
}
