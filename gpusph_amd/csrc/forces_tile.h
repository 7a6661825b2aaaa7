// forces_tile.h -- forces_tile_kernel, the tiled forces kernel ("Tiled path" below), with its modes: forces, SPS stress tensor,
// the SA_BOUNDARY sums.  It reads the tables of tile_format.h and keeps its list batches in the ring of tile_ring.h.
#ifndef SPHX_FORCES_TILE_H
#define SPHX_FORCES_TILE_H

#include "forces_pair.h"
#include "tile_format.h"
#include "tile_ring.h"

// the last workgroup of a launch re-arms the tile tickets for the next one (no memset launch in between)
__device__ __forceinline__ void tile_group_done(uint32_t *tileCtl)
{
	__threadfence();
	if (atomicAdd(tileCtl + 2, 1u) == gridDim.x - 1u) {
#pragma unroll
		for (int k = 0; k < 8; ++k) tileCtl[4 + k] = 0u;
		tileCtl[2] = 0u;
	}
}

// ==========================================================================================
// Tiled path (the fast one): LDS staging of the neighbour window per workgroup.
//
// A tile is a block of k x 2 x 2 cells (k consecutive cells along COORD1 in four adjacent grid rows) holding
// <= TILE_THREADS particles; its neighbour window is the (k+2) x 4 x 4 block around it, i.e. 16 contiguous
// particle ranges, because cells along COORD1 are contiguous in the sorted particle arrays.  The workgroup
// copies those ranges (pos, vel, EOS aux: 48 B/particle) into LDS once by DMA, then every thread walks its
// particle's neighbour list reading the neighbour rows from LDS with ds_read_b128 instead of gathering them
// through L1/L2 (where a 64-lane gather touches 12-20 different cache lines per instruction and the L2->L1
// line fills, ~1/4 used, were the bottleneck).  Tiles are produced by build_tiles_kernel (neibs.hip) at
// neighbour-list build time.  Persistent grid: one workgroup per CU (the window is the LDS), tiles handed out
// by per-XCD ticket counters.  DESIGN.md 5.2 has the full account.
// ==========================================================================================

// workgroup barrier that orders LDS traffic only.  __syncthreads() is a release/acquire fence over ALL address
// spaces: with global stores or loads in flight it drains vmcnt, i.e. it exposes an HBM round trip (the forces
// stores of the previous tile, the list batches just requested) at every barrier of the tile loop.
__device__ __forceinline__ void lds_barrier()
{
	__builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
	__builtin_amdgcn_s_barrier();
	__builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
}

__device__ __forceinline__ bool wave_any(bool x) { return __builtin_amdgcn_ballot_w64(x) != 0ull; }

// Tile lists.  The reference-format neighbour list (u16 entries: index within the neighbour cell, cell code on the
// first entry of each cell run) costs the pair loop a running cell code, two dependent LDS table look-ups (code ->
// first window slot of that cell as seen from the home cell, then the row itself), the shift of the own position into
// the neighbour's cell frame and a per-lane "still alive" flag: ~20 of ~70 vector instructions per pair plus a serial
// LDS round trip.  All of that depends only on the list and the tiling, i.e. it changes once per neighbour-list build,
// not once per forces pass (20 passes per build), so tile_lists_kernel (forces.hip) does it at build time and leaves, per
// stored neighbour, one uint16: the byte offset of the neighbour's row in the tile's window (slot * 16; the window arrays
// are parallel, 16 B per row, <= 4095 rows).  The cell shift is gone from the pair altogether because the window holds
// positions in one frame per tile (tile_shift, sphx_internal.h): the wave that stages a window row converts it.
// (Round 2 kept cell-local positions and a 4-bit code advance in the entry: 7 more vector instructions and one more
// 16-byte LDS read per pair.)
// Rows [0, nF) hold the fluid section, rows [R-nB, R) the boundary section (first entry in row R-1, like the
// reference's list runs down from neibboundpos); nF and nB are PER WAVE (multiples of TILE_LIST_BATCH): lanes with
// shorter lists are padded with offset 0, a dummy row (mass 0, far away), so the pair loop has a scalar trip
// count, no terminator test and no validity flag.  In memory the four rows of a batch are interleaved per particle
// ([batch][particle][4] uint16), so a lane fetches a whole batch with ONE 8-byte buffer load -- a quarter of the vector
// memory instructions of a row-per-load layout, whose 2-byte loads kept the CU's address unit busy for half of the
// pair loop's duration.  The pair loop is wave-uniform, so the batch number is a scalar: SGPR descriptor (slab base) +
// the per-lane byte offset index*8, which is fixed for the whole tile -- no vector address arithmetic at all.
struct StressAcc { float x, y, z, w, u; };   // stress mode: the accumulators that do not fit the float4 of the forces

// one pair of SPSstressMatrixDevice (src/cuda/visc_kernel.cu:759-811) in the tiled kernel: dv_ab -= (v_a - nv_a) r_b F m/rho_n,
// the nine sums in the order and arithmetic of sps_kernel, so both give the same bits (single fluid: rho_n from the
// neighbour's relative density); acc = dv[0..3], acc2 = dv[4..8]
template<int KERNEL>
__device__ __forceinline__ void stress_interact(const DevParams &p, const Self &s, float inv_h, float qx, float qy, float qz,
	const float4 &npos, const float4 &nvel, bool valid, float4 &acc, StressAcc &acc2)
{
	const float rx = qx - npos.x, ry = qy - npos.y, rz = qz - npos.z;
	const float r = fast_sqrt(fmaf(rz, rz, fmaf(ry, ry, rx*rx)));
	const bool on = valid && is_active_w(npos.w) && r < p.influenceradius;
	const float n_rho = (nvel.w + 1.0f)*p.rho0[0];
	const float wgt = kernel_F<KERNEL>(p, r, inv_h)*npos.w*fast_rcp(n_rho);
	const float weight = on ? wgt : 0.0f;
	const float mx = rx*weight, my = ry*weight, mz = rz*weight;
	const float vx = s.vel.x - nvel.x, vy = s.vel.y - nvel.y, vz = s.vel.z - nvel.z;
	acc.x -= vx*mx; acc.y -= vx*my; acc.z -= vx*mz;
	acc.w -= vy*mx; acc2.x -= vy*my; acc2.y -= vy*mz;
	acc2.z -= vz*mx; acc2.w -= vz*my; acc2.u -= vz*mz;
}

// SA_BOUNDARY, density summation (densitySumVolumicDevice, src/cuda/density_sum_kernel.cu:206-250): -m W(r^n) for every stored
// neighbour, + m W(r^n+1) for those still in range, as two sums (acc.x, acc.y).  The window holds the positions at step n and, in
// place of the velocities, the displacement n -> n+1 of every particle: r^n+1 = r^n + (d_i - d_j).  Pad entries have mass 0.
__device__ __forceinline__ void sa_dsum_interact(const DevParams &p, const Self &s, float inv_h, float qx, float qy, float qz,
	const float4 &npos, const float4 &ndisp, bool valid, float4 &acc)
{
	const float rx = qx - npos.x, ry = qy - npos.y, rz = qz - npos.z;
	const float m = valid ? npos.w : 0.0f;
	auto W = [&](float r) {
		const float R = r*inv_h;
		float val = fmaf(-0.5f, R, 1.0f);
		val *= val; val *= val;
		return val*fmaf(2.0f, R, 1.0f)*p.wcoeff;
	};
	const float rN = fast_sqrt(fmaf(rz, rz, fmaf(ry, ry, rx*rx)));
	acc.x = fmaf(-m, W(rN), acc.x);
	const float ux = rx + (s.vel.x - ndisp.x), uy = ry + (s.vel.y - ndisp.y), uz = rz + (s.vel.z - ndisp.z);
	const float rNp1 = fast_sqrt(fmaf(uz, uz, fmaf(uy, uy, ux*ux)));
	acc.y = fmaf((rNp1 < p.influenceradius) ? m : 0.0f, W(rNp1), acc.y);
}

// SA_BOUNDARY, Brezzi density diffusion (computeDensityDiffusionDevice, src/cuda/forces_kernel.def:1766-1783,4515-4560) of one
// fluid neighbour; the EOS rows give the neighbour's pressure and density.  acc.w accumulates, dt2rho = dt * 2 * rho_i
__device__ __forceinline__ void sa_diff_interact(const DevParams &p, const Self &s, float inv_h, float qx, float qy, float qz,
	const float4 &npos, const float4 &naux, bool valid, float dt2rho, float4 &acc)
{
	const float rx = qx - npos.x, ry = qy - npos.y, rz = qz - npos.z;
	const float r = fast_sqrt(fmaf(rz, rz, fmaf(ry, ry, rx*rx)));
	const bool on = valid && r < p.influenceradius;
	const float f = kernel_F<SPHX_WENDLAND>(p, r, inv_h);
	const float gdotr = fmaf(p.gravity[2], rz, fmaf(p.gravity[1], ry, p.gravity[0]*rx));
	const float n_rho = naux.w;
	const float t = p.densityDiffCoeff*fmaf(2.0f*fast_rcp(s.rho + n_rho), s.P - naux.z, -gdotr)*npos.w*fast_rcp(n_rho)*f*dt2rho;
	acc.w += on ? t : 0.0f;
}

#define TILE_HB 2   // pairs per pipeline stage ("half batch")
// window capacity of a tiled-kernel instantiation, and the LDS placement of the SPS rows behind the EOS rows
#define TILE_WC(T) ((TURB_MODEL(T) == SPHX_SPS) ? (((T) & SPHX_TURB_MF) ? TILE_WCAP_SPS : TILE_WCAP_SPS1) : TILE_WCAP)
// SPS, one fluid: no EOS rows in the window, see tau_pack_kernel
#define TILE_SPS_COMPACT(T) (TURB_MODEL(T) == SPHX_SPS && !((T) & SPHX_TURB_MF))
struct Gathered {
	float4 npos[TILE_HB], nvel[TILE_HB], naux[TILE_HB];
	float ntau[TILE_HB][6];   // SPS only
};

__device__ __forceinline__ const float4 &lds_row(const float4 *base, uint32_t byteOffset)
{
	return *reinterpret_cast<const float4*>(reinterpret_cast<const char*>(base) + byteOffset);
}

// stage 1 of the pair pipeline: issue the LDS reads of TILE_HB neighbours.  A tile-list entry IS the byte offset of the
// neighbour's row in the window arrays (positions in the tile's frame, see tile_shift): no decode, nothing here depends
// on a previous LDS read, so the round trips overlap with the arithmetic of the previous pairs.
template<int TURB>
__device__ __forceinline__ void gather_half(uint32_t packed, const float4 *sPos, const float4 *sVel, const float4 *sAux, float rho0, Gathered &g)
{
	static_assert(TILE_HB == 2, "a half batch is one 32-bit word of the tile list");
	constexpr uint32_t WS = TILE_WC(TURB) + 1u;
#pragma unroll
	for (int k = 0; k < TILE_HB; ++k) {
		const uint32_t L = LIST_HALF_OFFSET(packed, k);
		g.npos[k] = lds_row(sPos, L);
		if (!(TURB & SPHX_TURB_SA_DIFF)) g.nvel[k] = lds_row(sVel, L);
		if (TILE_SPS_COMPACT(TURB)) {      // two stress rows, the EOS values in the second one's spare slots (tau_pack_kernel)
			const float4 ta = lds_row(sAux, L), tb = lds_row(sAux + WS, L);
			g.ntau[k][0] = ta.x; g.ntau[k][1] = ta.y; g.ntau[k][2] = ta.z; g.ntau[k][3] = ta.w; g.ntau[k][4] = tb.x; g.ntau[k][5] = tb.y;
			// {P/rho^2, c, P, rho} as eos_kernel makes them; only one of c, P is there, the one the pair reads
			g.naux[k] = make_float4(tb.z, tb.w, tb.w, (g.nvel[k].w + 1.0f)*rho0);
			continue;
		}
		if (!(TURB & (SPHX_TURB_STRESS | SPHX_TURB_SA_DSUM))) g.naux[k] = lds_row(sAux, L);
		if (TURB_MODEL(TURB) == SPHX_SPS) {   // the SPS rows lie behind the EOS rows: sAux[WS + slot], sAux[2 WS + slot]
			const float4 ta = lds_row(sAux + WS, L), tb = lds_row(sAux + 2*WS, L);
			g.ntau[k][0] = ta.x; g.ntau[k][1] = ta.y; g.ntau[k][2] = ta.z; g.ntau[k][3] = ta.w; g.ntau[k][4] = tb.x; g.ntau[k][5] = tb.y;
		}
	}
}

// Two pairs at once on packed fp32 (v_pk_mul/add/fma_f32: two results per instruction at the issue cost of one).
// Same terms in the same order as pair_interact for each of the two pairs.  What is packed: everything computed from
// computed values (r^2, v.r, F, g.r, the viscous and diffusive coefficients).  What is not: the first consumer of every value
// read from LDS (the two rows sit in unrelated registers; pairing them up would cost the moves the packing saves),
// sqrt / rcp / min / compares / selects (no packed forms), and the accumulation into force (list order is kept).
// Instantiated for the Wendland kernel with artificial viscosity, one fluid, no or Colagrossi diffusion.
// Two things differ from pair_interact by rounding only: the positions are in the tile's frame (r_ij = x_i - x_j of two
// shifted positions instead of a shift applied to x_i alone), and the window stores m_j * fcoeff (the constant factor of F
// is folded into the mass when the window is staged), so F here is the bare (q - 2)^3.
// The momentum switch of a lane (boundary particles without force feedback accumulate no acceleration) is applied once per
// particle after the walk, not per pair.
typedef float v2f __attribute__((ext_vector_type(2)));
__device__ __forceinline__ v2f pk_fma(v2f a, v2f b, v2f c) { return __builtin_elementwise_fma(a, b, c); }
__device__ __forceinline__ v2f pk_splat(float a) { return v2f{a, a}; }

// A lane that does not take the section at all (another particle type, an idle lane) computes along and its accumulator is
// put back by the caller (walk_section_lds), so the pair has no validity flag; outside the kernel's support (q >= 2, which
// includes every pad entry: the dummy row is a thousand cells away) F = (q - 2)^3 >= 0 while it is negative inside, so the
// range test is min(m F, 0).
template<int COLAGROSSI>
__device__ __forceinline__ void pair_interact_pk(const DevParams &p, const Self &s, const float3 &q, float inv_h, const Gathered &g,
	bool rt_diffuse, float4 &force)
{
	static_assert(TILE_HB == 2, "two pairs per packed operation");
	const float4 &n0 = g.npos[0], &n1 = g.npos[1];
	const v2f rx = {q.x - n0.x, q.x - n1.x}, ry = {q.y - n0.y, q.y - n1.y}, rz = {q.z - n0.z, q.z - n1.z};
	const v2f r2 = pk_fma(rz, rz, pk_fma(ry, ry, rx*rx));
	const v2f r = {fast_sqrt(r2.x), fast_sqrt(r2.y)};
	const float4 &w0 = g.nvel[0], &w1 = g.nvel[1];
	const v2f vx = {s.vel.x - w0.x, s.vel.x - w1.x}, vy = {s.vel.y - w0.y, s.vel.y - w1.y}, vz = {s.vel.z - w0.z, s.vel.z - w1.z};
	const v2f vel_dot_pos = pk_fma(vz, rz, pk_fma(vy, ry, vx*rx));
	const v2f qm2 = pk_fma(r, pk_splat(inv_h), pk_splat(-2.0f));
	const v2f f = qm2*qm2*qm2;                       // fcoeff rides in the window's mass
	const float4 &a0 = g.naux[0], &a1 = g.naux[1];   // {P/rho^2, c, P, rho}
	const v2f mf = {fminf(n0.w*f.x, 0.0f), fminf(n1.w*f.y, 0.0f)};

	v2f dsel = {0.0f, 0.0f};
	if (COLAGROSSI == DIFF_COLAGROSSI || COLAGROSSI == DIFF_COLAGROSSI_GZ) {
		// DIFF_COLAGROSSI_GZ (chosen by the host for g_x = g_y = 0, plain_gravity_z): one packed multiply instead of a multiply
		// and two FMAs.  Same bits: the two terms left out are exact zeros, fma(g_z, r_z, +-0) rounds as g_z r_z, and where
		// r_z = 0 only the sign of a zero differs, which fabsf below takes off
		const v2f gdotr = COLAGROSSI == DIFF_COLAGROSSI_GZ ? pk_splat(p.gravity[2])*rz :
			pk_fma(pk_splat(p.gravity[2]), rz, pk_fma(pk_splat(p.gravity[1]), ry, pk_splat(p.gravity[0])*rx));
		const v2f gr = gdotr*pk_splat(s.rho);
		const bool d0 = rt_diffuse && !(fabsf(s.P - a0.z) < fabsf(gr.x)), d1 = rt_diffuse && !(fabsf(s.P - a1.z) < fabsf(gr.y));
		const v2f ratio = {fmaf(a0.w, s.inv_rho, -1.0f), fmaf(a1.w, s.inv_rho, -1.0f)};
		const v2f dterm = pk_splat(p.densityDiffCoeff*p.sscoeff[s.fl])*ratio*mf;
		dsel = v2f{d0 ? dterm.x : 0.0f, d1 ? dterm.y : 0.0f};
	}
	const v2f drdt = pk_fma(mf, vel_dot_pos, -dsel);
	force.w += drdt.x;
	force.w += drdt.y;

	// compute_pressure_contrib + artvisc, as in pair_interact
	const v2f pgrad = {s.p_precalc + a0.x, s.p_precalc + a1.x};
	v2f kk = -pgrad*mf;
	const v2f vdpn = {fminf(fminf(vel_dot_pos.x, 0.0f), fabsf(w0.w)), fminf(fminf(vel_dot_pos.y, 0.0f), fabsf(w1.w))};
	const v2f ssum = {s.sspeed + a0.y, s.sspeed + a1.y};
	const v2f rsum = {s.rho + a0.w, s.rho + a1.w};
	const v2f den = (r2 + pk_splat(p.epsartvisc))*rsum;
	const v2f iden = {fast_rcp(den.x), fast_rcp(den.y)};
	const v2f visc = vdpn*pk_splat(p.slength*p.artvisccoeff)*ssum*iden;
	kk = pk_fma(visc, mf, kk);
	force.x = fmaf(kk.x, rx.x, force.x); force.y = fmaf(kk.x, ry.x, force.y); force.z = fmaf(kk.x, rz.x, force.z);
	force.x = fmaf(kk.y, rx.y, force.x); force.y = fmaf(kk.y, ry.y, force.y); force.z = fmaf(kk.y, rz.y, force.z);
}

// the instantiations whose pair loop is pair_interact_pk: their window holds m * fcoeff
template<int KERNEL, int TURB, int COLAGROSSI, bool LJ>
struct TilePk { static constexpr bool value = KERNEL == SPHX_WENDLAND && TURB == SPHX_ARTIFICIAL && COLAGROSSI != DIFF_FERRARI && !LJ; };

// the instantiations whose list ring is hand-managed (tile_ring.h, AccRing): those that keep every value in registers.  The SPS
// ones spill (their pair holds twelve more values per neighbour) and stay on compiler-managed loads
template<int TURB>
struct TileAsmRing { static constexpr bool value = TURB_MODEL(TURB) != SPHX_SPS; };

// stage 2: the pair interactions of a gathered half, in list order; q = own position in the tile's frame
// LJ = the run uses LJ_BOUNDARY: pairs of the boundary section (ljsec, wave-uniform) and all pairs of boundary
// particles with force feedback (ljlane) are Lennard-Jones repulsions instead of SPH interactions
template<int KERNEL, int TURB, int COLAGROSSI, bool LJ>
__device__ __forceinline__ void compute_half(const DevParams &p, const Gathered &g, const Self &s, const float3 &q, float inv_h,
	bool take, bool momentum, bool diffuse, bool ljsec, bool ljlane, float4 &force, StressAcc &fx)
{
	if (TURB & SPHX_TURB_STRESS) {   // velocity-gradient sums of the SPS stress tensor: force = dv[0..3], fx = dv[4..8]
#pragma unroll
		for (int k = 0; k < TILE_HB; ++k)
			stress_interact<KERNEL>(p, s, inv_h, q.x, q.y, q.z, g.npos[k], g.nvel[k], take, force, fx);
		return;
	}
	if (TURB & SPHX_TURB_SA_DSUM) {
#pragma unroll
		for (int k = 0; k < TILE_HB; ++k)
			sa_dsum_interact(p, s, inv_h, q.x, q.y, q.z, g.npos[k], g.nvel[k], take, force);
		return;
	}
	if (TURB & SPHX_TURB_SA_DIFF) {
#pragma unroll
		for (int k = 0; k < TILE_HB; ++k)
			sa_diff_interact(p, s, inv_h, q.x, q.y, q.z, g.npos[k], g.naux[k], take, s.sa_dt2rho, force);
		return;
	}
	if (LJ && ljsec) {
#pragma unroll
		for (int k = 0; k < TILE_HB; ++k)
			lj_interact(p, q.x, q.y, q.z, g.npos[k], take, force);
		return;
	}
	if (TilePk<KERNEL, TURB, COLAGROSSI, LJ>::value) {
		pair_interact_pk<COLAGROSSI>(p, s, q, inv_h, g, diffuse, force);
		return;
	}
	const bool anyLj = LJ && wave_any(ljlane);
#pragma unroll
	for (int k = 0; k < TILE_HB; ++k) {
		uint32_t nfl = 0u;
		if (TURB & SPHX_TURB_MF) nfl = __float_as_uint(g.naux[k].y) & 3u;     // fluid number tag of the EOS row
		pair_interact<KERNEL, TURB, COLAGROSSI, true, true>(p, s, inv_h, q.x, q.y, q.z,
			g.npos[k], g.nvel[k], g.naux[k], nfl == s.fl, take && !(LJ && ljlane), g.ntau[k], force, momentum, diffuse, nfl, false);
		if (anyLj)
			lj_interact(p, q.x, q.y, q.z, g.npos[k], take && ljlane, force);
	}
}

// Walk the runs of one wave of a tile against the LDS window.
//
// The neighbour lists of a tile's home particles are dealt out to the eight waves of the workgroup BATCH BY BATCH, not
// particle by particle (tile_lists_kernel): the home particles are sorted by list length and cut into chunks of 64 (one per
// lane), the list batches of all chunks are laid end to end -- chunk after chunk, fluid section then second section, every
// section padded to the chunk's longest list -- and every wave takes an eighth of that sequence.  A RUN is the part of one
// chunk's batches that one wave walks; a wave has one to three of them per tile.  At the start of a run the lanes load their
// particle of that chunk (own row from the window), at its end they park the accumulator in LDS (sPart, one slot per run);
// when all waves are through, the finalize stage adds up the slots of each chunk in list order.  What this buys: all eight
// waves (two per SIMD: the fp32 issue rate needs both) stay busy to the end of every tile whatever its number of particles
// and however uneven their lists -- with whole chunks per wave a tile of 363 particles occupied six waves, a tile took as long
// as its longest chunk, and a wave alone on its SIMD issued at half rate.
//  * WAVE-UNIFORM control with scalar trip counts: pad entries are pairs of weight 0 (slot 0 of the window is a dummy record a
//    kilometre away), pair_interact is branch-free, a lane that does not take a section computes along and gets its
//    accumulator back at the end of the section;
//  * the wave's batches are ONE stream in memory (512 B per batch: 64 lanes x 4 window offsets), fetched TILE_AHEAD batches
//    ahead into a ring of register buffers that runs through the section and run boundaries (rotated by unrolling, not by
//    copying: a copy of an in-flight load would wait for it); its first batches are requested one tile ahead;
//  * the LDS reads of the next TILE_HB pairs are issued before the current TILE_HB pairs are computed;
//  * section, momentum and diffusion switches are run-time values so that the pair code exists once in the kernel.

// the part of a tile's run table a wave works from (all scalar)
struct WaveJob { uint32_t firstRun, nRuns, firstBatch, nBatches, laneBase, chunks; };
__device__ __forceinline__ WaveJob wave_job(uint32_t rt /* this lane's word of the run table */, uint32_t dw /* ... of the descriptor */, uint32_t wave)
{
	WaveJob j;
	const uint32_t w = (uint32_t)__builtin_amdgcn_readlane((int)rt, (int)wave);
	j.firstRun = TILE_RT_WAVE_FIRST_RUN(w); j.nRuns = TILE_RT_WAVE_RUNS(w);
	j.firstBatch = (uint32_t)__builtin_amdgcn_readlane((int)dw, TILE_D_LISTBASE) + TILE_RT_WAVE_FIRST_BATCH(w);
	j.nBatches = TILE_RT_WAVE_BATCHES(w);
	j.laneBase = (uint32_t)__builtin_amdgcn_readlane((int)dw, TILE_D_LANEBASE);
	j.chunks = TILE_RT_TILE_CHUNKS((uint32_t)__builtin_amdgcn_readlane((int)rt, TILE_RT_TILE));
	return j;
}

template<int KERNEL, int TURB, int COLAGROSSI, bool LJ, bool HIW>
__device__ __forceinline__ void walk_runs(const DevParams &p, const ForcesArgs &a, const ListStream &ls, const WaveJob &wj, uint32_t rt,
	uint32_t lane, float inv_h, const float4 *sPos, const float4 *sVel, const float4 *sAux, float4 *sPart, const uint32_t *sLaneRec,
	float *sVal, ListWindow &lw /* batches 0..TILE_AHEAD-1 of the wave's stream, already requested */)
{
	static_assert(TILE_AHEAD == 4 && TILE_NB == 2*TILE_HB, "the ring below is unrolled by hand: 4 buffers of 2 halves");
	constexpr uint32_t WC = TILE_WC(TURB), WS = WC + 1;
	constexpr bool SPSW = TURB_MODEL(TURB) == SPHX_SPS, SPSC = TILE_SPS_COMPACT(TURB), STRESS = (TURB & SPHX_TURB_STRESS) != 0;
	constexpr bool PREMUL = TilePk<KERNEL, TURB, COLAGROSSI, LJ>::value;
	constexpr bool SA = (TURB & SPHX_TURB_SA_ANY) != 0, SA_DSUM = (TURB & SPHX_TURB_SA_DSUM) != 0, SA_DIFF = (TURB & SPHX_TURB_SA_DIFF) != 0;
	constexpr bool NOAUX = STRESS || SA_DSUM || SPSC, NOVEL = SA_DIFF;
	constexpr uint32_t TAU0 = SPSC ? 0u : WS;
	constexpr bool ASMR = TileAsmRing<TURB>::value;
	const uint32_t lane8 = lane*(uint32_t)(TILE_NB*sizeof(uint16_t));
	const int last = (int)wj.nBatches - 1;
	const bool dyn = p.boundarytype == SPHX_DYN_BOUNDARY;
	int next = TILE_AHEAD;                 // next batch of the stream to fetch (scalar)
	uint32_t run = wj.firstRun;            // scalar
	const uint32_t runsEnd = wj.firstRun + wj.nRuns;

	// state of the run / section being walked
	Self s;
	float3 q = make_float3(0.0f, 0.0f, 0.0f);
	float4 force = make_float4(0.0f, 0.0f, 0.0f, 0.0f), keep = force;
	StressAcc fx = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
	bool take = false, take0 = false, take1 = false, momentum = false, ljlane = false, diffuse = true;
	int sec = 0, leftSeg = 0;
	uint32_t secondLeft = 0;               // batches of the run's second section still to come (scalar)
	uint32_t runWord = 0;                  // the run's table word (scalar)
	s.pos = make_float4(0.0f, 0.0f, 0.0f, 0.0f); s.gridPos = make_int3(0, 0, 0); s.fl = 0u;

	auto start_run = [&]() {
		const uint32_t w = (uint32_t)__builtin_amdgcn_readlane((int)rt, (int)(TILE_RT_RUN + run));
		runWord = w;
		const uint32_t nF = TILE_RT_RUN_BATCHES_F(w);
		secondLeft = TILE_RT_RUN_BATCHES_SECOND(w);
		// the lanes' particles of this run's chunk.  From LDS (staged with the window): a global load here would sit between
		// the loads of the list ring, whose in-order completion count (s_waitcnt vmcnt(N)) the compiler can then no longer tell
		const uint32_t rec = sLaneRec[TILE_RT_RUN_CHUNK(w)*64u + lane];
		const uint32_t oslot = LANE_REC_OFFSET(rec), fl = LANE_REC_FLAGS(rec);
		// own rows from the window (already in the tile's frame); idle lanes read the dummy row
		const float4 opos = lds_row(sPos, oslot), ovel = NOVEL ? make_float4(0.0f, 0.0f, 0.0f, 0.0f) : lds_row(sVel, oslot);
		q = make_float3(opos.x, opos.y, opos.z);
		s.vel = ovel;
		s.fl = (TURB & SPHX_TURB_MF) ? LANE_FLAGS_FLUID(fl) : 0u;
		if (STRESS) {
			s.rho = (ovel.w + 1.0f)*p.rho0[0];
		} else if (SPSC) {      // no EOS rows in the window: P/rho^2 and the one of {c, P} the pair reads ride in the stress rows
			const float4 tb = lds_row(sAux + TAU0 + WS, oslot);
			s.p_precalc = tb.z; s.sspeed = tb.w; s.P = tb.w; s.rho = (ovel.w + 1.0f)*p.rho0[0];
			s.inv_rho = fast_rcp(s.rho);
		} else if (!NOAUX) {
			const float4 oaux = lds_row(sAux, oslot);
			s.p_precalc = oaux.x; s.sspeed = oaux.y; s.P = oaux.z; s.rho = oaux.w;
			s.inv_rho = fast_rcp(oaux.w);
		}
		if (SA_DIFF) s.sa_dt2rho = a.saDt*2.0f*s.rho;
		if (TURB & SPHX_TURB_NEWT) init_visc(p, s);
		if (SPSW) {   // own stress tensor
			const float4 ta = lds_row(sAux + TAU0, oslot), tb = lds_row(sAux + TAU0 + WS, oslot);
			s.tau[0] = ta.x; s.tau[1] = ta.y; s.tau[2] = ta.z; s.tau[3] = ta.w; s.tau[4] = tb.x; s.tau[5] = tb.y;
		}
		const uint32_t ptype = fl & LANE_TYPE_MASK;
		const bool active = (fl & LANE_VALID) != 0u, hasCF = (fl & LANE_COMPUTE_FORCE) != 0u;
		const bool isFluid = ptype == PT_FLUID, isBound = ptype == PT_BOUNDARY, isDynBound = isBound && dyn;
		// fluid: fluid section then boundary section (DYN: SPH pairs, LJ: repulsion); DYN boundary: fluid section
		// only, with the momentum part only for bodies with force feedback (forces_kernel.def:3650-3679);
		// LJ boundary: fluid section only for bodies with force feedback, when object forces are asked for (:3620-3645)
		momentum = isFluid || hasCF;
		ljlane = LJ && isBound;
		// SA_BOUNDARY modes: fluid particles only, fluid section then vertex section (none in the diffusion)
		take0 = active && (SA ? isFluid : (STRESS || isFluid || isDynBound || (ljlane && hasCF && a.compute_object_forces)));
		take1 = active && (SA ? (isFluid && !SA_DIFF) : (STRESS || (isFluid && (dyn || LJ))));
		force = make_float4(0.0f, 0.0f, 0.0f, 0.0f); keep = force;
		fx.x = 0.0f; fx.y = 0.0f; fx.z = 0.0f; fx.w = 0.0f; fx.u = 0.0f;
		if (nF) { sec = 0; leftSeg = (int)nF; take = take0; diffuse = true; }
		else { sec = 1; leftSeg = (int)secondLeft; secondLeft = 0u; take = take1; diffuse = false; }
	};
	// end of a section: false when the wave has walked its last run
	auto end_segment = [&]() -> bool {
		// pair_interact_pk has no per-lane validity flag: a lane that does not take the section gets its accumulator back
		force.x = take ? force.x : keep.x; force.y = take ? force.y : keep.y; force.z = take ? force.z : keep.z; force.w = take ? force.w : keep.w;
		if (sec == 0 && secondLeft) {
			sec = 1; leftSeg = (int)secondLeft; secondLeft = 0u; take = take1; diffuse = false; keep = force;
			return true;
		}
		if (PREMUL && !momentum) { force.x = 0.0f; force.y = 0.0f; force.z = 0.0f; }   // ... and no momentum switch
		float4 *dst = sPart + (size_t)run*64u + lane;
		dst[0] = force;
		if (STRESS) {
			dst[TILE_RUNS_MAX*64] = make_float4(fx.x, fx.y, fx.z, fx.w);
			dst[2*TILE_RUNS_MAX*64] = make_float4(fx.u, 0.0f, 0.0f, 0.0f);
		}
		// the chunk's last run leaves what the finalize stage needs of the particle itself: its sound speed (CFL term), or in
		// stress mode its relative density
		if (runWord & TILE_RUN_LAST) sVal[TILE_RT_RUN_CHUNK(runWord)*64u + lane] = STRESS ? s.vel.w : s.sspeed;
		if (++run == runsEnd) return false;
		start_run();
		return true;
	};

	start_run();
	Gathered A, B;
	// one batch per step; the first half of the NEXT batch is gathered before the second half of this one is computed,
	// also after the last batch (a clamped, in-bounds prefetch whose rows are never computed).
	// The two waves of a SIMD (w and w + 4) take turns at being the one the issue arbiter prefers, batch by batch (priorities
	// 3,3,0,0 against 2,1,2,1): left alone the older wave always wins and the younger one is starved while both have work
	constexpr bool hiw = HIW;      // which of the two waves of its SIMD this one is: a copy of the walk per value, no branch per batch
#define SPHX_RING_PRIO(J) \
	if (hiw) { if ((J) & 1) __builtin_amdgcn_s_setprio(1); else __builtin_amdgcn_s_setprio(2); } \
	else { if ((J) < 2) __builtin_amdgcn_s_setprio(3); else __builtin_amdgcn_s_setprio(0); }
	if (ASMR) {
		// the ring lives in a0..a7 (AccRing, tile_ring.h); `cur` is the batch being walked, in ordinary registers
		acc_start_ring(lw);
		const char *ringBase = reinterpret_cast<const char*>(ls.list + ((size_t)__builtin_amdgcn_readfirstlane(wj.firstBatch) + TILE_AHEAD)*64u);
		uint2 cur = lw.q[0];
		gather_half<TURB>(cur.x, sPos, sVel, sAux, p.rho0[0], A);
#define SPHX_RING_STEP(J, JN, WAIT) \
		SPHX_RING_PRIO(J) \
		gather_half<TURB>(cur.y, sPos, sVel, sAux, p.rho0[0], B); \
		compute_half<KERNEL, TURB, COLAGROSSI, LJ>(p, A, s, q, inv_h, take, momentum, diffuse, sec == 1, ljlane, force, fx); \
		acc_load_at<2*(J), (J)*512>(ringBase, lane8);      /* buffer J is free: its batch is in `cur` */ \
		if ((J) == TILE_AHEAD - 1) ringBase += TILE_AHEAD*512; \
		/* the batch to gather next: requested a tile ahead if it is one of the first TILE_AHEAD (then fewer than TILE_AHEAD loads \
		 * are in flight and the wait is a no-op), else TILE_AHEAD - 1 loads ago */ \
		/* ... and the first TILE_AHEAD - 1 steps of a tile take buffers that acc_start_ring wrote from ordinary registers: in the \
		 * peeled first cycle they do not wait at all -- vmcnt(3) there waited for the requests made for the NEXT tile moments before     \
		 * (four list batches, two lane-index rows: all older than the ring's first load), a memory latency per tile that nothing  \
		 * needed: -0.9 % per launch at 32 M, -0.7 % at 8 M (profiles/r06_tile_chain_experiments.txt) */ \
		if (WAIT) acc_wait(); \
		cur = acc_read<2*(JN)>(); \
		gather_half<TURB>(cur.x, sPos, sVel, sAux, p.rho0[0], A); \
		compute_half<KERNEL, TURB, COLAGROSSI, LJ>(p, B, s, q, inv_h, take, momentum, diffuse, sec == 1, ljlane, force, fx); \
		if (--leftSeg == 0) { if (!end_segment()) { __builtin_amdgcn_s_setprio(0); return; } }
		// (not for the LJ_BOUNDARY instantiations: with a second copy of their pair code the compiler parks values in a0 inside the
		// walk -- scripts/check_ring_isa.py finds it --, and they are not what a step of theirs waits for)
		if (!LJ) {      // the tile's first ring cycle, peeled: nothing to wait for in its first TILE_AHEAD - 1 steps
			SPHX_RING_STEP(0, 1, false)
			SPHX_RING_STEP(1, 2, false)
			SPHX_RING_STEP(2, 3, false)
			SPHX_RING_STEP(3, 0, true)
		}
		for (;;) {
			SPHX_RING_STEP(0, 1, true)
			SPHX_RING_STEP(1, 2, true)
			SPHX_RING_STEP(2, 3, true)
			SPHX_RING_STEP(3, 0, true)
		}
#undef SPHX_RING_STEP
	} else {
		gather_half<TURB>(lw.q[0].x, sPos, sVel, sAux, p.rho0[0], A);
#define SPHX_RING_STEP(J, JN) \
		SPHX_RING_PRIO(J) \
		gather_half<TURB>(lw.q[J].y, sPos, sVel, sAux, p.rho0[0], B); \
		compute_half<KERNEL, TURB, COLAGROSSI, LJ>(p, A, s, q, inv_h, take, momentum, diffuse, sec == 1, ljlane, force, fx); \
		load_list_b(ls, wj.firstBatch, next, last, lane8, lw.q[J]); \
		pin_batch(ls, lw.q[J]); \
		++next; \
		gather_half<TURB>(lw.q[JN].x, sPos, sVel, sAux, p.rho0[0], A); \
		compute_half<KERNEL, TURB, COLAGROSSI, LJ>(p, B, s, q, inv_h, take, momentum, diffuse, sec == 1, ljlane, force, fx); \
		if (--leftSeg == 0) { if (!end_segment()) { __builtin_amdgcn_s_setprio(0); return; } }
		for (;;) {
			SPHX_RING_STEP(0, 1)
			SPHX_RING_STEP(1, 2)
			SPHX_RING_STEP(2, 3)
			SPHX_RING_STEP(3, 0)
		}
	}
#undef SPHX_RING_PRIO
#undef SPHX_RING_STEP
}

// tail of SPSstressMatrixDevice (src/cuda/visc_kernel.cu:780-811): shear rate -> nu_SPS, tau
__device__ __forceinline__ void stress_finalize(const DevParams &p, const ForcesArgs &a, uint32_t index, float rho,
	const float4 &acc, const StressAcc &acc2)
{
	float txx = acc.x, txy = acc.y + acc.w, txz = acc.z + acc2.z;
	float tyy = acc2.x, tyz = acc2.y + acc2.w, tzz = acc2.u;
	const float SijSij_bytwo = 2.0f*(txx*txx + tyy*tyy + tzz*tzz) + (txy*txy + txz*txz + tyz*tyz);
	const float S = sqrtf(SijSij_bytwo);
	const float nu_SPS = p.smagfactor*S;
	const float divu_SPS = 0.6666666666f*nu_SPS*(txx + tyy + tzz);
	const float Blinetal_SPS = p.kspsfactor*SijSij_bytwo;
	if (a.oturbvisc) a.oturbvisc[index] = nu_SPS;
	if (a.otau0) {
		txx = (nu_SPS*(txx + txx) - divu_SPS - Blinetal_SPS)/rho;
		txy *= nu_SPS/rho;
		txz *= nu_SPS/rho;
		tyy = (nu_SPS*(tyy + tyy) - divu_SPS - Blinetal_SPS)/rho;
		tyz *= nu_SPS/rho;
		tzz = (nu_SPS*(tzz + tzz) - divu_SPS - Blinetal_SPS)/rho;
		a.otau0[index] = make_float2(txx, txy);
		a.otau1[index] = make_float2(txz, tyy);
		a.otau2[index] = make_float2(tyz, tzz);
	}
}

// the two window rows a wave stages (wave w: rows w and w + 8), from tile_rows.  The table is requested one tile
// ahead and only turned into scalars (the LDS-DMA destination and the trip counts derive from them) when its tile
// starts: a readlane at request time would wait for the load there and then
// (a workgroup of TILE_WAVES waves: wave w stages the TILE_RPW rows w, w + TILE_WAVES, ...)
static_assert(TILE_WAVES*TILE_RPW == TILE_WROWS && (TILE_WAVES % 2) == 0 && TILE_ROWDESC == 32 && TILE_DESC == 16, "the window rows are dealt out evenly, two rows per table word; tables of 32 and 16 words");
static_assert((TILE_WAVES == 8 || TILE_WAVES == 4) && TILE_CHUNKS <= 2*TILE_WAVES && TILE_CHUNKS <= 15 && TILE_RUNS_MAX <= 24 && TILE_RT_RUN + TILE_RUNS_MAX <= TILE_RUNTAB && TILE_RUNTAB <= 64,
	"run table: a wave finalizes the chunks w and w + TILE_WAVES; chunk numbers are 4 bits, run numbers 5; one table word per lane");
// (every 64-lane load costs the CU's address unit the same ~16 cycles however little it fetches, and that unit is what bounds the
// staging of a tile: a table is fetched with ONE load, a word per lane, and read out with v_readlane)
struct RowJobs { uint32_t start[TILE_RPW], total[TILE_RPW], base[TILE_RPW]; bool contig[TILE_RPW]; };
__device__ __forceinline__ uint32_t request_row_jobs(const uint32_t *__restrict__ tileRows, uint32_t tile, uint32_t lane)
{
	return tileRows[(size_t)TILE_ROWDESC*tile + (lane & (uint32_t)(TILE_ROWDESC - 1))];
}
__device__ __forceinline__ void resolve_row_jobs(uint32_t rr /* this lane's word of the tile's row table */, uint32_t wave, RowJobs &j)
{
	const uint32_t sh = TILE_ROWS_SHIFT(wave);
#pragma unroll
	for (int k = 0; k < TILE_RPW; ++k) {
		const uint32_t row = wave + (uint32_t)(TILE_WAVES*k);      // same parity as the wave: TILE_WAVES is even
		j.start[k] = (uint32_t)__builtin_amdgcn_readlane((int)rr, (int)row);
		const uint32_t tb = TILE_ROWS_HALF((uint32_t)__builtin_amdgcn_readlane((int)rr, (int)(TILE_ROWS_TOTAL + TILE_ROWS_PAIR(row))), sh);
		const uint32_t bb = TILE_ROWS_HALF((uint32_t)__builtin_amdgcn_readlane((int)rr, (int)(TILE_ROWS_BASE + TILE_ROWS_PAIR(row))), sh);
		j.total[k] = tb; j.base[k] = TILE_ROWS_HALF_BASE(bb); j.contig[k] = TILE_ROWS_HALF_CONTIG(bb);
	}
}

#define TILE_HCH (TILE_RPW > 2 ? 3 : 5)   // 64-record chunks of a window row whose cell hashes are fetched along with the DMA (longer rows: later)

// does the tile hold particles of [fromParticle, toParticle)?  (multi-GPU stripes launch the kernel on a range)
__device__ __forceinline__ bool tile_in_range(uint32_t dw /* this lane's word of the descriptor */, uint32_t fromParticle, uint32_t toParticle)
{
	uint32_t firstMin = 0xFFFFFFFFu, lastMax = 0u;
#pragma unroll
	for (int r = 0; r < TILE_HROWS; ++r) {
		const uint32_t first = (uint32_t)__builtin_amdgcn_readlane((int)dw, TILE_D_FIRST + r), cnt = (uint32_t)__builtin_amdgcn_readlane((int)dw, TILE_D_COUNT + r);
		if (cnt) { firstMin = min(firstMin, first); lastMax = max(lastMax, first + cnt); }
	}
	return !(firstMin >= toParticle || lastMax <= fromParticle);
}

template<int KERNEL, int TURB, int COLAGROSSI, bool LJ>
__global__ void __launch_bounds__(TILE_THREADS, 2)
forces_tile_kernel(DevParams p, ForcesArgs a, const uint32_t *__restrict__ tiles,
	uint32_t *tileCtl /* [0]=count, [1]=overflow, [2]=finished workgroups, [4..11]=per-XCD tile tickets */,
	const uint32_t *__restrict__ cellEnd)
{
	constexpr uint32_t WC = TILE_WC(TURB);
	constexpr bool SPSW = TURB_MODEL(TURB) == SPHX_SPS;
	constexpr bool SPSC = TILE_SPS_COMPACT(TURB);      // ... whose window holds no EOS rows (one fluid)
	constexpr bool STRESS = (TURB & SPHX_TURB_STRESS) != 0;   // stress mode: no EOS rows, every active particle walks both sections
	constexpr bool PREMUL = TilePk<KERNEL, TURB, COLAGROSSI, LJ>::value;   // the window holds m * fcoeff (pair_interact_pk)
	// SA_BOUNDARY modes: sums over the fluid and vertex neighbours of the fluid particles, finished by sa_bounds.hip
	constexpr bool SA = (TURB & SPHX_TURB_SA_ANY) != 0, SA_DSUM = (TURB & SPHX_TURB_SA_DSUM) != 0, SA_DIFF = (TURB & SPHX_TURB_SA_DIFF) != 0;
	constexpr bool NOAUX = STRESS || SA_DSUM || SPSC;   // no EOS rows in the window
	constexpr bool NOVEL = SA_DIFF;             // no velocity rows
	// positions through registers on their way into the window (stage_window_row): in the plain forces pass only.  The rows held in
	// flight cost registers; every other instantiation pays for them in its pair loop.  Measured per option set with and without
	// (scripts/measure_options.sh, M updates/s): SPS at 8 M 1122 -> 1251 (forces 1.85 -> 1.61 ms, stress 1.18 -> 1.06), two fluids
	// 2268 -> 2389, laminar + Ferrari (StillWater 4 M) 2022 -> 2129, WaveTank 904 -> 972, SA walls with density summation 485 -> 508
	constexpr bool POS_REG = !SPSW && !STRESS && !SA && !(TURB & (SPHX_TURB_MF | SPHX_TURB_NEWT));
	constexpr uint32_t WS = WC + 1;   // window arrays: the dummy row the pad entries of the tile lists point to (slot 0) + WC records
	constexpr int PARTV = STRESS ? 3 : 1;      // float4 rows per lane of a run's partial sums
	__shared__ __attribute__((aligned(16))) float4 sPos[WS];
	__shared__ __attribute__((aligned(16))) float4 sVel[NOVEL ? 1 : WS];
	// SPS: EOS rows, then tau {xx,xy,xz,yy}, then {yz,zz,-,-}; with one fluid only the two stress rows (SPSC)
	__shared__ __attribute__((aligned(16))) float4 sAux[SPSC ? 2*WS : SPSW ? 3*WS : (NOAUX ? 1 : WS)];
	__shared__ __attribute__((aligned(16))) float4 sPart[PARTV*TILE_RUNS_MAX*64];   // partial sums of the tile's runs (walk_runs)
	// lane records of the tile's chunks (own window row | flags << 16): of the tile being walked and of the one being finalized
	__shared__ uint32_t sLaneRec[2][TILE_CHUNKS*64];
	__shared__ float sVal[TILE_CHUNKS*64];                         // per lane of every chunk: see walk_runs
	// the own value the finalize stage needs comes from LDS (sVal) unless the window does not hold it: SPS with one fluid keeps
	// P instead of c with Colagrossi diffusion; SA diffusion needs gamma, the other SA modes nothing
	constexpr bool VAL_LDS = !SPSC && !SA;
	constexpr uint32_t TAU0 = SPSC ? 0u : WS;     // where the stress rows start in sAux
	__shared__ uint32_t sTileQ[2];                                 // [0] first tile, [1] next tile of this workgroup

	if (tileCtl[1]) return;                 // tiling overflowed: the generic kernel handles this launch
	const uint32_t numTiles = tileCtl[0];
	const uint32_t tid = threadIdx.x;
	const uint32_t lane = tid & 63u, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
	// XCD-aware tile assignment: workgroup b runs on XCD b % 8 (MI355X_MICROARCH.md), each XCD has its own
	// 4 MB L2.  Consecutive tiles are neighbouring row bundles that share window rows, so in every round of
	// gridDim tiles XCD x takes the 32 CONSECUTIVE tiles [x*32, x*32+32) instead of every 8th one: the
	// shared rows then hit in that XCD's L2.  Rounds still interleave all XCDs, which keeps them balanced
	// (giving each XCD one contiguous eighth of the list measured 40 % slower: unequal work per eighth).
	// Placement only affects speed, never results.
	// Tiles are handed out dynamically, one ticket counter per XCD: ticket n of XCD x is tile
	// (n / perRound)*gridDim + x*perRound + n % perRound, i.e. the same placement as above, but a workgroup that
	// drew cheap tiles simply draws more (static round-robin left the slowest workgroup ~5 % behind the mean).
	// Tickets are drawn two tiles ahead by thread 0 and published through LDS, so the atomic's latency is hidden.
	const bool xcdAware = (gridDim.x & 7u) == 0u;
	const uint32_t xcd = xcdAware ? (blockIdx.x & 7u) : 0u;
	const uint32_t perRound = xcdAware ? (gridDim.x >> 3) : 1u;
	uint32_t src = xcd;   // XCD whose tickets this workgroup currently draws (thread 0 only): its own, until they run out
	auto tile_of = [&](uint32_t from, uint32_t n) -> uint32_t {
		return xcdAware ? (n / perRound)*gridDim.x + from*perRound + n % perRound : n;
	};
	const uint32_t tileEnd = numTiles;
	// a ticket past the end of `src`'s share: steal from the other XCDs' shares (synchronous atomics, but only in
	// the last few tiles of a launch); returns a tile >= tileEnd once every share is exhausted
	auto resolve = [&](uint32_t n) -> uint32_t {
		uint32_t t = tile_of(src, n);
		for (int tries = 1; t >= tileEnd && xcdAware && tries < 8; ++tries) {
			src = (src + 1u) & 7u;
			t = tile_of(src, atomicAdd(tileCtl + 4 + src, 1u));
		}
		return t;
	};
	if (tid == 0) {
		const uint32_t n0 = atomicAdd(tileCtl + 4 + src, 1u);
		sTileQ[0] = resolve(n0);
		const uint32_t n1 = atomicAdd(tileCtl + 4 + src, 1u);
		sTileQ[1] = resolve(n1);
	}
	__syncthreads();
	uint32_t tile = __builtin_amdgcn_readfirstlane(sTileQ[0]);
	if (tile >= tileEnd) {
		if (tid == 0) tile_group_done(tileCtl);
		return;
	}

	if (tid == 32) {   // the dummy row (slot 0): no mass, a kilometre away, finite everywhere -> every term of the pair is +-0
		sPos[0] = make_float4(1.0e3f, 1.0e3f, 1.0e3f, 0.0f);
		sVel[0] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
		sAux[0] = make_float4(0.0f, 1.0f, 0.0f, 1.0f);
		if (SPSW) { sAux[TAU0] = make_float4(0.0f, 0.0f, 0.0f, 0.0f); sAux[TAU0 + WS] = make_float4(0.0f, 0.0f, 0.0f, 1.0f); }
	}
	const float inv_h = fast_rcp(p.slength);
	ListStream stream; stream.list = a.tileList; stream.pin = a.pin;

	// software pipeline over tiles: descriptor, window rows, run table, the lanes' first run and their first list batches of
	// the NEXT tile are fetched while the current one computes, so a tile costs one memory round trip (the window DMA); the
	// particles of the PREVIOUS tile are finalized while that DMA is in flight
	// the tile's descriptor, row table and run table: one load each, a word per lane
	uint32_t dwc = tiles[(size_t)TILE_DESC*tile + (lane & (uint32_t)(TILE_DESC - 1))], dwn = 0u;
	uint32_t rrc = request_row_jobs(a.tileRows, tile, lane), rrn = 0u;
	uint32_t rtc = a.tileRuns[(size_t)TILE_RUNTAB*tile + min(lane, (uint32_t)(TILE_RUNTAB - 1))], rtn = 0u;
	__builtin_amdgcn_s_waitcnt(0x0F70);   // vmcnt(0): first descriptor, first run table
	const bool wholeRange = a.wholeRange != 0;

	// what a wave asks for one tile ahead, once that tile's descriptor and run table are there: the first batches of its list
	// stream and the particles it will finalize (chunks `wave` and `wave + 8`)
	struct Ahead { ListWindow lw; uint32_t idx[2]; };
	auto request_ahead = [&](uint32_t dw, uint32_t rt, Ahead &o) {
		const WaveJob j = wave_job(rt, dw, wave);
		if (j.nRuns) {
			const uint32_t lane8 = lane*(uint32_t)(TILE_NB*sizeof(uint16_t));
			if (TileAsmRing<TURB>::value) {
				acc_load<8>(stream, j.firstBatch, 0, (int)j.nBatches - 1, lane8); acc_load<10>(stream, j.firstBatch, 1, (int)j.nBatches - 1, lane8);
				acc_load<12>(stream, j.firstBatch, 2, (int)j.nBatches - 1, lane8); acc_load<14>(stream, j.firstBatch, 3, (int)j.nBatches - 1, lane8);
			} else {
#pragma unroll
				for (int k = 0; k < TILE_AHEAD; ++k) load_list_b(stream, j.firstBatch, k, (int)j.nBatches - 1, lane8, o.lw.q[k]);
			}
		}
#pragma unroll
		for (int k = 0; k < 2; ++k) {
			const uint32_t c = wave + (uint32_t)(TILE_WAVES*k);
			o.idx[k] = (c < j.chunks) ? a.tileLaneIndex[j.laneBase + c*64u + lane] : 0xFFFFFFFFu;
		}
	};
	Ahead ac, an;
	ac.idx[0] = ac.idx[1] = 0xFFFFFFFFu;
#pragma unroll
	for (int k = 0; k < TILE_AHEAD; ++k) ac.lw.q[k] = make_uint2(0u, 0u);
	an = ac;
	if (wholeRange || tile_in_range(dwc, a.fromParticle, a.toParticle)) request_ahead(dwc, rtc, ac);

	// the particles of the tile whose pair phase has just ended, waiting to be finalized: particle, where its partial sums
	// lie, and (where LDS does not have it, see VAL_LDS) one value of its own
	uint32_t fIdx[2] = {0xFFFFFFFFu, 0xFFFFFFFFu};
	float fVal[2] = {0.0f, 0.0f};
	uint32_t par = 0u;                     // scalar: which half of sLaneRec the tile being walked uses
	uint32_t fTab[2] = {0u, 0u};           // scalar: first run | runs << 8 of the chunks this wave finalizes
	bool havePrev = false;
	float cflRun = 0.0f;   // largest CFL term of this lane's particles over all tiles of the workgroup
#ifdef SPHX_TILE_DEBUG_BUILD
	// phase timers (shader cycles, per wave): 0 total, 1 top barrier, 2 descriptor + DMA issue, 3 finalize of the previous tile,
	// 4 landing of the DMA, 5 conversion, 6 window barrier, 7 requests, 8 pair phase, 9 tiles
	const bool prof = a.prof != nullptr;
	unsigned long long tBegin = prof ? __builtin_amdgcn_s_memtime() : 0ull, tp = tBegin, pacc[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
#define SPHX_PROF(K) do { if (prof) { const unsigned long long tq = __builtin_amdgcn_s_memtime(); pacc[K] += tq - tp; tp = tq; } } while (0)
#else
#define SPHX_PROF(K) do { } while (0)
#endif

	auto finalize_prev = [&]() {
#pragma unroll
		for (int k = 0; k < 2; ++k) {
			const uint32_t rf = TILE_RT_CHUNK_FIRST_RUN(fTab[k]), rn = TILE_RT_CHUNK_RUNS(fTab[k]);     // scalar
			if (k && !__builtin_amdgcn_ballot_w64(fIdx[k] != 0xFFFFFFFFu)) continue;
			// the chunk's sums: its runs in list order
			float4 force = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
			StressAcc fx = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
			for (uint32_t j = 0; j < rn; ++j) {
				const float4 *src = sPart + (size_t)(rf + j)*64u + lane;
				const float4 f0 = src[0];
				force.x += f0.x; force.y += f0.y; force.z += f0.z; force.w += f0.w;
				if (STRESS) {
					const float4 f1 = src[TILE_RUNS_MAX*64], f2 = src[2*TILE_RUNS_MAX*64];
					fx.x += f1.x; fx.y += f1.y; fx.z += f1.z; fx.w += f1.w; fx.u += f2.x;
				}
			}
			const uint32_t index = fIdx[k];
			const bool mine = index != 0xFFFFFFFFu && (wholeRange || (index >= a.fromParticle && index < a.toParticle));
			// the lane's flags: the record of the finalized tile is in the other half of sLaneRec
			const uint32_t c = wave + (uint32_t)(TILE_WAVES*k);
			const uint32_t fl = LANE_REC_FLAGS(sLaneRec[par ^ 1u][min(c, (uint32_t)(TILE_CHUNKS - 1))*64u + lane]);
			float val = fVal[k];
			if (VAL_LDS) {
				val = sVal[min(c, (uint32_t)(TILE_CHUNKS - 1))*64u + lane];
				// a chunk none of whose lists has an entry has no run to leave the value: from memory (the forces need it of fluid
				// particles only, the stress tensor of every particle)
				if (rn == 0u && __builtin_amdgcn_ballot_w64(mine && (STRESS || (fl & LANE_TYPE_MASK) == PT_FLUID)))
					val = mine ? (STRESS ? reinterpret_cast<const float*>(a.vel)[4u*(size_t)index + 3u] : reinterpret_cast<const float*>(a.aux)[4u*(size_t)index + 1u]) : 0.0f;
			}
			if (!mine) continue;
			particleinfo info;      // what the finalize stage reads of it: type, force-feedback flag, fluid (rigid-body rows: the real one)
			info.x = (unsigned short)((fl & LANE_TYPE_MASK) | ((fl & LANE_COMPUTE_FORCE) ? FG_COMPUTE_FORCE : 0u));
			info.y = (unsigned short)(LANE_FLAGS_FLUID(fl) << 12); info.z = 0; info.w = 0;
			if (STRESS) stress_finalize(p, a, index, (val + 1.0f)*p.rho0[0], force, fx);
			else if (SA) {
				if (PART_TYPE(info) == PT_FLUID) {
					if (SA_DSUM) a.forces[index].w = force.y + force.x + 0.0f;     // sumPmwNp1 + sumPmwN
					else if (SA_DIFF) a.forces[index].w = (force.w/val)/p.rho0[0];
					else {
						if (p.simflags & SPHX_ENABLE_DENSITY_SUM) force.w = 0.0f;   // no continuity equation then
						a.forces[index] = force;      // unfinished: sa_forces_kernel adds the boundary elements, divides by gamma, ...
					}
				}
			} else {
				Self s;
				s.pos = make_float4(0.0f, 0.0f, 0.0f, 0.0f); s.gridPos = make_int3(0, 0, 0);
				s.vel = make_float4(0.0f, 0.0f, 0.0f, 0.0f); s.rho = 0.0f;
				s.fl = (TURB & SPHX_TURB_MF) ? FLUID_NUM(info) : 0u;
				s.sspeed = val;
				// planes, terrain and rigid-body rows need the cell-local position, the mass, the cell (and plane friction the
				// velocity and the density): few runs, few particles
				const bool geom = (PART_TYPE(info) == PT_FLUID && (p.simflags & (SPHX_ENABLE_PLANES | SPHX_ENABLE_DEM))) ||
					(HAS_COMPUTE_FORCE(info) && a.rbforces);
				if (geom) {
					s.pos = a.pos[index]; s.gridPos = grid_pos_from_hash(p, a.hash[index] & CELLTYPE_BITMASK);
					s.vel = a.vel[index]; s.rho = a.aux[index].w;
					info = a.info[index];
				}
				cflRun = fmaxf(cflRun, finalize_particle(p, a, index, info, s, force));
			}
		}
	};

	const int gs1 = p.gs1;
	for (;;) {
		uint32_t drawn = 0;
		if (tid == 0) drawn = atomicAdd(tileCtl + 4 + src, 1u);   // the tile after next; consumed after the window barrier
		const int g2 = __builtin_amdgcn_readlane((int)dwc, TILE_D_G2), g3 = __builtin_amdgcn_readlane((int)dwc, TILE_D_G3);
		const int ca = __builtin_amdgcn_readlane((int)dwc, TILE_D_FIRSTCELL), ncells = __builtin_amdgcn_readlane((int)dwc, TILE_D_NCELLS);
		const bool inRange = wholeRange || tile_in_range(dwc, a.fromParticle, a.toParticle);   // tiles outside [fromParticle, toParticle) (multi-GPU stripes) are skipped whole
		const bool pairs = ((uint32_t)__builtin_amdgcn_readlane((int)dwc, TILE_D_FLAGS) & TILE_DF_FLUID) || STRESS;   // no fluid anywhere in the window: nothing interacts

		SPHX_PROF(8);
		lds_barrier();   // the previous tile's pair phase is over: its partial sums are complete, the window is free
		SPHX_PROF(1);
		// everything requested so far landed long ago (the requests were made before the pair phase); waiting for it HERE
		// keeps the finalize stage below from queueing behind the DMA that is issued next
		__builtin_amdgcn_s_waitcnt(0x0F70);
#pragma unroll
		for (int k = 0; k < 2; ++k) asm volatile("" : "+v"(fVal[k]), "+v"(fIdx[k]));
		// ... which includes what the previous tile's ring fetched past its end and the batches requested for this tile
		if (TileAsmRing<TURB>::value) acc_fetch_ahead(ac.lw);
		const uint32_t nextTile = __builtin_amdgcn_readfirstlane(sTileQ[1]);
		const bool haveNext = nextTile < tileEnd;
		if (haveNext) dwn = tiles[(size_t)TILE_DESC*nextTile + (lane & (uint32_t)(TILE_DESC - 1))];
		RowJobs rjc;
		resolve_row_jobs(rrc, wave, rjc);

		// 1. the window: wave w stages rows w and w + 8 (a row is ~3 chunks of 64 records per array) by LDS DMA and fetches
		//    the cell hash of every record along with it; when both have landed it moves ITS rows into the tile's frame
		//    (tile_shift of the record's cell: row from the row number, column from the hash) -- no other wave has to wait for
		//    that, the one barrier below publishes the finished window
		uint32_t hsh[TILE_RPW][TILE_HCH];
		float4 posr[TILE_RPW][TILE_HCH];
		auto stage_window_row = [&](int k) {
			const uint32_t total = rjc.total[k], base = rjc.base[k], rs = rjc.start[k];
#pragma unroll
			for (int c = 0; c < TILE_HCH; ++c) hsh[k][c] = 0u;
			if (!(inRange && pairs) || !total || base + total > WC || !rjc.contig[k]) return;
			// positions go through registers: they are moved into the tile's frame on their way into the window (a DMA'd row had to
			// be read back from LDS for that); everything else by DMA.  Rows longer than TILE_HCH chunks: the rest by DMA + a pass
			if (POS_REG) {
#pragma unroll
				for (int c = 0; c < TILE_HCH; ++c)
					if ((uint32_t)c*64u + lane < total) posr[k][c] = a.pos[rs + (uint32_t)c*64u + lane];
				if (total > (uint32_t)TILE_HCH*64u)
					stage_row_wave(a.pos + rs + TILE_HCH*64, sPos + 1 + base + TILE_HCH*64, total - (uint32_t)TILE_HCH*64u, lane);
			} else
				stage_row_wave(a.pos + rs, sPos + 1 + base, total, lane);
			if (!NOVEL) stage_row_wave(a.vel + rs, sVel + 1 + base, total, lane);
			if (!NOAUX) stage_row_wave(a.aux + rs, sAux + 1 + base, total, lane);
			if (SPSW) {
				stage_row_wave(a.tauPack + rs, sAux + TAU0 + 1 + base, total, lane);
				stage_row_wave(a.tauPack + a.tauPackN + rs, sAux + TAU0 + WS + 1 + base, total, lane);
			}
#pragma unroll
			for (int c = 0; c < TILE_HCH; ++c)
				if ((uint32_t)c*64u + lane < total) hsh[k][c] = a.hash[rs + (uint32_t)c*64u + lane];
		};
#pragma unroll
		for (int k = 0; k < TILE_RPW; ++k) stage_window_row(k);
		const WaveJob wj = wave_job(rtc, dwc, wave);
		if (inRange) {      // ... and the lane records of the chunks (wave w: chunks w and w + 8), 4 bytes per lane
#pragma unroll
			for (int k = 0; k < 2; ++k) {
				const uint32_t c = wave + (uint32_t)(TILE_WAVES*k);
				if (c < wj.chunks)
					__builtin_amdgcn_global_load_lds((gptr_t)(a.tileLaneRec + wj.laneBase + c*64u + lane), (lptr_t)(sLaneRec[par] + c*64u), 4, 0, 0);
			}
		}
		if (haveNext) {   // behind the DMA in the memory pipeline, consumed when the next tile starts
			rrn = request_row_jobs(a.tileRows, nextTile, lane);
			rtn = a.tileRuns[(size_t)TILE_RUNTAB*nextTile + min(lane, (uint32_t)(TILE_RUNTAB - 1))];
		}
		SPHX_PROF(2);
		// 2. finalize the previous tile while the DMA drains: partial sums from LDS, the particle's own data from LDS and
		//    registers, results to memory.  (What bounds the staging is the rate at which the CU's address unit takes the DMA
		//    instructions, ~16 cycles each; they are all queued first.  Measured: with the finalize stage between the two rows
		//    of a wave the unit runs dry while all eight waves compute, 3.90 -> 4.02 ms per launch)
		if (havePrev) finalize_prev();
		SPHX_PROF(3);
		__builtin_amdgcn_s_waitcnt(0x0F70);   // vmcnt(0): this wave's LDS-DMA and hashes have landed
		SPHX_PROF(4);
		if (inRange && pairs) {
#pragma unroll
			for (int k = 0; k < TILE_RPW; ++k) {
				const uint32_t total = rjc.total[k], base = rjc.base[k], rs = rjc.start[k];
				const int r = (int)wave + TILE_WAVES*k;
				if (!total || base + total > WC) continue;     // cannot overflow for tiles of build_tiles_kernel
				if (rjc.contig[k]) {
					const int h0 = window_row_hash0(p, g2, g3, r) + ca - 1;      // cell hash of window column 0 of this row
					// shift of a record of window cell (r, col): the row's part is wave-uniform, the column's part is col * cell size
					// along COORD1 (home particles read their own row from the window, so nothing else has to reproduce this sum)
					const float3 sh0 = tile_shift(p, ncells, r, 0);
					const float stx = (p.c1 == 0) ? p.csc1 : 0.0f, sty = (p.c1 == 1) ? p.csc1 : 0.0f, stz = (p.c1 == 2) ? p.csc1 : 0.0f;
					const bool wrap1 = (p.periodic & (1u << p.c1)) != 0u;
					auto shifted = [&](float4 P, uint32_t h) {
						int col = (int)(h & CELLTYPE_BITMASK) - h0;
						if (wrap1) {      // the window wraps around a periodic COORD1
							if (col > ncells + 1) col -= gs1;
							if (col < 0) col += gs1;
						}
						const float fc = (float)col;
						P.x += fmaf(fc, stx, sh0.x); P.y += fmaf(fc, sty, sh0.y); P.z += fmaf(fc, stz, sh0.z);
						if (PREMUL) P.w *= p.fcoeff;
						return P;
					};
#pragma unroll
					for (int c = 0; c < TILE_HCH; ++c)
						if ((uint32_t)c*64u + lane < total) {
							const uint32_t w = 1u + base + (uint32_t)c*64u + lane;
							sPos[w] = shifted(POS_REG ? posr[k][c] : sPos[w], hsh[k][c]);
						}
					for (uint32_t q = (uint32_t)TILE_HCH*64u + lane; q < total; q += 64u) sPos[1u + base + q] = shifted(sPos[1u + base + q], a.hash[rs + q]);
				} else {   // a row that is not one range in memory (cell-type segments of a device map not split on COORD3,
					       // a periodic row lying wholly inside the window): cell by cell, in window order
					uint32_t off = 0;
					for (int col = 0; col < ncells + 2; ++col) {
						const uint32_t h = window_cell_hash(p, g2, g3, ca, ncells, r, col);
						if (h == 0xFFFFFFFFu) continue;
						const uint32_t st = a.cellStart[h];
						if (st == CELL_EMPTY) continue;
						const uint32_t cnt = cellEnd[h] - st, cb = 1u + base + off;
						const float3 sh0 = tile_shift(p, ncells, r, 0);
						const float fc = (float)col;
						const float3 sh = make_float3(fmaf(fc, (p.c1 == 0) ? p.csc1 : 0.0f, sh0.x), fmaf(fc, (p.c1 == 1) ? p.csc1 : 0.0f, sh0.y),
							fmaf(fc, (p.c1 == 2) ? p.csc1 : 0.0f, sh0.z));
						for (uint32_t q = lane; q < cnt; q += 64u) {
							float4 P = a.pos[st + q];
							P.x += sh.x; P.y += sh.y; P.z += sh.z;
							if (PREMUL) P.w *= p.fcoeff;
							sPos[cb + q] = P;
							if (!NOVEL) sVel[cb + q] = a.vel[st + q];
							if (!NOAUX) sAux[cb + q] = a.aux[st + q];
							if (SPSW) { sAux[TAU0 + cb + q] = a.tauPack[st + q]; sAux[TAU0 + WS + cb + q] = a.tauPack[a.tauPackN + st + q]; }
						}
						off += cnt;
					}
				}
			}
		}
		SPHX_PROF(5);
		__syncthreads();                      // everybody's rows are in place and converted; the previous tile's sums are consumed
		SPHX_PROF(6);
		if (tid == 0) sTileQ[1] = resolve(drawn);   // read after the first barrier of the next iteration
		// 3. requests: the next tile's first batches and lanes; the own data of THIS tile's particles for its finalize stage
		const bool nextInRange = haveNext && (wholeRange || tile_in_range(dwn, a.fromParticle, a.toParticle));
		if (nextInRange) request_ahead(dwn, rtn, an);
#pragma unroll
		for (int k = 0; k < 2; ++k) {
			const uint32_t c = wave + (uint32_t)(TILE_WAVES*k);
			fIdx[k] = inRange ? ac.idx[k] : 0xFFFFFFFFu;
			// a tile whose window was not staged (no fluid in reach) has only wall particles at home: no runs were walked
			fTab[k] = (inRange && pairs && c < wj.chunks) ? (uint32_t)__builtin_amdgcn_readlane((int)rtc, (int)(TILE_RT_CHUNK + c)) : 0u;
			if (!VAL_LDS && SA_DIFF && (k == 0 || __builtin_amdgcn_ballot_w64(fIdx[k] != 0xFFFFFFFFu))) {
				const uint32_t li = (fIdx[k] != 0xFFFFFFFFu) ? fIdx[k] : 0u;
				fVal[k] = reinterpret_cast<const float*>(a.saGam)[4u*(size_t)li + 3u];
			}
			if (!VAL_LDS && SPSC && (k == 0 || __builtin_amdgcn_ballot_w64(fIdx[k] != 0xFFFFFFFFu))) {
				const uint32_t li = (fIdx[k] != 0xFFFFFFFFu) ? fIdx[k] : 0u;
				fVal[k] = reinterpret_cast<const float*>(a.aux)[4u*(size_t)li + 1u];
			}
		}

		SPHX_PROF(7);
		// 4. the pair phase: this wave's share of the tile's list batches
		if (inRange && pairs && wj.nRuns) {
			if ((TILE_WAVES > 4) ? (__builtin_amdgcn_readfirstlane(threadIdx.x >> 8) != 0) : (((blockIdx.x/256u) & 1u) != 0u))
				walk_runs<KERNEL, TURB, COLAGROSSI, LJ, true>(p, a, stream, wj, rtc, lane, inv_h, sPos, sVel, sAux, sPart, sLaneRec[par], sVal, ac.lw);
			else
				walk_runs<KERNEL, TURB, COLAGROSSI, LJ, false>(p, a, stream, wj, rtc, lane, inv_h, sPos, sVel, sAux, sPart, sLaneRec[par], sVal, ac.lw);
		}
		havePrev = inRange;
#ifdef SPHX_TILE_DEBUG_BUILD
		if (prof) pacc[9] += 1;
#endif
		if (!haveNext) break;
		tile = nextTile;
		dwc = dwn; rrc = rrn; rtc = rtn;
		ac = an;
		par ^= 1u;
	}
	lds_barrier();
	__builtin_amdgcn_s_waitcnt(0x0F70);
	par ^= 1u;      // finalize_prev reads the other half
	if (havePrev) finalize_prev();
	// CFL: the array is only ever max-reduced (fmaxDevice / dtreduce), so the maxima need not sit in the reference's
	// one-entry-per-128-particles places: every wave maxes its running value into one entry of the caller's range, once per
	// launch.  Non-negative floats order like their bit patterns; the caller zeroed CFL.
	if (!STRESS && !SA && a.cfl) {
#pragma unroll
		for (int dd = 32; dd > 0; dd >>= 1)
			cflRun = fmaxf(cflRun, __shfl_down(cflRun, dd));
		if (lane == 0 && a.numBlocks)
			atomicMax(reinterpret_cast<unsigned int*>(a.cfl + a.cflOffset + (blockIdx.x*(TILE_THREADS/64) + wave) % a.numBlocks), __float_as_uint(cflRun));
	}
	if (tid == 0) tile_group_done(tileCtl);
#ifdef SPHX_TILE_DEBUG_BUILD
	if (prof && lane == 0) {
		unsigned long long *o = a.prof + 10*((size_t)blockIdx.x*(TILE_THREADS/64) + wave);
		pacc[0] = __builtin_amdgcn_s_memtime() - tBegin;
#pragma unroll
		for (int k = 0; k < 10; ++k) o[k] = pacc[k];
	}
#endif
#undef SPHX_PROF
}

#endif
