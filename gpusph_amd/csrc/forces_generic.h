// forces_generic.h -- the kernels that walk the reference-format neighbour list of every particle: the forces pass and the SPS
// stress tensor.  They serve what the tiled kernel (forces_tile.h) does not, and stand by for it when a tiling overflowed.
#ifndef SPHX_FORCES_GENERIC_H
#define SPHX_FORCES_GENERIC_H

#include "forces_pair.h"

// ==========================================================================================
// Generic path: neighbour rows gathered through L2.  Used for multi-fluid and SPS runs, for
// neighbour lists not built by this context, and whenever the tiling below overflowed.
// ==========================================================================================
#define NB 4   // neighbours resolved per batch: list entries, cell bases and particle rows of a
               // batch are fetched with independent loads in flight (3 dependent round trips per NB
               // neighbours instead of per neighbour); the next batch's list entries are prefetched

// walk one typed section of the neighbour list (neiblist_iterator_simple,
// src/cuda/neibs_iteration.cuh:165-205; getNeibIndex src/cuda/cellgrid.cuh:200-228)
// LJW: the section is a Lennard-Jones repulsion walk (positions only): a template flag, so that the pair loop holds one
// interaction body
template<int KERNEL, int TURB, int COLAGROSSI, bool MULTIFLUID, int NPTYPE, bool MOMENTUM, bool DIFFUSE, bool LJW = false>
__device__ __forceinline__ void walk_section(const DevParams &p, const ForcesArgs &a, uint32_t index,
	const Self &s, float inv_h, float4 &force)
{
	int slot = (NPTYPE == PT_FLUID) ? 0 : (int)p.neibboundpos;
	uint32_t nd[NB], ndn[NB];
	load_list_batch<NPTYPE, NB>(p, a.neibsList, index, slot, nd);

	int cell = 0;
	uint32_t cell_base = 0;
	bool done = false;

	while (!done) {
		slot = (NPTYPE == PT_FLUID) ? slot + NB : slot - NB;
		load_list_batch<NPTYPE, NB>(p, a.neibsList, index, slot, ndn);

		// stage 1: decode entries, fetch the base index of every cell that changes in this batch
		bool valid[NB], enc[NB];
		int c[NB];
		uint32_t cb[NB];
		bool alive = true;
#pragma unroll
		for (int k = 0; k < NB; ++k) {
			const uint32_t d = nd[k];
			alive = alive && (d != NEIBS_END);
			valid[k] = alive;
			enc[k] = alive && (d >= CELLNUM_ENCODED);
			c[k] = enc[k] ? (int)(d >> CELLNUM_SHIFT) - 1 : (k ? c[k > 0 ? k - 1 : 0] : cell);
			cb[k] = 0;
			if (enc[k]) {
				const int cz = c[k]/9, cy = (c[k] - cz*9)/3, cx = c[k] - cz*9 - cy*3;
				cb[k] = a.cellStart[grid_hash_periodic(p, s.gridPos.x + cx - 1, s.gridPos.y + cy - 1, s.gridPos.z + cz - 1)];
			}
		}
		done = !alive;
#pragma unroll
		for (int k = 0; k < NB; ++k)
			if (!enc[k]) cb[k] = k ? cb[k > 0 ? k - 1 : 0] : cell_base;
		cell = c[NB - 1];
		cell_base = cb[NB - 1];

		// stage 2: gather the neighbour rows of the whole batch
		float4 npos[NB], nvel[NB], naux[NB];
		bool same[NB];
		uint32_t nfl[NB];
		float ntau[NB][6];
#pragma unroll
		for (int k = 0; k < NB; ++k) {
			const uint32_t j = valid[k] ? cb[k] + (nd[k] & NEIBINDEX_MASK) : index;
			npos[k] = a.pos[j];
			nvel[k] = a.vel[j];
			naux[k] = a.aux[j];
			same[k] = true; nfl[k] = 0u;
			if (MULTIFLUID) { nfl[k] = FLUID_NUM(a.info[j]); same[k] = nfl[k] == s.fl; }
			if (TURB_MODEL(TURB) == SPHX_SPS && MOMENTUM) {
				const float2 t0 = a.tau0[j], t1 = a.tau1[j], t2 = a.tau2[j];
				ntau[k][0] = t0.x; ntau[k][1] = t0.y; ntau[k][2] = t1.x; ntau[k][3] = t1.y; ntau[k][4] = t2.x; ntau[k][5] = t2.y;
			}
		}

		// stage 3: pair interactions, in list order
#pragma unroll
		for (int k = 0; k < NB; ++k) {
			const int cz = c[k]/9, cy = (c[k] - cz*9)/3, cx = c[k] - cz*9 - cy*3;
			const float pcx = fmaf(-(float)(cx - 1), p.cs[0], s.pos.x);
			const float pcy = fmaf(-(float)(cy - 1), p.cs[1], s.pos.y);
			const float pcz = fmaf(-(float)(cz - 1), p.cs[2], s.pos.z);
			if (LJW)
				lj_interact(p, pcx, pcy, pcz, npos[k], valid[k], force);
			else
				pair_interact<KERNEL, TURB, COLAGROSSI, MOMENTUM, DIFFUSE>(p, s, inv_h, pcx, pcy, pcz,
					npos[k], nvel[k], naux[k], same[k], valid[k], ntau[k], force, true, true, nfl[k], true);
		}
#pragma unroll
		for (int k = 0; k < NB; ++k) nd[k] = ndn[k];
	}
}

template<int KERNEL, int TURB, int COLAGROSSI, bool MULTIFLUID>
__global__ void __launch_bounds__(SPHX_BLOCK_FORCES)
forces_kernel(DevParams p, ForcesArgs a, const uint32_t *__restrict__ runIfNonZero)
{
	// when the tiled kernel handles this launch the generic one is skipped on the device side
	if (runIfNonZero && *runIfNonZero == 0) return;
	// block-stride loop: as the stand-by of the tiled kernel this one is launched with a small grid (a quarter
	// of a million workgroups that return at once cost 50 us), and still covers every block if it has to run
	for (uint32_t blk = blockIdx.x; blk < a.numBlocks; blk += gridDim.x) {
	const uint32_t index = blk*SPHX_BLOCK_FORCES + threadIdx.x + a.fromParticle;
	float cfl_term = 0.0f;

	do {
		if (index >= a.toParticle) break;
		const particleinfo info = a.info[index];
		const uint32_t ptype = PART_TYPE(info);
		const float4 pos = a.pos[index];
		if (!is_active_w(pos.w)) break;

		Self s;
		load_self<TURB>(p, a, index, info, pos, MULTIFLUID, s);
		const float inv_h = fast_rcp(p.slength);
		const bool dyn = p.boundarytype == SPHX_DYN_BOUNDARY, lj = p.boundarytype == SPHX_LJ_BOUNDARY;

		// the caller clobbers FORCES to 0 before basicstep (src/GPUWorker.cc:1949): the accumulator
		// starts from that value without re-reading it
		float4 force = make_float4(0.0f, 0.0f, 0.0f, 0.0f);

		if (ptype == PT_FLUID) {
			// fluid <- fluid : compute_all_pp_interaction (forces_kernel.def:3565-3610)
			walk_section<KERNEL, TURB, COLAGROSSI, MULTIFLUID, PT_FLUID, true, true>(p, a, index, s, inv_h, force);
			// fluid <- boundary : same interaction for DYN_BOUNDARY (forces_kernel.def:3717-3726),
			// no density diffusion from boundary neighbours (:1596-1606)
			// ... Lennard-Jones repulsion for LJ_BOUNDARY (:3688-3705)
			if (dyn)
				walk_section<KERNEL, TURB, COLAGROSSI, MULTIFLUID, PT_BOUNDARY, true, false>(p, a, index, s, inv_h, force);
			else if (lj)
				walk_section<KERNEL, TURB, COLAGROSSI, MULTIFLUID, PT_BOUNDARY, true, false, true>(p, a, index, s, inv_h, force);
		} else if (ptype == PT_BOUNDARY && lj) {
			// boundary <- fluid with LJ_BOUNDARY (:3620-3645): only particles of bodies with force feedback, and only
			// when the caller asked for object forces (run_forces launches this pass only then, src/cuda/forces.cu:775-782)
			if (HAS_COMPUTE_FORCE(info) && a.compute_object_forces)
				walk_section<KERNEL, TURB, COLAGROSSI, MULTIFLUID, PT_FLUID, true, false, true>(p, a, index, s, inv_h, force);
		} else if (ptype == PT_BOUNDARY && dyn) {
			// boundary <- fluid (forces_kernel.def:3650-3679): DYN always evolves density; momentum
			// only for particles of bodies with force feedback
			if (HAS_COMPUTE_FORCE(info))
				walk_section<KERNEL, TURB, COLAGROSSI, MULTIFLUID, PT_FLUID, true, true>(p, a, index, s, inv_h, force);
			else
				walk_section<KERNEL, TURB, COLAGROSSI, MULTIFLUID, PT_FLUID, false, true>(p, a, index, s, inv_h, force);
		}
		cfl_term = finalize_particle(p, a, index, info, s, force);
	} while (0);

	// maxBlockReduce (src/cuda/device_core.cu:40-59) as wave shuffles + one LDS word per wave
	if (a.cfl) {
		__shared__ float wave_max[SPHX_BLOCK_FORCES/64];
#pragma unroll
		for (int d = 32; d > 0; d >>= 1)
			cfl_term = fmaxf(cfl_term, __shfl_down(cfl_term, d));
		if ((threadIdx.x & 63u) == 0) wave_max[threadIdx.x >> 6] = cfl_term;
		__syncthreads();
		if (threadIdx.x == 0) {
			float m = wave_max[0];
			for (int w = 1; w < SPHX_BLOCK_FORCES/64; ++w) m = fmaxf(m, wave_max[w]);
			a.cfl[a.cflOffset + blk] = m;
		}
		__syncthreads();   // wave_max is reused by the next block of this workgroup
	}
	}
}

// ------------------------------------------------------------------------------------------
// SPS stress tensor: SPSstressMatrixDevice (src/cuda/visc_kernel.cu:759-811), shearRate :307-367
// ------------------------------------------------------------------------------------------
// one typed section of the list, NB entries per batch like walk_section: the list entries of the next batch, the cell bases
// and the neighbour rows of a batch are independent loads in flight together (the one-neighbour-at-a-time version spent
// 8.6 ms per call at 8 M particles on dependent L2 round trips); branch-free, rejected pairs get weight 0
template<int KERNEL, int NPTYPE, bool MULTIFLUID>
__device__ __forceinline__ void sps_section(const DevParams &p, const SpsArgs &a, uint32_t index,
	const float4 &pos, const float4 &vel, const int3 &gridPos, float inv_h, float dv[9])
{
	int slot = (NPTYPE == PT_FLUID) ? 0 : (int)p.neibboundpos;
	uint32_t nd[NB], ndn[NB];
	load_list_batch<NPTYPE, NB>(p, a.neibsList, index, slot, nd);
	int cell = 0;
	uint32_t cell_base = 0;
	bool done = false;
	while (!done) {
		slot = (NPTYPE == PT_FLUID) ? slot + NB : slot - NB;
		load_list_batch<NPTYPE, NB>(p, a.neibsList, index, slot, ndn);
		bool valid[NB], enc[NB];
		int c[NB];
		uint32_t cb[NB];
		bool alive = true;
#pragma unroll
		for (int k = 0; k < NB; ++k) {
			const uint32_t d = nd[k];
			alive = alive && (d != NEIBS_END);
			valid[k] = alive;
			enc[k] = alive && (d >= CELLNUM_ENCODED);
			c[k] = enc[k] ? (int)(d >> CELLNUM_SHIFT) - 1 : (k ? c[k > 0 ? k - 1 : 0] : cell);
			cb[k] = 0;
			if (enc[k]) {
				const int cz = c[k]/9, cy = (c[k] - cz*9)/3, cx = c[k] - cz*9 - cy*3;
				cb[k] = a.cellStart[grid_hash_periodic(p, gridPos.x + cx - 1, gridPos.y + cy - 1, gridPos.z + cz - 1)];
			}
		}
		done = !alive;
#pragma unroll
		for (int k = 0; k < NB; ++k)
			if (!enc[k]) cb[k] = k ? cb[k > 0 ? k - 1 : 0] : cell_base;
		cell = c[NB - 1];
		cell_base = cb[NB - 1];
		float4 npos[NB], nvel[NB];
		uint32_t nfl[NB];
#pragma unroll
		for (int k = 0; k < NB; ++k) {
			const uint32_t j = valid[k] ? cb[k] + (nd[k] & NEIBINDEX_MASK) : index;
			npos[k] = a.pos[j];
			nvel[k] = a.vel[j];
			nfl[k] = 0u;
			if (MULTIFLUID) nfl[k] = FLUID_NUM(a.info[j]);
		}
#pragma unroll
		for (int k = 0; k < NB; ++k) {
			const int cz = c[k]/9, cy = (c[k] - cz*9)/3, cx = c[k] - cz*9 - cy*3;
			const float rx = fmaf(-(float)(cx - 1), p.cs[0], pos.x) - npos[k].x;
			const float ry = fmaf(-(float)(cy - 1), p.cs[1], pos.y) - npos[k].y;
			const float rz = fmaf(-(float)(cz - 1), p.cs[2], pos.z) - npos[k].z;
			const float r = fast_sqrt(fmaf(rz, rz, fmaf(ry, ry, rx*rx)));
			const bool on = valid[k] && is_active_w(npos[k].w) && r < p.influenceradius;
			const float n_rho = (nvel[k].w + 1.0f)*p.rho0[nfl[k]];
			const float wgt = kernel_F<KERNEL>(p, r, inv_h)*npos[k].w*fast_rcp(n_rho);
			const float weight = on ? wgt : 0.0f;
			const float mx = rx*weight, my = ry*weight, mz = rz*weight;
			const float vx = vel.x - nvel[k].x, vy = vel.y - nvel[k].y, vz = vel.z - nvel[k].z;
			dv[0] -= vx*mx; dv[1] -= vx*my; dv[2] -= vx*mz;
			dv[3] -= vy*mx; dv[4] -= vy*my; dv[5] -= vy*mz;
			dv[6] -= vz*mx; dv[7] -= vz*my; dv[8] -= vz*mz;
		}
#pragma unroll
		for (int k = 0; k < NB; ++k) nd[k] = ndn[k];
	}
}

template<int KERNEL, bool MULTIFLUID>
__global__ void __launch_bounds__(128)
sps_kernel(DevParams p, SpsArgs a, const uint32_t *runIfNonZero)
{
	if (runIfNonZero && !*runIfNonZero) return;   // the tiled stress pass covered this launch
	// block-stride loop: as the stand-by of the tiled pass this kernel is launched with a capped grid (see forces_kernel)
	for (uint32_t blk = blockIdx.x; blk*128u < a.numParticles; blk += gridDim.x) {
	const uint32_t index = blk*128 + threadIdx.x;
	if (index >= a.numParticles) continue;
	const float4 pos = a.pos[index];
	if (!is_active_w(pos.w)) continue;
	const float4 vel = a.vel[index];
	const particleinfo info = a.info[index];
	const int3 gridPos = grid_pos_from_hash(p, a.hash[index] & CELLTYPE_BITMASK);
	const float inv_h = fast_rcp(p.slength);
	float dv[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
	sps_section<KERNEL, PT_FLUID, MULTIFLUID>(p, a, index, pos, vel, gridPos, inv_h, dv);
	sps_section<KERNEL, PT_BOUNDARY, MULTIFLUID>(p, a, index, pos, vel, gridPos, inv_h, dv);

	float txx = dv[0], txy = dv[1] + dv[3], txz = dv[2] + dv[6];
	float tyy = dv[4], tyz = dv[5] + dv[7], tzz = dv[8];
	const float SijSij_bytwo = 2.0f*(txx*txx + tyy*tyy + tzz*tzz) + (txy*txy + txz*txz + tyz*tyz);
	const float S = sqrtf(SijSij_bytwo);
	const float nu_SPS = p.smagfactor*S;
	const float divu_SPS = 0.6666666666f*nu_SPS*(txx + tyy + tzz);
	const float Blinetal_SPS = p.kspsfactor*SijSij_bytwo;
	if (a.turbvisc) a.turbvisc[index] = nu_SPS;
	if (a.tau0) {
		const float rho = (vel.w + 1.0f)*p.rho0[FLUID_NUM(info)];
		txx = (nu_SPS*(txx + txx) - divu_SPS - Blinetal_SPS)/rho;
		txy *= nu_SPS/rho;
		txz *= nu_SPS/rho;
		tyy = (nu_SPS*(tyy + tyy) - divu_SPS - Blinetal_SPS)/rho;
		tyz *= nu_SPS/rho;
		tzz = (nu_SPS*(tzz + tzz) - divu_SPS - Blinetal_SPS)/rho;
		a.tau0[index] = make_float2(txx, txy);
		a.tau1[index] = make_float2(txz, tyy);
		a.tau2[index] = make_float2(tyz, tzz);
	}
	}
}

#endif
