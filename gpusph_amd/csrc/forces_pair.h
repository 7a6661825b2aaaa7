// forces_pair.h -- the pair physics of the forces engine: what one particle takes from one neighbour, and what is done to its
// sums afterwards.  Shared by the list-walking kernels (forces_generic.h) and the tiled kernel (forces_tile.h).
//
// Numerics: accumulation order per particle is the reference's (list order, fluid section then
// boundary section), so results differ from oracle/sph_oracle.c only through the fast
// transcendental path (v_log_f32/v_exp_f32 for the Tait EOS instead of powf, v_rcp_f32,
// v_sqrt_f32), the same class of deviation the reference's own __powf has.
#ifndef SPHX_FORCES_PAIR_H
#define SPHX_FORCES_PAIR_H

#include "forces_args.h"

__device__ __forceinline__ float fast_rcp(float x) { return __builtin_amdgcn_rcpf(x); }
__device__ __forceinline__ float fast_sqrt(float x) { return __builtin_amdgcn_sqrtf(x); }
__device__ __forceinline__ float fast_exp2(float x) { return __builtin_amdgcn_exp2f(x); }

// F<kerneltype>(r, h): src/cuda/sph_core.cu:146-191
template<int KERNEL>
__device__ __forceinline__ float kernel_F(const DevParams &p, float r, float inv_h)
{
	if (KERNEL == SPHX_WENDLAND) {
		const float qm2 = fmaf(r, inv_h, -2.0f);
		return qm2*qm2*qm2*p.fcoeff;
	} else if (KERNEL == SPHX_CUBICSPLINE) {
		const float R = r*inv_h;
		const float val = (R < 1.0f) ? (-4.0f + 3.0f*R)*inv_h : -(-2.0f + R)*(-2.0f + R)*fast_rcp(r);
		return val*p.fcoeff;
	} else if (KERNEL == SPHX_QUADRATIC) {
		const float R = r*inv_h;
		return (-2.0f + R)*fast_rcp(r)*p.fcoeff;
	} else {
		const float R = r*inv_h;
		return -fast_exp2(-R*R*1.44269504088896340736f)*p.fcoeff;
	}
}

struct Self {
	float4 pos, vel;
	int3 gridPos;
	float p_precalc, sspeed, P, rho, inv_rho;
	uint32_t fl;
	float tau[6];
	// NEWTONIAN rheology: own viscosity terms and the averaging selectors, per lane (see laminar_factor)
	float visc_c, visc_mu, visc_kin, visc_onemk, visc_wA, visc_wH, visc_wG;
	uint32_t visc_constmask, visc_ownmask;
	uint32_t f2mask;   // all ones for SPH_F2 (generic kernel only), per lane like the viscosity selectors
	float sa_dt2rho;   // SA density diffusion mode of the tiled kernel: dt * 2 * rho_i
};

// select chain on the (at most four) kernel-argument values instead of a lane-indexed load from the argument block
__device__ __forceinline__ float visc_of(const DevParams &p, uint32_t fl)
{
	const float lo = (fl & 1u) ? p.visccoeff[1] : p.visccoeff[0], hi = (fl & 1u) ? p.visccoeff[3] : p.visccoeff[2];
	return (fl & 2u) ? hi : lo;
}

// visc_avg (src/cuda/visc_avg.cu:40-190) without the neighbour mass: the per-pair factor of the laminar Morris term,
// nu-or-mu averaged over the pair / densities.  Every flavour of the reference is one instance of
//   mu_i = c_i rho_i^k , mu_j = c'_j rho_j^k  (k = 1 kinematic, 0 dynamic; c'_j = c_i when the viscosity is declared
//   constant, the neighbour's fluid coefficient otherwise),
//   arithmetic (mu_i + mu_j)/(rho_i rho_j), harmonic 4 mu_i mu_j/((mu_i + mu_j) rho_i rho_j), geometric 2 sqrt(mu_i mu_j)/(rho_i rho_j)
// (the constant-viscosity shortcuts of visc_avg.cu are these with c'_j = c_i, up to rounding).  It is evaluated
// branch-free with per-lane selector values prepared once per particle (init_visc) instead of wave-uniform branches on
// the kernel arguments: with the branches, the generic kernel took the constant-viscosity path from the second list
// batch of the boundary section on (the uniform condition did not survive that loop), which the two-fluid
// non-constant-viscosity parity test exposed; the select form is also what keeps the tiled and generic kernels bit-equal.
__device__ __forceinline__ void init_visc(const DevParams &p, Self &s)
{
	float c = visc_of(p, s.fl);
	uint32_t cm = p.is_const_visc ? 0xFFFFFFFFu : 0u;
	float kin = (p.compvisc == SPHX_KINEMATIC) ? 1.0f : 0.0f;
	float wA = (p.avgop == SPHX_ARITHMETIC) ? 1.0f : 0.0f, wH = (p.avgop == SPHX_HARMONIC) ? 4.0f : 0.0f,
		wG = (p.avgop == SPHX_GEOMETRIC) ? 2.0f : 0.0f;
	// a single-fluid framework forced to non-constant KINEMATIC viscosity: the reference's with_computational_visc<DYNAMIC>
	// re-derives is_const_visc = true (src/visc_spec.h:268-272,298-300, src/cuda/visc_avg.cu:180-190) and evaluates the
	// constant dynamic formula 2 mu_i/(rho_i rho_j): mu_j := mu_i with the arithmetic weights (pinned by ref_viscavg.npz)
	const bool own = !p.is_const_visc && p.compvisc == SPHX_KINEMATIC && !(p.simflags & SPHX_ENABLE_MULTIFLUID) && p.rheology == SPHX_NEWTONIAN;
	uint32_t om = own ? 0xFFFFFFFFu : 0u;
	if (own) { wA = 1.0f; wH = 0.0f; wG = 0.0f; }
	asm volatile("" : "+v"(c), "+v"(cm), "+v"(kin), "+v"(wA), "+v"(wH), "+v"(wG), "+v"(om));   // keep them per-lane values
	s.visc_c = c; s.visc_constmask = cm; s.visc_ownmask = om; s.visc_kin = kin; s.visc_onemk = 1.0f - kin;
	s.visc_wA = wA; s.visc_wH = wH; s.visc_wG = wG;
	s.visc_mu = c*fmaf(kin, s.rho, s.visc_onemk);      // c rho or c, exactly
}

__device__ __forceinline__ float laminar_factor(const DevParams &p, const Self &s, uint32_t nfl, float n_rho)
{
	const uint32_t cb = __float_as_uint(s.visc_c), nb = __float_as_uint(visc_of(p, nfl));
	const float nc = __uint_as_float((cb & s.visc_constmask) | (nb & ~s.visc_constmask));
	const float nmu0 = nc*fmaf(s.visc_kin, n_rho, s.visc_onemk);
	const float nmu = __uint_as_float((__float_as_uint(s.visc_mu) & s.visc_ownmask) | (__float_as_uint(nmu0) & ~s.visc_ownmask));
	const float S = s.visc_mu + nmu, P = s.visc_mu*nmu;
	const float num = fmaf(s.visc_wA, S, fmaf(s.visc_wH*P, fast_rcp(fmaxf(S, 1.0e-30f)), s.visc_wG*fast_sqrt(P)));
	return num*fast_rcp(s.rho*n_rho);
}

// one pair (i <- j).  Terms, in the reference's order (compute_all_pp_interaction,
// forces_kernel.def:3565-3610): continuity + density diffusion -> force.w; pressure + viscous ->
// force.xyz.  (pcx,pcy,pcz) = own position shifted into the neighbour's cell frame.
template<int KERNEL, int TURB, int COLAGROSSI, bool MOMENTUM, bool DIFFUSE>
__device__ __forceinline__ void pair_interact(const DevParams &p, const Self &s, float inv_h,
	float pcx, float pcy, float pcz, const float4 &npos, const float4 &nvel, const float4 &naux,
	bool same_fluid, bool valid, const float *ntau, float4 &force, bool rt_momentum = true, bool rt_diffuse = true,
	uint32_t nfl = 0, bool f2cap = false, float range = -1.0f)
{
	// range: the influence radius as the caller holds it (the tiled kernel reads it from the shift-table row so that the
	// row is read whole); < 0 = the kernel argument
	// Branch-free on purpose: a rejected pair (list terminator passed, r >= influence radius) gets the weight
	// m_j F_ij = 0 and every term below becomes +-0, which leaves the accumulators untouched -- the same result
	// as the reference's `continue`, without ~6 exec-mask branch sequences per pair and without paying for lane
	// divergence inside a wave.  (Inactive particles sit outside every cell after the sort, so they are never
	// listed and need no test here.)
	// Multiply-adds are written as explicit fmaf where nvcc's default -fmad=true contracts them in the
	// reference as well: the pair loop is VALU-bound and these are ~10 % of its instructions.
	const float rx = pcx - npos.x, ry = pcy - npos.y, rz = pcz - npos.z;
	const float nmass = npos.w;
	const float r2 = fmaf(rz, rz, fmaf(ry, ry, rx*rx));
	const float r = fast_sqrt(r2);
	const bool on = valid && (r < (range < 0.0f ? p.influenceradius : range));

	const float vx = s.vel.x - nvel.x, vy = s.vel.y - nvel.y, vz = s.vel.z - nvel.z;
	const float vel_dot_pos = fmaf(vz, rz, fmaf(vy, ry, vx*rx));
	const float f = kernel_F<KERNEL>(p, r, inv_h);
	const float n_precalc = naux.x, n_sspeed = naux.y, n_P = naux.z, n_rho = naux.w;
	const float mf = on ? nmass*f : 0.0f;

	// mass_continuity_div_vel_term (forces_kernel.def:2140-2151)
	float dsel = 0.0f;
	if (COLAGROSSI == DIFF_FERRARI && DIFFUSE) { // compute_density_diffusion, Ferrari (forces_kernel.def:1607-1635)
		const float gdotr = fmaf(p.gravity[2], rz, fmaf(p.gravity[1], ry, p.gravity[0]*rx));
		const float c0 = p.sscoeff[s.fl];
		const float grav_corr = -gdotr*p.rho0[s.fl]*fast_rcp(c0*c0);
		const float sc = fmaxf(s.sspeed, n_sspeed)*(s.rho - n_rho + grav_corr)*s.inv_rho*fast_rcp(r);
		const float fterm = p.densityDiffCoeff*mf*(sc*r2);
		dsel = (rt_diffuse && r > 1e-4f*p.slength) ? -fterm : 0.0f;
	}
	if (COLAGROSSI == DIFF_COLAGROSSI && DIFFUSE) { // compute_density_diffusion (forces_kernel.def:1916-1952)
		const float gdotr = fmaf(p.gravity[2], rz, fmaf(p.gravity[1], ry, p.gravity[0]*rx));
		const bool diff = same_fluid && rt_diffuse && !(fabsf(s.P - n_P) < fabsf(gdotr*s.rho));
		const float dterm = p.densityDiffCoeff*p.sscoeff[s.fl]*fmaf(n_rho, s.inv_rho, -1.0f)*mf;
		dsel = diff ? dterm : 0.0f;
	}
	float drdt = fmaf(mf, vel_dot_pos, -dsel);
	if (f2cap) {   // SPH_F2: density ratio applied after the diffusion term (mass_continuity_density_ratio :2154-2165)
		const float ratio = s.rho*fast_rcp(n_rho);
		drdt *= __uint_as_float((__float_as_uint(ratio) & s.f2mask) | (0x3f800000u & ~s.f2mask));
	}
	force.w += drdt;

	if (MOMENTUM) {
		// compute_pressure_contrib (forces_kernel.def:2451-2466): -(P_i/rho_i^2 + P_j/rho_j^2) m_j F r_ij
		float pgrad = s.p_precalc + n_precalc;
		if (f2cap) {   // SPH_F2: (P_i + P_j)/(rho_i rho_j) (pressure_gradient_term :2253-2266)
			const float pg2 = (s.P + n_P)*fast_rcp(s.rho*n_rho);
			pgrad = __uint_as_float((__float_as_uint(pg2) & s.f2mask) | (__float_as_uint(pgrad) & ~s.f2mask));
		}
		float kk = -pgrad*mf;
		if (TURB_MODEL(TURB) == SPHX_ARTIFICIAL) {
			// artvisc (src/cuda/visc_kernel.cu:74-85, forces_kernel.def:2748-2764): only for approaching pairs
			// |rho~_j| >= 0 never wins the minimum: it only keeps the fourth component of the neighbour's velocity row live,
			// so that the tiled kernel reads the row as one 16-byte LDS access (v_min3_f32 with an abs modifier: no extra
			// instruction; a 12-byte read costs twice the LDS cycles)
			const float vdpn = fminf(fminf(vel_dot_pos, 0.0f), fabsf(nvel.w));
			const float visc = vdpn*(p.slength*p.artvisccoeff)*(s.sspeed + n_sspeed)*
				fast_rcp((r2 + p.epsartvisc)*(s.rho + n_rho));
			kk = fmaf(visc, mf, kk);
		}
		kk = rt_momentum ? kk : 0.0f;
		if (TURB_MODEL(TURB) == SPHX_SPS) { // forces_kernel.def:2777-2798
			const float mg = rt_momentum ? mf : 0.0f;
			const float xx = s.tau[0] + ntau[0], xy = s.tau[1] + ntau[1], xz = s.tau[2] + ntau[2];
			const float yy = s.tau[3] + ntau[3], yz = s.tau[4] + ntau[4], zz = s.tau[5] + ntau[5];
			force.x = fmaf(mg, fmaf(xz, rz, fmaf(xy, ry, xx*rx)), force.x);
			force.y = fmaf(mg, fmaf(yz, rz, fmaf(yy, ry, xy*rx)), force.y);
			force.z = fmaf(mg, fmaf(zz, rz, fmaf(yz, ry, xz*rx)), force.z);
		}
		force.x = fmaf(kk, rx, force.x); force.y = fmaf(kk, ry, force.y); force.z = fmaf(kk, rz, force.z);
		if (TURB & SPHX_TURB_NEWT) {
			// compute_laminar_visc_contrib, MORRIS (forces_kernel.def:2606-2625): visc_avg * F * (v_i - v_j), after the
			// turbulent term (compute_viscous_contrib :2881-2886)
			const float lv = rt_momentum ? laminar_factor(p, s, nfl, n_rho)*mf : 0.0f;
			force.x = fmaf(lv, vx, force.x); force.y = fmaf(lv, vy, force.y); force.z = fmaf(lv, vz, force.z);
		}
	}
}

// Lennard-Jones repulsion of a boundary particle (compute_repulsive_force forces_kernel.def:3001-3016, LJForce
// src/cuda/forces_kernel.cu:94-103): the whole fluid<-boundary (and, for bodies with force feedback,
// boundary<-fluid) interaction of LJ_BOUNDARY.  Few pairs, generic kernel only: accurate powf and IEEE division.
__device__ __forceinline__ void lj_interact(const DevParams &p, float pcx, float pcy, float pcz,
	const float4 &npos, bool valid, float4 &force)
{
	const float rx = pcx - npos.x, ry = pcy - npos.y, rz = pcz - npos.z;
	const float r = sqrtf(fmaf(rz, rz, fmaf(ry, ry, rx*rx)));
	const bool in = valid && is_active_w(npos.w) && r < p.influenceradius;
	float ljf = 0.0f;
	if (in && r <= p.r0)
		ljf = p.dcoeff*(powf(p.r0/r, p.p1coeff) - powf(p.r0/r, p.p2coeff))/(r*r);
	// Monaghan-Kajtar law (MKForce src/cuda/forces_kernel.cu:105-133, both masses = the central particle's, so they
	// cancel): K w(q)/(beta max(eps, r - d) r), w = 1.8 (1 - q/2)^4 (2q + 1); chosen per lane by a mask
	const float qq = r/p.slength, om = 1.0f - 0.5f*qq;
	const float w = 1.8f*((om*om)*(om*om))*(2.0f*qq + 1.0f);
	const float mkf = (in && r <= 2.0f*p.slength) ? p.MK_K*w/(p.MK_beta*fmaxf(p.epsartvisc, r - p.MK_d)*r) : 0.0f;
	uint32_t mk = p.mk_mask;
	asm volatile("" : "+v"(mk));
	ljf = __uint_as_float((__float_as_uint(mkf) & mk) | (__float_as_uint(ljf) & ~mk));
	force.x += ljf*rx; force.y += ljf*ry; force.z += ljf*rz;
}

// finalizeforcesDevice (forces_kernel.def:4032-4150) for one particle; returns its CFL term
__device__ __forceinline__ float finalize_particle(const DevParams &p, const ForcesArgs &a, uint32_t index,
	const particleinfo &info, const Self &s, float4 force)
{
	float cfl_term = 0.0f;
	const uint32_t ptype = PART_TYPE(info);
	force.w /= p.rho0[s.fl]; // forces_fixup :3212-3218
	if (ptype == PT_FLUID) {
		force.x += p.gravity[0]; force.y += p.gravity[1]; force.z += p.gravity[2];
		// GeometryForce / PlaneForce (src/cuda/forces_kernel.cu:140-203): Lennard-Jones repulsion along the plane
		// normal; the friction term vanishes for the inviscid rheology built here (viscous_plane_coefficient :3103-3107)
		// PlaneForce (:140-185) of a plane given by its unit normal and the grid + local position of a point on it
		auto plane_force = [&](const float nrm[3], const int pgp[3], const float ppos[3]) {
			const float dx = (s.gridPos.x - pgp[0])*p.cs[0] + (s.pos.x - ppos[0]);
			const float dy = (s.gridPos.y - pgp[1])*p.cs[1] + (s.pos.y - ppos[1]);
			const float dz = (s.gridPos.z - pgp[2])*p.cs[2] + (s.pos.z - ppos[2]);
			const float r = fabsf(dx*nrm[0] + dy*nrm[1] + dz*nrm[2]);
			if (r < p.r0) {
				const float DvDt = p.dcoeff*(powf(p.r0/r, p.p1coeff) - powf(p.r0/r, p.p2coeff))/(r*r);
				const float qx = nrm[0]*r, qy = nrm[1]*r, qz = nrm[2]*r;
				force.x += DvDt*qx; force.y += DvDt*qy; force.z += DvDt*qz;
				if (p.rheology == SPHX_NEWTONIAN) {
					// wall friction of PlaneForce (:153-185): -mu partsurf/(m r) v_t, mu = get_laminar_dyn_visc
					const float dynvisc = (p.compvisc == SPHX_KINEMATIC) ? p.visccoeff[s.fl]*s.rho : p.visccoeff[s.fl];
					const float d = (s.vel.x*qx + s.vel.y*qy + s.vel.z*qz)/r, inv = 1.0f/r;
					const float coeff = -dynvisc*p.partsurf/(s.pos.w*r);
					force.x += coeff*(s.vel.x - (d*qx)*inv); force.y += coeff*(s.vel.y - (d*qy)*inv);
					force.z += coeff*(s.vel.z - (d*qz)*inv);
				}
			}
		};
		// DemLJForce (src/cuda/forces_kernel.cu:205-226), the LJ_BOUNDARY case of the finalize kernel (forces_kernel.def:4093-4102):
		// a particle less than demzmin above the terrain is repelled by the terrain's tangent plane below it
		if ((p.simflags & SPHX_ENABLE_DEM) && p.dem && p.boundarytype == SPHX_LJ_BOUNDARY && !p.mk_mask) {
			float nrm[3], ppos[3]; int pgp[3];
			if (dem_plane(p, s.gridPos, s.pos.x, s.pos.y, s.pos.z, nrm, pgp, ppos)) plane_force(nrm, pgp, ppos);
		}
		if ((p.simflags & SPHX_ENABLE_PLANES) && p.numplanes) {
			for (uint32_t k = 0; k < p.numplanes; ++k) plane_force(p.plane_normal[k], p.plane_gridpos[k], p.plane_pos[k]);
		}
		// dyndt_forces_shared_data::store (:3436-3457)
		const float amag = sqrtf(fmaf(force.z, force.z, fmaf(force.y, force.y, force.x*force.x)));
		cfl_term = fmaxf(amag, s.sspeed*s.sspeed/p.slength);
	}
	if (HAS_COMPUTE_FORCE(info) && ptype != PT_VERTEX && a.rbforces) { // :4121-4142
		force.x *= s.pos.w; force.y *= s.pos.w; force.z *= s.pos.w;
		const uint32_t obj = OBJECT_NUM(info);
		const uint32_t rbindex = (uint32_t)((int)info_id(info) + a.rb->rbstart[obj]);
		a.rbforces[rbindex] = force;
		const float armx = (s.gridPos.x - a.rb->cgGridPos[obj][0])*p.cs[0] + (s.pos.x - a.rb->cgPos[obj][0]);
		const float army = (s.gridPos.y - a.rb->cgGridPos[obj][1])*p.cs[1] + (s.pos.y - a.rb->cgPos[obj][1]);
		const float armz = (s.gridPos.z - a.rb->cgGridPos[obj][2])*p.cs[2] + (s.pos.z - a.rb->cgPos[obj][2]);
		a.rbtorques[rbindex] = make_float4(army*force.z - armz*force.y,
			armz*force.x - armx*force.z, armx*force.y - army*force.x, 0.0f);
	}
	a.forces[index] = force;
	return cfl_term;
}

template<int TURB>
__device__ __forceinline__ void load_self(const DevParams &p, const ForcesArgs &a, uint32_t index,
	const particleinfo &info, const float4 &pos, bool multifluid, Self &s)
{
	s.pos = pos;
	s.vel = a.vel[index];
	s.gridPos = grid_pos_from_hash(p, a.hash[index] & CELLTYPE_BITMASK);
	s.fl = multifluid ? FLUID_NUM(info) : 0u;
	const float4 ax = a.aux[index];
	s.p_precalc = ax.x; s.sspeed = ax.y; s.P = ax.z; s.rho = ax.w;
	s.inv_rho = fast_rcp(ax.w);
	if (TURB & SPHX_TURB_NEWT) init_visc(p, s);
	uint32_t f2 = (p.formulation == SPHX_SPH_F2) ? 0xFFFFFFFFu : 0u;
	asm volatile("" : "+v"(f2));
	s.f2mask = f2;
	if (TURB_MODEL(TURB) == SPHX_SPS) {
		const float2 t0 = a.tau0[index], t1 = a.tau1[index], t2 = a.tau2[index];
		s.tau[0] = t0.x; s.tau[1] = t0.y; s.tau[2] = t1.x; s.tau[3] = t1.y; s.tau[4] = t2.x; s.tau[5] = t2.y;
	}
}

// run-time section: sec 0 = fluid neighbours (slots 0 upward), sec 1 = boundary neighbours
// (slots neibboundpos downward); `batch` counts TILE_NB-entry batches from the section start
__device__ __forceinline__ void load_list_rt(const DevParams &p, const neibdata *__restrict__ list,
	uint32_t index, int sec, int batch, uint32_t nd[TILE_NB])
{
#pragma unroll
	for (int k = 0; k < TILE_NB; ++k) {
		const int e = batch*TILE_NB + k;
		const int sl = sec ? max((int)p.neibboundpos - e, 0) : min(e, (int)p.neiblistsize - 1);
		nd[k] = list[(size_t)sl*p.stride + index];
	}
}

template<int NPTYPE, int N>
__device__ __forceinline__ void load_list_batch(const DevParams &p, const neibdata *__restrict__ list,
	uint32_t index, int slot, uint32_t nd[N])
{
#pragma unroll
	for (int k = 0; k < N; ++k) {
		// entries past the terminator are never used; the clamp only keeps the address in bounds
		const int sl = (NPTYPE == PT_FLUID) ? min(slot + k, (int)p.neiblistsize - 1) : max(slot - k, 0);
		nd[k] = list[(size_t)sl*p.stride + index];
	}
}

#endif
