// forces_args.h -- what the C ABI of the forces engine (forces.hip) and the translation units that hold the pair loops
// (forces_part.hip, forces_sa.hip, forces_probe.hip) share: the argument blocks, the template codes and the launchers' names.
#ifndef SPHX_FORCES_ARGS_H
#define SPHX_FORCES_ARGS_H

#include "sphx_internal.h"

struct ForcesArgs {
	float4 *forces;
	float  *cfl;
	float4 *rbforces;
	float4 *rbtorques;
	const float4 *pos;
	const float4 *vel;
	const particleinfo *info;
	const uint32_t *hash;
	const uint32_t *cellStart;
	const neibdata *neibsList;
	const float2 *tau0, *tau1, *tau2;
	const float4 *aux;   // per-particle EOS pre-pass {P/rho^2, c, P, rho}
	float2 *otau0, *otau1, *otau2; float *oturbvisc;   // stress mode of the tiled kernel (SPHX_TURB_STRESS): outputs
	const float4 *tauPack;   // SPS + tiled kernel: [0,n) = {xx,xy,xz,yy}, [n,2n) = {yz,zz,P/rho^2,c or P} (tau_pack_kernel); tauPackN = n
	uint32_t tauPackN;
	// tiled kernel: the tile lists of this neighbour list (tile_lists_kernel)
	const uint2 *tileList;       // the stream of list batches: [batch][64 lanes] x 4 uint16 window offsets
	const uint32_t *tileRuns;    // [tile][TILE_RUNTAB]: which wave walks which batches of which chunk (tile_format.h)
	const uint32_t *tileRows;    // [tile][TILE_ROWDESC]: the window rows
	const uint32_t *tileLaneRec; // per lane of every chunk: byte offset of the particle's own row in its tile's window | flags << 16
	const uint32_t *tileLaneIndex; // ... the particle (0xFFFFFFFF: idle lane)
	float4 *xsph;        // ENABLE_XSPH: mean velocity correction of fluid particles, else NULL
	const float4 *saGam; // SA_BOUNDARY modes of the tiled kernel (SPHX_TURB_SA*): gamma in .w (diffusion mode), the step's dt
	float saDt;
	const RbParams *rb;
	uint32_t fromParticle, toParticle, cflOffset;
	int wholeRange;       // tiled kernel: [fromParticle, toParticle) holds every tiled particle (no per-tile / per-particle range test)
	uint32_t numBlocks;   // generic kernel: blocks of SPHX_BLOCK_FORCES particles to cover
	int compute_object_forces;
	uint32_t *pin;              // always NULL (see pin_batch)
#ifdef SPHX_TILE_DEBUG_BUILD
	unsigned long long *prof;   // per wave of every workgroup: cycles per phase of the tile loop (SPHX_TILE_DEBUG=16), else NULL
#endif
};

// density-diffusion template codes (the parameter keeps its historical name COLAGROSSI): 1 keeps `true` = Colagrossi
#define DIFF_NONE 0
#define DIFF_COLAGROSSI 1
#define DIFF_FERRARI 2
// Colagrossi with a gravity that has a z component only: g.r is the one product g_z r_z (pair_interact_pk; the plain tiled pass only)
#define DIFF_COLAGROSSI_GZ 3

// TURB template codes: the turbulence model in the low bits, SPHX_TURB_NEWT set for the NEWTONIAN rheology
#define SPHX_TURB_NEWT 8
#define SPHX_TURB_MF 16     // tiled kernel only: more than one fluid, the neighbour's fluid number rides in the EOS row (eos_kernel)
#define SPHX_TURB_STRESS 32 // tiled kernel only: not a forces pass but the SPS stress tensor (SPSstressMatrixDevice) over the same tiles
// SA_BOUNDARY over the same tiles (sa_bounds.hip finishes each of them with the boundary-element terms, by the list walker):
// the particle <- particle sums of the forces (fluid and vertex neighbours; the vertex section takes the place of the boundary
// section in the tile lists), of the density summation and of the Brezzi density diffusion
#define SPHX_TURB_SA 64
#define SPHX_TURB_SA_DSUM 128
#define SPHX_TURB_SA_DIFF 256
#define SPHX_TURB_SA_ANY (SPHX_TURB_SA | SPHX_TURB_SA_DSUM | SPHX_TURB_SA_DIFF)
#define TURB_MODEL(T) ((T) & 7)

// the SPS stress tensor by the list walker (sps_kernel, forces_generic.h)
struct SpsArgs {
	float2 *tau0, *tau1, *tau2;
	float *turbvisc;
	const float4 *pos, *vel;
	const particleinfo *info;
	const uint32_t *hash, *cellStart;
	const neibdata *neibsList;
	uint32_t numParticles;
};

// forces_part.hip is compiled once per SPH kernel type with SPHX_FORCES_PART = that type (see the Makefile), for the template
// instantiations of the type (each is minutes of compile time: ~30 tiled + ~30 generic kernels); the C ABI reaches them through
// the sphx_part_* functions below.
#define SPHX_PART_DECL(K) \
	int sphx_part_forces_k##K(const sphx_ctx *ctx, dim3 grid, hipStream_t stream, const ForcesArgs &a, bool use_tiles); \
	void sphx_part_stress_k##K(const sphx_ctx *ctx, hipStream_t stream, const ForcesArgs &fa); \
	void sphx_part_sps_k##K(const sphx_ctx *ctx, dim3 grid, hipStream_t stream, const SpsArgs &a, const uint32_t *guard);
SPHX_PART_DECL(1) SPHX_PART_DECL(2) SPHX_PART_DECL(3) SPHX_PART_DECL(4)
#undef SPHX_PART_DECL
// SA_BOUNDARY modes of the tiled kernel (Wendland; its own translation unit: forces_sa.hip)
void sphx_part_sa_tile(const sphx_ctx *ctx, hipStream_t stream, const ForcesArgs &fa, int mode, bool newtonian);
static_assert(SPHX_CUBICSPLINE == 1 && SPHX_QUADRATIC == 2 && SPHX_WENDLAND == 3 && SPHX_GAUSSIAN == 4, "part numbering = kernel type");

// sphx_forces_timing: HIP events on the launch stream around the dominant kernel of a forces pass
struct ForcesTimer {
	const sphx_ctx *ctx; hipStream_t stream; hipEvent_t stop;
	ForcesTimer(const sphx_ctx *c, hipStream_t s, bool on) : ctx(c), stream(s), stop(nullptr) {
		if (!on || !c->time_forces || !c->forces_events) return;
		hipEvent_t e0, e1;
		if (hipEventCreate(&e0) != hipSuccess || hipEventCreate(&e1) != hipSuccess) return;
		(void)hipEventRecord(e0, s);
		c->forces_events->push_back(std::make_pair(e0, e1));
		stop = e1;
	}
	~ForcesTimer() { if (stop) (void)hipEventRecord(stop, stream); }
};

// The plain pass (pair_interact_pk with the Colagrossi term) has a second instantiation for a gravity along z, which is what
// nearly every problem has: is this launch one of its?  The values are the context's own, so a gravity that changes during
// a run is looked at again at every launch; -0.0f counts as zero.  sphx_dbg_forces_general_gravity turns it off for a context.
static bool plain_gravity_z(const sphx_ctx *ctx)
{
	const DevParams &p = ctx->dev;
	return !ctx->general_gravity && p.gravity[0] == 0.0f && p.gravity[1] == 0.0f &&
		p.kerneltype == SPHX_WENDLAND && p.turbmodel == SPHX_ARTIFICIAL && p.numfluids <= 1 && p.densitydiff == SPHX_COLAGROSSI &&
		p.boundarytype != SPHX_LJ_BOUNDARY;
}

#endif
