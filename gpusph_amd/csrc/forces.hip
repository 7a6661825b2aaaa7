// forces.hip -- forces engine for gfx950: fused pair summation (fluid<-fluid, fluid<-boundary,
// boundary<-fluid) + finalize + CFL block maxima in ONE launch, CFL reduction -> dt on the
// device, rigid-body force totals, SPS stress tensor.
// Replaces CUDAForcesEngine / CUDAViscEngine (GPUSPH src/cuda/forces.cu:252-1006,
// src/cuda/forces_kernel.def:3914-4150, src/cuda/visc_kernel.cu:759-811).
//
// Why one launch: the reference launches forcesDevice 3x + finalizeforcesDevice, each doing a
// read-modify-write of forces[] (16 B x 2 x 4 per particle) and re-reading pos/vel/info/hash.
// The neighbour list is typed (fluid slots grow up from 0, boundary slots down from
// neibboundpos), so a single thread can walk both sections in the reference's order and keep the
// accumulator in registers: forces[] is written once, own data is read once.
//
// This file is the C ABI with its small kernels and tile_lists_kernel, the producer of the tables the tiled kernel walks (their
// format: tile_format.h).  The pair loops are instantiated elsewhere and reached through the sphx_part_* functions of
// forces_args.h: forces_part.hip (per SPH kernel type; forces_generic.h, forces_tile.h over forces_pair.h) and forces_sa.hip.
#include "forces_args.h"
#include "tile_format.h"

// ------------------------------------------------------------------------------------------
// per-particle EOS pre-pass: aux[i] = {P/rho^2, c, P, rho}.
// The reference recomputes P (__powf), soundSpeed (__powf) and P/rho^2 (division) of the
// NEIGHBOUR inside every pair (forces_kernel.def:690-702,1126-1128; phys_core.cu:99-135).  They are
// pure functions of the neighbour's own rho~, so evaluating them once per particle and gathering
// 16 B gives the same numbers with ~20 fewer issue slots per pair -- and, being per particle, can
// afford the accurate powf and IEEE division (closer to the oracle than __powf would be).
// ------------------------------------------------------------------------------------------
static __global__ void __launch_bounds__(256)
eos_kernel(DevParams p, const float4 *__restrict__ vel, const particleinfo *__restrict__ info,
	float4 *__restrict__ aux, uint32_t n)
{
	const uint32_t i = blockIdx.x*256 + threadIdx.x;
	if (i >= n) return;
	const uint32_t fl = (p.numfluids > 1) ? FLUID_NUM(info[i]) : 0u;
	const float ratio = vel[i].w + 1.0f;
	const float P = p.bcoeff[fl]*(powf(ratio, p.gammacoeff[fl]) - 1.0f);
	float c = p.sscoeff[fl]*powf(ratio, p.sspowercoeff[fl]);
	// multi-fluid runs: the fluid number replaces the two lowest mantissa bits of the sound speed (2^-22 relative; c only
	// enters the artificial viscosity, Ferrari and CFL terms), so that the LDS window of the tiled kernel, which holds
	// pos / vel / this row but not the particle info, can tell same-fluid pairs and per-fluid viscosities.  Both forces
	// kernels read the same tagged value; single-fluid runs are untouched.
	if (p.numfluids > 1) c = __uint_as_float((__float_as_uint(c) & ~3u) | fl);
	const float rho = ratio*p.rho0[fl];
	aux[i] = make_float4(P/(rho*rho), c, P, rho);
}

// SPS + tiled kernel: the three float2 arrays of BUFFER_TAU repacked as two float4 rows per particle, so that the window
// rows can be staged with the same 16-byte LDS DMA as pos / vel / the EOS row.  The two free slots of the second row carry what
// a pair needs of the neighbour's EOS row besides the density (which is one add and one multiply away from the velocity row's
// rho~): P/rho^2 and the one of {sound speed, pressure} the run's density diffusion reads (Ferrari / none: c; Colagrossi: P).
// With one fluid the window of an SPS run then needs no EOS rows at all: 64 instead of 80 bytes per record, tiles of six
// instead of four cells (TILE_WCAP_SPS1), 82 % instead of 55 % of the lanes of a tile occupied.
static __global__ void __launch_bounds__(256)
tau_pack_kernel(const float2 *__restrict__ t0, const float2 *__restrict__ t1, const float2 *__restrict__ t2,
	const float4 *__restrict__ aux, int wantPressure, float4 *__restrict__ out, uint32_t n)
{
	const uint32_t i = blockIdx.x*256 + threadIdx.x;
	if (i >= n) return;
	const float2 a = t0[i], b = t1[i], c = t2[i];
	const float4 e = aux[i];
	out[i] = make_float4(a.x, a.y, b.x, b.y);
	out[(size_t)n + i] = make_float4(c.x, c.y, e.x, wantPressure ? e.z : e.y);
}

// ------------------------------------------------------------------------------------------
// CFL reduction -> dt.  fmaxDevice (src/cuda/forces_kernel.cu:734-793) + dtreduce
// (src/cuda/forces.cu:556-606), finished on the device so that the adaptive dt never has to
// visit the host inside a step.
// ------------------------------------------------------------------------------------------
#define BLOCK_FMAX 256

__device__ __forceinline__ float block_max_256(float v)
{
	__shared__ float wm[4];
#pragma unroll
	for (int d = 32; d > 0; d >>= 1) v = fmaxf(v, __shfl_down(v, d));
	if ((threadIdx.x & 63u) == 0) wm[threadIdx.x >> 6] = v;
	__syncthreads();
	v = fmaxf(fmaxf(wm[0], wm[1]), fmaxf(wm[2], wm[3]));
	__syncthreads();
	return v;
}

static __global__ void __launch_bounds__(BLOCK_FMAX)
fmax_kernel(float *__restrict__ output, const float4 *__restrict__ input, uint32_t numquarts)
{
	float m = 0.0f;
	for (uint32_t i = blockIdx.x*BLOCK_FMAX + threadIdx.x; i < numquarts; i += BLOCK_FMAX*gridDim.x) {
		const float4 v = input[i];
		m = fmaxf(m, fmaxf(fmaxf(v.x, v.y), fmaxf(v.z, v.w)));
	}
	m = block_max_256(m);
	if (threadIdx.x == 0) output[blockIdx.x] = m;
}

static __global__ void __launch_bounds__(BLOCK_FMAX)
dt_final_kernel(float *__restrict__ d_dt, const float *__restrict__ partial, uint32_t numPartials,
	float slength, float dtadaptfactor, float sspeed_cfl, float max_kinematic, int viscous, int combine_min)
{
	float m = 0.0f;
	for (uint32_t i = threadIdx.x; i < numPartials; i += BLOCK_FMAX) m = fmaxf(m, partial[i]);
	m = block_max_256(m);
	if (threadIdx.x == 0) {
		float dt = dtadaptfactor*fminf(sqrtf(slength/m), slength/sspeed_cfl);
		if (viscous) {
			float dt_visc = slength*slength/max_kinematic;
			dt_visc = (float)((double)dt_visc*0.125);
			if (dt_visc < dt) dt = dt_visc;
		}
		d_dt[0] = combine_min ? fminf(d_dt[0], dt) : dt;
	}
}

// ------------------------------------------------------------------------------------------
// rigid-body totals: the reference does two thrust::inclusive_scan_by_key and reads the last
// element of each segment (src/cuda/forces.cu:966-1004); only those totals are consumed
// (src/GPUWorker.cc REDUCE_BODIES_FORCES), so they are produced directly: one block per body.
// ------------------------------------------------------------------------------------------
static __global__ void __launch_bounds__(256)
rb_reduce_kernel(const float4 *__restrict__ rbforces, const float4 *__restrict__ rbtorques,
	const uint32_t *__restrict__ rbnum, const uint32_t *__restrict__ lastindex,
	float *__restrict__ totals /* 6 per body */, uint32_t numParts)
{
	const uint32_t body = blockIdx.x;
	const uint32_t last = lastindex[body];
	const uint32_t key = rbnum[last];
	float fx = 0, fy = 0, fz = 0, tx = 0, ty = 0, tz = 0;
	for (uint32_t i = threadIdx.x; i < numParts && i <= last; i += 256) {
		if (rbnum[i] == key) {
			const float4 f = rbforces[i], t = rbtorques[i];
			fx += f.x; fy += f.y; fz += f.z; tx += t.x; ty += t.y; tz += t.z;
		}
	}
	__shared__ float red[6][4];
	float v[6] = { fx, fy, fz, tx, ty, tz };
#pragma unroll
	for (int c = 0; c < 6; ++c) {
#pragma unroll
		for (int d = 32; d > 0; d >>= 1) v[c] += __shfl_down(v[c], d);
		if ((threadIdx.x & 63u) == 0) red[c][threadIdx.x >> 6] = v[c];
	}
	__syncthreads();
	if (threadIdx.x < 6)
		totals[6*body + threadIdx.x] = red[threadIdx.x][0] + red[threadIdx.x][1] + red[threadIdx.x][2] + red[threadIdx.x][3];
}

// ------------------------------------------------------------------------------------------
// C ABI
// ------------------------------------------------------------------------------------------
extern "C" uint32_t sphx_forces_fmax_elements(uint32_t n) { return round_up_u(div_up_u(n, SPHX_BLOCK_FORCES), 4u); }
extern "C" uint32_t sphx_forces_fmax_temp_elements(uint32_t nels)
{
	const uint32_t numquarts = nels/4;
	uint32_t numBlocks = div_up_u(numquarts, BLOCK_FMAX);
	if (numBlocks > 1) {
		numBlocks = round_up_u(numBlocks, 4u);
		if (numBlocks > BLOCK_FMAX*4) numBlocks = BLOCK_FMAX*4;
	}
	return numBlocks;
}
extern "C" uint32_t sphx_forces_round_particles(uint32_t n) { return (n/SPHX_BLOCK_FORCES)*SPHX_BLOCK_FORCES; }

// ------------------------------------------------------------------------------------------
// Tile lists: the reference-format neighbour lists of the tiled particles, translated once per neighbour-list build
// into the form the tiled pair loop walks (see walk_runs, forces_tile.h).  One workgroup per tile, one thread per home particle:
//  1. the window layout of the tile (tile_rows: first record, length and first slot of each of the 16 rows, and whether the
//     row is one range in memory): window row r holds the cells of grid row (g2-1+(r&3), g3-1+(r>>2)) from column ca-1 on, rows
//     follow each other without gaps, so the slot of a record is (records of the rows before) + (records of the cells before
//     it in its row) + its index in its cell;
//  2. the home particles sorted by the length of their fluid section, longest first (a stable counting sort on the lengths the
//     list builder left in neib_counts), and cut into chunks of 64: the lanes of a wave then walk lists of nearly equal
//     length (in home order a chunk is padded to its longest list: 14 % of the pair slots were padding);
//  3. the schedule: all batches of the tile (chunk after chunk, fluid section then second section, each padded to the chunk's
//     longest) split evenly over the eight waves of the forces kernel -> runs (a wave's stretch of one chunk), the run table;
//  4. space for the tile's list stream and lane tables from two global cursors (tile_ctl[12], [13]);
//  5. the translation: every lane rewrites its particle's entries as window offsets (slot * 16: the byte offset of the
//     neighbour's row in the window arrays, used as the LDS address as it is), four to a batch, padded with offset 0 (the
//     dummy record), straight into the stream position its wave will read it from (512-byte coalesced stores).
// ------------------------------------------------------------------------------------------
#define TL_THREADS TILE_PMAX
#define TL_BINS 132      // list lengths 0..128 (+ padding)

// which home particle of the tile thread t stands for: the four home rows one after the other (build_tiles_kernel)
struct TileHome { uint32_t index; int hrow; };
__device__ __forceinline__ TileHome tile_home(uint32_t dw /* this lane's word of the descriptor */, uint32_t t)
{
	TileHome h;
	const uint32_t c0 = (uint32_t)__builtin_amdgcn_readlane((int)dw, TILE_D_COUNT), c1n = (uint32_t)__builtin_amdgcn_readlane((int)dw, TILE_D_COUNT + 1),
		c2n = (uint32_t)__builtin_amdgcn_readlane((int)dw, TILE_D_COUNT + 2);
	int hrow = 0; uint32_t hoff = t;
	if (hoff >= c0) { hoff -= c0; hrow = 1; if (hoff >= c1n) { hoff -= c1n; hrow = 2; if (hoff >= c2n) { hoff -= c2n; hrow = 3; } } }
	const uint32_t f0 = (uint32_t)__builtin_amdgcn_readlane((int)dw, TILE_D_FIRST), f1 = (uint32_t)__builtin_amdgcn_readlane((int)dw, TILE_D_FIRST + 1),
		f2 = (uint32_t)__builtin_amdgcn_readlane((int)dw, TILE_D_FIRST + 2), f3 = (uint32_t)__builtin_amdgcn_readlane((int)dw, TILE_D_FIRST + 3);
	const uint32_t hfirst = (hrow == 0) ? f0 : (hrow == 1) ? f1 : (hrow == 2) ? f2 : f3;
	h.hrow = hrow;
	h.index = hfirst + hoff;
	return h;
}

// The share of a tile's batches that each wave of the forces kernel walks, in 1/256: `lo` for each of the waves 0..3, 64 - lo
// for each of the waves 4..7 (the second wave of every SIMD).  Even shares (lo = 32) for every kernel but one: in the plain
// forces pass (artificial or no viscosity, one fluid, no SA walls) the second wave of a SIMD reaches the end of its pair phase
// first when the shares are equal (phase timers, profiles/r04_tile_phases_32M.txt: waves 0..7 wait 0.06, 0.18, 0.24, 0.37, 0.81,
// 0.77, 0.69, 1.16 M cycles of 9.26 M at the barrier on top of the next tile), and the tile ends when the last wave does.
// Measured at 32 M particles, two boxes (scripts/ab_forces.sh; ms per launch): lo = 32: 3.877;  31: 3.874;  30: 3.822;  29: 3.837;
// weights in proportion to the measured waits (29 30 30 31 34 33 33 36): 3.860, twice that correction: 3.919 -- the waits are not
// pair work that can be handed over one for one (the two waves of a SIMD share its issue slots).  The other instantiations
// LOSE with lo = 30 (scripts/measure_all.sh: SPS forces at 8 M 1.75 -> 1.90 ms per launch, two fluids 1.24 -> 1.35, the laminar +
// Ferrari pass of the StillWater mirror 4.5 % per step): their waves are balanced differently, so they keep even shares
#define TILE_SHARE_LO_PLAIN 30u
__device__ __forceinline__ uint32_t tile_share_start(uint32_t w, uint32_t lo)     // sum of the weights of the waves before w; 256 for w = 8
{
	return w <= 4u ? w*lo : 4u*lo + (w - 4u)*(64u - lo);
}

// Measured at 32 M particles (scripts/ab_builder.sh, round 4; linearisation xzy).  First a warning: with the sixteen list loads
// of the translation loop each under a condition of its own, the compiler made every load wait for all the earlier ones
// (s_waitcnt vmcnt(0) in front of each) in SOME builds, depending on edits elsewhere in the kernel -- the same source ran 7.4 or
// 11.3 ms per launch, and every A/B of this kernel made before that was found compared the two states of the compiler as much as
// the two variants.  The loads are unconditional now (the address is valid for every thread) and issue back to back (checked in
// the ISA): 6.3 ms.  With that: 8 / 16 / 24 / 32 loads in flight per lane 6.58 / 6.27 / 6.81 / 6.71 ms; two workgroups per CU
// 7.24; the tile's stream assembled in LDS and written as one linear copy instead of eight-byte stores from all over the tile
// 6.85 against 6.65 (yzx: 7.49 against 7.25): neither the latency of the loads nor the scattered stores bound it.  Without the
// translation (sections 1 to 4 alone) 2.29 ms, with the fluid section only 5.89: the 3.6 ms of the fluid section are its
// ~15 vector instructions and one LDS look-up per entry at ten waves per CU.  (Tried before the loads were fixed, and to be read
// with the warning above: a second, wave-major copy of the list written by build_neibs_kernel's ring -- this kernel 7.36 -> 6.37 ms,
// build_neibs_kernel 12.9 -> 14.1 ms for the extra stores.)
#define TL_MINWAVES 1
#define TL_LOADS 16
#define TL_GRIDMUL 8
__global__ void __launch_bounds__(TL_THREADS, TL_MINWAVES)
tile_lists_kernel(DevParams p, const neibdata *__restrict__ list, const uint32_t *__restrict__ neibCounts,
	const particleinfo *__restrict__ info, const uint32_t *__restrict__ hash,
	const uint32_t *__restrict__ cellStart, const uint32_t *__restrict__ cellEnd,
	uint32_t *__restrict__ tiles, uint32_t *tileCtl, uint32_t *__restrict__ tileRows, uint32_t *__restrict__ tileRuns,
	uint2 *__restrict__ tileList, uint32_t listCapBatches, uint32_t *__restrict__ laneRec, uint32_t *__restrict__ laneIndex,
	uint32_t laneCap, int saVertex /* SA_BOUNDARY lists: the second section is the VERTEX section */,
	uint32_t shareLo /* tile_share_start */)
{
	__shared__ uint32_t sCellRel[TILE_WROWS*TILE_KW], sCellBase[TILE_WROWS*TILE_KW], sCellStart[TILE_WROWS*TILE_KW];
	__shared__ uint32_t sRowTotal[TILE_WROWS], sRowStart[TILE_WROWS], sRowContig[TILE_WROWS], sRowBase[TILE_WROWS];
	__shared__ int sCodeOff[32];                                   // cell code-1 -> window-table offset
	__shared__ uint16_t sCB[TILE_HROWS*TILE_MAXCELLS*27 + 8];      // [home cell][code] -> slot of the cell's first record
	__shared__ uint16_t sHist[TILE_CHUNKS][TL_BINS];               // per wave: particles with a fluid section of that length; then: ... in the waves before
	__shared__ uint16_t sBinStart[TL_BINS];
	__shared__ uint32_t sBinWave[4];
	__shared__ uint16_t sLaneOf[TILE_PMAX], sLenF[TILE_PMAX], sLenB[TILE_PMAX];   // lane of the tile by home-order number; list lengths by lane
	__shared__ uint32_t sChunkF[TILE_CHUNKS + 1], sChunkB[TILE_CHUNKS + 1], sChunkStart[TILE_CHUNKS + 1];   // batches per section; first batch
	__shared__ uint32_t sSorted[32];
	__shared__ uint32_t sRunTab[TILE_RUNTAB];
	__shared__ uint32_t sBase[4];                                  // list base, lane base, overflow
	const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
	// tiling overflowed: the generic kernel handles this list.  (One read per workgroup: another workgroup of this very kernel may
	// raise the flag at any time, and threads that disagree about it would not meet at the barriers below)
	if (tid == 0) sBase[3] = tileCtl[1];
	__syncthreads();
	if (sBase[3]) return;
	const uint32_t numTiles = tileCtl[0];
	// neighbour-cell offset (ox,oy,oz) -> index of that cell in the window table, relative to the
	// particle's own (row, column): o1 + KW*(o2+1) + 4*KW*(o3+1) + 1 with (o1,o2,o3) the offsets along COORD1..3
	if (tid < 27) {
		const int c = (int)tid;                    // d_cell_to_offset order: c = (x+1) + 3(y+1) + 9(z+1)
		const int cz = c/9, cy = (c - cz*9)/3;
		const int ox = c - cz*9 - cy*3 - 1, oy = cy - 1, oz = cz - 1;
		const int mx = (p.c1 == 0) ? 1 : (p.c2 == 0) ? TILE_KW : 4*TILE_KW;
		const int my = (p.c1 == 1) ? 1 : (p.c2 == 1) ? TILE_KW : 4*TILE_KW;
		const int mz = (p.c1 == 2) ? 1 : (p.c2 == 2) ? TILE_KW : 4*TILE_KW;
		sCodeOff[c] = ox*mx + oy*my + oz*mz + 1 + TILE_KW + 4*TILE_KW;
	}
	const int wr = (int)(tid/TILE_KW), wcol = (int)(tid - (tid/TILE_KW)*TILE_KW);   // my window cell (tid < 256)
	const size_t stride = (size_t)p.stride;
	// Everything a tile's setup reads from memory -- its descriptor, the window's cells (section 1), the list lengths / hash / info of the
	// thread's home particle (sections 2 and 5) -- depends on the tile's number alone, and the setup is a chain of barriers with nothing to
	// hide a round trip behind (~8 us per tile, half the kernel).  So it is asked for one tile ahead (the descriptor two ahead): while a
	// tile's lists are translated the next tile's rows arrive.  (Round 6: 4.61 -> 4.28 ms at 32 M with the loads at the top of the same
	// tile's setup, profiles/r06_tile_lists_prefetch_ab.txt.)
	struct TilePre { uint32_t index, cnt, hash; particleinfo info; uint32_t wStart, wEnd; };
	auto desc_of = [&](uint32_t t) -> uint32_t { return t < numTiles ? tiles[(size_t)TILE_DESC*t + (lane & (uint32_t)(TILE_DESC - 1))] : 0u; };
	auto ask = [&](uint32_t dd, bool real, TilePre &q) {
		q.index = 0u; q.cnt = 0u; q.hash = 0u; q.info = particleinfo{0, 0, 0, 0}; q.wStart = CELL_EMPTY; q.wEnd = 0u;
		if (!real) return;
		const uint32_t Pn = (uint32_t)(__builtin_amdgcn_readlane((int)dd, TILE_D_COUNT) + __builtin_amdgcn_readlane((int)dd, TILE_D_COUNT + 1) +
			__builtin_amdgcn_readlane((int)dd, TILE_D_COUNT + 2) + __builtin_amdgcn_readlane((int)dd, TILE_D_COUNT + 3));
		q.index = tile_home(dd, tid < Pn ? tid : 0u).index;
		q.cnt = neibCounts[q.index]; q.hash = hash[q.index]; q.info = info[q.index];
		if (tid < TILE_WROWS*TILE_KW) {
			const uint32_t h = window_cell_hash(p, __builtin_amdgcn_readlane((int)dd, TILE_D_G2), __builtin_amdgcn_readlane((int)dd, TILE_D_G3),
				__builtin_amdgcn_readlane((int)dd, TILE_D_FIRSTCELL), __builtin_amdgcn_readlane((int)dd, TILE_D_NCELLS), wr, wcol);
			if (h != 0xFFFFFFFFu) { q.wStart = cellStart[h]; q.wEnd = cellEnd[h]; }
		}
	};
	uint32_t dAhead = desc_of(blockIdx.x);
	TilePre ahead;
	ask(dAhead, blockIdx.x < numTiles, ahead);
	uint32_t dAhead2 = desc_of(blockIdx.x + gridDim.x);
	for (uint32_t tile = blockIdx.x; tile < numTiles; tile += gridDim.x) {
		__syncthreads();   // the previous tile's tables are no longer read
		const uint32_t d = dAhead;      // the descriptor, a word per lane
		const TilePre pre = ahead;
		dAhead = dAhead2;
		ask(dAhead, tile + gridDim.x < numTiles, ahead);
		dAhead2 = desc_of(tile + 2u*gridDim.x);
		const int ca = __builtin_amdgcn_readlane((int)d, TILE_D_FIRSTCELL);
		const uint32_t P = (uint32_t)(__builtin_amdgcn_readlane((int)d, TILE_D_COUNT) + __builtin_amdgcn_readlane((int)d, TILE_D_COUNT + 1) +
			__builtin_amdgcn_readlane((int)d, TILE_D_COUNT + 2) + __builtin_amdgcn_readlane((int)d, TILE_D_COUNT + 3));        // home particles (<= TILE_PMAX)
		const uint32_t C = (P + 63u)/64u;
		const uint32_t preCnt = pre.cnt, preHash = pre.hash;
		const particleinfo preInfo = pre.info;
		for (uint32_t e = tid; e < TILE_CHUNKS*TL_BINS; e += TL_THREADS) (&sHist[0][0])[e] = 0;
		if (tid < TILE_WROWS*TILE_KW) {
			uint32_t wStart = 0, wCnt = 0;      // window_cell, asked for a tile ahead
			if (pre.wStart != CELL_EMPTY) { wStart = pre.wStart; wCnt = pre.wEnd - pre.wStart; }
			uint32_t incl = wCnt;
			uint32_t lo = wCnt ? wStart : 0xFFFFFFFFu;
			uint32_t hi = wCnt ? wStart + wCnt : 0u;
#pragma unroll
			for (int dd = 1; dd < TILE_KW; dd <<= 1) {
				const uint32_t t = __shfl_up(incl, dd, TILE_KW);
				if (wcol >= dd) incl += t;
			}
#pragma unroll
			for (int dd = TILE_KW/2; dd > 0; dd >>= 1) {
				lo = min(lo, (uint32_t)__shfl_xor(lo, dd, TILE_KW));
				hi = max(hi, (uint32_t)__shfl_xor(hi, dd, TILE_KW));
			}
			sCellRel[tid] = incl - wCnt;
			sCellStart[tid] = wStart;
			// one DMA per row needs the cells to lie in memory in window order: each non-empty cell starts where
			// the previous ones end.  (Extent == count alone is not enough: a periodic row that is wholly inside
			// the window has the wrapped column first in the window but last in memory.)
			uint32_t inOrder = (wCnt == 0u || wStart - lo == incl - wCnt) ? 1u : 0u;
#pragma unroll
			for (int dd = TILE_KW/2; dd > 0; dd >>= 1)
				inOrder &= (uint32_t)__shfl_xor(inOrder, dd, TILE_KW);
			if (wcol == TILE_KW - 1) {
				sRowTotal[wr] = incl;
				sRowStart[wr] = incl ? lo : 0u;
				sRowContig[wr] = (incl == 0u || (hi - lo == incl && inOrder)) ? 1u : 0u;
			}
		}
		__syncthreads();
		if (tid < TILE_WROWS*TILE_KW) {
			uint32_t base = 0;
			for (int r = 0; r < wr; ++r) base += sRowTotal[r];
			sCellBase[tid] = sCellRel[tid] + base;
			if (wcol == 0) sRowBase[wr] = base;
		}
		__syncthreads();
		if (tid < TILE_WROWS) tileRows[(size_t)TILE_ROWDESC*tile + tid] = sRowStart[tid];
		else if (tid < TILE_WROWS + 8u) {
			const uint32_t k = tid - TILE_WROWS;
			tileRows[(size_t)TILE_ROWDESC*tile + TILE_ROWS_TOTAL + k] = tile_rows_pack_total(sRowTotal[2*k], sRowTotal[2*k + 1]);
		} else if (tid < TILE_WROWS + 16u) {
			const uint32_t k = tid - TILE_WROWS - 8u;
			const uint32_t b0 = tile_rows_base_half(sRowBase[2*k], sRowContig[2*k]);
			const uint32_t b1 = tile_rows_base_half(sRowBase[2*k + 1], sRowContig[2*k + 1]);
			tileRows[(size_t)TILE_ROWDESC*tile + TILE_ROWS_BASE + k] = tile_rows_pack_base(b0, b1);
		}
		for (uint32_t e = tid; e < TILE_HROWS*TILE_MAXCELLS*27; e += TL_THREADS) {
			const uint32_t m = e/27u, c1 = e - m*27u;
			const uint32_t hr = m/TILE_MAXCELLS, col = m - hr*TILE_MAXCELLS;
			sCB[e + 1] = (uint16_t)sCellBase[sCodeOff[c1] + (int)(((hr & 1u) + 4u*(hr >> 1))*TILE_KW + col)];
		}

		// ---- 2. sort the home particles by the length of their fluid section, longest first; equal lengths keep their home order
		bool overflow = false;
		uint32_t F = 0, B = 0;
		const bool inHome = tid < P;
		if (inHome) {
			const uint32_t cnt = preCnt;
			F = cnt & 0xFFFFu; B = cnt >> 16;
			// A list that overflowed while it was built (build_neibs_kernel: nf >= neibboundpos, nf + nb >= neibboundpos, with
			// SA_BOUNDARY nv >= neiblistsize - neibboundpos - 1) keeps COUNTING its entries but stops writing them: its counts
			// name slots of the other section, or slots that were never written.  Such a tiling goes to the generic kernel
			const bool unwritten = F >= p.neibboundpos || (saVertex ? B >= p.neiblistsize - p.neibboundpos - 1u : F + B >= p.neibboundpos);
			if (F > 128u || B > 128u || unwritten) { overflow = true; F = 0; B = 0; }
		}
		uint32_t rankInWave = 0;
		{
			unsigned long long rem = __builtin_amdgcn_ballot_w64(inHome);
			while (rem) {
				const int lead = __builtin_ctzll(rem);
				const uint32_t v = (uint32_t)__builtin_amdgcn_readlane((int)F, lead);
				const unsigned long long m = __builtin_amdgcn_ballot_w64(inHome && F == v);
				if (inHome && F == v) rankInWave = (uint32_t)__builtin_popcountll(m & ((1ull << lane) - 1ull));
				if ((int)lane == lead) sHist[wave][v] = (uint16_t)__builtin_popcountll(m);
				rem &= ~m;
			}
		}
		__syncthreads();
		uint32_t binTot = 0, binSuffix = 0;      // threads 0..128: particles of this length; ... of this length and the longer ones of my wave's 64 lengths
		if (tid < 192u) {      // per length: particles in the waves before each wave, and in all
			if (tid < 129u)
				for (uint32_t w = 0; w < TILE_CHUNKS; ++w) { const uint32_t c = sHist[w][tid]; sHist[w][tid] = (uint16_t)binTot; binTot += c; }
			// longest first: a length starts behind all longer ones -- a suffix scan over the 129 lengths in three waves (a loop
			// over the longer lengths per thread was 128 dependent LDS reads for length 0: ~3 us of the ~8 a tile takes before
			// its lists are translated)
			binSuffix = binTot;
#pragma unroll
			for (int dd = 1; dd < 64; dd <<= 1) {
				const uint32_t t2 = (uint32_t)__shfl_down((int)binSuffix, dd);
				if (lane + (uint32_t)dd < 64u) binSuffix += t2;
			}
			if (lane == 0) sBinWave[wave] = binSuffix;
		}
		__syncthreads();
		if (tid < 129u) {
			uint32_t behind = 0;
			for (uint32_t w2 = wave + 1u; w2 < 3u; ++w2) behind += sBinWave[w2];
			sBinStart[tid] = (uint16_t)(binSuffix - binTot + behind);
		}
		__syncthreads();
		if (inHome) {
			const uint32_t pos = (uint32_t)sBinStart[F] + sHist[wave][F] + rankInWave;
			sLaneOf[tid] = (uint16_t)pos; sLenF[pos] = (uint16_t)F; sLenB[pos] = (uint16_t)B;
		}
		__syncthreads();
		// for a moment thread L is LANE L of the tile (lane L & 63 of chunk L >> 6 = this thread's wave)
		const uint32_t L = tid;
		const uint32_t myF = L < P ? sLenF[L] : 0u, myB = L < P ? sLenB[L] : 0u;
		{	// the chunk's sections are padded to its longest list, in whole batches
			uint32_t mxF = myF, mxB = myB;
#pragma unroll
			for (int dd = 32; dd > 0; dd >>= 1) {
				mxF = max(mxF, (uint32_t)__shfl_xor(mxF, dd)); mxB = max(mxB, (uint32_t)__shfl_xor(mxB, dd));
			}
			if (lane == 0) { sChunkF[wave] = (mxF + TILE_NB - 1u)/TILE_NB; sChunkB[wave] = (mxB + TILE_NB - 1u)/TILE_NB; }
		}
		__syncthreads();
		// ---- 3. + 4. the schedule, by the first wave.  Lane c < 10 stands for chunk c, lane 16 + w for wave w.  The batches of
		// the tile are numbered 0..T-1 (chunk after chunk); wave w walks [w share, (w+1) share).  A run starts wherever a chunk
		// or a wave's share starts: the run boundaries are the set S of those numbers, a run's number is its rank in S.
		if (wave == 0) {
			uint32_t nF = 0, nB = 0;
			if (lane < C) { nF = sChunkF[lane]; nB = sChunkB[lane]; }
			uint32_t incl = nF + nB;            // inclusive scan over the chunk lanes -> first batch of every chunk
#pragma unroll
			for (int dd = 1; dd < 16; dd <<= 1) {
				const uint32_t t = __shfl_up(incl, dd, 16);
				if ((lane & 15u) >= (uint32_t)dd) incl += t;
			}
			const uint32_t T = (uint32_t)__builtin_amdgcn_readlane((int)incl, 15);
			// wave w walks the batches [T c(w), T c(w+1)) / 256, c = the running sum of the waves' weights (tile_share_start)
			const uint32_t share = (T*max(shareLo, 64u - shareLo) + 255u) >> 8;
			const uint32_t cStart = incl - (nF + nB), cEnd = incl;
			const bool isChunk = lane < C && nF + nB > 0u;
			const bool isWave = lane >= 16u && lane < 16u + TILE_WAVES;
			const uint32_t wv = lane - 16u;
			// even shares: T/8 batches each, the T % 8 left over go one each to the first waves, i.e. to different SIMDs
			const uint32_t sbase = T/TILE_WAVES, srem = T - sbase*TILE_WAVES;
			const bool even = shareLo == 32u;
			const uint32_t ws = !isWave ? 0u : even ? wv*sbase + min(wv, srem) : (T*tile_share_start(wv, shareLo) + 128u) >> 8;
			const uint32_t we = !isWave ? 0u : even ? ws + sbase + (wv < srem ? 1u : 0u) : (T*tile_share_start(wv + 1u, shareLo) + 128u) >> 8;
			// my boundary point (chunk lanes: the chunk's first batch; wave lanes: the share's first batch) and the range I ask about
			const uint32_t lo = isChunk ? cStart : ws, hi = isChunk ? cEnd : we;
			// a wave's start that is also a chunk's start is one boundary, the chunk's
			bool dup = false;
			uint32_t cntLt = 0, cntIn = 0, cstar = 0;
			// chunk lanes first: which wave starts coincide with a chunk start
			for (int q = 0; q < (int)TILE_CHUNKS; ++q) {
				const bool qv = (__builtin_amdgcn_ballot_w64(isChunk) >> q) & 1ull;
				if (!qv) continue;
				const uint32_t x = (uint32_t)__builtin_amdgcn_readlane((int)cStart, q);
				if (isWave && x == ws) dup = true;
				if (x <= lo) cstar = (uint32_t)q;                    // the chunk my boundary point lies in (the last one starting at or before it)
				cntLt += (x < lo) ? 1u : 0u; cntIn += (x >= lo && x < hi) ? 1u : 0u;
			}
			const bool inS = isChunk || (isWave && ws < we && !dup);
			for (int q = 16; q < 16 + (int)TILE_WAVES; ++q) {
				const bool qv = (__builtin_amdgcn_ballot_w64(inS) >> q) & 1ull;
				if (!qv) continue;
				const uint32_t x = (uint32_t)__builtin_amdgcn_readlane((int)ws, q);
				cntLt += (x < lo) ? 1u : 0u; cntIn += (x >= lo && x < hi) ? 1u : 0u;
			}
			const uint32_t R = (uint32_t)__builtin_popcountll(__builtin_amdgcn_ballot_w64(inS));   // runs of the tile
			if (inS) sSorted[cntLt] = lo;         // cntLt = my rank in S
			if (lane < TILE_RUNTAB) sRunTab[lane] = 0u;
			// (one wave: its LDS operations execute in order; the fences only keep the compiler from moving them)
			__builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront", "local");
			__builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront", "local");
			const uint32_t chunkSel = isChunk ? lane : cstar;
			const uint32_t chStart = __shfl(cStart, (int)chunkSel), chF = __shfl(nF, (int)chunkSel), chEnd = __shfl(cEnd, (int)chunkSel);
			if (inS) {         // my run: from my boundary point to the next one
				const uint32_t r = cntLt;
				const uint32_t end = (r + 1u < R) ? sSorted[r + 1u] : T;
				const uint32_t a0 = lo - chStart, len = end - lo;
				const uint32_t runF = (a0 < chF) ? min(chF - a0, len) : 0u;
				sRunTab[TILE_RT_RUN + min(r, (uint32_t)(TILE_RUNS_MAX - 1))] = tile_rt_pack_run(chunkSel, runF, len - runF, end == chEnd);
			}
			// wave (lane - 16): first run (the one starting at its first batch: that batch is a boundary), the runs that start
			// inside its share, first batch, batches
			if (isWave) sRunTab[lane - 16u] = (ws < we) ? TILE_RT_PACK_WAVE(cntLt, cntIn, ws, we - ws) : 0u;
			if (lane < TILE_CHUNKS) {
				sRunTab[TILE_RT_CHUNK + lane] = isChunk ? tile_rt_pack_chunk(cntLt, cntIn) : 0u;
				sChunkStart[lane] = cStart;
			}
			if (lane == 0) {
				sRunTab[TILE_RT_TILE] = tile_rt_pack_tile(C, P, R);
				// ---- 4. room in the list stream and in the lane tables
				const uint32_t lb = atomicAdd(tileCtl + 12, T), nb2 = atomicAdd(tileCtl + 13, C*64u);
				const bool ovf = (uint64_t)lb + T > listCapBatches || (uint64_t)nb2 + C*64u > laneCap || R > TILE_RUNS_MAX || T >= TILE_RT_FIRSTBATCH_END || share >= TILE_RT_BATCHES_END;
				sBase[0] = lb; sBase[1] = nb2; sBase[2] = ovf ? 1u : 0u;
			}
		}
		__syncthreads();
		if (sBase[2]) overflow = true;
		const uint32_t listBase = sBase[0], laneBase = sBase[1];
		if (!sBase[2]) {
			if (tid == 0) { tiles[(size_t)TILE_DESC*tile + TILE_D_LISTBASE] = listBase; tiles[(size_t)TILE_DESC*tile + TILE_D_LANEBASE] = laneBase; }
			if (tid < TILE_RUNTAB) tileRuns[(size_t)TILE_RUNTAB*tile + tid] = sRunTab[tid];
		}
		// ---- 5. the lane tables and the translated lists.  Back in home order: thread t stands for home particle t (consecutive
		// threads read consecutive columns of the neighbour list: whole lines; in lane order a wave gathered two-byte entries
		// from all over the tile) and, from P on, for the idle lanes of the last chunk.  The eight-byte stores go to the lane's
		// place in its chunk's batches (scattered, but a quarter as many as the loads)
		const bool isHome = tid < P, isLane = tid < C*64u;
		const uint32_t myLane = isHome ? (uint32_t)sLaneOf[tid] : tid;
		const uint32_t ch = min(myLane >> 6, (uint32_t)(TILE_CHUNKS - 1)), ln = myLane & 63u;
		const TileHome h = tile_home(d, isHome ? tid : 0u);
		const uint32_t index = h.index;
		const int3 gp = grid_pos_from_hash(p, preHash & CELLTYPE_BITMASK);
		const int myG1 = (p.c1 == 0) ? gp.x : (p.c1 == 1) ? gp.y : gp.z;
		const int myCol = min(max(myG1 - ca, 0), TILE_MAXCELLS - 1);
		const uint16_t *myCB = sCB + (h.hrow*TILE_MAXCELLS + myCol)*27;
		if (!sBase[2]) {
			if (isLane) {
				uint32_t rec = 0u, idx = 0xFFFFFFFFu;
				if (isHome) {   // the particle's own row in the window (the forces kernel reads its position, velocity and EOS row there)
					const int wc = (5 + (h.hrow & 1) + 4*(h.hrow >> 1))*TILE_KW + myCol + 1;
					const uint32_t slot = 1u + sCellBase[wc] + (index - sCellStart[wc]);
					if (slot > TILE_SLOT_MAX) overflow = true;
					const particleinfo pi = preInfo;
					const uint32_t flags = PART_TYPE(pi) | (HAS_COMPUTE_FORCE(pi) ? LANE_COMPUTE_FORCE : 0u) | ((FLUID_NUM(pi) & 3u) << LANE_FLUID_SHIFT) | LANE_VALID;
					rec = lane_rec_pack(slot, flags);
					idx = index;
				}
				laneRec[laneBase + myLane] = rec; laneIndex[laneBase + myLane] = idx;
			}
			const uint32_t chunkStart = sChunkStart[ch], chF = sChunkF[ch], chB = sChunkB[ch];
#pragma unroll 1
			for (int sec = 0; sec < 2; ++sec) {
				// section 0: slots 0 upward, section 1: slots neibboundpos downward (SA_BOUNDARY: the vertex section, slots
				// neibboundpos + 1 upward; the boundary elements are not particles of a window).  Every lane of a chunk writes all
				// the chunk's batches of the section, padded with the dummy row's offset
				const uint32_t nbat = isLane ? (sec ? chB : chF) : 0u;
				const uint32_t cnt = isHome ? (sec ? B : F) : 0u;
				uint2 *out = tileList + ((size_t)listBase + chunkStart + (sec ? chF : 0u))*64u + ln;
				uint32_t nbatWave = nbat;      // the wave walks to the longest of its lanes' chunks
#pragma unroll
				for (int dd = 32; dd > 0; dd >>= 1) nbatWave = max(nbatWave, (uint32_t)__shfl_xor(nbatWave, dd));
				uint32_t code = 0;
				// entry sl of the section: slot sl, or neibboundpos - sl, or neibboundpos + 1 + sl -- a base and a signed step, both
				// the same for every lane; the lane's part of the address is its particle's index alone, ONE 32-bit offset for all
				// the loads of the loop (with an address pair per load the compiler recycled the pairs as load destinations and
				// waited for the loads in flight before each re-use)
				const neibdata *const secList = list + (size_t)(!sec ? 0u : saVertex ? p.neibboundpos + 1u : p.neibboundpos)*stride;
				const long long secStep = (sec && !saVertex) ? -(long long)stride : (long long)stride;
				const uint32_t secCap = !sec ? p.neiblistsize : saVertex ? p.neiblistsize - p.neibboundpos - 1u : p.neibboundpos + 1u;
				constexpr int LOADS = TL_LOADS;   // entries per lane in flight: the walk is latency bound
#pragma unroll 1
				for (uint32_t b0 = 0; b0 < nbatWave; b0 += LOADS/TILE_NB) {
					uint32_t e[LOADS];
#pragma unroll
					for (int k = 0; k < LOADS; ++k) {
						const uint32_t sl = min(b0*TILE_NB + (uint32_t)k, secCap - 1u);   // the same slot for every lane; past a lane's list the entry is not used
						// (unconditional: the address is valid for every thread, and a load under a branch of its own made the compiler
						// wait for all the earlier ones before it in some builds -- 7 to 13 ms per launch depending on unrelated edits)
						e[k] = (uint32_t)(secList + (long long)sl*secStep)[index];
					}
					uint32_t val[LOADS];
#pragma unroll
					for (int k = 0; k < LOADS; ++k) {
						const uint32_t dd = e[k];
						const bool live = b0*TILE_NB + (uint32_t)k < cnt;
						// (the list is build_neibs_kernel's own, written moments ago, and its section lengths were checked against the
						// list's geometry above: the entries are not validated one by one -- that was a third of this loop's
						// instructions -- only that the section opened with a cell code, below)
						code = (live && dd >= CELLNUM_ENCODED) ? (dd >> CELLNUM_SHIFT) : code;
						const uint32_t slot = 1u + (uint32_t)myCB[min(code, 27u)] + (dd & NEIBINDEX_MASK);   // slot 0 = dummy
						if (live && slot > TILE_SLOT_MAX) overflow = true;
						val[k] = live ? tile_slot_offset(slot) : 0u;
					}
#pragma unroll
					for (int k = 0; k < LOADS/TILE_NB; ++k)
						if (b0 + (uint32_t)k < nbat)
							out[(size_t)(b0 + (uint32_t)k)*64u] = make_uint2(list_pack_half(val[4*k], val[4*k + 1]), list_pack_half(val[4*k + 2], val[4*k + 3]));
				}
				if (cnt && code == 0u) overflow = true;      // a section that never named a cell: not a list of the builder
			}
		}
		if (overflow) tileCtl[1] = 1u;      // generic kernel
	}
}

int sphx_tile_lists_launch(sphx_ctx *ctx, const uint16_t *neibsList, const void *info, const uint32_t *hash, const uint32_t *cellStart, bool sa, hipStream_t st)
{
	if (!ctx->tile_list || !ctx->tile_runs || !ctx->tile_rows || !ctx->tile_lane_rec || !ctx->tile_lane_index || !ctx->neib_counts) {
		sphx_tiles_invalidate(ctx);
		return SPHX_OK;
	}
	const uint32_t grid = ctx->tile_grid*TL_GRIDMUL < ctx->tile_capacity ? ctx->tile_grid*TL_GRIDMUL : ctx->tile_capacity;
	// the plain forces pass is the only walker of these lists that gains from uneven shares (tile_share_start)
	const bool plain = !sa && ctx->dev.turbmodel == SPHX_ARTIFICIAL && ctx->dev.numfluids == 1 && ctx->dev.boundarytype == SPHX_DYN_BOUNDARY;
	tile_lists_kernel<<<grid, TL_THREADS, 0, st>>>(ctx->dev, neibsList, ctx->neib_counts, (const particleinfo*)info, hash, cellStart, ctx->cell_end_copy,
		ctx->tiles, ctx->tile_ctl, ctx->tile_rows, ctx->tile_runs, ctx->tile_list, ctx->tile_list_batches, ctx->tile_lane_rec, ctx->tile_lane_index,
		ctx->tile_lane_cap, sa ? 1 : 0, plain ? TILE_SHARE_LO_PLAIN : 32u);
	SPHX_LAUNCH_CHECK("tile_lists_kernel");
	return SPHX_OK;
}

// the tables of the tiling, for a launch of the tiled kernel
static void set_tile_tables(ForcesArgs &a, const sphx_ctx *ctx)
{
	a.tileList = ctx->tile_list; a.tileRuns = ctx->tile_runs; a.tileRows = ctx->tile_rows;
	a.tileLaneRec = ctx->tile_lane_rec; a.tileLaneIndex = ctx->tile_lane_index;
}

// the launchers of each SPH kernel type's translation unit: forces_parts[kerneltype - 1] (set_constants admits 1..4 only)
static const struct ForcesPart {
	decltype(&sphx_part_forces_k1) forces; decltype(&sphx_part_stress_k1) stress; decltype(&sphx_part_sps_k1) sps;      // SPHX_PART_DECL
} forces_parts[4] = {
#define SPHX_PART(K) { sphx_part_forces_k##K, sphx_part_stress_k##K, sphx_part_sps_k##K }
	SPHX_PART(1), SPHX_PART(2), SPHX_PART(3), SPHX_PART(4)
#undef SPHX_PART
};

extern "C" int sphx_forces_basicstep(sphx_ctx *ctx,
	void *forces, float *cfl, void *rbforces, void *rbtorques,
	const void *pos, const void *vel, const void *info, const uint32_t *hash,
	const uint32_t *cellStart, const uint16_t *neibsList,
	const void *tau0, const void *tau1, const void *tau2, void *xsph,
	uint32_t numParticles, uint32_t fromParticle, uint32_t toParticle,
	float deltap, float slength, float dtadaptfactor, float influenceradius,
	uint32_t cflOffset, int run_mode, int step, float dt, int compute_object_forces,
	uint32_t *h_numBlocks, void *stream)
{
	(void)dtadaptfactor; (void)step; (void)dt;
	SPHX_REQUIRE(ctx && ctx->have_params, "sphx_forces_basicstep: constants not set");
	SPHX_REQUIRE(forces && pos && vel && info && hash && cellStart && neibsList, "sphx_forces_basicstep: missing buffer");
	SPHX_REQUIRE(fromParticle <= toParticle && toParticle <= numParticles, "sphx_forces_basicstep: invalid particle range");
	SPHX_REQUIRE(slength == ctx->params.slength && influenceradius == ctx->params.influenceradius,
		"sphx_forces_basicstep: slength/influenceradius differ from set_constants");
	if (run_mode != SPHX_SIMULATE && run_mode != SPHX_REPACK)
		return sphx_set_error(SPHX_ERR_INVALID, "sphx_forces_basicstep: invalid run mode");
	if (ctx->dev.boundarytype != SPHX_DYN_BOUNDARY && ctx->dev.boundarytype != SPHX_LJ_BOUNDARY)
		return sphx_set_error(SPHX_ERR_UNSUPPORTED, "sphx_forces_basicstep: only DYN_BOUNDARY and LJ_BOUNDARY pair interactions are built");
	if (ctx->params.rheologytype > SPHX_NEWTONIAN && run_mode == SPHX_SIMULATE)
		return sphx_set_error(SPHX_ERR_INVALID, "sphx_forces_basicstep: generalized Newtonian rheologies read BUFFER_EFFVISC, use sphx_forces_basicstep_effvisc");
	if ((ctx->params.sph_formulation == SPHX_SPH_HA || (ctx->params.rheologytype == SPHX_NEWTONIAN && ctx->params.viscmodel != SPHX_MORRIS)) &&
		run_mode == SPHX_SIMULATE) {      // Hu & Adams, MONAGHAN / ESPANOL_REVENGA viscous models: rheology.hip
		if (compute_object_forces || rbforces)
			return sphx_set_error(SPHX_ERR_UNSUPPORTED, "sphx_forces_basicstep: SPH_HA / MONAGHAN / ESPANOL_REVENGA with bodies that feel the fluid are not built");
		return sphx_fidelity_forces_launch(ctx, forces, cfl, pos, vel, info, hash, cellStart, neibsList, nullptr, numParticles, fromParticle,
			toParticle, slength, influenceradius, cflOffset, h_numBlocks, stream);
	}
	if (ctx->params.sph_formulation == SPHX_SPH_GRENIER && run_mode == SPHX_SIMULATE)
		return sphx_set_error(SPHX_ERR_INVALID, "sphx_forces_basicstep: SPH_GRENIER reads BUFFER_SIGMA, use sphx_forces_basicstep_grenier");
	if (ctx->dev.turbmodel == SPHX_SPS && run_mode == SPHX_SIMULATE)
		SPHX_REQUIRE(tau0 && tau1 && tau2, "sphx_forces_basicstep: SPS needs the three TAU arrays");
	if ((ctx->dev.simflags & SPHX_ENABLE_DTADAPT))
		SPHX_REQUIRE(cfl != nullptr, "sphx_forces_basicstep: ENABLE_DTADAPT needs the CFL buffer");
	SPHX_REQUIRE((rbforces == nullptr) == (rbtorques == nullptr), "sphx_forces_basicstep: RB_FORCES and RB_TORQUES must come together");
	if ((ctx->dev.simflags & SPHX_ENABLE_XSPH) && run_mode == SPHX_SIMULATE)
		SPHX_REQUIRE(xsph != nullptr, "sphx_forces_basicstep: ENABLE_XSPH needs the XSPH buffer");

	const uint32_t nrange = toParticle - fromParticle;
	const uint32_t numBlocks = round_up_u(div_up_u(nrange, SPHX_BLOCK_FORCES), 4u);
	if (h_numBlocks) *h_numBlocks = numBlocks;
	if (!numBlocks) return SPHX_OK;
	{ const int rcf = sphx_rb_flush(ctx, (hipStream_t)stream); if (rcf != SPHX_OK) return rcf; }
	if (run_mode == SPHX_REPACK)   // run_repack, src/cuda/forces.cu:828-896 (filters.hip)
		return sphx_repack_launch(ctx, forces, cfl, rbforces, rbtorques, pos, vel, info, hash, cellStart, neibsList,
			fromParticle, toParticle, cflOffset, numBlocks, deltap, (hipStream_t)stream);

	{	// EOS pre-pass over ALL particles: neighbours may lie outside [fromParticle,toParticle)
		int rc0 = sphx_ensure_scratch(ctx, numParticles);
		if (rc0 != SPHX_OK) return rc0;
		// ... unless the Euler step that wrote these densities left the rows behind and the caller vouches for the buffer
		// (sphx_eos_rows_current, euler.hip)
		const bool current = ctx->eos_armed && ctx->eos_tag_vel == vel && ctx->eos_tag_n == numParticles;
		ctx->eos_armed = false;
		if (!current) {
			// the rows are this buffer's from here on (a second stripe of the same pass may be vouched for as well)
			ctx->eos_tag_vel = ctx->eos_follow ? vel : nullptr;
			ctx->eos_tag_n = numParticles;
			eos_kernel<<<div_up_u(numParticles, 256), 256, 0, (hipStream_t)stream>>>(ctx->dev, (const float4*)vel,
				(const particleinfo*)info, ctx->eos_aux, numParticles);
			SPHX_LAUNCH_CHECK("eos_kernel");
		}
	}
	ForcesArgs a;
	a.forces = (float4*)forces; a.cfl = (ctx->dev.simflags & SPHX_ENABLE_DTADAPT) ? cfl : nullptr;
	a.rbforces = (float4*)rbforces; a.rbtorques = (float4*)rbtorques;
	a.pos = (const float4*)pos; a.vel = (const float4*)vel; a.info = (const particleinfo*)info;
	a.hash = hash; a.cellStart = cellStart; a.neibsList = neibsList;
	a.tau0 = (const float2*)tau0; a.tau1 = (const float2*)tau1; a.tau2 = (const float2*)tau2;
	a.rb = ctx->rb_dev;
	a.aux = ctx->eos_aux;
	set_tile_tables(a, ctx);
	a.xsph = (float4*)xsph;
	a.fromParticle = fromParticle; a.toParticle = toParticle; a.cflOffset = cflOffset;
	a.wholeRange = (fromParticle == 0u && toParticle == numParticles) ? 1 : 0;
	a.numBlocks = numBlocks;
	a.compute_object_forces = compute_object_forces;
	a.pin = nullptr;
#ifdef SPHX_TILE_DEBUG_BUILD
	a.prof = nullptr;
	if (ctx->tile_debug & 16) {
		if (!ctx->tile_prof && hipMalloc((void**)&ctx->tile_prof, 10*(TILE_THREADS/64)*sizeof(unsigned long long)*ctx->tile_grid) != hipSuccess)
			return sphx_set_error(SPHX_ERR_RUNTIME, "sphx_forces_basicstep: cannot allocate the tile profile buffer");
		a.prof = ctx->tile_prof;
	}
#endif

	const bool use_tiles = sphx_tiles_current(ctx, cellStart, neibsList) && sphx_tiles_opts_forces(ctx->dev);
	a.tauPack = nullptr; a.tauPackN = 0;
	a.otau0 = a.otau1 = a.otau2 = nullptr; a.oturbvisc = nullptr;
	if (use_tiles && ctx->dev.turbmodel == SPHX_SPS) {   // window rows of the stress tensor (see tau_pack_kernel)
		SPHX_REQUIRE(ctx->tau_pack != nullptr && numParticles <= ctx->reserved_particles, "sphx_forces_basicstep: SPS scratch not reserved");
		tau_pack_kernel<<<div_up_u(numParticles, 256), 256, 0, (hipStream_t)stream>>>((const float2*)tau0, (const float2*)tau1,
			(const float2*)tau2, ctx->eos_aux, ctx->dev.densitydiff == SPHX_COLAGROSSI ? 1 : 0, ctx->tau_pack, numParticles);
		SPHX_LAUNCH_CHECK("tau_pack_kernel");
		a.tauPack = ctx->tau_pack; a.tauPackN = numParticles;
	}
	if (ctx->dev.kerneltype < SPHX_CUBICSPLINE || ctx->dev.kerneltype > SPHX_GAUSSIAN)
		return sphx_set_error(SPHX_ERR_INVALID, "sphx_forces_basicstep: invalid kernel type");
	const int rc = forces_parts[ctx->dev.kerneltype - 1].forces(ctx, dim3(numBlocks), (hipStream_t)stream, a, use_tiles);
	if (rc != SPHX_OK) return rc;
	SPHX_LAUNCH_CHECK("forces_kernel");
	if (ctx->dev.simflags & SPHX_ENABLE_XSPH)   // mean neighbourhood velocity of the fluid particles (filters.hip)
		return sphx_xsph_launch(ctx, xsph, pos, vel, info, hash, cellStart, neibsList, fromParticle, toParticle, (hipStream_t)stream);
	return SPHX_OK;
}

// displacement of every particle over the step (cell-local positions of the same cell: the hash only changes at the next sort)
static __global__ void __launch_bounds__(256)
sa_displacement_kernel(const float4 *__restrict__ oldPos, const float4 *__restrict__ newPos, float4 *__restrict__ disp, uint32_t n)
{
	const uint32_t i = blockIdx.x*256 + threadIdx.x;
	if (i >= n) return;
	const float4 a = oldPos[i], b = newPos[i];
	disp[i] = make_float4(b.x - a.x, b.y - a.y, b.z - a.z, 0.0f);
}

// The particle <- particle sums of an SA_BOUNDARY engine over the tiles of the current neighbour list (see SPHX_TURB_SA).
// *used = the tiled kernel was launched: the caller's list-walker kernel then only finishes the particles (boundary elements,
// division by gamma, ...) unless the device-side overflow flag *guard says the tiles could not be used after all.
int sphx_sa_tiles_run(sphx_ctx *ctx, int mode, void *forces, const void *pos, const void *vel, const void *newPos,
	const void *info, const uint32_t *hash, const uint32_t *cellStart, const uint16_t *neibsList, const void *gGam,
	uint32_t numParticles, uint32_t fromParticle, uint32_t toParticle, float dt, hipStream_t stream,
	bool *used, const uint32_t **guard)
{
	*used = false; *guard = nullptr;
	const DevParams &d = ctx->dev;
	if (!sphx_tiles_current(ctx, cellStart, neibsList) || !sphx_tiles_opts_sa(d, mode) || numParticles > ctx->reserved_particles ||
		fromParticle >= toParticle) return SPHX_OK;
	ForcesArgs a = {};
	a.forces = (float4*)forces;
	a.pos = (const float4*)pos; a.vel = (const float4*)vel; a.info = (const particleinfo*)info;
	a.hash = hash; a.cellStart = cellStart; a.neibsList = neibsList;
	a.aux = ctx->eos_aux;
	ctx->eos_tag_vel = nullptr;      // the scratch rows change hands
	if (mode == SPHX_SA_TILE_DSUM) {      // the window's second array holds the displacements
		sa_displacement_kernel<<<div_up_u(numParticles, 256), 256, 0, stream>>>((const float4*)pos, (const float4*)newPos, ctx->eos_aux, numParticles);
		SPHX_LAUNCH_CHECK("sa_displacement_kernel");
		a.vel = ctx->eos_aux;
	} else {
		eos_kernel<<<div_up_u(numParticles, 256), 256, 0, stream>>>(ctx->dev, (const float4*)vel, (const particleinfo*)info, ctx->eos_aux, numParticles);
		SPHX_LAUNCH_CHECK("eos_kernel");
	}
	set_tile_tables(a, ctx);
	a.saGam = (const float4*)gGam; a.saDt = dt;
	a.rb = ctx->rb_dev;
	a.fromParticle = fromParticle; a.toParticle = toParticle;
	a.wholeRange = (fromParticle == 0u && toParticle == numParticles) ? 1 : 0;
	sphx_part_sa_tile(ctx, stream, a, mode, d.rheology == SPHX_NEWTONIAN);
	SPHX_LAUNCH_CHECK("forces_tile_kernel (SA_BOUNDARY)");
	*used = true;
	*guard = sphx_tiles_standby_guard(ctx);
	return SPHX_OK;
}

extern "C" int sphx_forces_reserve_cus(sphx_ctx *ctx, uint32_t cus)
{
	SPHX_REQUIRE(ctx != nullptr, "sphx_forces_reserve_cus: NULL ctx");
	int total = 0;
	SPHX_HIP(hipDeviceGetAttribute(&total, hipDeviceAttributeMultiprocessorCount, ctx->device));
	const uint32_t all = (uint32_t)(total > 0 ? total : 256);
	const uint32_t k = (cus + 7u)/8u*8u;
	SPHX_REQUIRE(k < all, "sphx_forces_reserve_cus: more CUs reserved than the device has");
	ctx->tile_grid = (all - k)*TILE_WGS_PER_CU;
	return SPHX_OK;
}

static int dtreduce_launch(sphx_ctx *ctx, float slength, float dtadaptfactor, float sspeed_cfl,
	float max_kinematic, const float *cfl, float *cflTemp, uint32_t numBlocks,
	float *d_dt, int combine_min, hipStream_t stream)
{
	SPHX_REQUIRE(ctx && ctx->have_params, "sphx_forces_dtreduce: constants not set");
	SPHX_REQUIRE(cfl && cflTemp && d_dt, "sphx_forces_dtreduce: missing buffer (CFL, CFL_TEMP)");
	SPHX_REQUIRE((numBlocks & 3u) == 0 && numBlocks > 0, "sphx_forces_dtreduce: number of elements to reduce is not a multiple of 4");
	const uint32_t nPartials = sphx_forces_fmax_temp_elements(numBlocks);
	fmax_kernel<<<nPartials, BLOCK_FMAX, 0, stream>>>(cflTemp, (const float4*)cfl, numBlocks/4);
	const int viscous = (ctx->dev.rheology != SPHX_INVISCID || ctx->dev.turbmodel > SPHX_ARTIFICIAL) ? 1 : 0;
	dt_final_kernel<<<1, BLOCK_FMAX, 0, stream>>>(d_dt, cflTemp, nPartials, slength, dtadaptfactor, sspeed_cfl,
		max_kinematic, viscous, combine_min);
	SPHX_LAUNCH_CHECK("fmax_kernel/dt_final_kernel");
	return SPHX_OK;
}

extern "C" int sphx_forces_dtreduce_device(sphx_ctx *ctx, float slength, float dtadaptfactor, float sspeed_cfl,
	float max_kinematic, const float *cfl, float *cflTemp, uint32_t numBlocks,
	float *d_dt, int combine_min, void *stream)
{
	return dtreduce_launch(ctx, slength, dtadaptfactor, sspeed_cfl, max_kinematic, cfl, cflTemp, numBlocks,
		d_dt, combine_min, (hipStream_t)stream);
}

extern "C" int sphx_forces_dtreduce(sphx_ctx *ctx, float slength, float dtadaptfactor, float sspeed_cfl,
	float max_kinematic, const float *cfl, float *cflTemp, uint32_t numBlocks,
	float *h_dt, void *stream)
{
	SPHX_REQUIRE(h_dt != nullptr, "sphx_forces_dtreduce: h_dt is NULL");
	int rc = dtreduce_launch(ctx, slength, dtadaptfactor, sspeed_cfl, max_kinematic, cfl, cflTemp, numBlocks,
		ctx ? ctx->dt_scratch : nullptr, 0, (hipStream_t)stream);
	if (rc != SPHX_OK) return rc;
	SPHX_HIP(hipMemcpyAsync(h_dt, ctx->dt_scratch, sizeof(float), hipMemcpyDeviceToHost, (hipStream_t)stream));
	SPHX_HIP(hipStreamSynchronize((hipStream_t)stream));
	return SPHX_OK;
}

extern "C" int sphx_reduce_rb_forces(sphx_ctx *ctx, void *rbforces, void *rbtorques, const uint32_t *rbnum,
	const uint32_t *h_lastindex, float *h_totalforce3, float *h_totaltorque3,
	uint32_t numforcesbodies, uint32_t numForcesBodiesParticles, void *stream_)
{
	SPHX_REQUIRE(ctx && rbforces && rbtorques && rbnum && h_lastindex && h_totalforce3 && h_totaltorque3,
		"sphx_reduce_rb_forces: NULL argument");
	SPHX_REQUIRE(numforcesbodies <= SPHX_MAX_BODIES, "sphx_reduce_rb_forces: too many bodies");
	if (!numforcesbodies) return SPHX_OK;
	hipStream_t stream = (hipStream_t)stream_;
	uint32_t *d_last = nullptr; float *d_tot = nullptr;
	SPHX_HIP(hipMalloc((void**)&d_last, sizeof(uint32_t)*numforcesbodies));
	SPHX_HIP(hipMalloc((void**)&d_tot, sizeof(float)*6*numforcesbodies));
	SPHX_HIP(hipMemcpyAsync(d_last, h_lastindex, sizeof(uint32_t)*numforcesbodies, hipMemcpyHostToDevice, stream));
	rb_reduce_kernel<<<numforcesbodies, 256, 0, stream>>>((const float4*)rbforces, (const float4*)rbtorques,
		rbnum, d_last, d_tot, numForcesBodiesParticles);
	float tot[6*SPHX_MAX_BODIES];
	SPHX_HIP(hipMemcpyAsync(tot, d_tot, sizeof(float)*6*numforcesbodies, hipMemcpyDeviceToHost, stream));
	SPHX_HIP(hipStreamSynchronize(stream));
	(void)hipFree(d_last); (void)hipFree(d_tot);
	for (uint32_t b = 0; b < numforcesbodies; ++b)
		for (int c = 0; c < 3; ++c) {
			h_totalforce3[3*b + c] = tot[6*b + c];
			h_totaltorque3[3*b + c] = tot[6*b + 3 + c];
		}
	return SPHX_OK;
}

extern "C" int sphx_calc_visc(sphx_ctx *ctx, void *tau0, void *tau1, void *tau2, float *spsturbvisc,
	const void *pos, const void *vel, const void *info, const uint32_t *hash,
	const uint32_t *cellStart, const uint16_t *neibsList,
	uint32_t numParticles, uint32_t particleRangeEnd,
	float deltap, float slength, float influenceradius, void *stream)
{
	(void)deltap; (void)numParticles;
	SPHX_REQUIRE(ctx && ctx->have_params, "sphx_calc_visc: constants not set");
	if (ctx->dev.turbmodel != SPHX_SPS)
		return sphx_set_error(SPHX_ERR_UNSUPPORTED, "sphx_calc_visc: only the SPS branch is built");
	SPHX_REQUIRE(pos && vel && info && hash && cellStart && neibsList, "sphx_calc_visc: missing buffer");
	SPHX_REQUIRE((tau0 && tau1 && tau2) || (!tau0 && !tau1 && !tau2), "sphx_calc_visc: the three TAU arrays must come together");
	SPHX_REQUIRE(slength == ctx->params.slength && influenceradius == ctx->params.influenceradius,
		"sphx_calc_visc: slength/influenceradius differ from set_constants");
	if (!particleRangeEnd) return SPHX_OK;
	SpsArgs a;
	a.tau0 = (float2*)tau0; a.tau1 = (float2*)tau1; a.tau2 = (float2*)tau2; a.turbvisc = spsturbvisc;
	a.pos = (const float4*)pos; a.vel = (const float4*)vel; a.info = (const particleinfo*)info;
	a.hash = hash; a.cellStart = cellStart; a.neibsList = neibsList; a.numParticles = particleRangeEnd;
	dim3 grid(div_up_u(particleRangeEnd, 128));
	const ForcesPart &part = forces_parts[ctx->dev.kerneltype - 1];
	// single fluid with the tiling of this neighbour list at hand: the stress mode of the tiled kernel (neighbour rows from
	// the LDS window instead of gathers), then the gather kernel as a stand-by guarded by the tiling's overflow flag
	const uint32_t *guard = nullptr;
	if (sphx_tiles_current(ctx, cellStart, neibsList) && sphx_tiles_opts_stress(ctx->dev)) {
		ForcesArgs fa = ForcesArgs();
		fa.pos = a.pos; fa.vel = a.vel; fa.info = a.info; fa.hash = hash; fa.cellStart = cellStart; fa.neibsList = neibsList;
		fa.otau0 = a.tau0; fa.otau1 = a.tau1; fa.otau2 = a.tau2; fa.oturbvisc = spsturbvisc;
		fa.fromParticle = 0; fa.toParticle = particleRangeEnd;
		set_tile_tables(fa, ctx);
		part.stress(ctx, (hipStream_t)stream, fa);
		SPHX_LAUNCH_CHECK("forces_tile_kernel (SPS stress)");
		guard = sphx_tiles_standby_guard(ctx);
		if (!guard) return SPHX_OK;
		grid.x = grid.x < 2048u ? grid.x : 2048u;   // stand-by launch: every block returns at once unless the tiling overflowed
	}
	part.sps(ctx, grid, (hipStream_t)stream, a, guard);
	SPHX_LAUNCH_CHECK("sps_kernel");
	return SPHX_OK;
}

#ifdef SPHX_TILE_DEBUG_BUILD
// timing experiments only (library built with -DSPHX_TILE_DEBUG_BUILD, SPHX_TILE_DEBUG=16): cycles per phase of every wave of
// the last tiled forces launch
extern "C" int sphx_dbg_tile_profile(sphx_ctx *ctx, unsigned long long *host, uint32_t maxGroups)
{
	if (!ctx || !ctx->tile_prof) return -1;
	const uint32_t n = maxGroups < ctx->tile_grid ? maxGroups : ctx->tile_grid;
	if (hipMemcpy(host, ctx->tile_prof, 10*(TILE_THREADS/64)*sizeof(unsigned long long)*n, hipMemcpyDeviceToHost) != hipSuccess) return -1;
	return (int)n;
}
#endif

// timing experiments only, not part of include/sphx.h: the tile descriptors of the last neighbour-list build
extern "C" int sphx_dbg_tiles(sphx_ctx *ctx, uint32_t *host, uint32_t maxTiles)
{
	if (!ctx || !ctx->tiles || !ctx->tiles_built) return -1;
	uint32_t ctl[4];
	if (hipMemcpy(ctl, ctx->tile_ctl, sizeof(ctl), hipMemcpyDeviceToHost) != hipSuccess) return -1;
	const uint32_t n = ctl[0] < maxTiles ? ctl[0] : maxTiles;
	if (hipMemcpy(host, ctx->tiles, (size_t)TILE_DESC*sizeof(uint32_t)*n, hipMemcpyDeviceToHost) != hipSuccess) return -1;
	return (int)n;
}

// diagnostics only, not part of include/sphx.h: raw copies of the tiling's tables (0 descriptors, 1 run tables, 2 lane records,
// 3 lane particles, 4 the list stream, 5 tile_ctl, 6 window rows), `bytes` from the start; synchronises
extern "C" int sphx_dbg_tile_table(sphx_ctx *ctx, int which, void *host, size_t bytes)
{
	if (!ctx || !host) return -1;
	const void *src = which == 0 ? (const void*)ctx->tiles : which == 1 ? (const void*)ctx->tile_runs : which == 2 ? (const void*)ctx->tile_lane_rec :
		which == 3 ? (const void*)ctx->tile_lane_index : which == 4 ? (const void*)ctx->tile_list : which == 5 ? (const void*)ctx->tile_ctl :
		which == 6 ? (const void*)ctx->tile_rows : nullptr;
	if (!src) return -1;
	return hipMemcpy(host, src, bytes, hipMemcpyDeviceToHost) == hipSuccess ? 0 : -1;
}

// tests only, not part of include/sphx.h: 1 when the last neighbour-list build left a usable tiling (built, lists allocated, no
// overflow), i.e. the tiled kernels are the ones that run; synchronises
extern "C" int sphx_dbg_tiles_usable(sphx_ctx *ctx)
{
	if (!ctx || !ctx->tiles || !ctx->tiles_built || !ctx->tile_list || ctx->disable_tiles) return 0;
	uint32_t ctl[2];
	if (hipMemcpy(ctl, ctx->tile_ctl, sizeof(ctl), hipMemcpyDeviceToHost) != hipSuccess) return -1;
	return (ctl[0] > 0u && ctl[1] == 0u) ? 1 : 0;
}

// tests only, not part of include/sphx.h: on != 0 keeps the plain tiled pass of this context on the instantiation for any gravity
// (plain_gravity_z), so that a test can hold the one for a gravity along z against it bit for bit; on < 0 changes nothing.
// -> 1 when a tiled plain pass of this context now takes the instantiation for a gravity along z, 0 when it does not
extern "C" int sphx_dbg_forces_general_gravity(sphx_ctx *ctx, int on)
{
	if (!ctx) return -1;
	if (on >= 0) ctx->general_gravity = on != 0;
	return plain_gravity_z(ctx) ? 1 : 0;
}

// Optional profiling hook (bench.py): when enabled, every forces pass records a pair of HIP events on its launch
// stream around its dominant kernel (forces_tile_kernel, or forces_kernel when the tiling is not used);
// sphx_forces_timing_read synchronises the recorded events, returns their summed elapsed time and count, and
// releases them.
extern "C" int sphx_forces_timing(sphx_ctx *ctx, int enable)
{
	SPHX_REQUIRE(ctx != nullptr, "sphx_forces_timing: NULL ctx");
	if (!ctx->forces_events) ctx->forces_events = new std::vector<std::pair<hipEvent_t, hipEvent_t> >();
	ctx->time_forces = enable != 0;
	return SPHX_OK;
}

extern "C" int sphx_forces_timing_read(sphx_ctx *ctx, double *total_ms, uint32_t *launches)
{
	SPHX_REQUIRE(ctx && total_ms && launches, "sphx_forces_timing_read: NULL argument");
	double sum = 0.0; uint32_t n = 0;
	if (ctx->forces_events) {
		for (auto &e : *ctx->forces_events) {
			float ms = 0.0f;
			if (hipEventSynchronize(e.second) == hipSuccess && hipEventElapsedTime(&ms, e.first, e.second) == hipSuccess) { sum += ms; ++n; }
			(void)hipEventDestroy(e.first); (void)hipEventDestroy(e.second);
		}
		ctx->forces_events->clear();
	}
	*total_ms = sum; *launches = n;
	return SPHX_OK;
}
