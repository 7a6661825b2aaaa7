// tile_ring.h -- the ring of list batches in flight of the tiled forces kernel (walk_runs, forces_tile.h), and nothing else:
// the loads the compiler sees (load_list_b, pin_batch) and the hand-managed ring in a0..a15 ("AccRing").
// Contract with scripts/check_ring_isa.py, which the Makefile runs on every object that holds the ring: every statement that
// names an accumulation register is an asm volatile of this file, carries the mark "; ACCRING" on each of its instructions and
// lists SPHX_ACC_CLOBBERS; the statement that reads a15 (acc_fetch_ahead) is what ends a tile's use of the ring.
#ifndef SPHX_TILE_RING_H
#define SPHX_TILE_RING_H

#include "sphx_internal.h"

// list entries of one section, TILE_AHEAD batches deep: buffer q[j] holds batch j (mod TILE_AHEAD)
struct ListWindow { uint2 q[TILE_AHEAD]; };   // a batch = 4 uint16 entries in 8 bytes

struct ListStream { const uint2 *list; uint32_t *pin; };

typedef uint32_t list_u32x2 __attribute__((ext_vector_type(2)));
// A buffer load the compiler sees.  It then also decides where to wait for it, and in the four-buffer ring of walk_runs it
// decides badly: it rotates the buffers with register copies at the loop latch and has to drain the whole ring
// (s_waitcnt vmcnt(0)) in front of the copies -- once every four batches the walk waits out the latency of its youngest load,
// which was issued one batch before (the state of rounds 1-3: the ISA shows it, the source did not).  Kept for the
// instantiations that spill (AccRing below explains why) and for the requests made one tile ahead.
__device__ __forceinline__ void load_list_b(const ListStream &ls, uint32_t firstBatch /* of this wave, absolute */,
	int batch /* relative */, int lastBatch, uint32_t lane8, uint2 &nd)
{
	// batches past the end are never computed (the walk stops there); the clamp only keeps the prefetch inside the tile's
	// stream.  No branch around the load: one load per step, whatever happens.
	const int b = min(__builtin_amdgcn_readfirstlane(batch), lastBatch);
	const char *base = reinterpret_cast<const char*>(ls.list + ((size_t)__builtin_amdgcn_readfirstlane(firstBatch) + (uint32_t)b)*64u);
	const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<char*>(base), 0, 0xFFFFFFFF, 0x00020000);
	const list_u32x2 d = __builtin_amdgcn_raw_buffer_load_b64(rsrc, (int)lane8, 0, 0);
	nd = make_uint2(d.x, d.y);
}

// The hand-managed ring: the list batches in flight live in ACCUMULATION registers, which the compiler does not use in a kernel
// that spills nothing (gfx950 gives a wave 512 registers, 256 of them a0..a255; with two waves per SIMD the 256 a wave may
// have are split as the kernel declares).  A value in flight in a register the compiler manages can be copied or spilled by
// it at any moment -- it has no idea the load has not landed (tried: tied asm operands; the compiler peeled the loop and moved
// the buffers between registers) --, a register it never touches cannot.
//   a[2J : 2J+1], J < 4      buffer J of the running tile's ring
//   a[8+2k : 9+2k], k < 4    batch k of the NEXT tile's stream, requested one tile ahead
// All statements are asm volatile (kept in order among themselves) and name the registers in the clobber list, which is also
// what makes the compiler count them in the kernel's register budget.  vmcnt counts loads in issue order and the ring issues
// exactly one load per batch, so "at most three younger loads outstanding" (acc_wait) is "this buffer has landed".
// scripts/check_ring_isa.py verifies on the ISA that nothing but these statements touches an accumulation register.
#define SPHX_ACC_CLOBBERS "a0", "a1", "a2", "a3", "a4", "a5", "a6", "a7", "a8", "a9", "a10", "a11", "a12", "a13", "a14", "a15"
template<int REG>
__device__ __forceinline__ void acc_load(const ListStream &ls, uint32_t firstBatch, int batch, int lastBatch, uint32_t lane8)
{
	const int b = min(__builtin_amdgcn_readfirstlane(batch), lastBatch);
	const char *base = reinterpret_cast<const char*>(ls.list + ((size_t)__builtin_amdgcn_readfirstlane(firstBatch) + (uint32_t)b)*64u);
	static_assert(REG >= 0 && REG < 16 && (REG & 1) == 0, "a register pair");
#define SPHX_ACC_LOAD(R0, R1) asm volatile("global_load_dwordx2 a[" #R0 ":" #R1 "], %0, %1 ; ACCRING" :: "v"(lane8), "s"(base) : SPHX_ACC_CLOBBERS)
	if (REG == 0) SPHX_ACC_LOAD(0, 1); else if (REG == 2) SPHX_ACC_LOAD(2, 3); else if (REG == 4) SPHX_ACC_LOAD(4, 5);
	else if (REG == 6) SPHX_ACC_LOAD(6, 7); else if (REG == 8) SPHX_ACC_LOAD(8, 9); else if (REG == 10) SPHX_ACC_LOAD(10, 11);
	else if (REG == 12) SPHX_ACC_LOAD(12, 13); else SPHX_ACC_LOAD(14, 15);
#undef SPHX_ACC_LOAD
}
// the ring's own loads inside the pair loop: a running scalar base (advanced once per ring cycle by the caller) and an immediate
// offset per buffer -- no clamp, no index arithmetic per batch: past the end of a wave's share the loads read the next share (or the
// allocation's slack behind the last one, sphx_ensure_tile_lists), rows that are gathered and never computed
template<int REG, int OFF>
__device__ __forceinline__ void acc_load_at(const char *base, uint32_t lane8)
{
	static_assert(REG >= 0 && REG < 8 && (REG & 1) == 0 && OFF >= 0 && OFF < 4096, "a register pair of the ring, a 12-bit offset");
#define SPHX_ACC_LOAD_AT(R0, R1) asm volatile("global_load_dwordx2 a[" #R0 ":" #R1 "], %0, %1 offset:%2 ; ACCRING" :: "v"(lane8), "s"(base), "n"(OFF) : SPHX_ACC_CLOBBERS)
	if (REG == 0) SPHX_ACC_LOAD_AT(0, 1); else if (REG == 2) SPHX_ACC_LOAD_AT(2, 3); else if (REG == 4) SPHX_ACC_LOAD_AT(4, 5); else SPHX_ACC_LOAD_AT(6, 7);
#undef SPHX_ACC_LOAD_AT
}
// buffer REG/2 of the ring -> two ordinary registers (the batch has landed: acc_wait, or it was requested a tile ahead)
template<int REG>
__device__ __forceinline__ uint2 acc_read()
{
	uint2 r;
#define SPHX_ACC_READ(R0, R1) asm volatile("v_accvgpr_read_b32 %0, a" #R0 " ; ACCRING\n\tv_accvgpr_read_b32 %1, a" #R1 " ; ACCRING" : "=v"(r.x), "=v"(r.y) :: SPHX_ACC_CLOBBERS)
	if (REG == 0) SPHX_ACC_READ(0, 1); else if (REG == 2) SPHX_ACC_READ(2, 3); else if (REG == 4) SPHX_ACC_READ(4, 5); else if (REG == 6) SPHX_ACC_READ(6, 7);
	else if (REG == 8) SPHX_ACC_READ(8, 9); else if (REG == 10) SPHX_ACC_READ(10, 11); else if (REG == 12) SPHX_ACC_READ(12, 13); else SPHX_ACC_READ(14, 15);
#undef SPHX_ACC_READ
	return r;
}
__device__ __forceinline__ void acc_wait()
{
	static_assert(TILE_AHEAD == 4, "vmcnt(TILE_AHEAD - 1)");
	asm volatile("s_waitcnt vmcnt(3) ; ACCRING" ::: SPHX_ACC_CLOBBERS);
}
// The batches requested one tile ahead (a8..a15) spend the stretch between two pair phases -- the finalize stage, the window
// conversion: long code with temporaries of its own, where the compiler does reach for low accumulation registers -- in ordinary
// registers: acc_fetch_ahead once everything has landed (the caller waited vmcnt(0)), acc_start_ring right before the walk.
// What is left for the compiler to respect are the gaps between the ring's own statements inside the pair loop.
__device__ __forceinline__ void acc_fetch_ahead(ListWindow &lw)
{
	lw.q[0] = acc_read<8>(); lw.q[1] = acc_read<10>(); lw.q[2] = acc_read<12>(); lw.q[3] = acc_read<14>();
}
__device__ __forceinline__ void acc_start_ring(const ListWindow &lw)
{
	asm volatile("v_accvgpr_write_b32 a0, %0 ; ACCRING\n\tv_accvgpr_write_b32 a1, %1 ; ACCRING\n\tv_accvgpr_write_b32 a2, %2 ; ACCRING\n\t"
		"v_accvgpr_write_b32 a3, %3 ; ACCRING\n\tv_accvgpr_write_b32 a4, %4 ; ACCRING\n\tv_accvgpr_write_b32 a5, %5 ; ACCRING\n\t"
		"v_accvgpr_write_b32 a6, %6 ; ACCRING\n\tv_accvgpr_write_b32 a7, %7 ; ACCRING"
		:: "v"(lw.q[0].x), "v"(lw.q[0].y), "v"(lw.q[1].x), "v"(lw.q[1].y), "v"(lw.q[2].x), "v"(lw.q[2].y), "v"(lw.q[3].x), "v"(lw.q[3].y)
		: SPHX_ACC_CLOBBERS);
}

// (compiler-managed ring) LLVM sinks a load whose first use is three ring steps (and several side exits) away down to that use, which
// undoes the prefetch distance.  A use in a never-taken side block (pin is always NULL, but a kernel argument
// the compiler cannot see through) keeps the loads where they are issued; the main path pays one scalar branch.
__device__ __forceinline__ void pin_batch(const ListStream &ls, const uint2 &nd)
{
	if (__builtin_expect(ls.pin != nullptr, 0))
		ls.pin[threadIdx.x] = nd.x ^ nd.y;
}

#endif
