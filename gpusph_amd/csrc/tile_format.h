// tile_format.h -- the tables of the forces tiling, word by word: what build_tiles_kernel (neibs.hip) and tile_lists_kernel
// (forces.hip) write and forces_tile_kernel (forces_tile.h) reads.  Every packed word is packed and unpacked here and nowhere
// else; the static_asserts under each pair round-trip the field limits.  The pack side is constexpr functions.  The unpack side
// (and TILE_RT_PACK_WAVE) is MACROS that spell the expressions the kernels were written with: forces_tile_kernel and
// tile_lists_kernel compile to other code -- other register allocation throughout -- when some of these expressions reach them
// through an inlined function (found by comparing the assembly kernel by kernel), and forces_tile_kernel has no register to spare.
// The capacities (TILE_PMAX, TILE_WCAP*, TILE_DESC, TILE_ROWDESC, TILE_RUNTAB, ...) are in sphx_internal.h, where the context's
// allocations read them.
#ifndef SPHX_TILE_FORMAT_H
#define SPHX_TILE_FORMAT_H

#include "sphx_internal.h"

#define TILE_FMT constexpr __host__ __device__ __forceinline__

// ---- tiles: TILE_DESC uint32 per tile.  Words 0..13 by build_tiles_kernel, 14 and 15 by tile_lists_kernel -----------------------
#define TILE_D_G2        0    // the tile's row bundle: first grid row along COORD2 ...
#define TILE_D_G3        1    // ... and along COORD3
#define TILE_D_FIRSTCELL 2    // first home cell along COORD1
#define TILE_D_NCELLS    3    // home cells along COORD1
#define TILE_D_FIRST     4    // [+ r], r < TILE_HROWS: first particle of home row r
#define TILE_D_COUNT     8    // [+ r]: particles of home row r
#define TILE_D_WINDOW    12   // records in the window
#define TILE_D_FLAGS     13   // TILE_DF_*
#define TILE_D_LISTBASE  14   // first batch of the tile's list stream
#define TILE_D_LANEBASE  15   // first entry of the tile's lane tables
#define TILE_DF_FLUID    1u   // a cell of the window holds fluid
static_assert(TILE_D_FIRST + TILE_HROWS == TILE_D_COUNT && TILE_D_COUNT + TILE_HROWS == TILE_D_WINDOW && TILE_D_LANEBASE + 1 == TILE_DESC,
	"descriptor words");

// ---- tile_rows: TILE_ROWDESC uint32 per tile (tile_lists_kernel): [r], r < 16: first record of window row r in memory;
// [TILE_ROWS_TOTAL + r/2]: records of rows r (low half) and r + 1; [TILE_ROWS_BASE + r/2]: window slot of the row's first record,
// bit 15 set when the row is not one range in memory, again as a pair of halves
#define TILE_ROWS_TOTAL 16u
#define TILE_ROWS_BASE  24u
TILE_FMT uint32_t tile_rows_pack_total(uint32_t even, uint32_t odd) { return (even & 0xFFFFu) | (odd << 16); }
TILE_FMT uint32_t tile_rows_base_half(uint32_t base, bool contig) { return (base & 0x7FFFu) | (contig ? 0u : 0x8000u); }
TILE_FMT uint32_t tile_rows_pack_base(uint32_t evenHalf, uint32_t oddHalf) { return evenHalf | (oddHalf << 16); }
#define TILE_ROWS_PAIR(row) ((row) >> 1)                         // which word of its table holds the row's half
#define TILE_ROWS_SHIFT(row) (16u*((row) & 1u))                  // ... and where the half starts in it
#define TILE_ROWS_HALF(word, shift) (((word) >> (shift)) & 0xFFFFu)
#define TILE_ROWS_HALF_BASE(half) ((half) & 0x7FFFu)
#define TILE_ROWS_HALF_CONTIG(half) (!((half) & 0x8000u))
static_assert(TILE_ROWS_HALF(tile_rows_pack_total(0xFFFFu, 0u), TILE_ROWS_SHIFT(0u)) == 0xFFFFu && TILE_ROWS_HALF(tile_rows_pack_total(0xFFFFu, 0u), TILE_ROWS_SHIFT(1u)) == 0u &&
	TILE_ROWS_HALF(tile_rows_pack_total(0u, 0xFFFFu), TILE_ROWS_SHIFT(1u)) == 0xFFFFu && TILE_ROWS_HALF(tile_rows_pack_total(0u, 0xFFFFu), TILE_ROWS_SHIFT(0u)) == 0u, "records per row: 16 bits");
static_assert(TILE_ROWS_HALF_BASE(TILE_ROWS_HALF(tile_rows_pack_base(tile_rows_base_half(0x7FFFu, true), tile_rows_base_half(0u, false)), TILE_ROWS_SHIFT(0u))) == 0x7FFFu &&
	TILE_ROWS_HALF_CONTIG(TILE_ROWS_HALF(tile_rows_pack_base(tile_rows_base_half(0x7FFFu, true), tile_rows_base_half(0u, false)), TILE_ROWS_SHIFT(0u))) &&
	TILE_ROWS_HALF_BASE(TILE_ROWS_HALF(tile_rows_pack_base(tile_rows_base_half(0x7FFFu, true), tile_rows_base_half(0u, false)), TILE_ROWS_SHIFT(1u))) == 0u &&
	!TILE_ROWS_HALF_CONTIG(TILE_ROWS_HALF(tile_rows_pack_base(tile_rows_base_half(0x7FFFu, true), tile_rows_base_half(0u, false)), TILE_ROWS_SHIFT(1u))), "first slot of a row: 15 bits and a flag");
static_assert(TILE_ROWS_TOTAL == TILE_WROWS && TILE_ROWS_BASE == TILE_ROWS_TOTAL + TILE_WROWS/2 && TILE_ROWS_BASE + TILE_WROWS/2 == TILE_ROWDESC && TILE_WCAP <= 0x7FFF, "row tables");

// ---- tile_runs: TILE_RUNTAB uint32 per tile (tile_lists_kernel): who walks what.
//   [w], w < 8                 wave w: first run | runs << 5 | first batch (tile-relative) << 10 | batches << 22
//   [TILE_RT_TILE]             chunks | home particles << 8 | runs << 24
//   [TILE_RT_CHUNK + c], c < 10   chunk c: first run | runs << 8   (its partial sums, in list order)
//   [TILE_RT_RUN + r], r < 17  run r: chunk | batches of the fluid section << 4 | batches of the second section << 12 | TILE_RUN_LAST if it ends its chunk
#define TILE_RT_TILE  8
#define TILE_RT_CHUNK 9
#define TILE_RT_RUN   24
#define TILE_RUN_LAST (1u << 20)
// what the wave word can hold: a tile with as many batches, or a share of as many, goes to the generic kernel
#define TILE_RT_FIRSTBATCH_END 4096u
#define TILE_RT_BATCHES_END    1024u

#define TILE_RT_PACK_WAVE(firstRun, runs, firstBatch, batches) ((firstRun) | ((runs) << 5) | ((firstBatch) << 10) | ((batches) << 22))
#define TILE_RT_WAVE_FIRST_RUN(w) ((w) & 31u)
#define TILE_RT_WAVE_RUNS(w) (((w) >> 5) & 31u)
#define TILE_RT_WAVE_FIRST_BATCH(w) (((w) >> 10) & 4095u)
#define TILE_RT_WAVE_BATCHES(w) ((w) >> 22)
static_assert(TILE_RT_WAVE_FIRST_RUN(TILE_RT_PACK_WAVE(31u, 0u, 0u, 0u)) == 31u && TILE_RT_PACK_WAVE(31u, 0u, 0u, 0u) == 31u, "first run: 5 bits");
static_assert(TILE_RT_WAVE_RUNS(TILE_RT_PACK_WAVE(0u, 31u, 0u, 0u)) == 31u && TILE_RT_WAVE_FIRST_RUN(TILE_RT_PACK_WAVE(0u, 31u, 0u, 0u)) == 0u &&
	TILE_RT_WAVE_FIRST_BATCH(TILE_RT_PACK_WAVE(0u, 31u, 0u, 0u)) == 0u, "runs: 5 bits");
static_assert(TILE_RT_WAVE_FIRST_BATCH(TILE_RT_PACK_WAVE(0u, 0u, TILE_RT_FIRSTBATCH_END - 1u, 0u)) == TILE_RT_FIRSTBATCH_END - 1u &&
	TILE_RT_WAVE_RUNS(TILE_RT_PACK_WAVE(0u, 0u, TILE_RT_FIRSTBATCH_END - 1u, 0u)) == 0u && TILE_RT_WAVE_BATCHES(TILE_RT_PACK_WAVE(0u, 0u, TILE_RT_FIRSTBATCH_END - 1u, 0u)) == 0u,
	"tile-relative first batch: 12 bits");
static_assert(TILE_RT_WAVE_BATCHES(TILE_RT_PACK_WAVE(0u, 0u, 0u, TILE_RT_BATCHES_END - 1u)) == TILE_RT_BATCHES_END - 1u &&
	TILE_RT_WAVE_FIRST_BATCH(TILE_RT_PACK_WAVE(0u, 0u, 0u, TILE_RT_BATCHES_END - 1u)) == 0u, "batches: 10 bits");
static_assert(TILE_RT_PACK_WAVE(31u, 31u, TILE_RT_FIRSTBATCH_END - 1u, TILE_RT_BATCHES_END - 1u) == 0xFFFFFFFFu && TILE_RUNS_MAX <= 32, "the wave word is full");

TILE_FMT uint32_t tile_rt_pack_tile(uint32_t chunks, uint32_t particles, uint32_t runs) { return chunks | (particles << 8) | (runs << 24); }
#define TILE_RT_TILE_CHUNKS(w) ((w) & 255u)
static_assert(TILE_RT_TILE_CHUNKS(tile_rt_pack_tile(TILE_CHUNKS, TILE_PMAX, TILE_RUNS_MAX)) == TILE_CHUNKS && TILE_PMAX < (1u << 16) && TILE_RUNS_MAX < (1u << 8),
	"chunks: 8 bits, home particles: 16, runs: 8");

TILE_FMT uint32_t tile_rt_pack_chunk(uint32_t firstRun, uint32_t runs) { return firstRun | (runs << 8); }
#define TILE_RT_CHUNK_FIRST_RUN(w) ((w) & 255u)
#define TILE_RT_CHUNK_RUNS(w) (((w) >> 8) & 255u)
static_assert(TILE_RT_CHUNK_FIRST_RUN(tile_rt_pack_chunk(255u, 0u)) == 255u && TILE_RT_CHUNK_RUNS(tile_rt_pack_chunk(255u, 0u)) == 0u &&
	TILE_RT_CHUNK_RUNS(tile_rt_pack_chunk(0u, 255u)) == 255u && TILE_RT_CHUNK_FIRST_RUN(tile_rt_pack_chunk(0u, 255u)) == 0u, "a chunk's first run and runs: 8 bits each");

TILE_FMT uint32_t tile_rt_pack_run(uint32_t chunk, uint32_t batchesF, uint32_t batchesSecond, bool endsChunk)
{
	return chunk | (batchesF << 4) | (batchesSecond << 12) | (endsChunk ? TILE_RUN_LAST : 0u);
}
#define TILE_RT_RUN_CHUNK(w) ((w) & 15u)
#define TILE_RT_RUN_BATCHES_F(w) (((w) >> 4) & 255u)
#define TILE_RT_RUN_BATCHES_SECOND(w) (((w) >> 12) & 255u)
static_assert(TILE_RT_RUN_CHUNK(tile_rt_pack_run(15u, 0u, 0u, false)) == 15u && TILE_RT_RUN_BATCHES_F(tile_rt_pack_run(15u, 0u, 0u, false)) == 0u &&
	TILE_CHUNKS <= 15, "chunk number: 4 bits");
static_assert(TILE_RT_RUN_BATCHES_F(tile_rt_pack_run(0u, 255u, 0u, false)) == 255u && TILE_RT_RUN_CHUNK(tile_rt_pack_run(0u, 255u, 0u, false)) == 0u &&
	TILE_RT_RUN_BATCHES_SECOND(tile_rt_pack_run(0u, 255u, 0u, false)) == 0u, "batches of the fluid section: 8 bits");
static_assert(TILE_RT_RUN_BATCHES_SECOND(tile_rt_pack_run(0u, 0u, 255u, false)) == 255u && TILE_RT_RUN_BATCHES_F(tile_rt_pack_run(0u, 0u, 255u, false)) == 0u &&
	!(tile_rt_pack_run(0u, 0u, 255u, false) & TILE_RUN_LAST) && tile_rt_pack_run(0u, 0u, 0u, true) == TILE_RUN_LAST, "batches of the second section: 8 bits, the flag above them");

// ---- window offsets: a stored neighbour and a particle's own row are named by the byte offset of the row in the window arrays
// (slot * 16, used as the LDS address as it is; slot 0 is the dummy row)
#define TILE_SLOT_MAX 4095u      // a tile with a record behind it goes to the generic kernel
TILE_FMT uint32_t tile_slot_offset(uint32_t slot) { return (slot << 4) & 0xFFFFu; }
static_assert(tile_slot_offset(TILE_SLOT_MAX) == TILE_SLOT_MAX*16u && TILE_SLOT_MAX*sizeof(float4) < (1u << 16) && TILE_WCAP <= TILE_SLOT_MAX, "slot << 4 in 16 bits");

// ---- lane records (tile_lane_rec): per lane of every chunk, the offset of the particle's own row | LANE_* flags << 16: what the
// pair loop needs of the particle info
#define LANE_TYPE_MASK 7u
#define LANE_COMPUTE_FORCE 8u
#define LANE_FLUID_SHIFT 4
#define LANE_VALID 64u
TILE_FMT uint32_t lane_rec_pack(uint32_t slot, uint32_t flags) { return tile_slot_offset(slot) | (flags << 16); }
#define LANE_REC_OFFSET(rec) ((rec) & 0xFFFFu)
#define LANE_REC_FLAGS(rec) ((rec) >> 16)
#define LANE_FLAGS_FLUID(flags) (((flags) >> LANE_FLUID_SHIFT) & 3u)
static_assert(LANE_REC_OFFSET(lane_rec_pack(TILE_SLOT_MAX, 0u)) == TILE_SLOT_MAX*16u && LANE_REC_FLAGS(lane_rec_pack(TILE_SLOT_MAX, 0u)) == 0u &&
	LANE_REC_FLAGS(lane_rec_pack(0u, 0xFFFFu)) == 0xFFFFu && LANE_REC_OFFSET(lane_rec_pack(0u, 0xFFFFu)) == 0u, "slot << 4 in 16 bits with the flags above it");
static_assert(LANE_FLAGS_FLUID(LANE_TYPE_MASK | LANE_COMPUTE_FORCE | LANE_VALID) == 0u && LANE_FLAGS_FLUID(3u << LANE_FLUID_SHIFT) == 3u &&
	!((3u << LANE_FLUID_SHIFT) & (LANE_TYPE_MASK | LANE_COMPUTE_FORCE | LANE_VALID)), "the flags do not overlap");

// ---- list batches (tile_list): [batch][64 lanes] uint2 = TILE_NB window offsets, two to a word in list order
TILE_FMT uint32_t list_pack_half(uint32_t off0, uint32_t off1) { return off0 | (off1 << 16); }
#define LIST_HALF_OFFSET(half, k) ((k) ? (half) >> 16 : (half) & 0xFFFFu)
static_assert(LIST_HALF_OFFSET(list_pack_half(0xFFF0u, 0u), 0) == 0xFFF0u && LIST_HALF_OFFSET(list_pack_half(0xFFF0u, 0u), 1) == 0u &&
	LIST_HALF_OFFSET(list_pack_half(0u, 0xFFF0u), 1) == 0xFFF0u && LIST_HALF_OFFSET(list_pack_half(0u, 0xFFF0u), 0) == 0u && TILE_NB == 4, "two offsets of 16 bits");

#undef TILE_FMT
#endif
