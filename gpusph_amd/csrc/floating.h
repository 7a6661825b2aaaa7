// floating.h -- what a context holds for its floating bodies (floating.hip), kept beside the context instead of inside it for the
// reason gages.h and diagnostics.h give: sphx_internal.h is part of the hash that ties the committed profile set to the kernel
// sources, and no kernel those profiles measure knows about floating bodies.
//
// The table is all sphx_api.hip sees of the feature: sphx_rb_flush asks it whether slots 0 .. numfloating-1 of the rigid-body table
// belong to the device, and reaches floating.hip's merge launch through a pointer kept here, so that a build of sphx_api.hip alone
// (the host emulations of other tests) links without floating.hip.
#pragma once
#include "sphx_internal.h"
#include <mutex>
#include <unordered_map>

#ifndef FLOAT_MAX_BLOCKS
#define FLOAT_MAX_BLOCKS 64       // blocks per body of floating_partials_kernel at the most (the host emulation builds with a small cap)
#endif
#define FLOAT_BLOCK    256
#define FLOAT_WAVES    (FLOAT_BLOCK/64)
#define FLOAT_STATE    SPHX_FLOATING_STATE_DOUBLES      // x 3, q 4, v 3, omega 3, total force 3, total torque 3
#define FLOAT_KEPT     13                               // ... of which the first 13 are the state a substep starts from

// the size of floating_exact.h's FloatingExactDev: per body, block and component SPHX_FLOATING_LIMBS 64-bit integers
#define FLOAT_EXACT_BYTES ((size_t)SPHX_MAX_BODIES*FLOAT_MAX_BLOCKS*6*SPHX_FLOATING_LIMBS*sizeof(long long))

// everything of a context's floating bodies that lives in device memory, one allocation
struct FloatingDev {
	double   state[SPHX_MAX_BODIES][FLOAT_STATE];
	double   saved[SPHX_MAX_BODIES][FLOAT_KEPT];        // the state of step n (step 1 saves it, step 2 starts from it)
	double   consts[SPHX_MAX_BODIES][4];                // mass, principal inertia
	uint32_t rowstart[SPHX_MAX_BODIES + 1];             // rows [rowstart[b], rowstart[b+1]) of RB_FORCES / RB_TORQUES are body b's
	double   partials[SPHX_MAX_BODIES][FLOAT_MAX_BLOCKS][6];
};

struct FloatingEntry {
	int          numfloating;
	uint32_t     blocks;           // blocks per body: a function of the row counts alone
	FloatingDev *dev;
	RbParams    *rb_image;         // where host uploads land once the device owns slots 0 .. numfloating-1 of rb_dev
	bool         whole_upload;     // sphx_floating_setup has put the bodies' first slots into the host mirror: the next flush copies all of it
	int        (*merge)(sphx_ctx *ctx, const FloatingEntry *e, hipStream_t st);      // rb_image -> rb_dev, the other bodies' slots only
	// floating.hip's step launch over dev->partials[body][0 .. blocksPerBody-1], for floating_exact.hip, which puts the exactly
	// rounded totals into block 0 and has the rule applied by the one kernel that states it
	int        (*step)(sphx_ctx *ctx, const FloatingEntry *e, uint32_t blocksPerBody, int step, const float *d_dt, hipStream_t st);
	void        *exact;            // floating_exact.hip's per-block limbs (FloatingExactDev), FLOAT_EXACT_BYTES, allocated with dev
};

struct FloatingTable {
	std::mutex lock;      // contexts belong to worker threads of their own (halo.hip)
	std::unordered_map<const sphx_ctx*, FloatingEntry> rows;
};
inline FloatingTable g_floating;

// the context's entry, or NULL: entries are made by sphx_floating_setup only and stay where they are until sphx_destroy
inline FloatingEntry *sphx_floating_entry(const sphx_ctx *ctx, bool create = false)
{
	std::lock_guard<std::mutex> hold(g_floating.lock);
	auto it = g_floating.rows.find(ctx);
	if (it != g_floating.rows.end()) return &it->second;
	if (!create) return nullptr;
	return &g_floating.rows.emplace(ctx, FloatingEntry{0, 1u, nullptr, nullptr, false, nullptr, nullptr, nullptr}).first->second;
}

inline void sphx_floating_release(const sphx_ctx *ctx)
{
	std::lock_guard<std::mutex> hold(g_floating.lock);
	auto it = g_floating.rows.find(ctx);
	if (it == g_floating.rows.end()) return;
	if (it->second.dev) (void)hipFree(it->second.dev);
	if (it->second.rb_image) (void)hipFree(it->second.rb_image);
	if (it->second.exact) (void)hipFree(it->second.exact);
	g_floating.rows.erase(it);
}
