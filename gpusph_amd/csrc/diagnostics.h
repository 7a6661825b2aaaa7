// diagnostics.h -- the scratch of sphx_save_diagnostics (diagnostics.hip) per context: the per-block partials of its first pass,
// [DIAG_MAX_BLOCKS][SPHX_DIAG_DOUBLES] doubles, allocated at a context's first call and released by sphx_destroy.  Kept beside the
// context instead of inside it for the reason gages.h gives: sphx_internal.h is part of the hash that ties the committed profile set
// to the kernel sources, and the diagnostics are no part of what those profiles measure.
#pragma once
#include "sphx_internal.h"
#include <mutex>
#include <unordered_map>

#ifndef DIAG_MAX_BLOCKS
#define DIAG_MAX_BLOCKS 1024      // (the host emulation of the tests builds with a small cap: several rounds of the grid-stride loop at small n)
#endif

struct DiagScratchTable {
	std::mutex lock;      // contexts belong to worker threads of their own (halo.hip)
	std::unordered_map<const sphx_ctx*, double*> rows;
};
inline DiagScratchTable g_diag_scratch;

// the context's scratch, allocated on first use; NULL when the allocation fails
inline double *sphx_diag_scratch(const sphx_ctx *ctx)
{
	std::lock_guard<std::mutex> hold(g_diag_scratch.lock);
	double *&p = g_diag_scratch.rows[ctx];
	if (!p && hipMalloc((void**)&p, sizeof(double)*SPHX_DIAG_DOUBLES*DIAG_MAX_BLOCKS) != hipSuccess) { (void)hipGetLastError(); p = nullptr; }
	return p;
}

inline void sphx_diag_scratch_release(const sphx_ctx *ctx)
{
	std::lock_guard<std::mutex> hold(g_diag_scratch.lock);
	auto it = g_diag_scratch.rows.find(ctx);
	if (it == g_diag_scratch.rows.end()) return;
	if (it->second) (void)hipFree(it->second);
	g_diag_scratch.rows.erase(it);
}
