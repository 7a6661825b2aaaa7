// gages.h -- the scratch of sphx_wave_gages (gages.hip) per context: the per-block partials of its first pass,
// [GAGE_MAX_BLOCKS][SPHX_MAX_GAGES][3] doubles, allocated at a context's first call and released by sphx_destroy.  Kept beside the
// context instead of inside it: sphx_internal.h is part of the hash that ties the committed profile set to the kernel sources
// (scripts/make_traffic_json.py), and the gages are no part of what those profiles measure.
#pragma once
#include "sphx_internal.h"
#include <mutex>
#include <unordered_map>

#define GAGE_MAX_BLOCKS 1024

struct GageScratchTable {
	std::mutex lock;      // contexts belong to worker threads of their own (halo.hip)
	std::unordered_map<const sphx_ctx*, double*> rows;
};
inline GageScratchTable g_gage_scratch;

// the context's scratch, allocated on first use; NULL when the allocation fails
inline double *sphx_gage_scratch(const sphx_ctx *ctx)
{
	std::lock_guard<std::mutex> hold(g_gage_scratch.lock);
	double *&p = g_gage_scratch.rows[ctx];
	if (!p && hipMalloc((void**)&p, sizeof(double)*3u*SPHX_MAX_GAGES*GAGE_MAX_BLOCKS) != hipSuccess) { (void)hipGetLastError(); p = nullptr; }
	return p;
}

inline void sphx_gage_scratch_release(const sphx_ctx *ctx)
{
	std::lock_guard<std::mutex> hold(g_gage_scratch.lock);
	auto it = g_gage_scratch.rows.find(ctx);
	if (it == g_gage_scratch.rows.end()) return;
	if (it->second) (void)hipFree(it->second);
	g_gage_scratch.rows.erase(it);
}
