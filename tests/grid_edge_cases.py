"""Periodic boxes on grids of one to three cells per axis, for tests/test_grid_edge_cases.py (the CPU oracle against a float64 sum over
periodic images) and tests/test_gpu_grid_edge_cases.py (the device).  TEST INFRASTRUCTURE, no GPU.

On such a grid a cell appears in the 4 x 4 x (k + 2) window of a forces tile more than once, each copy at a shift of its own, and a
pair of particles interacts through more than one periodic image.  A wrong shift gives a wrong force and no crash, and the tiled and
the generic kernels take their shifts from the same helpers (sphx_internal.h), so the reference of these cases is one that knows no
cells at all: tests/allpairs_ref.py with the list of image shifts of image_shifts().

Every case is PeriodicBox(0.05, jitter=0.2, **kwargs) and `usable`: what sphx_dbg_tiles_usable has to say after the list build
(1: the forces pass is the tiled kernels'; 0: the generic kernels').  Grid sizes are (x, y, z); COORD1..3 follow the linearisation.

  one-cell       1 x 1 x 1, 27 particles: every window cell is the one cell; most pairs interact through more than one image
  one-cell-wave  1 x 1 x 1, 64 particles.  usable = 0: the window of the one tile holds 3 columns x 16 rows = 48 copies of the cell,
                 3072 records where TILE_WCAP is 2876; build_tiles_kernel raises the overflow flag and every pass is the generic
                 kernels' (window_overflow() computes this from the sources' limits; the CPU test holds it for every case)
  two-each       2 x 2 x 2: every neighbour cell is reached through two offsets, one image of it in reach
  3x2x1          gs1 = 3 periodic (the row lies wholly in the window: cell-by-cell staging), gs2 = 2, gs3 = 1
  3x2x1-zxy      COORD1 = z with gs1 = 1
  3x1x2-yzx      gs1 = 1 along y
  1x3x2          gs3 = 1 behind an odd gs1
  slab-y         the thin periodic slab (a quasi-2D channel): free faces on the other two axes
  slab-free      the same grid without any wrap: window rows outside the grid
  odd-5x3x1      odd on all three axes: half-empty last row bundles
  rod-full       tile_cols (cells/2 + 1024 words) filled to its last word: tiles usable
  rod-over       one more column of cells: tiling_wanted is false, generic kernels"""
import itertools
import os
import re

import numpy as np

from gpusph_amd import defs as D
from gpusph_amd.problem import PeriodicBox
from tiling_overflow_cases import CSRC, limits

XYZ = D.PERIODIC_X | D.PERIODIC_Y | D.PERIODIC_Z
G0, GZ, GS = (0.0, 0.0, 0.0), (0.0, 0.0, -9.81), (3.0, -2.0, -9.0)

# name -> (PeriodicBox kwargs, grid (x, y, z), tiles usable, pairs through more than one image: True where a periodic side is
# shorter than two influence radii (0.26), False where none is, None where one is so by less than the jitter (nothing claimed))
CASES = {
    "one-cell":      (dict(n=(3, 3, 3), periodic=XYZ, linearization="xyz", gravity=GZ), (1, 1, 1), 1, True),
    "one-cell-wave": (dict(n=(4, 4, 4), periodic=XYZ, linearization="xyz", gravity=G0), (1, 1, 1), 0, True),
    "two-each":      (dict(n=(6, 6, 6), periodic=XYZ, linearization="yzx", gravity=GZ), (2, 2, 2), 1, False),
    "3x2x1":         (dict(n=(8, 6, 3), periodic=XYZ, linearization="xyz", gravity=GZ), (3, 2, 1), 1, True),
    "3x2x1-zxy":     (dict(n=(8, 6, 3), periodic=XYZ, linearization="zxy", gravity=GS), (3, 2, 1), 1, True),
    "3x1x2-yzx":     (dict(n=(8, 3, 6), periodic=XYZ, linearization="yzx", gravity=G0), (3, 1, 2), 1, True),
    "1x3x2":         (dict(n=(3, 8, 6), periodic=XYZ, linearization="yzx", gravity=GS), (1, 3, 2), 1, True),
    "slab-y":        (dict(n=(16, 3, 8), periodic=D.PERIODIC_Y, linearization="xzy", gravity=GS), (6, 1, 3), 1, True),
    "slab-free":     (dict(n=(16, 3, 8), periodic=D.PERIODIC_NONE, linearization="xzy", gravity=G0), (6, 1, 3), 1, False),
    "odd-5x3x1":     (dict(n=(14, 8, 5), periodic=D.PERIODIC_X | D.PERIODIC_Z, linearization="xyz", gravity=GZ), (5, 3, 1), 1, None),
    "rod-full":      (dict(n=(5325, 3, 3), periodic=XYZ, linearization="xyz", gravity=G0), (2048, 1, 1), 1, True),
    "rod-over":      (dict(n=(5328, 3, 3), periodic=XYZ, linearization="xyz", gravity=G0), (2049, 1, 1), 0, True),
}
# the cases that also go through SPS, the filters, XSPH and a trajectory
DEEP = ("one-cell", "3x2x1", "two-each", "slab-y")
MEAN_VELOCITY = (4.0, -3.0, 2.0)
TRAJ_STEPS, TRAJ_REBUILD = 12, 4


def problem(name, **more):
    kw = dict(CASES[name][0])
    kw.update(more)
    return PeriodicBox(0.05, jitter=0.2, **kw)


def grid(name):
    return CASES[name][1]


def usable(name):
    return CASES[name][2]


def multi_image(name):
    return CASES[name][3]


def trajectory_problem(name):
    prob = problem(name, velocity=MEAN_VELOCITY)
    prob.simparams.buildneibsfreq = TRAJ_REBUILD
    return prob


def image_shifts(prob):
    """the periodic images within reach of the 27 cell offsets: every combination of -1, 0, +1 box lengths along the periodic axes"""
    per = int(prob.simparams.periodicbound)
    axes = [(-1.0, 0.0, 1.0) if per & (1 << a) else (0.0,) for a in range(3)]
    size = np.asarray(prob.m_size, dtype=np.float64)
    return [np.array(s)*size for s in itertools.product(*axes)]


def _coord_sizes(prob):
    c1, c2, c3 = D.LINEARIZATIONS[prob.linearization]
    gs = [int(v) for v in prob.m_gridsize]
    return (c1, c2, c3), (gs[c1], gs[c2], gs[c3])


def tile_cols_sides(prob):
    """both sides of tiling_wanted's last condition (neibs.hip): the row bundles times the columns of the grid, and the words of the
    tile_cols allocation (sphx_api.hip: cells/2 + 1024), the latter read from the source so that a change there moves the cases"""
    with open(os.path.join(CSRC, "sphx_api.hip")) as f:
        m = re.search(r"tile_cols, sizeof\(uint32_t\)\*\(\(size_t\)ctx->cells_reserved/(\d+) \+ (\d+)\)", f.read())
    assert m, "sphx_api.hip no longer allocates tile_cols as cells_reserved/a + b: adjust the rods to it"
    _, (gs1, gs2, gs3) = _coord_sizes(prob)
    return ((gs2 + 1)//2)*((gs3 + 1)//2)*gs1, prob.grid_cells//int(m.group(1)) + int(m.group(2))


def window_overflow(prob, hash_, n, sps=False):
    """does build_tiles_kernel raise the tiling's overflow flag on these cells?  A column of a row bundle that holds home particles
    cannot join or start a tile when it holds more than TILE_PMAX of them or when the window columns c - 1 .. c + 1 (sixteen rows
    each, every periodic copy counted: tile_columns_kernel) hold more records than the window has room for; every other column
    does one or the other.  -> (overflows, the largest three-column window, the largest home column)"""
    lim = limits()
    wcap = lim["wcap_sps1"] if sps else lim["wcap"]
    (c1, c2, c3), (gs1, gs2, gs3) = _coord_sizes(prob)
    per = int(prob.simparams.periodicbound)
    per1, per2, per3 = bool(per & (1 << c1)), bool(per & (1 << c2)), bool(per & (1 << c3))
    cells = np.bincount(np.asarray(hash_[:n], dtype=np.int64) & D.CELLTYPE_BITMASK, minlength=gs1*gs2*gs3).reshape(gs3, gs2, gs1)

    def wrapped(v, gs, periodic):      # the kernels' rule: one step outside wraps to the far end, never a modulo
        if v < 0:
            return gs - 1 if periodic else None
        if v >= gs:
            return 0 if periodic else None
        return v

    worst_w = worst_h = 0
    over = False
    for g3 in range(0, gs3, 2):
        for g2 in range(0, gs2, 2):
            col = np.zeros(gs1, dtype=np.int64)
            for d3 in range(-1, 3):
                for d2 in range(-1, 3):
                    v2, v3 = wrapped(g2 + d2, gs2, per2), wrapped(g3 + d3, gs3, per3)
                    if v2 is not None and v3 is not None:
                        col += cells[v3, v2]
            home = sum(cells[g3 + a, g2 + b] for a in (0, 1) for b in (0, 1) if g3 + a < gs3 and g2 + b < gs2)
            prev = np.roll(col, 1) if per1 else np.concatenate([[0], col[:-1]])
            nxt = np.roll(col, -1) if per1 else np.concatenate([col[1:], [0]])
            win = (prev + col + nxt)[home > 0]
            worst_w, worst_h = max(worst_w, int(win.max(initial=0))), max(worst_h, int(home.max()))
            over = over or bool((win > wcap).any() or (home > lim["pmax"]).any())
    return over, worst_w, worst_h


def perturb(sim, seed=5):
    """the state of the float64 comparison: velocity noise normal(0, 0.3), rho~ noise uniform(-4e-3, 4e-3)"""
    n = sim.n
    rng = np.random.default_rng(seed)
    sim.vel[:n, :3] += rng.normal(0, 0.3, size=(n, 3)).astype(np.float32)
    sim.vel[:n, 3] += rng.uniform(-4e-3, 4e-3, size=n).astype(np.float32)


def wendland_F(k):
    return lambda r: (r/k["h"] - 2.0)**3*k["fcoeff"]


def image_pairs_beyond_one(nbs):
    """ordered pairs (i, j) that an image sum's neighbour arrays (allpairs_ref.neighbours) count more than once"""
    return int(sum((np.unique(nb, return_counts=True)[1] > 1).sum() for nb in nbs))
