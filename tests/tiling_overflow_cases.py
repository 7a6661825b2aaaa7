"""Problems whose forces TILING overflows while no NEIGHBOUR LIST does, for tests/test_tiling_overflow_cases.py (the CPU oracle proves
that precondition of every case) and tests/test_gpu_tiling_overflow.py (the device).  TEST INFRASTRUCTURE.

The tiling of a neighbour-list build raises its overflow flag (tile_ctl[1]) in build_tiles_kernel (neibs.hip: a 2 x 2 home column
of more than TILE_PMAX particles, a three-column window of more than TILE_WCAP records, a full tile table) and in tile_lists_kernel
(forces.hip: a home particle with more than 128 entries in its fluid or in its second list section).  Every pass then has to be the
generic kernels' alone.  A forces pass over a neighbour LIST that did not fit is outside the contract (its slots are unspecified,
test_neighbour_list_overflow_is_reported): none of these cases may have one, and every user checks that first.

  gaussian  the Gaussian kernel's radius of 3 h: about 250 neighbours in the bulk (list-length trigger)
  wide      a smoothing factor of 1.7 instead of 1.3 on the Wendland kernel: a few rows beyond 128, columns and windows well inside
            their limits (the list-length trigger alone)
  clump     the fluid around one cell drawn into that cell: more than TILE_PMAX particles in a home column (build_tiles_kernel's trigger)
  sa-wide   the smoothing factor of 1.7 on the semi-analytical tanks (density summation, Ferrari, a moving wall, open boundaries)"""
import os
import re

import numpy as np

from gpusph_amd import defs as D
from gpusph_amd.problem import DamBreak3D, SABox, SAChannelIO, SAPaddleBox

CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "gpusph_amd", "csrc")
WIDE_SFACTOR = 1.7
CLUMP_CELL = (3, 4, 3)
CLUMP_REACH = 0.18
CLUMP_FACTOR = 0.2


def limits():
    """the tiling's limits as the sources state them: dict(list=128, pmax=TILE_PMAX, wcap=TILE_WCAP, wcap_sps1=..., wcap_sps=...)"""
    with open(os.path.join(CSRC, "sphx_internal.h")) as f:
        head = f.read()
    with open(os.path.join(CSRC, "forces.hip")) as f:
        forces = f.read()

    def define(name):
        m = re.search(r"^#define\s+%s\s+(\d+)\b" % name, head, re.M)
        assert m, "sphx_internal.h no longer defines %s" % name
        return int(m.group(1))

    m = re.search(r"F > (\d+)u \|\| B > (\d+)u \|\| unwritten", forces)
    assert m and m.group(1) == m.group(2), "tile_lists_kernel's test of the section lengths has changed: adjust the cases to it"
    return dict(list=int(m.group(1)), pmax=define("TILE_PMAX"), wcap=define("TILE_WCAP"), wcap_sps1=define("TILE_WCAP_SPS1"),
                wcap_sps=define("TILE_WCAP_SPS"))


def wide(cls, sfactor=WIDE_SFACTOR):
    """cls with another smoothing factor: set before the problem derives its smoothing length, grid and time step from it"""
    class Wide(cls):
        def set_deltap(self, dp):
            self.simparams.sfactor = sfactor
            super().set_deltap(dp)
    Wide.__name__ = Wide.__qualname__ = "Wide" + cls.__name__
    return Wide


def _resize(prob, neiblistsize, neibboundpos):
    prob.simparams.neiblistsize, prob.simparams.neibboundpos = int(neiblistsize), int(neibboundpos)
    return prob


def gaussian(**opts):
    return DamBreak3D(0.05, obstacle=False, jitter=0.1, hydrostatic=False, kerneltype=D.GAUSSIAN, **opts)


WIDE_VARIANTS = {
    "plain": dict(),
    "sps": dict(viscosity="SPSVISC"),
    "two-fluids-ferrari": dict(two_fluids=True, density_diffusion=D.FERRARI),      # tiled on the Wendland kernel only: this one
    "lj": dict(boundary=D.LJ_BOUNDARY),
}


def wide_dambreak(**opts):
    return _resize(wide(DamBreak3D)(0.05, obstacle=False, jitter=0.1, hydrostatic=False, **opts), 288, 287)


def unclumped():
    """the problem `clump` is made from, with its list sizes: a tiling that succeeds"""
    return _resize(DamBreak3D(0.03, obstacle=False, jitter=0.1, hydrostatic=False), 2048, 2047)


def clump():
    """every fluid particle within CLUMP_REACH of the centre of the cell CLUMP_CELL (along each axis) drawn towards that centre by
    CLUMP_FACTOR: they end up in that one cell, more than TILE_PMAX of them and fewer than the 2047 a list entry can index"""
    prob = unclumped()
    g = prob.parts.pos_global
    centre = prob.m_origin + (np.array(CLUMP_CELL) + 0.5)*prob.m_cellsize
    fluid = (prob.parts.info[:, 0] & 7) == D.PT_FLUID
    near = fluid & (np.abs(g[:, :3] - centre) <= CLUMP_REACH).all(axis=1)
    g[near, :3] = centre + CLUMP_FACTOR*(g[near, :3] - centre)
    prob.clumped = int(near.sum())
    return prob


SA_VARIANTS = {
    "density-sum": (SABox, dict()),                                  # StillWaterSA's set: density summation + Brezzi diffusion
    "ferrari": (SABox, dict(options="Spheric2SA")),                  # continuity equation, Ferrari term in the tiled SA forces
    "paddle": (SAPaddleBox, dict()),                                 # a moving wall
    "channel-io": (SAChannelIO, dict()),                             # open boundaries, a rebuild in every step
}


def sa_wide(variant="density-sum"):
    cls, kw = SA_VARIANTS[variant]
    prob = wide(cls)(0.05, jitter=0.1, **kw)
    prob.simparams.neibboundpos, prob.simparams.neiblistsize = 383, 512
    return prob


def _case(fn, *a, **kw):
    return lambda: fn(*a, **kw)


CASES = {"gaussian": gaussian, "gaussian-sps": _case(gaussian, viscosity="SPSVISC"), "clump": clump}
CASES.update({"wide-" + k: _case(wide_dambreak, **v) for k, v in WIDE_VARIANTS.items()})
CASES.update({"sa-wide-" + k: _case(sa_wide, k) for k in SA_VARIANTS})


# ---------------------------------------------------------------------------------------------------------------------------------
# what the oracle's build says about a case

def survey(prob):
    """the oracle's neighbour-list build of the problem's initial state -> dict(n, too_many = hasTooManyNeibs (-1: every list fits),
    first / second = section_lengths, home / window = columns, listsize)"""
    sp = prob.simparams
    sa = sp.boundarytype == D.SA_BOUNDARY
    if sa:
        from sa_helpers import sa_oracle_state
        st = sa_oracle_state(prob)
        n, nl, hash_, info, stride = st["n"], st["nl"], st["hash"], st["neibs_info"], st["n"]
    else:
        import oracle_lib as ol
        sim = ol.OracleSim(prob)
        sim.build_neibs()
        n, nl, hash_, info, stride = sim.n, sim.nl, sim.hash, sim.neibs_info, len(sim.pos)
    first, second = section_lengths(nl, n, stride, int(sp.neiblistsize), int(sp.neibboundpos), sa)
    home, window = columns(prob, hash_, n)
    return dict(n=n, too_many=int(info.hasTooManyNeibs), first=first, second=second, home=home, window=window,
                listsize=(int(sp.neiblistsize), int(sp.neibboundpos)))

def section_lengths(nl, n, stride, neiblistsize, neibboundpos, sa):
    """(entries of the fluid section, entries of the second section) of every row below n of an oracle-format list.  The second
    section is what tile_lists_kernel counts next to the fluid section: the boundary section (downwards from neibboundpos), with
    SA_BOUNDARY the VERTEX section (upwards from neibboundpos + 1)."""
    t = np.asarray(nl).reshape(neiblistsize, stride)[:, :n]
    end = t == 0xFFFF

    def run(rows):       # entries before the first terminator, walking `rows` in order; all of them if there is none
        e = end[rows]
        return np.where(e.any(axis=0), e.argmax(axis=0), len(rows))

    first = run(np.arange(0, neiblistsize))
    if sa:
        second = run(np.arange(neibboundpos + 1, neiblistsize))
    else:
        second = run(np.arange(neibboundpos, -1, -1))
    return first, second


def columns(prob, hash_, n):
    """(particles of every 2 x 2 home column, records of every three-column window) as build_tiles_kernel counts them: home columns
    are the cells (c, g2 .. g2 + 1, g3 .. g3 + 1) with even g2, g3 along the second and third axis of the linearisation, the window
    of a tile that starts at column c the cells (c - 1 .. c + 1, g2 - 1 .. g2 + 2, g3 - 1 .. g3 + 2).  No periodicity."""
    c1, c2, c3 = D.LINEARIZATIONS[prob.linearization]
    gs = [int(v) for v in prob.m_gridsize]
    cells = np.bincount(np.asarray(hash_[:n], dtype=np.int64) & D.CELLTYPE_BITMASK, minlength=gs[0]*gs[1]*gs[2])
    grid = cells.reshape(gs[c3], gs[c2], gs[c1])
    pad = np.zeros((gs[c3] + 4, gs[c2] + 4, gs[c1] + 2), dtype=np.int64)
    pad[1:1 + gs[c3], 1:1 + gs[c2], 1:1 + gs[c1]] = grid
    home, window = [], []
    for g3 in range(0, gs[c3], 2):
        for g2 in range(0, gs[c2], 2):
            home.append(pad[g3 + 1:g3 + 3, g2 + 1:g2 + 3, 1:1 + gs[c1]].sum(axis=(0, 1)))
            col = pad[g3:g3 + 4, g2:g2 + 4, :].sum(axis=(0, 1))
            window.append(col[:-2] + col[1:-1] + col[2:])
    return np.array(home), np.array(window)
