"""Whose tiling is it?  The forces tiles of a context belong to the neighbour list it built last, from the very buffers of that
build (sphx_tiles_current, sphx_internal.h): a pass that is handed another list or another cellStart -- equal contents, another
address -- must run on the generic kernels, and take the tiling again when the buffers of the build come back.

The tiled and the generic kernels form the same sums in another frame of reference, so their results differ in some bits
(asserted below: otherwise nothing here could tell which kernel ran; about a tenth of the force words and a sixth of the stress
words on this problem, no jitter needed), while each of them repeats itself to the bit.  That makes
"equal to the generic context's result, bit for bit" a statement about the kernel that ran."""
import numpy as np
import pytest

from gpusph_amd.problem import DamBreak3D

pytestmark = pytest.mark.gpu


def _bits(t, n):
    return t.cpu().numpy()[:n].view(np.uint32).copy()


def _context(opts, monkeypatch, disable_tiles):
    """the problem of smoke() with the seeded velocity perturbation of test_tiled_and_generic_kernels_agree, list built"""
    import torch
    from gpusph_amd.engine import TimestepEngine
    monkeypatch.setenv("SPHX_DISABLE_TILES", "1" if disable_tiles else "0")      # read when the context is created
    eng = TimestepEngine(DamBreak3D(0.04, obstacle=True, hydrostatic=False, **opts), device="cuda:0", clobber_neibslist=True)
    eng.build_neibs()
    n = eng.n
    rng = np.random.default_rng(11)
    vel = eng.vel.cpu().numpy().copy()
    vel[:n, :3] += rng.uniform(-0.3, 0.3, size=(n, 3)).astype(np.float32)
    vel[:n, 3] += rng.uniform(0, 2e-3, size=n).astype(np.float32)
    eng.vel.copy_(torch.from_numpy(vel).to(eng.device))
    return eng


def _forces_pass(eng):
    """one forces pass (with SPS: the stress pass before it) -> bits of the forces, the next dt, bits of the stress tensor"""
    eng._forces(eng.pos, eng.vel, 1, 0)
    n = eng.n
    tau = np.concatenate([_bits(t, n) for t in eng.tau], axis=1) if getattr(eng, "tau", None) else np.zeros((n, 6), np.uint32)
    return _bits(eng.forces, n), float(eng.d_dt_next.item()), tau


def _same(a, b):
    return np.array_equal(a[0], b[0]) and a[1] == b[1] and np.array_equal(a[2], b[2])


@pytest.mark.parametrize("opts", [dict(), dict(viscosity="SPSVISC")], ids=["plain", "sps"])
def test_tiling_belongs_to_the_buffers_of_its_build(opts, monkeypatch):
    sps = bool(opts)
    gen = _context(opts, monkeypatch, disable_tiles=True)
    assert int(gen.k.lib.sphx_dbg_tiles_usable(gen.k.ctx.handle)) == 0
    G = _forces_pass(gen)
    assert _same(_forces_pass(gen), G)      # the generic kernels repeat themselves
    del gen

    eng = _context(opts, monkeypatch, disable_tiles=False)
    assert int(eng.k.lib.sphx_dbg_tiles_usable(eng.k.ctx.handle)) == 1
    T = _forces_pass(eng)
    nf, nt = int((T[0] != G[0]).sum()), int((T[2] != G[2]).sum())
    print("words that differ between the tiled and the generic kernels: forces %d of %d, stress tensor %d of %d, dt %r | %r"
          % (nf, T[0].size, nt, T[2].size, T[1], G[1]))
    assert nf > 0, "the tiled and the generic forces agree to the bit: this test cannot see which of them ran"
    if sps:
        assert nt > 0, "the tiled and the generic stress pass agree to the bit: this test cannot see which of them ran"
        assert np.abs(T[2].view(np.float32)).max() > 0

    own_list, own_cells = eng.neibslist, eng.cellStart
    # a foreign neighbour list: the same contents at another address
    eng.neibslist = own_list.clone()
    assert eng.neibslist.data_ptr() != own_list.data_ptr()
    assert _same(_forces_pass(eng), G)
    eng.neibslist = own_list
    # a foreign cellStart, the list of the build
    eng.cellStart = own_cells.clone()
    assert eng.cellStart.data_ptr() != own_cells.data_ptr()
    assert _same(_forces_pass(eng), G)
    eng.cellStart = own_cells
    # the buffers of the build again: the tiling is theirs
    assert _same(_forces_pass(eng), T)
    # ... and so is that of another build
    eng.build_neibs()
    assert int(eng.k.lib.sphx_dbg_tiles_usable(eng.k.ctx.handle)) == 1
    assert _same(_forces_pass(eng), T)
