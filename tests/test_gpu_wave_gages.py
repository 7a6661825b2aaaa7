"""Wave gages on the GPU (gages.hip behind Engine.wave_gages): the level at a few (x, y) from the free-surface particles, against
the gage rule of tests/sa_postprocess_ref.py fed the device's own FG_SURFACE flags -- 1e-12 relative with a smoothing length (double
sums over a few hundred terms; only the order and FMA contraction differ), exactly in nearest mode (the test first makes sure
that the nearest and the second-nearest particle of a gage differ by more than 1e-9 relative) -- on the SA probe tank and on a
small DamBreak3D with DYN walls, over dry ground, twice on one state, with too many gages, cut into two slabs on one device, and
into WaveGage.txt.  Without the feature sphx_wave_gages does not exist."""
import threading

import numpy as np
import pytest

from gpusph_amd import capi, defs as D
from gpusph_amd.problem import DamBreak3D
import sa_postprocess_cases as cases

pytestmark = pytest.mark.gpu


def _np(t, dtype=None):
    a = t.cpu().numpy()
    return a.view(dtype) if dtype is not None else a


def _engine(problem, **kw):
    import torch
    from gpusph_amd.engine import TimestepEngine
    assert torch.cuda.is_available()
    return TimestepEngine(problem, device="cuda:0", **kw)


def _state(eng):
    n = eng.n
    return _np(eng.pos)[:n].copy(), _np(eng.hash, np.uint32)[:n].copy(), _np(eng.info)[:n].view(np.uint16).reshape(-1, 4).copy()


@pytest.mark.parametrize("jitter", [0.0, 0.1])
def test_gages_of_the_sa_probe_tank(jitter, tmp_path):
    import torch
    eng = _engine(cases.probe_box(jitter))
    eng.build_neibs()
    g = np.array(eng.problem.gages)
    assert (g[:, 3] > 0).sum() == 4 and (g[:, 3] == 0).sum() == 2
    before = _state(eng)[2]
    z = eng.wave_gages()                                   # runs the surface detection first: nobody has on this state
    pos, hash_, info = _state(eng)
    flagged = (info[:, 0] & D.FG_SURFACE) != 0
    assert not (before[:, 0] & D.FG_SURFACE).any() and 40 < flagged.sum() < 110
    want = cases.check_gages(eng.problem, pos, hash_, info, g, z, "SAProbeBox jitter %g" % jitter)
    assert np.isnan(z[3]) and abs(z[0] - eng.problem.water_level) < 0.6*eng.problem.m_deltap      # dry ground; the water level
    # twice on one state: the same bits (and the detection does not run again: stale flags planted now stay)
    z2 = eng.wave_gages()
    assert np.array_equal(z.view(np.uint64), z2.view(np.uint64))
    # no surface particle at all: NaN with a smoothing length, 0 in nearest mode
    n, dev = eng.n, eng.device
    clear = torch.from_numpy((info & ~np.uint16(D.FG_SURFACE)).view(np.int16)).to(dev)
    d_g = torch.from_numpy(g).to(dev)
    part = torch.zeros((len(g), 4), dtype=torch.float64, device=dev)
    zz = torch.zeros(len(g), dtype=torch.float64, device=dev)
    eng.k.wave_gages(part, d_g, len(g), eng.pos, clear, eng.hash, n)
    eng.k.wave_gages_finish(zz, part, d_g, len(g))
    zz = _np(zz)
    assert np.isnan(zz[g[:, 3] > 0]).all() and not zz[g[:, 3] == 0].any()
    # 64 gages run, 65 are refused
    many = np.tile(g[0], (65, 1))
    assert np.array_equal(eng.wave_gages(many[:64]).view(np.uint64), np.tile(z[:1], 64).view(np.uint64))
    with pytest.raises(capi.SphxInvalidArgument, match="SPHX_MAX_GAGES"):
        eng.wave_gages(many)
    # the writer: header and one line per call
    path = tmp_path / "WaveGage.txt"
    eng.write_wave_gages(str(path))
    eng.write_wave_gages(str(path))
    lines = path.read_text().split("\n")
    assert lines[0] == "time" + "".join("\tzgage%d" % k for k in range(len(g))) and lines[3] == "" and len(lines) == 4
    assert lines[1] == lines[2] == "0" + "".join("\t%.9g" % v for v in want)


def test_gages_of_a_dam_break_with_dyn_walls():
    pr = DamBreak3D(0.04, obstacle=True, jitter=0.05, hydrostatic=False)
    x0, y0 = 0.2, 0.33
    for g in ((x0, y0, 0.1), (0.31, 0.52, 0.06), (x0 + 0.013, y0 - 0.007), (3.0, 0.3, 0.1), (1.5, 0.21)):
        pr.add_gage(*g)
    eng = _engine(pr)
    for _ in range(3):
        eng.step()
    z = eng.wave_gages()
    pos, hash_, info = _state(eng)
    assert 50 < ((info[:, 0] & D.FG_SURFACE) != 0).sum() < eng.n//3
    cases.check_gages(pr, pos, hash_, info, np.array(pr.gages), z, "DamBreak3D")
    assert np.isnan(z[3]) and 0.3 < z[0] < 0.45 and np.isfinite(z[4])
    eng.step()
    z2 = eng.wave_gages()                                  # a new state: detected again
    pos, hash_, info = _state(eng)
    cases.check_gages(pr, pos, hash_, info, np.array(pr.gages), z2, "DamBreak3D, a step later")
    assert not np.array_equal(z[:3], z2[:3])


@pytest.mark.timeout(300)
def test_two_slabs_read_what_the_single_domain_reads(monkeypatch):
    """the arrangement of tests/test_gpu_halo.py: two slabs on the one device, two worker threads, the exchange through sphx_halo_*;
    every slab counts the rows it owns, the partial sums are all-reduced in double, the nearest particle is the nearest of both.
    One smoothed and one nearest-mode gage sit on the cut.  Same readings as the single domain: 1e-12 relative / exact"""
    import torch
    from gpusph_amd import capi
    from gpusph_amd.halo import CapiTransport
    from gpusph_amd.multigpu import MultiGpuEngine, SlabPartition
    monkeypatch.setenv("SPHX_DISABLE_TILES", "1")
    kw = dict(deltap=0.03, obstacle=True, jitter=0.05, linearization="xzy")
    pr = DamBreak3D(**kw)
    part = SlabPartition(pr, 2)
    c3 = D.LINEARIZATIONS["xzy"][2]
    assert c3 == 1
    ycut = pr.m_origin[1] + part.hi[0]*pr.m_cellsize[1]
    gages = [(0.2, ycut, 0.09), (0.2013, ycut + 0.0004), (0.25, ycut - 0.2, 0.06), (0.15, ycut + 0.15, 0.05), (0.1, 0.1), (3.0, ycut, 0.05)]
    g = np.zeros((len(gages), 4))
    for k, v in enumerate(gages):
        g[k, :2] = v[:2]
        g[k, 3] = v[2] if len(v) > 2 else 0.0
    steps = 2
    lib = capi.load()
    group = CapiTransport.new_group(lib, 2)
    out, errors = [None, None], []

    def worker(rank):
        try:
            torch.cuda.set_device(0)
            eng = MultiGpuEngine(DamBreak3D(**kw), "cuda:0", rank, 2, transport=lambda k: CapiTransport(k, rank, 2, group=group))
            for _ in range(steps):
                eng.step()
            z = eng.wave_gages(g)
            torch.cuda.synchronize()
            info = _np(eng.info)[:eng.n_local].view(np.uint16).reshape(-1, 4)
            out[rank] = (z, eng.n_int, eng.n_local, int(((info[:eng.n_int, 0] & D.FG_SURFACE) != 0).sum()))
            eng.transport.close()
        except BaseException as e:      # the other thread would wait at a barrier for ever: pytest's timeout ends the test
            errors.append((rank, repr(e)))
            raise

    threads = [threading.Thread(target=worker, args=(r,), daemon=True) for r in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(timeout=120)
    assert not errors, errors
    assert all(o is not None for o in out), "a worker did not finish"
    lib.sphx_halo_group_destroy(group)

    ref = _engine(DamBreak3D(**kw))
    for _ in range(steps):
        ref.step()
    z = ref.wave_gages(g)
    pos, hash_, info = _state(ref)
    cases.check_gages(ref.problem, pos, hash_, info, g, z, "single domain")
    nsurf = int(((info[:, 0] & D.FG_SURFACE) != 0).sum())
    assert out[0][3] + out[1][3] == nsurf and all(o[2] > o[1] for o in out)      # the owned rows' flags add up; both hold a halo
    gp = cases.global_pos_f64(ref.problem, pos, hash_)
    surf = (info[:, 0] & D.FG_SURFACE) != 0
    near = surf & (np.hypot(gp[:, 0] - g[0, 0], gp[:, 1] - g[0, 1]) < 2*g[0, 3])
    assert (gp[near, 1] < ycut).sum() > 5 and (gp[near, 1] >= ycut).sum() > 5              # the gage on the cut reads both slabs
    for o in out:
        assert np.array_equal(np.isnan(o[0]), np.isnan(z)) and np.isnan(z[5])
        sm = (g[:, 3] > 0) & ~np.isnan(z)
        assert (np.abs(o[0][sm] - z[sm]) <= 1e-12*np.abs(z[sm])).all(), (o[0], z)
        assert np.array_equal(o[0][g[:, 3] == 0], z[g[:, 3] == 0])
