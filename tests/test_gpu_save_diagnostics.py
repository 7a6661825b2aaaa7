"""The save-time diagnostics on the GPU (diagnostics.hip behind Engine.save_diagnostics): kinetic, potential and internal energy per
fluid, the largest particle speed and the first particle without a finite position, against the float64 rule of
tests/diagnostics_ref.py on the downloaded state -- every sum to (n + 8) 2^-52 sum|term| of its class (the bound of any summation
order over bit-identical terms: derived, not measured), the row counts, the speed and the row exactly -- on a small two-fluid
DamBreak3D with internal energy and without, on states whose answer can be counted, with inactive rows and NaNs, on more rows than
the capped grid has threads, the peak tracking and its line, energy.txt, and cut into two slabs on one device.  Without the feature
sphx_save_diagnostics does not exist."""
import threading
import warnings

import numpy as np
import pytest

from gpusph_amd import commonwriter, defs as D
from gpusph_amd.problem import DamBreak3D, info_type
import diagnostics_ref as ref

pytestmark = pytest.mark.gpu

KW = dict(deltap=0.03, two_fluids=True, internal_energy=True, jitter=0.05)
NF = D.MAX_FLUID_TYPES


def _engine(problem, **kw):
    import torch
    from gpusph_amd.engine import TimestepEngine
    assert torch.cuda.is_available()
    return TimestepEngine(problem, device="cuda:0", **kw)


def _state(eng):
    st = eng.download()
    return dict(pos=st["pos"], vel=st["vel"], info=st["info"].reshape(-1, 4), hash=st["hash"], energy=st.get("energy"))


def _rule(eng, st, **over):
    s = dict(st, **over)
    return ref.rule(eng.problem, s["pos"], s["vel"], s["info"], s["hash"], s["energy"])


def _raw(eng, st, **over):
    """sphx_save_diagnostics on (modified) copies of the state -> the DOUBLES float64 of its result"""
    import torch
    s = dict(st, **over)
    dev = eng.device
    up = lambda a, view=None: torch.from_numpy(np.ascontiguousarray(a if view is None else a.view(view))).to(dev)
    out = torch.full((ref.DOUBLES,), -7.0, dtype=torch.float64, device=dev)
    eng.k.save_diagnostics(out, up(s["pos"]), up(s["vel"]), up(s["info"], np.int16), up(s["hash"], np.int32),
                           None if s["energy"] is None else up(s["energy"]), len(s["pos"]))
    return out.cpu().numpy()


def _check(d, want, what):
    ref.check_sums(d["energy"], d["rows"], want, what)
    assert d["energy"].dtype == np.float64 and d["energy"].shape == (NF + 1, 3)
    assert d["max_speed"].dtype == np.float32 and d["max_speed"].view(np.uint32) == want["max_speed"].view(np.uint32), (what, d["max_speed"], want["max_speed"])
    assert d["nan_row"] == (None if want["nan_row"] is None else (0, want["nan_row"]))


def _same_bits(a, b):
    return (np.array_equal(a["energy"].view(np.uint64), b["energy"].view(np.uint64)) and np.array_equal(a["rows"], b["rows"])
            and a["max_speed"].view(np.uint32) == b["max_speed"].view(np.uint32) and a["nan_row"] == b["nan_row"])


@pytest.fixture(scope="module")
def small():
    eng = _engine(DamBreak3D(**KW))
    for _ in range(3):
        eng.step()
    return eng, _state(eng)


def test_small_engine_against_the_rule(small):
    eng, st = small
    assert eng.n == 16274 and eng.energy_on
    d = eng.save_diagnostics()
    want = _rule(eng, st)
    _check(d, want, "DamBreak3D two fluids, internal energy")
    assert (want["rows"][[0, 1, NF]] > 500).all() and not want["rows"][2:NF].any() and want["max_speed"] > 0
    assert st["energy"].any() and want["energy"][:, 2].any()      # internal energy has moved in three steps
    assert _same_bits(d, eng.save_diagnostics())
    ref.check_out(_raw(eng, st), want, "the entry point on a copy of the state")


def test_counting_and_nan_cases(small):
    eng, st = small
    n = eng.n
    cls = np.where(info_type(st["info"]) == D.PT_FLUID, (st["info"][:, 1] >> 12).astype(np.int64), NF)
    counts = np.bincount(cls, minlength=NF + 1).astype(np.float64)
    # mass 1, velocity (1, 0, 0), energy 0.25: every sum is a count
    pos, vel = st["pos"].copy(), st["vel"].copy()
    pos[:, 3] = 1.0
    vel[:, :3] = (1.0, 0.0, 0.0)
    out = _raw(eng, st, pos=pos, vel=vel, energy=np.full(n, 0.25, dtype=np.float32))
    s = out[:ref.MAXSQ].reshape(-1, 4)
    assert np.array_equal(s[:, 3], counts) and np.array_equal(s[:, 0], 0.5*counts) and np.array_equal(s[:, 2], 0.25*counts)
    assert out[ref.MAXSQ] == 1.0 and out[ref.NANROW] == ref.NO_ROW
    # inactive rows drop out of sums, counts and the speed, even with the largest velocity and a NaN position
    pos, vel = st["pos"].copy(), st["vel"].copy()
    gone = np.array([0, 5, 640, 4097, n - 1])
    pos[gone, 3] = np.nan
    vel[gone[2], :3] = (50.0, -60.0, 70.0)
    pos[gone[3], 0] = np.nan
    out = _raw(eng, st, pos=pos, vel=vel)
    want = _rule(eng, st, pos=pos, vel=vel)
    ref.check_out(out, want, "inactive rows")
    assert want["rows"].sum() == n - len(gone) and want["max_speed"] < 50 and not np.isnan(out).any()
    # a NaN velocity: the kinetic energy of its class, not the speed
    base = _raw(eng, st)
    vel = st["vel"].copy()
    vel[1234, 1] = np.nan
    out = _raw(eng, st, vel=vel)
    ref.check_out(out, _rule(eng, st, vel=vel), "NaN velocity")
    s = out[:ref.MAXSQ].reshape(-1, 4)
    assert np.isnan(s[cls[1234], 0]) and np.isnan(s).sum() == 1 and out[ref.MAXSQ] == base[ref.MAXSQ]
    # NaN positions in two rows of the second fluid: the lower row, and the potential energy of that class
    fl = np.nonzero(cls == 1)[0]
    a, b = int(fl[len(fl)//2]), int(fl[20])
    pos = st["pos"].copy()
    pos[[a, b], 0] = np.nan
    out = _raw(eng, st, pos=pos)
    ref.check_out(out, _rule(eng, st, pos=pos), "NaN positions")
    s = out[:ref.MAXSQ].reshape(-1, 4)
    assert b < a and out[ref.NANROW] == b and np.isnan(s[1, 1]) and np.isnan(s).sum() == 1


def test_the_driver_warns_about_a_nan_position(small):
    import torch
    eng, st = small
    row = 321
    keep = eng.pos[row].clone()
    eng.pos[row, 2] = float("nan")
    try:
        with pytest.warns(RuntimeWarning, match="particle %d " % row):
            d = eng.save_diagnostics()
    finally:
        eng.pos[row] = keep
        torch.cuda.synchronize()
    assert d["nan_row"] == (0, row)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        assert eng.save_diagnostics()["nan_row"] is None


def test_without_internal_energy():
    kw = dict(KW, internal_energy=False)
    eng = _engine(DamBreak3D(**kw))
    for _ in range(3):
        eng.step()
    assert not eng.energy_on
    st = _state(eng)
    assert st["energy"] is None
    d = eng.save_diagnostics()
    _check(d, _rule(eng, st), "no internal energy")
    assert not d["energy"][:, 2].any() and (d["energy"][[0, 1, NF], 1] != 0).all() and (d["energy"][[0, 1], 0] > 0).all()


def test_more_rows_than_the_capped_grid_has_threads(small):
    eng, st = small
    k = (1024*256)//eng.n + 1
    big = {name: (None if a is None else np.concatenate([a]*k)) for name, a in st.items()}
    n = len(big["pos"])
    assert n > 1024*256 and n % 256
    big["vel"][n - 3, :3] = (9.0, 0.0, 0.0)                        # the largest speed sits in the last round of the loop
    want = ref.rule(eng.problem, big["pos"], big["vel"], big["info"], big["hash"], big["energy"])
    assert want["max_speed"] == 9.0
    ref.check_out(_raw(eng, big), want, "%d rows" % n)


def test_peak_tracking_and_its_line():
    eng = _engine(DamBreak3D(**KW))
    assert eng.peak_particle_speed == 0 and eng.peak_particle_speed_time == 0
    speeds, times = [], []
    for _ in range(6):
        eng.step()
        speeds.append(eng.save_diagnostics()["max_speed"])
        times.append(eng.time())
    best = int(np.argmax(speeds))                                    # (the first of equals: the update is a strict >)
    assert speeds[best] > 0 and eng.peak_particle_speed == max(speeds) and eng.peak_particle_speed_time == times[best]
    v = float(speeds[best])
    assert eng.peak_speed_line() == ("Peak particle speed was ~%g m/s at %g s -> can set maximum vel %.2g for this problem\n"
                                     % (v, times[best], v*1.1))
    # a slower state later does not move the peak
    eng.vel[:eng.n, :3] *= 0.5
    assert eng.save_diagnostics()["max_speed"] < speeds[best]
    assert eng.peak_particle_speed == speeds[best] and eng.peak_particle_speed_time == times[best]


def test_write_energy(small, tmp_path):
    eng, _ = small
    path = tmp_path / "energy.txt"
    d1 = eng.write_energy(str(path))
    d2 = eng.write_energy(str(path))
    assert _same_bits(d1, d2)
    lines = path.read_text().split("\n")
    assert len(lines) == 4 and lines[3] == ""
    assert lines[0] + "\n" == commonwriter.energy_header(2) and lines[0].count("\t") == 10
    assert lines[1] + "\n" == lines[2] + "\n" == commonwriter.energy_line(eng.time(), d1["energy"], 2)
    assert float(lines[1].split("\t")[-1]) == commonwriter.energy_total(d1["energy"], 2)


@pytest.mark.timeout(300)
def test_two_slabs_add_up_to_the_single_domain(monkeypatch):
    """the arrangement of tests/test_gpu_wave_gages.py: two slabs on the one device, two worker threads, the exchange through
    sphx_halo_*; every slab counts the rows it owns, the sums are all-reduced in double, the largest speed is the larger one"""
    import torch
    from gpusph_amd import capi
    from gpusph_amd.halo import CapiTransport
    from gpusph_amd.multigpu import MultiGpuEngine
    monkeypatch.setenv("SPHX_DISABLE_TILES", "1")
    kw = dict(KW, obstacle=True, linearization="xzy")
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
            d = eng.save_diagnostics()
            own = torch.empty(eng.k.DIAG_DOUBLES, dtype=torch.float64, device=eng.device)
            eng.k.save_diagnostics(own, eng.pos, eng.vel, eng.info, eng.hash, eng.energy, eng.n_int)
            torch.cuda.synchronize()
            out[rank] = (d, own.cpu().numpy(), eng.n_int, eng.n_local)
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

    single = _engine(DamBreak3D(**kw))
    for _ in range(steps):
        single.step()
    st = _state(single)
    want = _rule(single, st)
    d = single.save_diagnostics()
    _check(d, want, "single domain")
    rows = [o[1][:ref.MAXSQ].reshape(-1, 4)[:, 3] for o in out]
    assert np.array_equal(rows[0] + rows[1], want["rows"].astype(np.float64)) and rows[0].sum() > 1000 and rows[1].sum() > 1000
    assert all(o[3] > o[2] for o in out) and out[0][2] + out[1][2] == single.n          # both hold a halo, which is not counted
    for o in out:
        _check(o[0], want, "two slabs")
    assert _same_bits(out[0][0], out[1][0])
