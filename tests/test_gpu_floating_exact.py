"""The exact, order-free body sums of floating bodies on the device (csrc/floating_exact.hip, sphx_floating_limbs /
sphx_floating_move_limbs): the limbs against the format in Python integers (tests/floating_exact_ref.py), array-equal; the totals
against math.fsum BIT FOR BIT, on rows of very mixed size and on rows whose sum is known by reasoning (the whole float range, ties at
53 bits, cancelling pairs, rows that are not finite); limbs of complementary subsets of the rows, added in either order, move the
body with the same bytes as the unsplit call; the default path beside it within its derived bound; whole runs beside the oracle,
without a host read, twice with the same bits; two slabs on one device bit-equal to the single domain; the refusals.
HipKernels of BuoyancyBox(deltap=0.1) with synthetic rows, BuoyancyBox(deltap=0.05) (16 k particles) for runs: every test takes
seconds.  Without the feature the entry points and the exact_sums keyword do not exist."""
import threading

import numpy as np
import pytest
import torch

import floating_exact_ref as fx
import floating_ref as fr
from gpusph_amd import capi, defs as D
from gpusph_amd.problem import BuoyancyBox
from forces_check import _engine
from test_gpu_floating import _bodies, _dev, _kernels, _rows

pytestmark = pytest.mark.gpu
DP = 0.05
DT = np.array([3e-4], dtype=np.float32)


@pytest.fixture(scope="module")
def small():
    return BuoyancyBox(deltap=0.1)


def _limbs_tensor(nf):
    return torch.full((nf, 6, capi.SPHX_FLOATING_LIMBS), -7.0, dtype=torch.float64, device="cuda:0")


def _exact_move(K, rbf, rbt, nf, step=1, d_dt=None):
    """limbs of the rows, then the move: -> the limbs as the device wrote them"""
    L = _limbs_tensor(nf)
    K.floating_limbs(_dev(rbf), _dev(rbt), L)
    got = L.cpu().numpy()
    K.floating_move_limbs(L, step, _dev(DT) if d_dt is None else d_dt)
    return got


@pytest.mark.parametrize("counts", [(0,), (1,), (63,), (64,), (65,), (257,), (16385, 300), (70000,)])
def test_totals_against_fsum_bit_for_bit(small, counts):
    """row counts around the wave and the block, one row over a round of 64 blocks, more than four rounds; two bodies with adjacent
    ranges; rows before the first and behind the last body that are never counted"""
    rng = np.random.default_rng(sum(counts))
    K = _kernels(small)
    bodies = _bodies(len(counts), rng)
    rowstart = np.concatenate([[2], 2 + np.cumsum(counts)]).astype(np.uint32)
    rbf, rbt = _rows(int(rowstart[-1]) + 9, rng)
    rbf[int(rowstart[-1]):, :3] = 7e9; rbf[:2, :3] = -7e9
    K.floating_setup(bodies, rowstart)
    got = _exact_move(K, rbf, rbt, len(counts))
    assert np.array_equal(got, fx.limbs(rbf, rbt, rowstart))
    state = K.floating_state()
    want = fr.fsum_rows(rbf, rbt, rowstart)
    assert fx.same_bits(state[:, 13:19], want), (state[:, 13:19], want)
    assert np.abs(state[:, 13:19]).max() < 1e9
    if counts == (0,):
        assert not state[:, 13:19].any() and not np.signbit(state[:, 13:19]).any()
    else:
        assert np.abs(state[:, 13:19]).min() > 0
    # the rule ran on these totals (floating_ref.check_state, as for the default path)
    ref = fr.RefBodies(bodies, fr.device_grid(small))
    for b in range(len(counts)):
        fr.check_state(state[b], ref.state[b, :13], state[b, 13:19], bodies[b].mass, bodies[b].inertia, ref.grid["gravity"],
                       0.5*float(DT[0]), "body %d" % b)


@pytest.mark.parametrize("which", range(len(fx.KNOWN_BODIES)))
def test_known_answers(small, which):
    """(b) the whole float range in one body: where FLT_MAX cancels, the 2^-149 is kept; (c) ties at 53 bits go to even and the
    smallest float decides them, both signs; (d) pairs x, -x give +0.0; (e) a NaN row, an infinite row, both infinities; the fourth
    component, +-1e30, is never counted"""
    names = fx.KNOWN_BODIES[which]
    rbf, rbt, want = fx.known_rows(names, first=2, behind=3)
    rowstart = np.array([2, len(rbf) - 3], dtype=np.uint32)
    K = _kernels(small)
    K.floating_setup(_bodies(1, np.random.default_rng(which)), rowstart)
    got = _exact_move(K, rbf, rbt, 1)
    assert np.array_equal(got, fx.limbs(rbf, rbt, rowstart))
    state = K.floating_state()
    assert fx.same_bits(state[0, 13:19], want), (names, state[0, 13:19], want)
    for c, name in enumerate(names):
        if name == "range_cancels":
            assert state[0, 13 + c] == 2.0**-149
        if name == "pairs":
            assert state[0, 13 + c] == 0.0 and not np.signbit(state[0, 13 + c])


def test_a_large_body_of_known_rows(small):
    """the known rows many times over (more rows than one round of the grid, so that every block and wave meets every kind):
    limbs against the format, totals against math.fsum"""
    reps = 3000
    rbf, rbt, _ = fx.known_rows(fx.KNOWN_BODIES[0])
    rbf2, rbt2, _ = fx.known_rows(fx.KNOWN_BODIES[1])
    n = min(len(rbf), len(rbf2))
    f = np.tile(np.concatenate([rbf[:n], rbf2[:n]]), (reps, 1)); t = np.tile(np.concatenate([rbt[:n], rbt2[:n]]), (reps, 1))
    extra_f, extra_t, _ = fx.known_rows(fx.KNOWN_BODIES[1])
    f, t = np.concatenate([f, extra_f]), np.concatenate([t, extra_t])
    rowstart = np.array([0, len(f)], dtype=np.uint32)
    assert len(f) > 16384
    K = _kernels(small)
    K.floating_setup(_bodies(1, np.random.default_rng(1)), rowstart)
    got = _exact_move(K, f, t, 1)
    assert np.array_equal(got, fx.limbs(f, t, rowstart))
    assert fx.same_bits(K.floating_state()[:, 13:19], fr.fsum_rows(f, t, rowstart))


def test_split_invariance_on_one_device(small):
    """complementary subsets of the rows (the others zeroed): contiguous halves, alternating rows, thirds.  One floating_limbs per
    subset, the limb tensors added with torch in both orders, one floating_move_limbs: state and slot byte-equal to the unsplit
    call"""
    rng = np.random.default_rng(9)
    bodies = _bodies(2, rng)
    rowstart = np.array([1, 20000, 20500], dtype=np.uint32)
    rbf, rbt = _rows(20500, rng)
    idx = np.arange(20500)
    d_dt = _dev(DT)

    def run(make):
        K = _kernels(small)
        K.floating_setup(bodies, rowstart)
        K.floating_move_limbs(make(K), 1, d_dt)
        return K.floating_state(slots=True)

    def whole(K):
        L = _limbs_tensor(2)
        K.floating_limbs(_dev(rbf), _dev(rbt), L)
        return L
    want = run(whole)
    assert fx.same_bits(want[0][:, 13:19], fr.fsum_rows(rbf, rbt, rowstart))
    for parts in ([idx < 10250, idx >= 10250], [idx % 2 == 0, idx % 2 == 1], [idx % 3 == 0, idx % 3 == 1, idx % 3 == 2]):
        for order in (parts, parts[::-1]):
            def summed(K):
                total = torch.zeros((2, 6, capi.SPHX_FLOATING_LIMBS), dtype=torch.float64, device="cuda:0")
                for keep in order:
                    f, t = rbf.copy(), rbt.copy()
                    f[~keep, :3] = 0.0; t[~keep, :3] = 0.0
                    L = _limbs_tensor(2)
                    K.floating_limbs(_dev(f), _dev(t), L)
                    total = total + L
                return total.contiguous()
            got = run(summed)
            assert np.array_equal(got[0].view(np.uint64), want[0].view(np.uint64))
            for k in want[1]:
                assert np.array_equal(got[1][k].view(np.uint32), want[1][k].view(np.uint32)), k


def test_beside_the_default_path(small):
    """the same rows through floating_move: its totals, n double additions in some order, are within n 2^-52 sum|term| of the exactly
    rounded sum (floating_ref.check_totals' bound, derived, not measured), which is what the exact path gives; and the default
    path's bits are its own as before (same rows twice: same bits)"""
    rng = np.random.default_rng(4)
    bodies = _bodies(2, rng)
    rowstart = np.array([0, 30000, 30700], dtype=np.uint32)
    rbf, rbt = _rows(30700, rng)
    d_dt = _dev(DT)
    K = _kernels(small)
    K.floating_setup(bodies, rowstart)
    _exact_move(K, rbf, rbt, 2)
    exact = K.floating_state()
    states = []
    for _ in range(2):
        K2 = _kernels(small)
        K2.floating_setup(bodies, rowstart)
        K2.floating_move(_dev(rbf), _dev(rbt), 1, d_dt)
        states.append(K2.floating_state())
    assert np.array_equal(states[0].view(np.uint64), states[1].view(np.uint64))
    want = fr.check_totals(states[0][:, 13:19], rbf, rbt, rowstart, "default path")
    assert fx.same_bits(exact[:, 13:19], want)
    for b in range(2):
        r0, r1 = int(rowstart[b]), int(rowstart[b + 1])
        rows = np.concatenate([rbf[r0:r1, :3], rbt[r0:r1, :3]], axis=1).astype(np.float64)
        assert (np.abs(states[0][b, 13:19] - exact[b, 13:19]) <= (r1 - r0)*fr.ULP*np.abs(rows).sum(axis=0)).all()


# ---- whole runs
def test_a_run_beside_the_oracle():
    """test_gpu_floating.py's "12 steps beside the oracle" with the exact sums, DYN_BOUNDARY, that test's bounds: every forces pass is
    within 2e-5 max|F| per row of the oracle's, a body row within that times the particle's mass, a total over `rows` rows within rows
    times that, the velocity after k substeps within k dt rows 2e-5 max|F_row| m_p / M, doubled for the feedback, the position within
    that times the elapsed time (the oracle sums with math.fsum: the exact path's own known answer)"""
    pr = BuoyancyBox(deltap=DP, exact_sums=True)
    eng = _engine(pr); sim = fr.FloatingOracleSim(pr)
    assert eng.floating_exact
    steps, M, rows, m_p = 12, pr.floating_bodies[0].mass, pr.num_obstacle, float(pr.parts.pos_global[0, 3])
    dtmax, frow = 0.0, 0.0
    for k in range(1, steps + 1):
        dtmax = max(dtmax, sim.dt)
        eng.step(); sim.step()
        frow = max(frow, float(np.abs(sim.forces[:sim.n, :3]).max()))
        s = eng.floating_state()[0]
        bound_v = 2*(2*k)*dtmax*(rows*2e-5*frow*m_p)/M
        dv, dx = np.abs(s[7:10] - sim.fl.state[0, 7:10]).max(), np.abs(s[0:3] - sim.fl.state[0, 0:3]).max()
        assert dv <= bound_v and dx <= bound_v*sim.t, (k, dv, dx, bound_v)
    out = eng.download()
    n = eng.n
    assert n == sim.n and np.array_equal(out["hash"], sim.hash[:n]) and np.array_equal(out["info"], sim.info[:n])
    cs = float(min(pr.m_cellsize))
    assert np.abs(out["pos"][:, :3] - sim.pos[:n, :3]).max() <= 1e-6*cs*steps
    assert np.abs(out["vel"][:, :3] - sim.vel[:n, :3]).max() <= 1e-3*np.abs(sim.vel[:n, :3]).max()
    assert abs(eng.time() - sim.t) <= 1e-6*sim.t
    assert frow > 0 and abs(sim.fl.state[0, 2] - pr.CENTRE[2]) > 1e-5
    # the totals of the last substep are the exactly rounded sums of the rows the last forces pass left
    rbf, rbt = eng.rbforces.cpu().numpy(), eng.rbtorques.cpu().numpy()
    assert fx.same_bits(eng.floating_state()[:, 13:19], fr.fsum_rows(rbf, rbt, pr.rb_rowstart))


def test_no_host_read_in_a_step_and_the_same_bits_twice(monkeypatch):
    """three steps with every way of reading a tensor to the host and the library's synchronous entry points patched to raise; a
    second engine without the patches ends with the same bits"""
    def make():
        return _engine(BuoyancyBox(deltap=DP, exact_sums=True), track_particle_count=False)
    eng = make()

    def refuse(*a, **k):
        raise AssertionError("a step read from the device")
    for name in ("item", "cpu", "tolist", "numpy"):
        monkeypatch.setattr(torch.Tensor, name, refuse)
    for name in ("sphx_forces_dtreduce", "sphx_reduce_rb_forces", "sphx_floating_state", "sphx_neibs_getinfo", "sphx_device_synchronize",
                 "sphx_memcpy_d2h", "sphx_floating_move"):
        monkeypatch.setattr(eng.lib, name, refuse)
    monkeypatch.setattr(type(eng.k), "neibs_info", refuse)
    monkeypatch.setattr(type(eng), "reduce_rb_forces", refuse)
    monkeypatch.setattr(type(eng), "current_dt", refuse)
    for _ in range(3):
        eng.step()
    monkeypatch.undo()
    s = eng.floating_state()
    assert eng.iterations == 3 and s[0, 2] > BuoyancyBox.CENTRE[2] and np.isfinite(s).all()
    again = make()
    for _ in range(3):
        again.step()
    assert np.array_equal(again.floating_state().view(np.uint64), s.view(np.uint64))
    a, b = eng.download(), again.download()
    for k in ("pos", "vel", "info", "hash"):
        assert np.array_equal(np.asarray(a[k]).view(np.uint8), np.asarray(b[k]).view(np.uint8)), k


@pytest.mark.timeout(300)
def test_two_slabs_move_the_cube_with_the_bits_of_the_single_domain(monkeypatch):
    """the arrangement of tests/test_gpu_halo.py: two slabs on the one device, two worker threads, the exchange and the all-reduce of
    the limbs through sphx_halo_*.  The cube (y in [0.3, 0.7]) straddles the cut of a split along y, which is asserted on the ranks'
    own rows; 12 steps across the rebuild at iteration 10; the body's state on both ranks and the gathered particles are bit-equal
    to the single domain with exact sums"""
    from gpusph_amd.halo import CapiTransport
    from gpusph_amd.multigpu import MultiGpuEngine
    monkeypatch.setenv("SPHX_DISABLE_TILES", "1")
    kw = dict(deltap=DP, linearization="xzy", exact_sums=True)
    steps = 12
    lib = capi.load()
    group = CapiTransport.new_group(lib, 2)
    out, errors = [None, None], []

    def worker(rank):
        try:
            torch.cuda.set_device(0)
            eng = MultiGpuEngine(BuoyancyBox(**kw), "cuda:0", rank, 2, transport=lambda k: CapiTransport(k, rank, 2, group=group))
            owned = []
            for _ in range(steps):
                eng.step()
                info = eng.info[:eng.n_int].cpu().numpy().view(np.uint16).reshape(-1, 4)
                owned.append(int(((info[:, 0] & D.FG_COMPUTE_FORCE) != 0).sum()))
            torch.cuda.synchronize()
            out[rank] = (eng.download_internal(), eng.floating_state(slots=True), owned, eng.current_dt(), eng.n_int, eng.n_local)
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

    ref = _engine(BuoyancyBox(**kw))
    for _ in range(steps):
        ref.step()
    want, wstate = ref.download_internal(), ref.floating_state(slots=True)
    nbody = ref.problem.num_obstacle
    for a, b in zip(out[0][2], out[1][2]):      # in every step both ranks own body particles, and together all of them
        assert a > 0 and b > 0 and a + b == nbody, (out[0][2], out[1][2])
    assert all(o[5] > o[4] for o in out) and out[0][4] + out[1][4] == ref.n
    ident = lambda info: info[:, 2].astype(np.uint32) | (info[:, 3].astype(np.uint32) << 16)
    ids = np.concatenate([ident(o[0]["info"]) for o in out])
    order, worder = np.argsort(ids), np.argsort(ident(want["info"]))
    assert np.array_equal(ids[order], ident(want["info"])[worder])
    for k in ("pos", "vel", "forces"):
        got = np.concatenate([o[0][k] for o in out])[order]
        assert np.array_equal(got.view(np.uint32), want[k][worder].view(np.uint32)), k
    for o in out:
        assert o[3] == ref.current_dt()
        assert np.array_equal(o[1][0].view(np.uint64), wstate[0].view(np.uint64))
        for k in wstate[1]:
            assert np.array_equal(o[1][1][k].view(np.uint32), wstate[1][k].view(np.uint32)), k
    assert wstate[0][0, 2] > BuoyancyBox.CENTRE[2] + 1e-6 and np.isfinite(wstate[0]).all()


def test_refusals(small):
    from gpusph_amd.multigpu import MultiGpuEngine
    with pytest.raises(NotImplementedError, match="exact body sums"):      # several slabs ask for the exact sums
        MultiGpuEngine(BuoyancyBox(deltap=0.1), "cuda:0", 0, 2)
    K = _kernels(small)
    L = _limbs_tensor(1)
    rbf, rbt = (_dev(a) for a in _rows(10, np.random.default_rng(2)))
    d_dt = _dev(DT)
    H = K.ctx.handle
    for call in (lambda: K.lib.sphx_floating_limbs(H, capi.ptr(rbf), capi.ptr(rbt), capi.ptr(L), K._s()),
                 lambda: K.lib.sphx_floating_move_limbs(H, capi.ptr(L), 1, capi.ptr(d_dt), K._s())):
        with pytest.raises(capi.SphxInvalidArgument, match="no floating bodies"):
            capi.check(call())
    K.floating_setup(_bodies(1, np.random.default_rng(1)), np.array([0, 10], dtype=np.uint32))
    seen = set()
    for call, text in ((lambda: K.lib.sphx_floating_limbs(H, None, capi.ptr(rbt), capi.ptr(L), K._s()), "missing buffer"),
                       (lambda: K.lib.sphx_floating_limbs(H, capi.ptr(rbf), None, capi.ptr(L), K._s()), "missing buffer"),
                       (lambda: K.lib.sphx_floating_limbs(H, capi.ptr(rbf), capi.ptr(rbt), None, K._s()), "NULL d_limbs"),
                       (lambda: K.lib.sphx_floating_move_limbs(H, capi.ptr(L), 0, capi.ptr(d_dt), K._s()), "step is 1"),
                       (lambda: K.lib.sphx_floating_move_limbs(H, capi.ptr(L), 3, capi.ptr(d_dt), K._s()), "step is 1"),
                       (lambda: K.lib.sphx_floating_move_limbs(H, capi.ptr(L), 1, None, K._s()), "missing buffer"),
                       (lambda: K.lib.sphx_floating_move_limbs(H, None, 1, capi.ptr(d_dt), K._s()), "NULL d_limbs")):
        with pytest.raises(capi.SphxInvalidArgument, match=text) as e:
            capi.check(call())
        seen.add(str(e.value))
    assert len(seen) == 5      # each refusal has a message of its own, naming its entry point
    # a refused call left the state alone, and both entry points still work
    before = K.floating_state()
    _exact_move(K, rbf.cpu().numpy(), rbt.cpu().numpy(), 1)
    assert not np.array_equal(K.floating_state()[:, :13], before[:, :13])
