"""An overflowed forces tiling must fall back on every pass.

Which implementation of a hot pass does the work -- the LDS-tiled kernel or the list-walking one behind it -- is decided on the
device by tile_ctl[1], the overflow flag of the last neighbour-list build; the host follows without waiting (sphx_ctx::tiles_overflow
-1 / 0 / 1, sphx_tiles_current, sphx_tiles_standby_guard in csrc/sphx_internal.h).  With the flag raised the tiled kernels return at
once, the SA wall kernels return, and the stand-by or the walker does the WHOLE pass.  So a context with tiles enabled must produce,
bit for bit, what a context created under SPHX_DISABLE_TILES=1 produces on the same inputs: forces, stress tensor, dt, densities,
gamma and whole trajectories.  No tolerance is involved; a mistake here (a stale cache, a row summed twice, a CFL slot nobody
wrote) shows as a differing word.

The cases are tests/tiling_overflow_cases.py's; tests/test_tiling_overflow_cases.py proves on the CPU oracle that their neighbour
lists fit and their tilings cannot.  Every engine here asserts the former (neibs_info) before its first forces pass."""
import numpy as np
import pytest

import tiling_overflow_cases as toc
from forces_check import _check_neibs_and_forces, tiles_usable

pytestmark = pytest.mark.gpu


def _engine(prob, monkeypatch, disable_tiles, **kw):
    from gpusph_amd.engine import TimestepEngine
    monkeypatch.setenv("SPHX_DISABLE_TILES", "1" if disable_tiles else "0")      # read when the context is created
    return TimestepEngine(prob, device="cuda:0", clobber_neibslist=True, **kw)


def _host_state(eng):
    """what the host knows of the tiling's overflow flag: -1 not seen yet, 0 usable, 1 overflowed.  Waits for nothing"""
    return int(eng.k.lib.sphx_dbg_tiles_host_state(eng.k.ctx.handle))


def _bits(t, n):
    return t.cpu().numpy()[:n].view(np.uint32).copy()


def _perturb(eng, seed=11):
    """the seeded velocity / density perturbation of the parity tests, on the sorted rows: velocities of the fluid, densities of all"""
    import torch
    n = eng.n
    rng = np.random.default_rng(seed)
    vel = eng.vel.cpu().numpy().copy()
    fluid = (eng.info.cpu().numpy().view(np.uint16)[:n, 0] & 7) == 0
    vel[:n][fluid, :3] += rng.uniform(-0.3, 0.3, size=(int(fluid.sum()), 3)).astype(np.float32)
    vel[:n, 3] += rng.uniform(0, 2e-3, size=n).astype(np.float32)
    eng.vel.copy_(torch.from_numpy(vel).to(eng.device))


def _checked_build(eng):
    eng.build_neibs()
    info = eng.neibs_info()      # raises on a list that did not fit
    assert info.hasTooManyNeibs == -1
    return info


def _launch(eng):
    """one forces pass (with SPS: the stress pass before it), enqueued only"""
    eng._forces(eng.pos, eng.vel, 1, 0)


def _result(eng):
    """-> bits of the forces, the next dt, bits of the stress tensor, bits of the body rows"""
    n = eng.n
    tau = np.concatenate([_bits(t, n) for t in eng.tau], axis=1) if eng.tau else np.zeros((n, 6), np.uint32)
    rb = (np.concatenate([_bits(eng.rbforces, len(eng.rbforces)), _bits(eng.rbtorques, len(eng.rbtorques))]) if eng.has_rb
          else np.zeros((0, 4), np.uint32))
    return _bits(eng.forces, n), float(eng.d_dt_next.item()), tau, rb


def _pass(eng):
    _launch(eng)
    return _result(eng)


def _same(a, b):
    return all(np.array_equal(x, y) if isinstance(x, np.ndarray) else x == y for x, y in zip(a, b))


def _differing(a, b):
    return "forces %d of %d words, dt %r | %r, stress %d of %d words, body rows %d words" % (
        int((a[0] != b[0]).sum()), a[0].size, a[1], b[1], int((a[2] != b[2]).sum()), a[2].size, int((a[3] != b[3]).sum()))


def _keep_the_device_busy(eng):
    """some ten milliseconds of fills (40 GiB written) in front of what the host enqueues next, so that the host gets to the forces
    pass before the device gets to the tiling of the build: the pass then finds the overflow flag `not seen yet`"""
    import torch
    pad = torch.empty(1 << 28, dtype=torch.uint8, device=eng.device)
    for k in range(160):
        pad.fill_(k)
    return pad


SINGLE = ["gaussian", "gaussian-sps", "clump"] + ["wide-" + k for k in toc.WIDE_VARIANTS]


@pytest.mark.parametrize("case", SINGLE)
def test_single_passes_on_an_overflowed_tiling(case, monkeypatch):
    """a. the pass behind a build (the host has not seen the flag: tiled launch + guarded stand-by) and the passes after the host
    has seen it (no tiled launch at all) are the generic context's, to the bit"""
    import torch
    make = toc.CASES[case]
    # no read-back of the particle count inside build_neibs (none of these problems loses particles): nothing between the build
    # and the pass behind it makes the host wait
    gen = _engine(make(), monkeypatch, True, track_particle_count=False)
    _checked_build(gen)
    assert tiles_usable(gen) == 0
    _perturb(gen)
    gen.build_neibs()
    G = _pass(gen)
    assert _same(_pass(gen), G)      # the generic kernels repeat themselves
    sps = gen.sps
    f = G[0].view(np.float32)
    assert np.isfinite(f).all() and np.abs(f[:, :3]).max() > 0 and np.abs(f[:, 3]).max() > 0 and np.isfinite(G[1]) and G[1] > 0
    if sps:
        t = G[2].view(np.float32)
        assert np.isfinite(t).all() and np.abs(t).max() > 0
    del gen

    eng = _engine(make(), monkeypatch, False, track_particle_count=False)
    _checked_build(eng)
    assert tiles_usable(eng) == 0
    _perturb(eng)
    pad = _keep_the_device_busy(eng)
    eng.build_neibs()
    assert _host_state(eng) == -1      # a build forgets what the host knew
    _launch(eng)
    seen = _host_state(eng)            # what the pass just enqueued went by
    P1 = _result(eng)
    print("%s: host state at the pass behind the build %d" % (case, seen))
    assert _same(P1, G), "the pass behind the build: " + _differing(P1, G)
    assert seen == -1, "the host had seen the flag before the pass behind the build: the guarded stand-by was not exercised"
    torch.cuda.synchronize()
    del pad
    for k in (2, 3):
        _launch(eng)
        assert _host_state(eng) == 1   # seen: these passes launch no tiled kernel
        P = _result(eng)
        assert _same(P, G), "pass %d: " % k + _differing(P, G)
    assert tiles_usable(eng) == 0


@pytest.mark.parametrize("case", ["wide-plain", "clump"])
def test_overflowed_tiling_against_the_oracle(case, monkeypatch):
    """b. the checks of the option tests (list bit-exact against the oracle, forces and dt within 2e-5 of it, tiled context
    against generic context) on a tiling that overflowed by the list-length trigger (wide) and by build_tiles_kernel's (clump)"""
    _check_neibs_and_forces(toc.CASES[case](), 51, monkeypatch, usable=0)


def _load(eng, arrs):
    """a problem's initial state (Problem.copy_to_array) into the buffers of an engine that has not stepped yet"""
    import torch
    n = len(arrs["hash"])
    assert n == eng.n and eng.iterations == 0
    eng.pos[:n].copy_(torch.from_numpy(arrs["pos"]).to(eng.device))
    eng.vel[:n].copy_(torch.from_numpy(arrs["vel"]).to(eng.device))
    eng.info[:n].copy_(torch.from_numpy(arrs["info"].view(np.int16)).to(eng.device))
    eng.hash[:n].copy_(torch.from_numpy(arrs["hash"].view(np.int32)).to(eng.device))


def test_a_rebuild_recovers_from_overflow(monkeypatch):
    """c. one tiled context: a state that tiles, the clumped state (overflow), the first state again.  The tiling is back with the
    rebuild, and with it the tiled kernels' own bits"""
    states = []
    for k, prob in enumerate((toc.unclumped(), toc.clump())):
        a = prob.copy_to_array()
        rng = np.random.default_rng(61 + k)
        fluid = (a["info"][:, 0] & 7) == 0
        a["vel"][fluid, :3] += rng.uniform(-0.3, 0.3, size=(int(fluid.sum()), 3)).astype(np.float32)
        a["vel"][:, 3] += rng.uniform(0, 2e-3, size=len(fluid)).astype(np.float32)
        states.append(a)
    A, B = states
    gen = _engine(toc.clump(), monkeypatch, True)
    G = []
    for a in (A, B):
        _load(gen, a)
        _checked_build(gen)
        G.append(_pass(gen))
        assert _same(_pass(gen), G[-1])
    del gen

    eng = _engine(toc.clump(), monkeypatch, False)
    _load(eng, A)
    _checked_build(eng)
    assert tiles_usable(eng) == 1
    T0 = _pass(eng)
    print("tiled against generic on the state that tiles: " + _differing(T0, G[0]))
    assert (T0[0] != G[0][0]).any(), "the tiled and the generic forces agree to the bit: this test cannot see which of them ran"
    _load(eng, B)
    _checked_build(eng)
    assert tiles_usable(eng) == 0
    P = _pass(eng)
    assert _same(P, G[1]), "overflowed: " + _differing(P, G[1])
    P = _pass(eng)
    assert _same(P, G[1]), "overflowed, second pass: " + _differing(P, G[1])
    _load(eng, A)
    _checked_build(eng)
    assert tiles_usable(eng) == 1
    P = _pass(eng)
    assert _same(P, T0), "recovered: " + _differing(P, T0)


STEPS = 12
TRAJECTORIES = ["gaussian", "wide-sps"] + ["sa-wide-" + k for k in toc.SA_VARIANTS]


def _words(t):
    import torch
    return t.contiguous().view(torch.int32)


def _tape_gamma_quadrature(eng, tape, replay):
    """The one pass of an SA run that differs between the two contexts for a reason other than the flag: the gamma quadrature of a
    continuity-equation run (sphx_sa_integrate_gamma, sa_bounds.hip) has no tiled part, so it does not ask about the tiling at all.
    It takes its wave-per-particle wall kernel (sa_integrate_gamma_wall_kernel: one element per lane, summed across the wave)
    whenever the context was not created with SPHX_DISABLE_TILES=1, overflow or not, and the one-thread walker otherwise: the same
    terms summed in another order.  So that pass is compared by its INPUTS, call by call, and the generic context goes on from the
    output the other context's call had; every other pass of the run stays held to the bit by the final state.
    replay False: record (old gamma, new positions, new gamma) of every call in `tape`; True: check the inputs against the tape and
    put the taped output in place of the own one.  -> [calls so far, words in which own output and tape differed]"""
    import torch
    inner = eng.k.sa_integrate_gamma
    stat = [0, 0]

    def wrapped(new_ggam, old_ggam, new_pos, *a, **kw):
        inner(new_ggam, old_ggam, new_pos, *a, **kw)
        if replay:
            og, ps, out = tape[stat[0]]
            assert torch.equal(_words(old_ggam), _words(og)) and torch.equal(_words(new_pos), _words(ps)), \
                "gamma quadrature, call %d: the two contexts hand it different inputs" % stat[0]
            stat[1] += int((_words(new_ggam) != _words(out)).sum().item())
            new_ggam.copy_(out)
        else:
            tape.append((old_ggam.clone(), new_pos.clone(), new_ggam.clone()))
        stat[0] += 1
    eng.k.sa_integrate_gamma = wrapped
    return stat


def _trajectory(prob, monkeypatch, disable_tiles, tape):
    """STEPS steps (a rebuild at step 10; with open boundaries in every step) -> every buffer of the final state, as bytes"""
    eng = _engine(prob, monkeypatch, disable_tiles)
    quad = _tape_gamma_quadrature(eng, tape, replay=disable_tiles) if eng.sa else None
    _checked_build(eng)
    freq = int(prob.simparams.buildneibsfreq)
    for s in range(STEPS):
        eng.step()
        if s % freq == 0:      # this step began with a build
            assert tiles_usable(eng) == 0
            info = eng.neibs_info()
            assert info.hasTooManyNeibs == -1
    out = dict(eng.download())
    n = eng.n
    out["dt"] = eng.d_dt.cpu().numpy(); out["dt_next"] = eng.d_dt_next.cpu().numpy(); out["t"] = eng.d_t.cpu().numpy()
    if eng.tau:
        for k, t in enumerate(eng.tau):
            out["tau%d" % k] = t[:n].cpu().numpy()
    if eng.io:
        out["eulervel"] = eng.eulervel[:n].cpu().numpy(); out["next_ids"] = eng.next_ids[:n].cpu().numpy()
    if quad is not None and disable_tiles:
        assert quad[0] == len(tape)
        print("gamma quadrature: %d calls, the walker's output differs from the wall kernel's in %d words in all" % (quad[0], quad[1]))
    return n, {k: np.ascontiguousarray(v).view(np.uint8).copy() for k, v in out.items()}


@pytest.mark.parametrize("case", TRAJECTORIES)
def test_trajectories_on_an_overflowed_tiling(case, monkeypatch):
    """d. tiles enabled against SPHX_DISABLE_TILES=1 over a rebuild: everything download() returns (with SA walls: gamma and its
    gradient, the boundary elements) and the time step, bit for bit.  With SA walls this pins the density summation, the Brezzi /
    Ferrari diffusion, the forces, the wall kernels' early returns and the walker's whole-pass branch to the flag at once.
    The gamma quadrature of the continuity-equation variant does not follow the flag: see _tape_gamma_quadrature"""
    make = toc.CASES[case]
    tape = []
    nt, got = _trajectory(make(), monkeypatch, False, tape)
    ng, want = _trajectory(make(), monkeypatch, True, tape)
    assert len(tape) == (2*STEPS if case == "sa-wide-ferrari" else 0)      # the quadrature is that variant's alone
    assert nt == ng and sorted(got) == sorted(want)
    vel = want["vel"].view(np.float32).reshape(-1, 4)
    assert np.isfinite(vel).all() and np.abs(vel[:, :3]).max() > 0
    diff = {k: int((got[k] != want[k]).sum()) for k in want if not np.array_equal(got[k], want[k])}
    assert not diff, "bytes that differ from the run without tiles: %r" % diff
