"""What the post-processing of a run with SA walls and the wave gages cost per call, on the SABox tank with a few probes: the numbers
of profiles/sa_postprocess_time.txt.  Three alternating rounds of
  * the three SA post-processing kernels (vorticity, surface detection with normals, test points),
  * sphx_wave_gages + sphx_wave_gages_finish with 12 gages (device time), and Engine.wave_gages() as a user calls it (with the
    upload of the gages, the read-back of 12 doubles and its synchronisation; the surface flags are current),
  * the reference's way: Engine.download() of the state plus the gage rule in numpy on the host copy.
usage: python scripts/time_postprocess.py [deltap] [calls per round]

python scripts/time_postprocess.py diagnostics [particles] [calls per round]: the save-time diagnostics (energies per fluid, peak
particle speed) on the DamBreak3D of bench.py, the numbers of profiles/save_diagnostics.txt.  Three alternating rounds of
  * sphx_save_diagnostics (device time of its two kernels), with the bytes it reads over that time as a share of the HBM bandwidth
    a streaming kernel reaches on this device (6.3 TB/s),
  * Engine.save_diagnostics() as a user calls it (with the read-back of 24 doubles and its synchronisation),
  * the reference's way: Engine.download() of the state plus the rule in numpy on the host copy."""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from gpusph_amd import defs as D
from gpusph_amd.problem import DamBreak3D, SAProbeBox
from gpusph_amd.engine import TimestepEngine


DIAG = len(sys.argv) > 1 and sys.argv[1] == "diagnostics"
if DIAG:
    del sys.argv[1]
calls = int(sys.argv[2]) if len(sys.argv) > 2 else 20


def device_ms(f):
    f(); torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ev[0].record()
    for _ in range(calls):
        f()
    ev[1].record(); torch.cuda.synchronize()
    return ev[0].elapsed_time(ev[1])/calls


def host_ms(f, reps):
    f(); torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(reps):
        out = f()
    torch.cuda.synchronize()
    return (time.perf_counter() - t)/reps*1e3, out


HBM_ACHIEVABLE = 6.3e12      # bytes/s of a streaming kernel on an MI355X (a float4 copy)


def diagnostics(particles):
    t0 = time.time()
    dp = DamBreak3D.deltap_for(particles)
    prob = DamBreak3D(dp, obstacle=True)
    eng = TimestepEngine(prob, device="cuda:0")
    eng.run(3)
    torch.cuda.synchronize()
    n = eng.n
    row = 44 + (4 if eng.energy_on else 0)
    print("DamBreak3D deltap %g: %d particles, %d B per particle (POS, VEL, INFO, HASH%s); %d calls per round; set-up %.0f s"
          % (dp, n, row, ", INTERNAL_ENERGY" if eng.energy_on else "", calls, time.time() - t0), flush=True)
    out = torch.zeros(eng.k.DIAG_DOUBLES, dtype=torch.float64, device=eng.device)
    energy = eng.energy if eng.energy_on else None
    g = np.asarray(prob.physparams.gravity, dtype=np.float32).astype(np.float64)

    def reference_way():
        st = eng.download()
        cell = prob.grid_pos_from_hash(st["hash"])
        gp = prob.m_cellsize.astype(np.float32).astype(np.float64)*(cell + 0.5) + st["pos"][:, :3].astype(np.float64) \
            + prob.m_origin.astype(np.float32).astype(np.float64)
        info = st["info"].reshape(-1, 4)
        m = st["pos"][:, 3].astype(np.float64)
        v = st["vel"]
        sq = v[:, 0]*v[:, 0] + v[:, 1]*v[:, 1] + v[:, 2]*v[:, 2]
        cls = np.where((info[:, 0] & 7) == D.PT_FLUID, info[:, 1] >> 12, D.MAX_FLUID_TYPES)
        e = np.zeros((D.MAX_FLUID_TYPES + 1, 3))
        for k, term in enumerate((m*(sq/np.float32(2)), -m*(gp[:, 0]*g[0] + gp[:, 1]*g[1] + gp[:, 2]*g[2]))):
            e[:, k] = np.bincount(cls, weights=term, minlength=D.MAX_FLUID_TYPES + 1)
        return e, np.sqrt(sq.max())

    for rnd in range(3):
        k = device_ms(lambda: eng.k.save_diagnostics(out, eng.pos, eng.vel, eng.info, eng.hash, energy, n))
        e, d = host_ms(eng.save_diagnostics, calls)
        r, (e_ref, v_ref) = host_ms(reference_way, 1)
        rel = np.abs(d["energy"][:, :2] - e_ref[:, :2]).max()/np.abs(e_ref).max()
        print("round %d  sphx_save_diagnostics %7.3f ms (%.2f TB/s, %.0f %% of %.1f TB/s)  Engine.save_diagnostics() %7.3f  "
              "download() + numpy rule %9.1f   ms per call   (device against host: largest difference %.2g of the largest energy, "
              "speed %s)" % (rnd, k, row*n/k/1e9, 100*row*n/(k*1e-3)/HBM_ACHIEVABLE, HBM_ACHIEVABLE/1e12, e, r, rel,
                             "equal" if d["max_speed"] == v_ref else "%g against %g" % (d["max_speed"], v_ref)), flush=True)
    print(eng.peak_speed_line(), end="")


if DIAG:
    diagnostics(float(sys.argv[1]) if len(sys.argv) > 1 else 32e6)
    sys.exit(0)

dp = float(sys.argv[1]) if len(sys.argv) > 1 else 0.008
t0 = time.time()
L, W, Hh, H = 1.6, 1.6, 1.0, 0.8
rng = np.random.default_rng(3)
probes = np.column_stack([rng.uniform(0.1, L - 0.1, 8), rng.uniform(0.1, W - 0.1, 8), rng.uniform(0.05, H - 0.05, 8)])
gages = [(x, y, 0.0 if k % 3 == 2 else 4*dp) for k, (x, y) in enumerate(zip(rng.uniform(0.2, L - 0.2, 12), rng.uniform(0.2, W - 0.2, 12)))]
prob = SAProbeBox(dp, l=L, w=W, h=Hh, H=H, options="Spheric2SA", testpoints=probes, gages=gages)
eng = TimestepEngine(prob, device="cuda:0")
eng.run(3)
torch.cuda.synchronize()
n = eng.n
print("SAProbeBox Spheric2SA, deltap %g: %d particles, 8 probes, 12 gages (4 in nearest mode); %d calls per round; set-up %.0f s"
      % (dp, n, calls, time.time() - t0), flush=True)


g = np.array(prob.gages)
d_g = torch.from_numpy(g).to(eng.device)
part = torch.zeros((len(g), 4), dtype=torch.float64, device=eng.device)
z = torch.zeros(len(g), dtype=torch.float64, device=eng.device)


def gage_kernels():
    eng.k.wave_gages(part, d_g, len(g), eng.pos, eng.info, eng.hash, n)
    eng.k.wave_gages_finish(z, part, d_g, len(g))


def reference_way():
    st = eng.download()
    # calcGlobalPosOffset: the float cell size and world origin widened to double, as the device forms it
    cell = prob.grid_pos_from_hash(st["hash"])
    gp = prob.m_cellsize.astype(np.float32).astype(np.float64)*(cell + 0.5) + st["pos"][:, :3].astype(np.float64) \
        + prob.m_origin.astype(np.float32).astype(np.float64)
    surf = (st["info"].reshape(-1, 4)[:, 0] & D.FG_SURFACE) != 0
    p = gp[surf]
    out = np.zeros(len(g))
    for k, (gx, gy, _, h) in enumerate(g):
        r = np.sqrt((p[:, 0] - gx)**2 + (p[:, 1] - gy)**2)
        if h > 0:
            m = r < 2*h
            q = r[m]/h
            w = 7.0/(4.0*np.pi*h*h)*(1 - q/2)**4*(2*q + 1)
            out[k] = (p[m, 2]*w).sum()/w.sum() if m.any() else np.nan
        else:
            out[k] = p[np.argmin(r), 2]
    return out


for rnd in range(3):
    v = device_ms(lambda: eng.postprocess(D.VORTICITY))
    s = device_ms(lambda: eng.postprocess(D.SURFACE_DETECTION, normals=True))
    t = device_ms(lambda: eng.postprocess(D.TESTPOINTS))
    k = device_ms(gage_kernels)
    e, z_dev = host_ms(eng.wave_gages, calls)
    r, z_ref = host_ms(reference_way, 3)
    ok = "largest relative difference %.2g" % np.nanmax(np.abs(z_dev - z_ref)/np.abs(z_ref))
    print("round %d  vorticity %7.3f  surface detection %7.3f  test points %7.3f  gage kernels %7.3f  Engine.wave_gages() %7.3f  "
          "download() + numpy gage rule %9.1f   ms per call   (device against host: %s)" % (rnd, v, s, t, k, e, r, ok), flush=True)
surf = int(((eng.info[:n, 0].to(torch.int32) & D.FG_SURFACE) != 0).sum().item())
print("surface particles: %d of %d; bytes of INFO read by the gage pass: %.1f MB" % (surf, n, 8*n/1e6))
