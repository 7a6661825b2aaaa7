#!/usr/bin/env python3
"""What the exact, order-free body sums of floating bodies (csrc/floating_exact.hip) cost, by HIP events on the device:
  step     ms/step of BuoyancyBox at about --particles particles with the default sums (floating_move) and with exact_sums=True
           (floating_limbs + floating_move_limbs), alternating, --reps repetitions of --steps steps from a fresh engine each
  baseline the same with the default sums alone: what a commit without the exact sums can run, so that a copy of this script in a
           checkout of such a commit gives the baseline under its own --label
  kernels  the body's own launches alone on synthetic rows, for bodies of --rows rows: floating_move (partials + step) against
           floating_limbs + floating_move_limbs (limbs + finish + round + step), --calls calls per timing, microseconds per call
  slabs    two slabs on the one device (two worker threads, the exchange and the all-reduce of the limbs through sphx_halo_*,
           forces without tiles as that arrangement needs) against the single domain under the same setting: ms/step by the host
           clock around a device synchronise, both ranks
Every timing is taken after --warmup steps (or calls).  The result is appended to --out with --label in front of every line.

    python scripts/measure_floating_slabs.py [--cases step,baseline,kernels,slabs] [--particles 0.95e6] [--steps 50] [--reps 3] [--label this]
"""
import argparse
import os
import sys
import threading
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--particles", type=float, default=0.95e6)
    ap.add_argument("--slab-particles", type=float, default=0.95e6)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--calls", type=int, default=2000)
    ap.add_argument("--rows", default="1000,20000,100000")
    ap.add_argument("--cases", default="step,kernels,slabs")
    ap.add_argument("--label", default="this commit")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "floating_slabs.txt"))
    a = ap.parse_args()
    import torch
    from gpusph_amd import capi, problem as P
    from gpusph_amd.engine import TimestepEngine
    from measure_floating import buoyancy_deltap
    assert torch.cuda.is_available(), "a measurement needs the device"
    cases = a.cases.split(",")
    lines = []

    def timed_steps(eng, steps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        eng.run(steps)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)/steps

    if "step" in cases or "baseline" in cases:
        variants = (False, True) if "step" in cases else (False,)
        dp = buoyancy_deltap(a.particles)
        ms, n, rows = {False: [], True: []}, 0, 0
        for _ in range(a.reps):
            for exact in variants:
                eng = TimestepEngine(P.BuoyancyBox(dp, **(dict(exact_sums=True) if exact else {})), device="cuda:0", track_particle_count=False)
                n, rows = eng.n, eng.problem.num_obstacle
                eng.run(a.warmup)
                ms[exact].append(timed_steps(eng, a.steps))
                del eng
        for exact in variants:
            v = np.array(ms[exact])
            lines.append("%s: step    BuoyancyBox, %-26s %8d particles, %6d body rows  %d steps x %d: %s ms/step, median %.4f, spread %.4f"
                         % (a.label, "exact sums" if exact else "default sums (double)", n, rows, a.steps, a.reps,
                            " ".join("%.4f" % x for x in v), float(np.median(v)), float(v.max() - v.min())))
        if True in variants:
            lines.append("%s: step    exact - default: %+.4f ms/step (%+.2f %% of the step)"
                         % (a.label, float(np.median(ms[True]) - np.median(ms[False])),
                            100.0*float(np.median(ms[True]) - np.median(ms[False]))/float(np.median(ms[False]))))

    if "kernels" in cases:
        from gpusph_amd.kernels import HipKernels
        from gpusph_amd.bodies import FloatingBody, box_inertia
        small = P.BuoyancyBox(0.1)
        rng = np.random.default_rng(1)
        d_dt = torch.full((1,), 3e-4, dtype=torch.float32, device="cuda:0")
        for nrows in (int(v) for v in a.rows.split(",")):
            K = HipKernels(small, len(small.parts.info), "cuda:0")
            K.floating_setup([FloatingBody(mass=32.0, inertia=box_inertia(32.0, (0.4,)*3), crot=np.array([0.5, 0.5, 0.3]))],
                             np.array([0, nrows], dtype=np.uint32))
            mk = lambda: torch.from_numpy((rng.normal(size=(nrows, 4))*5.0*10.0**rng.integers(-3, 3, size=(nrows, 1))).astype(np.float32)).to("cuda:0")
            rbf, rbt = mk(), mk()
            L = torch.zeros((1, 6, capi.SPHX_FLOATING_LIMBS), dtype=torch.float64, device="cuda:0")

            def default():
                K.floating_move(rbf, rbt, 1, d_dt)

            def exact():
                K.floating_limbs(rbf, rbt, L)
                K.floating_move_limbs(L, 1, d_dt)
            us = {}
            for name, call in (("default", default), ("exact", exact)):
                v = []
                for _ in range(a.reps):
                    for _ in range(a.warmup):
                        call()
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    torch.cuda.synchronize()
                    e0.record()
                    for _ in range(a.calls):
                        call()
                    e1.record()
                    torch.cuda.synchronize()
                    v.append(1000.0*e0.elapsed_time(e1)/a.calls)
                us[name] = np.array(v)
            lines.append("%s: kernels %7d rows  %d calls x %d: floating_move %s us (median %.2f), floating_limbs + floating_move_limbs %s us (median %.2f)"
                         % (a.label, nrows, a.calls, a.reps, " ".join("%.2f" % x for x in us["default"]), float(np.median(us["default"])),
                            " ".join("%.2f" % x for x in us["exact"]), float(np.median(us["exact"]))))
            del K

    if "slabs" in cases:
        from gpusph_amd.halo import CapiTransport
        from gpusph_amd.multigpu import MultiGpuEngine
        os.environ["SPHX_DISABLE_TILES"] = "1"
        kw = dict(deltap=buoyancy_deltap(a.slab_particles), linearization="xzy", exact_sums=True)
        lib = capi.load()
        group = CapiTransport.new_group(lib, 2)
        out, errors = [None, None], []
        gate = threading.Barrier(2)

        def worker(rank):
            try:
                torch.cuda.set_device(0)
                eng = MultiGpuEngine(P.BuoyancyBox(**kw), "cuda:0", rank, 2, transport=lambda k: CapiTransport(k, rank, 2, group=group),
                                     track_particle_count=False)
                eng.run(a.warmup)
                torch.cuda.synchronize()
                gate.wait(timeout=300)
                t0 = time.perf_counter()
                eng.run(a.steps)
                torch.cuda.synchronize()
                out[rank] = (1000.0*(time.perf_counter() - t0)/a.steps, eng.n_int, eng.n_local)
                eng.transport.close()
            except BaseException as e:
                errors.append((rank, repr(e)))
                gate.abort()
                raise
        threads = [threading.Thread(target=worker, args=(r,), daemon=True) for r in range(2)]
        for t in threads:
            t.start()
        for t in threads:
            t.join(timeout=600)
        if errors or any(o is None for o in out):
            raise SystemExit("two slabs: %s" % (errors or "a worker did not finish"))
        lib.sphx_halo_group_destroy(group)
        eng = TimestepEngine(P.BuoyancyBox(**kw), device="cuda:0", track_particle_count=False)
        eng.run(a.warmup)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        eng.run(a.steps)
        torch.cuda.synchronize()
        one = 1000.0*(time.perf_counter() - t0)/a.steps
        lines.append("%s: slabs   BuoyancyBox exact sums, forces without tiles, %d steps: single domain %d particles %.4f ms/step; two slabs on "
                     "one device (worker threads) %d + %d owned (%d + %d with halo) %.4f / %.4f ms/step"
                     % (a.label, a.steps, eng.n, one, out[0][1], out[1][1], out[0][2], out[1][2], out[0][0], out[1][0]))

    text = "".join("%s\n" % line for line in lines)
    print(text, end="")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "a") as f:
        f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
