#!/usr/bin/env python3
"""Step time of the SATwoFluidBox mirror (BiFluidPoiseuilleSA's option set: formulation<SPH_HA>, two fluids, SA walls, density
summation, Brezzi diffusion) at the size of the 4.3 M SA tank, beside the same two-fluid tank with formulation<SPH_F1> on the same
build.  Both run on the list walkers (more than one fluid declines the tiling for SPH_F1 as well), so the ratio is what the
Hu & Adams weights cost on that path.  HIP events around `steps` steps after `warmup` steps (a list rebuild falls into both), the
two variants alternating `repeats` times; the result goes to profiles/sa_ha_tank.txt.  Nothing is tuned here: the numbers are a record.

    python scripts/measure_sa_ha.py [--deltap 0.008] [--steps 20] [--warmup 11] [--repeats 3] [--out profiles/sa_ha_tank.txt]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--deltap", type=float, default=0.008)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=11)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sa_ha_tank.txt"))
    a = ap.parse_args()
    import torch
    from gpusph_amd import defs as D
    from gpusph_amd.engine import TimestepEngine
    from gpusph_amd.problem import SATwoFluidBox
    if not torch.cuda.is_available():
        raise SystemExit("measure_sa_ha.py needs a GPU: a step time is not measured anywhere else")

    def run(formulation):
        pr = SATwoFluidBox(a.deltap, l=1.6, w=1.6, h=1.0, H=0.8)
        pr.simparams.sph_formulation = formulation
        eng = TimestepEngine(pr, device="cuda:0")
        for _ in range(a.warmup):
            eng.step()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(a.steps):
            eng.step()
        e1.record()
        torch.cuda.synchronize()
        ms = e0.elapsed_time(e1)/a.steps
        usable = int(eng.k.lib.sphx_dbg_tiles_usable(eng.k.ctx.handle))
        finite = bool(torch.isfinite(eng.vel[:eng.n]).all())
        n = eng.n
        del eng
        torch.cuda.empty_cache()
        return n, ms, usable, finite

    lines = ["SATwoFluidBox (SA walls, two fluids rho0 4000 / 1000, density summation, Brezzi) at deltap %g: ms per step over %d steps after %d, "
             "the two formulations alternating" % (a.deltap, a.steps, a.warmup), "device: %s" % torch.cuda.get_device_name(0)]
    ms = {"SPH_HA": [], "SPH_F1": []}
    for _ in range(a.repeats):
        for name, form in (("SPH_HA", D.SPH_HA), ("SPH_F1", D.SPH_F1)):
            n, t, usable, finite = run(form)
            ms[name].append(t)
            lines.append("%s  %9d particles  %8.3f ms/step  %8.1f M particle-updates/s  tiles usable %d  finite %s"
                         % (name, n, t, n/t/1e3, usable, finite))
    med = {k: sorted(v)[len(v)//2] for k, v in ms.items()}
    lines.append("median SPH_HA %.3f ms/step, median SPH_F1 %.3f ms/step, ratio HA / F1 %.3f" % (med["SPH_HA"], med["SPH_F1"], med["SPH_HA"]/med["SPH_F1"]))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
