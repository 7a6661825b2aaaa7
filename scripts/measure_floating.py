#!/usr/bin/env python3
"""What a floating body costs per step, at about a million particles, by HIP events over --steps steps and --reps repetitions:
  (a) BuoyancyBox with the cube held at rest as a force-feedback body (no floating kernel runs),
  (b) the same box with the cube floating (two small launches per substep, no host read),
and, for comparisons between commits of the path every problem shares,
  (c) DamBreak3D(obstacle=True) without a callback at the same size.
Every run warms up for --warmup steps first; a repetition starts from a fresh engine.  The result is appended to --out with --label
in front of every line, so that the numbers of two commits can sit in one file (profiles/floating_bodies.txt).

    python scripts/measure_floating.py [--particles 1e6] [--steps 50] [--reps 3] [--cases a,b,c] [--label this] [--out FILE]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def buoyancy_deltap(target):
    """the spacing at which BuoyancyBox has about `target` particles: (N + 7)^3 lattice points minus the air above the water"""
    lo, hi = 20, 400
    while lo < hi:
        n = (lo + hi)//2
        count = (n + 7)**3 - (n + 1)**3 + (n + 1)**2*(int(round(0.6*n)) + 1)
        lo, hi = (n + 1, hi) if count < target else (lo, n)
    return 1.0/lo


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--particles", type=float, default=1.0e6)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--cases", default="a,b,c")
    ap.add_argument("--label", default="this commit")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "floating_bodies.txt"))
    a = ap.parse_args()
    import torch
    from gpusph_amd.engine import TimestepEngine
    from gpusph_amd import problem as P

    def make(case):
        if case == "c":
            return P.DamBreak3D(P.DamBreak3D.deltap_for(int(a.particles), True), obstacle=True)
        return P.BuoyancyBox(buoyancy_deltap(a.particles), floating=(case == "b"))

    names = dict(a="BuoyancyBox, cube at rest (force feedback)", b="BuoyancyBox, cube floating", c="DamBreak3D(obstacle=True), no callback")
    lines = []
    for case in a.cases.split(","):
        ms, n = [], 0
        for _ in range(a.reps):
            eng = TimestepEngine(make(case), device="cuda:0", track_particle_count=False)
            n = eng.n
            eng.run(a.warmup)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            eng.run(a.steps)
            e1.record()
            torch.cuda.synchronize()
            ms.append(e0.elapsed_time(e1)/a.steps)
            del eng
        ms = np.array(ms)
        lines.append("%s: (%s) %-44s %8d particles  %d steps x %d: %s ms/step, median %.4f, spread %.4f"
                     % (a.label, case, names[case], n, a.steps, a.reps, " ".join("%.4f" % v for v in ms), float(np.median(ms)),
                        float(ms.max() - ms.min())))
    text = "".join("%s\n" % line for line in lines)
    print(text, end="")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "a") as f:
        f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
