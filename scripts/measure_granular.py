#!/usr/bin/env python3
"""Time one effective-pressure solve of the GRANULAR rheology two ways on a LithostaticColumn of about a million particles:
through sphx_jacobi_solve (coefficients stored once, stop test on the device) and through the loop over the four entry points
with the reference's two host reads per iteration.  Both start from a zero field on the same state and must end with the same
bits.  HIP events around each, after one warm-up solve of each; the result goes to profiles/granular_solve.txt.

    python scripts/measure_granular.py [--columns 100] [--sediment 60] [--water 36] [--maxiter 2000] [--out profiles/granular_solve.txt]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--columns", type=int, default=100)
    ap.add_argument("--sediment", type=int, default=60)
    ap.add_argument("--water", type=int, default=36)
    ap.add_argument("--maxiter", type=int, default=2000, help="jacobi_maxiter of both solves (a bed this deep does not converge earlier)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "granular_solve.txt"))
    a = ap.parse_args()
    import torch
    from gpusph_amd.engine import TimestepEngine
    from gpusph_amd.problem import LithostaticColumn
    pr = LithostaticColumn(0.05, columns=(a.columns, a.columns), sediment_layers=a.sediment, water_layers=a.water, jitter=0.1,
                           lithostatic_init=False, jacobi_maxiter=a.maxiter)
    eng = TimestepEngine(pr, device="cuda:0")
    eng.build_neibs()
    K, n, sp = eng.k, eng.n, pr.simparams
    state = (eng.pos, eng.vel, eng.info, eng.hash, eng.cellStart, eng.neibslist)
    jac = torch.zeros((eng.alloc, 4), dtype=torch.float32, device=eng.device)

    def fused(p):
        return K.jacobi_solve(p, *state, n, n)

    def loop(p):
        K.jacobi_fs_boundary_conditions(p, eng.pos, eng.info, n, n)
        K.jacobi_wall_boundary_conditions(p, *state, n, n)
        counter = 0
        while True:
            K.jacobi_build_vectors(jac, p, *state, n, n)
            res = K.jacobi_update_effpres(p, jac, eng.info, n, n)
            err = K.jacobi_wall_boundary_conditions(p, *state, n, n)
            if (err < np.float32(sp.jacobi_backerr) and res < np.float32(sp.jacobi_residual)) or counter > sp.jacobi_maxiter:
                return counter, err, res
            counter += 1

    def timed(fn):
        p = torch.zeros(eng.alloc, dtype=torch.float32, device=eng.device)
        fn(p.clone())                                       # warm-up (scratch allocation of the fused solve included)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        out = fn(p)
        e1.record()
        torch.cuda.synchronize()
        return out, e0.elapsed_time(e1), p

    (it_f, err_f, res_f), ms_f, p_f = timed(fused)
    (it_l, err_l, res_l), ms_l, p_l = timed(loop)
    same = bool(torch.equal(p_f.view(torch.int32), p_l.view(torch.int32))) and (it_f, err_f, res_f) == (it_l, err_l, res_l)
    lines = [
        "effective-pressure solve, LithostaticColumn %d x %d columns, %d sediment + %d water layers: %d particles, jacobi_maxiter %d"
        % (a.columns, a.columns, a.sediment, a.water, n, a.maxiter),
        "device: %s" % torch.cuda.get_device_name(0),
        "sphx_jacobi_solve      counter %6d  sweeps %6d  %10.2f ms  %8.4f ms/sweep" % (it_f, it_f + 1, ms_f, ms_f / (it_f + 1)),
        "entry-point loop       counter %6d  sweeps %6d  %10.2f ms  %8.4f ms/sweep" % (it_l, it_l + 1, ms_l, ms_l / (it_l + 1)),
        "ratio loop / solve %.2f; same bits: %s; backward error %g, residual %g" % (ms_l / ms_f, same, err_f, res_f),
    ]
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
