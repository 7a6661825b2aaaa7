"""Step time of the SABox tank (walls at rest) in one of its option sets, through the fast path (tiled window + wall kernels) or,
with SPHX_DISABLE_TILES=1 in the environment, through the list walkers: the numbers of profiles/sa_ferrari_time.txt.
usage: python scripts/time_sa_options.py <StillWaterSA|StillWaterRepackSA|Spheric2SA|Spheric2SA-nodiff> [deltap] [steps]
(Spheric2SA-nodiff: the same framework line without its density diffusion, to read off what the term costs)"""
import sys, time, os
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from gpusph_amd import defs as D
from gpusph_amd.problem import SABox
from gpusph_amd.engine import TimestepEngine

options = sys.argv[1]
dp = float(sys.argv[2]) if len(sys.argv) > 2 else 0.008
steps = int(sys.argv[3]) if len(sys.argv) > 3 else 20
t0 = time.time()
prob = SABox(dp, l=1.6, w=1.6, h=1.0, H=0.8, options=options.split("-")[0])
if options.endswith("-nodiff"):
    prob.simparams.densitydiffusiontype = D.DENSITY_DIFFUSION_NONE
eng = TimestepEngine(prob, device="cuda:0")
eng.run(11)
torch.cuda.synchronize()
tiled = int(eng.k.lib.sphx_dbg_tiles_usable(eng.k.ctx.handle))
ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
ev[0].record(); eng.run(steps); ev[1].record(); torch.cuda.synchronize()
ms = ev[0].elapsed_time(ev[1])/steps
print("SABox %-20s %-12s %9d particles  %8.3f ms/step  %7.1f M particle-updates/s  (rebuild every %d steps; set-up %.0f s)" % (
    options, "fast path" if tiled else "list walkers", eng.n, ms, eng.n/ms/1e3, prob.simparams.buildneibsfreq, time.time() - t0), flush=True)
