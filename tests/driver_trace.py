"""The command sequence of the Python driver (gpusph_amd.multigpu / engine) as a record: every backend call of a few steps with
its arguments, for one case per option set, against records taken before the driver's buffer table was introduced
(tests/golden/driver_trace/*.json, tests/test_driver_trace.py).

A stand-in backend takes the place of the kernels (`kernels=` on device "cpu") and records every method call.  Scalars are recorded
as they are (floats by repr), a tensor as the name of its ALLOCATION: the engine attribute that held its storage right after
construction ("pos", "pos2", "ke2.eps", "_zeroed", ...), found through untyped_storage().data_ptr(), plus storage offset and
shape.  Such a label stays put when the driver renames pos <-> pos2, and depends on no arithmetic and on no machine.  The stand-in
computes only what the driver reads back: reorder writes n into new_num, the forces entries return a block count, jacobi_solve a
fixed triple, fmax_elements / fmax_temp_elements fixed functions of n; the io_count word is left as the driver set it.

Regenerate (only for a change that is meant to alter the sequence):  python tests/driver_trace.py
"""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if __name__ == "__main__":
    sys.path[:0] = [os.path.dirname(HERE), HERE]
GOLDEN = os.path.join(HERE, "golden", "driver_trace")
STEPS = 3


class Recorder:
    def __init__(self):
        self.calls = []
        self.on = True

    def enc(self, v):
        if isinstance(v, torch.Tensor):
            return ("T", v.untyped_storage().data_ptr(), int(v.storage_offset()), list(v.shape))
        if isinstance(v, (bool, np.bool_)):
            return bool(v)
        if isinstance(v, (int, np.integer)):
            return int(v)
        if isinstance(v, (float, np.floating)):
            return repr(float(v))
        if v is None or isinstance(v, str):
            return v
        if isinstance(v, dict):
            return {"dict": [[k, self.enc(x)] for k, x in v.items()]}      # in the dict's own order (tke, eps, turbvisc, eulervel)
        if isinstance(v, (list, tuple)):
            return [self.enc(x) for x in v]
        if isinstance(v, np.ndarray):
            return "ndarray %s %s" % (v.dtype, list(v.shape))
        return "object " + type(v).__name__

    def add(self, name, a, kw):
        if self.on:
            self.calls.append([name, [self.enc(x) for x in a], {k: self.enc(kw[k]) for k in sorted(kw)}])


class StandInKernels:
    """every method exists, is recorded, and computes only what the driver reads back"""

    def __init__(self, rec):
        self._rec = rec

    @staticmethod
    def fmax_elements(n):
        return (int(n) + 255) // 256

    @staticmethod
    def fmax_temp_elements(n):
        return (int(n) + 63) // 64

    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)

        def call(*a, **kw):
            self._rec.add(name, a, kw)
            if name == "reorder":
                a[-1][0] = a[-2]                   # new_num = n
            elif name == "jacobi_solve":
                return 3, 1.0e-6, 2.0e-6
            elif name.startswith("forces"):        # (..., from, to, offset into the CFL array): the blocks of the range
                return self.fmax_elements(a[-2] - a[-3])
            return None
        return call


def _allocations(eng):
    """storage pointer -> label, over the engine's attributes in name order (the first name wins: "_zeroed" before "cfl")"""
    lab = {}
    for name in sorted(vars(eng)):
        v = vars(eng)[name]
        items = ([(name, v)] if isinstance(v, torch.Tensor) else
                 [("%s[%d]" % (name, i), t) for i, t in enumerate(v)] if isinstance(v, list) else
                 [("%s.%s" % (name, k), t) for k, t in v.items()] if isinstance(v, dict) else [])
        for label, t in items:
            if isinstance(t, torch.Tensor):
                lab.setdefault(t.untyped_storage().data_ptr(), label)
    return lab


def _resolve(v, lab):
    if isinstance(v, tuple) and len(v) == 4 and v[0] == "T":
        return "%s+%d%s" % (lab.get(v[1], "?"), v[2], v[3])
    if isinstance(v, list):
        return [_resolve(x, lab) for x in v]
    if isinstance(v, dict):
        return {k: _resolve(x, lab) for k, x in v.items()}
    return v


def _attribute_map(eng, lab):
    out = {}
    for name in sorted(vars(eng)):
        v = vars(eng)[name]
        if isinstance(v, torch.Tensor):
            out[name] = lab.get(v.untyped_storage().data_ptr(), "?")
        elif isinstance(v, list) and v and all(isinstance(t, torch.Tensor) for t in v):
            out[name] = [lab.get(t.untyped_storage().data_ptr(), "?") for t in v]
        elif isinstance(v, dict) and v and all(isinstance(t, torch.Tensor) for t in v.values()):
            out[name] = [[k, lab.get(t.untyped_storage().data_ptr(), "?")] for k, t in v.items()]
    return out


class _HaloProbe:
    """a transport that shows what _update_segments_and_halo would exchange, without a second rank"""

    def __init__(self):
        self.tensors = None

    def allgather_pair(self, a, b, device):
        return [(a, b)]

    def exchange(self, tensors, *ranges):
        self.tensors = list(tensors)
        return 0


def make_engine(problem, rec):
    """a TimestepEngine over the stand-in on the CPU (its own constructor insists on a device and adds only views of the library)"""
    from gpusph_amd.engine import TimestepEngine
    from gpusph_amd.multigpu import MultiGpuEngine
    n = len(problem.parts.info)
    eng = TimestepEngine.__new__(TimestepEngine)
    MultiGpuEngine.__init__(eng, problem, "cpu", 0, 1, kernels=StandInKernels(rec),
                            allocated=problem.max_parts(n) if hasattr(problem, "max_parts") else n)
    if hasattr(problem, "impose_open_boundaries"):      # the problem's own pass over the state belongs to the sequence
        inner = problem.impose_open_boundaries

        def impose(*a):
            rec.add("problem.impose_open_boundaries", a, {})
            return inner(*a)
        problem.impose_open_boundaries = impose
    return eng


def _run(make, drive):
    rec = Recorder()
    eng = make_engine(make(), rec)
    lab = _allocations(eng)
    drive(eng)
    rec.on = False
    out = {"calls": _resolve(rec.calls, lab), "attributes": _attribute_map(eng, lab)}
    return eng, lab, out


def record(case):
    """the record of one case: a plain structure of lists, dicts, strings and numbers"""
    make, opts = _problems()[case]

    def steps(eng):
        for ftype, freq in opts.get("filters", ()):
            eng.add_filter(ftype, freq)
        for _ in range(STEPS):
            eng.step()
    eng, lab, out = _run(make, steps)
    out["hot_extra"] = sorted(eng._hot_extra())      # (a HotFile takes its order from hotfile.STORED)
    out["host_buffer_count"] = eng._host_buffer_count()
    out["download"] = sorted(eng.download())
    out["buildneibsfreq"] = int(eng.sp.buildneibsfreq)
    probe = _HaloProbe()
    eng.transport = probe
    eng._update_segments_and_halo()      # (last: it leaves the segments of a rank without particles behind)
    enc = Recorder().enc
    out["halo_state"] = _resolve([enc(t) for t in probe.tensors], lab)
    if hasattr(eng, "halo_state"):       # the same list, asked directly
        out["halo_state_method"] = _resolve([enc(t) for t in eng.halo_state()], lab)
    if opts.get("repack"):
        def repack(eng):
            eng.repack_step(); eng.repack_step()
        _, _, rp = _run(make, repack)
        out["repack"] = rp
    return json.loads(json.dumps(out))


def _problems():
    from gpusph_amd import defs as D
    from gpusph_amd import problem as P
    from grenier_helpers import grenier_problem

    def freq2(p):
        p.simparams.buildneibsfreq = 2      # a second re-sort inside the three steps
        return p
    sa = dict(l=0.3, w=0.3, h=0.3, H=0.2)
    io = dict(l=0.5, w=0.3, h=0.3, H=0.2)
    return {
        "dambreak": (lambda: freq2(P.DamBreak3D(0.1, obstacle=True)), {"repack": True}),
        "dambreak_sps_xsph_shepard": (lambda: freq2(_xsph(P.DamBreak3D(0.1, obstacle=True, viscosity="SPSVISC"))),
                                      {"filters": [(D.SHEPARD_FILTER, 2)]}),
        "wavetank": (lambda: freq2(P.WaveTank(0.1)), {}),
        "internal_energy": (lambda: freq2(P.DamBreak3D(0.1, obstacle=False, hydrostatic=False, internal_energy=True)), {}),
        "grenier": (lambda: freq2(grenier_problem(0.1)), {}),
        "poiseuille_papanastasiou": (lambda: freq2(P.Poiseuille(8, rheology=D.PAPANASTASIOU)), {}),
        "lithostatic_column": (lambda: freq2(P.LithostaticColumn(0.1, columns=(5, 5), sediment_layers=4, water_layers=3)), {}),
        "sabox_stillwater": (lambda: freq2(P.SABox(0.1, options="StillWaterSA", **sa)), {}),
        "sabox_repack": (lambda: freq2(P.SABox(0.1, options="StillWaterRepackSA", **sa)), {"repack": True}),
        "sabox_spheric2": (lambda: freq2(P.SABox(0.1, options="Spheric2SA", **sa)), {}),
        "spheric2_keps": (lambda: freq2(P.SABox(0.1, options="Spheric2SA", viscosity="KEPSVISC", **sa)), {}),
        "sapaddlebox": (lambda: freq2(P.SAPaddleBox(0.1, **sa)), {}),
        "satwofluidbox": (lambda: freq2(P.SATwoFluidBox(0.1, **sa)), {}),
        "sachannelio": (lambda: P.SAChannelIO(0.1, **io), {}),                # open boundaries: buildneibsfreq = 1
        "sachannelioflap": (lambda: P.SAChannelIOFlap(0.1, **io), {}),
        "periodicbox_repack": (lambda: freq2(P.PeriodicBox(0.1, n=(6, 6, 6), repacking=True)), {"repack": True}),
    }


def _xsph(p):
    from gpusph_amd import defs as D
    p.simparams.simflags |= D.ENABLE_XSPH
    return p


CASE_NAMES = tuple(_problems())


def golden_path(case):
    return os.path.join(GOLDEN, case + ".json")


def generate():
    os.makedirs(GOLDEN, exist_ok=True)
    for case in CASE_NAMES:
        rec = record(case)
        rec.pop("halo_state_method", None)
        with open(golden_path(case), "w") as f:
            json.dump(rec, f, indent=0, separators=(",", ":"))
            f.write("\n")
        print("%-28s %5d calls, halo %s" % (case, len(rec["calls"]), [s.split("+")[0] for s in rec["halo_state"]]))


if __name__ == "__main__":
    generate()
