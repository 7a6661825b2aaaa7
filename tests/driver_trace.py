"""The command sequence of the Python driver (gpusph_amd.multigpu / engine) as a record: every backend call of a few steps with
its arguments, for one case per option set, against records taken before the driver's buffer table was introduced
(tests/golden/driver_trace/*.json, tests/test_driver_trace.py).

A stand-in backend takes the place of the kernels (`kernels=` on device "cpu") and records every method call.  Scalars are recorded
as they are (floats by repr), a tensor as the name of its ALLOCATION: the engine attribute that held its storage right after
construction ("pos", "pos2", "ke2.eps", "_zeroed", ...), found through untyped_storage().data_ptr(), plus storage offset and
shape.  Such a label stays put when the driver renames pos <-> pos2, and depends on no arithmetic and on no machine.  The stand-in
computes only what the driver reads back: reorder writes n into new_num, the forces entries return a block count, jacobi_solve a
fixed triple, fmax_elements / fmax_temp_elements fixed functions of n; the io_count word is left as the driver set it.

Two things those records do not see have records of their own, taken from the driver as it stood before its predictor and
corrector became one substep:
  * ranks2_<case>.json: rank 0 of a world of two, in this process (record_ranks2).  The stand-in's reorder also writes the segment
    starts [0, 3n/4, n, EMPTY_SEGMENT], so the inner edge is the last quarter of the rows and a forces pass runs as two stripes;
    RecordingTransport takes the place of the transport and puts its exchanges (the allocation labels of the tensors in order,
    the two neighbours and the four ranges) and its reductions into the same call list, and so do the host's reads of device
    words (below).  An option set that the driver refuses on two ranks is recorded as its refusal.
  * host_reads.json: per case the calls of Tensor.item, .cpu, .tolist and .numpy while the steps of the one-domain record run
    (host_reads), as "host.<method>" entries with the allocation label ("?" for a temporary).

Regenerate (only for a change that is meant to alter the sequence):  python tests/driver_trace.py
"""
import contextlib
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
    def __init__(self, host_in_calls=False):
        self.calls = []
        self.host = self.calls if host_in_calls else []      # the host's reads of device words: their own list, or in line
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

    @contextlib.contextmanager
    def host_reads(self):
        """while it is open, Tensor.item / .cpu / .tolist / .numpy append a "host.<method>" entry to self.host"""
        saved = {}

        def wrap(name, inner):
            def method(t, *a, **kw):
                if self.on:
                    self.host.append(["host." + name, [self.enc(t)], {}])
                return inner(t, *a, **kw)
            return method
        for name in ("item", "cpu", "tolist", "numpy"):
            saved[name] = vars(torch.Tensor).get(name)
            setattr(torch.Tensor, name, wrap(name, getattr(torch.Tensor, name)))
        try:
            yield
        finally:
            for name, own in saved.items():
                if own is None:
                    delattr(torch.Tensor, name)
                else:
                    setattr(torch.Tensor, name, own)


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
                n = a[-2]
                a[-1][0] = n                       # new_num = n
                if a[0] is not None:               # several domains: inner | inner edge | no outer edge, no outer
                    a[0].copy_(torch.tensor([0, 3 * n // 4, n, -1], dtype=a[0].dtype))      # (EMPTY_SEGMENT as int32)
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


class RecordingTransport:
    """the transport of rank 0 in a world where every rank answers what rank 0 says; records what it is asked to move"""

    def __init__(self, rec, world):
        self._rec, self._world = rec, world

    def allgather_pair(self, a, b, device):
        return [(a, b)] * self._world

    def exchange(self, tensors, left, right, send_l, recv_l, send_r, recv_r):
        self._rec.add("transport.exchange", (list(tensors), left, right, send_l, recv_l, send_r, recv_r), {})
        return 0

    def allreduce_min(self, t):
        self._rec.add("transport.allreduce_min", (t,), {})

    def allreduce_sum(self, t):
        self._rec.add("transport.allreduce_sum", (t,), {})


def make_engine(problem, rec, world=1):
    """a TimestepEngine over the stand-in on the CPU (its own constructor insists on a device and adds only views of the library);
    with world > 1 rank 0 of that many, over a RecordingTransport"""
    from gpusph_amd.engine import TimestepEngine
    from gpusph_amd.multigpu import MultiGpuEngine
    n = len(problem.parts.info)
    eng = TimestepEngine.__new__(TimestepEngine)
    MultiGpuEngine.__init__(eng, problem, "cpu", 0, world, kernels=StandInKernels(rec),
                            allocated=problem.max_parts(n) if hasattr(problem, "max_parts") else n,
                            transport=RecordingTransport(rec, world) if world > 1 else None)
    if hasattr(problem, "impose_open_boundaries"):      # the problem's own pass over the state belongs to the sequence
        inner = problem.impose_open_boundaries

        def impose(*a):
            rec.add("problem.impose_open_boundaries", a, {})
            return inner(*a)
        problem.impose_open_boundaries = impose
    return eng


def _run(make, drive, world=1):
    rec = Recorder(host_in_calls=world > 1)
    eng = make_engine(make(), rec, world)
    lab = _allocations(eng)
    with rec.host_reads():
        drive(eng)
    rec.on = False
    out = {"calls": _resolve(rec.calls, lab), "attributes": _attribute_map(eng, lab)}
    if world == 1:
        out["host_reads"] = _resolve(rec.host, lab)
    return eng, lab, out


def _steps(opts):
    def steps(eng):
        for ftype, freq in opts.get("filters", ()):
            eng.add_filter(ftype, freq)
        for _ in range(STEPS):
            eng.step()
    return steps


def _repack(eng):
    eng.repack_step(); eng.repack_step()


def host_reads(case):
    """the host's reads of device words during the runs of record(case): "steps" and, where the case has one, "repack" """
    make, opts = _problems()[case]
    out = {"steps": _run(make, _steps(opts))[2]["host_reads"]}
    if opts.get("repack"):
        out["repack"] = _run(make, _repack)[2]["host_reads"]
    return json.loads(json.dumps(out))


def record_ranks2(case):
    """rank 0 of two: the backend calls, exchanges, reductions and host reads of three steps in one list; or the driver's refusal"""
    make, opts = _problems(ranks2=True)[case]
    try:
        _, _, out = _run(make, _steps(opts), world=2)
    except (NotImplementedError, ValueError) as e:
        out = {"refused": [type(e).__name__, str(e)]}
    return json.loads(json.dumps(out))


def record(case):
    """the record of one case: a plain structure of lists, dicts, strings and numbers"""
    make, opts = _problems()[case]
    eng, lab, out = _run(make, _steps(opts))
    del out["host_reads"]                # (host_reads.json has them: these records are older)
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
        _, _, rp = _run(make, _repack)
        del rp["host_reads"]
        out["repack"] = rp
    return json.loads(json.dumps(out))


def _problems(ranks2=False):
    from gpusph_amd import defs as D
    from gpusph_amd import problem as P
    from grenier_helpers import grenier_problem

    def freq2(p):
        p.simparams.buildneibsfreq = 2      # a second re-sort inside the three steps
        return p
    sa = dict(l=0.3, w=0.3, h=0.3, H=0.2)
    io = dict(l=0.5, w=0.3, h=0.3, H=0.2)
    pois, column = dict(ppH=8), dict(sediment_layers=4, water_layers=3)
    if ranks2:      # those have too few cell planes along the split axis for two slabs; these have six (476 particles), eight and seven
        sa = io = dict(l=1.4, w=0.3, h=0.3, H=0.2, linearization="yzx")
        pois, column = dict(ppH=16, linearization="xyz"), dict(sediment_layers=8, water_layers=6, linearization="xyz")
    return {
        "dambreak": (lambda: freq2(P.DamBreak3D(0.1, obstacle=True)), {"repack": True}),
        "dambreak_sps_xsph_shepard": (lambda: freq2(_xsph(P.DamBreak3D(0.1, obstacle=True, viscosity="SPSVISC"))),
                                      {"filters": [(D.SHEPARD_FILTER, 2)]}),
        "wavetank": (lambda: freq2(P.WaveTank(0.1)), {}),
        "internal_energy": (lambda: freq2(P.DamBreak3D(0.1, obstacle=False, hydrostatic=False, internal_energy=True)), {}),
        "grenier": (lambda: freq2(grenier_problem(0.1)), {}),
        "poiseuille_papanastasiou": (lambda: freq2(P.Poiseuille(rheology=D.PAPANASTASIOU, **pois)), {}),
        "lithostatic_column": (lambda: freq2(P.LithostaticColumn(0.1, columns=(5, 5), **column)), {}),
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
# (the repacking cases step like sabox_stillwater and dambreak; a repacking iteration is a single domain's)
RANKS2_CASE_NAMES = tuple(c for c in CASE_NAMES if not c.endswith("_repack"))


def golden_path(case, golden=GOLDEN):
    return os.path.join(golden, case + ".json")


def _dump(rec, path):
    with open(path, "w") as f:
        json.dump(rec, f, indent=0, separators=(",", ":"))
        f.write("\n")


def generate(golden=GOLDEN):
    os.makedirs(golden, exist_ok=True)
    for case in CASE_NAMES:
        rec = record(case)
        rec.pop("halo_state_method", None)
        _dump(rec, golden_path(case, golden))
        print("%-28s %5d calls, halo %s" % (case, len(rec["calls"]), [s.split("+")[0] for s in rec["halo_state"]]))
    for case in RANKS2_CASE_NAMES:
        rec = record_ranks2(case)
        _dump(rec, golden_path("ranks2_" + case, golden))
        names = [c[0] for c in rec.get("calls", ())]
        print("ranks2 %-28s %s" % (case, rec["refused"] if "refused" in rec else "%5d calls, %d exchanges, %d host reads"
                                   % (len(names), names.count("transport.exchange"), sum(n.startswith("host.") for n in names))))
    _dump({case: host_reads(case) for case in CASE_NAMES}, golden_path("host_reads", golden))


if __name__ == "__main__":
    generate(*sys.argv[1:2])      # (a directory: write the records there, to compare them with the committed ones)
