"""Slab-decomposed multi-GPU timestep driver: one process per GPU, halo exchange over torch.distributed
(backend "nccl" = RCCL over xGMI on ROCm; "gloo" on CPU in the test suite).

What it mirrors in GPUSPH (paths relative to the GPUSPH tree) and what it changes:
  * device map: equal split of the cells along COORD3, the slowest linearisation axis, so that each
    device's edge layer and each imported halo is ONE contiguous index range (src/linearization.h:28-35;
    ProblemCore::fillDeviceMapByAxis src/ProblemCore.cc:1061-1116).  DamBreak3D splits along Y
    (src/problems/DamBreak3D.cu:217-220): use linearisation "xzy" so that COORD3 = y.
  * cell types INNER / INNER_EDGE / OUTER_EDGE / OUTER in the two high hash bits
    (GPUWorker::createCompactDeviceMap src/GPUWorker.cc:1560-1634, src/multi_gpu_defines.h:56-83): the
    sort then orders particles [inner | inner edge | outer edge | outer] and REORDER returns the
    segment starts.
  * migration is implicit as in the reference (src/GPUWorker.cc:358-365,1432-1460): halo copies are
    integrated redundantly (EULER runs on all particles), a particle that crosses the slab boundary sorts
    into the other segment at the next rebuild, the old owner crops it, the new owner already has it.
  * halo import: the reference PULLS bursts with cudaMemcpyPeerAsync per (burst, buffer) and keeps the
    per-cell offsets on the host (src/GPUWorker.cc:711-921).  Here each rank SENDS its two edge layers
    (contiguous ranges) to its two neighbours and receives theirs, as ONE grouped send/recv per
    exchange on a dedicated stream: after each re-sort pos+vel+info+hash (44 B/particle), after each
    forces pass the forces (16 B/particle) -- strictly nearest-neighbour traffic, one xGMI link per
    pair of devices, no collective on the data path.  The forces of the edge stripe are computed
    first and exchanged while the inner stripe computes (FORCES_ENQUEUE/COMPLETE, GPUWorker.cc:2086-2185).
  * dt: min over devices (GPUSPH.cc:650-657) as an all_reduce(MIN) of one device float per step.
Results are bit-identical to the single-device run (same per-particle neighbour order and arithmetic).
"""
import os
from collections import namedtuple
from types import SimpleNamespace
import numpy as np
import torch

from . import defs as D

# ---------------------------------------------------------------------- the particle-state buffers of a step
# One row per buffer that holds one value per particle and exists twice: engine.<name> and engine.<name>2.  Allocation, the
# re-sort, the halo state, the renaming at the end of a step, download_internal and the HotFile set are loops over this table: a
# new property buffer is a new row, and what a row leaves out it leaves out on purpose.
#   has      which option sets have the buffer (a predicate on the engine)
#   dtype, row   of the device tensors: (allocated,) + row; a dict of rows for `ke`, which is a dict of tensors in that order
#   init     ARRAY: problem.copy_to_array()[name] (`view`: the dtype the host array is read or written as); FILL: stays at `fill`;
#            else the engine method (arrs, mask, n0) that sets it up once everything is allocated.  Both copies start from `fill`.
#   resort   GATHER: gather_rows into the second copy after every sort, then renamed; REORDER: inside the reorder pass itself
#   halo     exchanged by _update_segments_and_halo, in table order behind pos, vel, info and hash
#   stepped  a step writes the new state into the second copy, renamed at the end of the step (_state_of tells the two states apart);
#            where false the second copy is scratch of the re-sort only
#   evolves  a step integrates it from its own last value: repack(reset=True), which restarts positions, velocities and
#            densities only, refuses option sets that have such a buffer beyond pos and vel
#   hot      stored in a HotFile under its name (ke: its fields' names)
#   download returned by download_internal under its name (ke: its fields' names)
# The order is that of the gathers of a re-sort.  The halo state of the parent had vol and energy ahead of the SA buffers; the
# library refuses ENABLE_INTERNAL_ENERGY and SPH_GRENIER with SA_BOUNDARY and with each other (energy.hip, sphx_set_constants), so
# no run has two of the three and both ranks of every run see the order they always saw.
Buf = namedtuple("Buf", "name has dtype row view fill init resort halo stepped evolves hot download")
ARRAY, FILL, GATHER, REORDER = "array", "fill", "gather", "reorder"
_f32, _i32 = torch.float32, torch.int32
_yes, _no = (lambda e: True), (lambda e: False)
BUFFERS = (
    Buf("pos", _yes, _f32, (4,), None, 0, ARRAY, REORDER, True, _yes, _yes, False, True),
    Buf("vel", _yes, _f32, (4,), None, 0, ARRAY, REORDER, True, _yes, _yes, False, True),
    # SA_BOUNDARY: BUFFER_VERTICES (uint4: int32 on the device, uint32 in the host arrays and in a HotFile), BUFFER_BOUNDELEMENTS,
    # BUFFER_GRADGAMMA (float4), the optional arrays of reorderDataAndFindCellStart (src/cuda/buildneibs.cu:263-311).
    # download_internal leaves the vertices out.
    Buf("vertices", lambda e: e.sa, _i32, (4,), np.int32, 0, ARRAY, GATHER, True, _no, _no, True, False),
    # with bodies of prescribed motion the Euler step turns the normals of the moving segments and vertices: boundelements2 is
    # then the state n* / n+1 (PredictorCorrectorIntegrator.cc:408-418); a function of time, which repack(reset=True) lets pass
    Buf("boundelements", lambda e: e.sa, _f32, (4,), None, 0, ARRAY, GATHER, True, lambda e: e.sa_moving, _no, True, True),
    # gamma by quadrature is recomputed from the positions in every step, dynamic gamma is integrated
    Buf("gradgamma", lambda e: e.sa, _f32, (4,), None, 0, ARRAY, GATHER, True, _yes, lambda e: e.sa_dynamic_gamma, True, True),
    # open boundaries: BUFFER_EULERVEL (the halo's vertices and segments enter the forces with theirs) and BUFFER_NEXTID; neither is
    # in a HotFile or in download_internal
    Buf("eulervel", lambda e: e.io, _f32, (4,), None, 0, FILL, GATHER, True, _yes, _yes, False, False),
    Buf("next_ids", lambda e: e.io, _i32, (), None, -1, "_init_next_ids", GATHER, False, _no, _no, False, False),
    # ENABLE_INTERNAL_ENERGY: BUFFER_INTERNAL_ENERGY starts from zero (init_internal_energy)
    Buf("energy", lambda e: e.energy_on, _f32, (), None, 0, FILL, GATHER, True, _yes, _yes, True, True),
    # turbulence<KEPSILON>: BUFFER_TKE / EPSILON / TURBVISC / EULERVEL as one dict in that order; its eulervel is not the open
    # boundaries' (open boundaries refuse k-epsilon)
    Buf("ke", lambda e: e.keps, _f32, dict(tke=(), eps=(), turbvisc=(), eulervel=(4,)), None, 0, "_init_keps", GATHER, True, _yes, _yes,
        True, True),
    # SPH_GRENIER: BUFFER_VOLUME; the halo copies integrate theirs from the exchanged forces
    Buf("vol", lambda e: e.grenier, _f32, (4,), None, 0, "_init_volume", GATHER, True, _yes, _yes, True, True),
    # GRANULAR: BUFFER_EFFPRES starts from the problem's field and every solve starts from the last one's result, in place.  It is
    # neither halo state nor in a HotFile: runs on several domains and checkpoints of GRANULAR are refused with their messages
    Buf("effpres", lambda e: e.granular, _f32, (), None, 0, ARRAY, GATHER, False, _no, _no, False, True),
)


def _tensors(v):
    return list(v.values()) if isinstance(v, dict) else [v]


def _items(name, v):
    return list(v.items()) if isinstance(v, dict) else [(name, v)]


class SlabPartition:
    """equal split of the COORD3 planes among `world` devices"""

    def __init__(self, problem, world):
        c1, c2, c3 = D.LINEARIZATIONS[problem.linearization]
        gs = problem.m_gridsize
        self.gs3 = int(gs[c3])
        self.plane = int(gs[c1]) * int(gs[c2])          # cells per COORD3 plane = contiguous hash range
        self.world = world
        # a split axis that is periodic closes the chain of slabs into a ring: the first and the last slab are neighbours through
        # the periodic face and exchange their outermost planes like any two neighbours (in the reference this falls out of the
        # device map and the periodic neighbour cells, src/ProblemCore.cc:1061-1116).  Two slabs on a ring are each other's
        # neighbour on both sides: the transports order their receives for that (halo.py, halo.hip).
        self.ring = world > 1 and bool(problem.simparams.periodicbound & (1 << c3))
        # fillDeviceMapByAxis (src/ProblemCore.cc:1061-1116): fewer than 3 planes per device on average are refused; a device
        # takes round(planes / devices) planes, the last one what is left
        if world > 1 and self.gs3 / float(world) < 3.0:
            raise ValueError("not enough cells along the split axis (%d planes, %d devices: fewer than 3 per device; "
                             "src/ProblemCore.cc:1089-1090)" % (self.gs3, world))
        per = int(np.floor(self.gs3 / float(world) + 0.5))
        self.lo = [min(d * per, self.gs3) for d in range(world)]
        self.hi = [min((d + 1) * per, self.gs3) for d in range(world)]
        self.hi[-1] = self.gs3
        # the rounding rule can starve the last device (28 planes on 8 devices: 7 x 4 and nothing left; 21 on 6: one plane),
        # which the average test above does not see.  A slab needs its two edge planes to be different planes (each is sent
        # to one neighbour and has its own outer edge plane behind it), so such a split is replaced by the even one:
        # floor(planes / devices) each, the first planes % devices slabs one more
        if world > 1 and min(h - l for l, h in zip(self.lo, self.hi)) < 2:
            base, rem = divmod(self.gs3, world)
            counts = [base + (1 if d < rem else 0) for d in range(world)]
            self.lo = [sum(counts[:d]) for d in range(world)]
            self.hi = [self.lo[d] + counts[d] for d in range(world)]
        if world > 1 and min(h - l for l, h in zip(self.lo, self.hi)) < 2:
            raise ValueError("slab split of %d planes over %d devices leaves a device with fewer than 2 planes: %s"
                             % (self.gs3, world, list(zip(self.lo, self.hi))))

    def plane_types(self, rank):
        """CELLTYPE_* of every COORD3 plane as seen by `rank`"""
        t = np.full(self.gs3, D.CELLTYPE_OUTER_CELL, dtype=np.uint32)
        lo, hi = self.lo[rank], self.hi[rank]
        t[lo:hi] = D.CELLTYPE_INNER_CELL
        if rank > 0 or self.ring:
            t[lo] = D.CELLTYPE_INNER_EDGE_CELL
            t[(lo - 1) % self.gs3] = D.CELLTYPE_OUTER_EDGE_CELL
        if rank < self.world - 1 or self.ring:
            t[hi - 1] = D.CELLTYPE_INNER_EDGE_CELL
            t[hi % self.gs3] = D.CELLTYPE_OUTER_EDGE_CELL
        return t

    def compact_device_map(self, rank):
        """per-cell CELLTYPE_*_SHIFTED (BUFFER_COMPACT_DEV_MAP)"""
        return np.repeat(self.plane_types(rank) << np.uint32(30), self.plane).astype(np.uint32)

    def local_mask(self, rank, hashes):
        """particles a rank holds initially: its own planes plus the one-plane halo on each side"""
        c3 = (hashes & D.CELLTYPE_BITMASK) // self.plane
        return self.plane_types(rank)[c3] != D.CELLTYPE_OUTER_CELL


class MultiGpuEngine:
    def __init__(self, problem, device, rank, world, kernels=None, track_particle_count=True, margin=1.25,
                 overlap=True, allocated=None, clobber_neibslist=False, transport=None):
        self.sa = problem.simparams.boundarytype == D.SA_BOUNDARY
        self.grenier = problem.simparams.sph_formulation == D.SPH_GRENIER
        self.effvisc_on = problem.simparams.rheologytype > D.NEWTONIAN        # NEEDS_EFFECTIVE_VISC
        self.keps = problem.simparams.turbmodel == D.KEPSILON
        self.problem = problem
        self.rank, self.world = rank, world
        self.device = torch.device(device)
        self.is_cuda = self.device.type == "cuda"
        self.sp = problem.simparams
        # formulation<SPH_HA> with SA walls (BiFluidPoiseuilleSA's set) takes the SA density-summation sequence as it is; slabs of it
        # have never run
        if self.sa and self.sp.sph_formulation == D.SPH_HA and world > 1:
            raise NotImplementedError("SPH_HA with SA_BOUNDARY is built for a single domain")
        # floating bodies (bodies 0 .. len-1): their dynamics run on the device (csrc/floating.hip); what is not built is refused
        self.floating = list(getattr(problem, "floating_bodies", None) or ())
        if self.floating:
            # several slabs: every rank sums the rows of the body particles it owns into exact fixed-point limbs, the limbs are added
            # across the ranks, and every rank rounds the sum once and applies the rule to it (csrc/floating_exact.hip): the same
            # bits as the single domain with exact sums.  The default sums are a double addition whose bits depend on the order
            if world > 1 and not getattr(problem, "floating_exact_sums", False):
                raise NotImplementedError("floating bodies on several slabs need the exact body sums (Problem.floating_exact_sums, "
                                          "BuoyancyBox(exact_sums=True)): the default sums in double are built for a single domain")
            if self.sa:
                raise NotImplementedError("floating bodies with SA_BOUNDARY are not built")
            if self.grenier:
                raise NotImplementedError("floating bodies with SPH_GRENIER are not built")
            if self.sp.rheologytype == D.GRANULAR:
                raise NotImplementedError("floating bodies with the GRANULAR rheology are not built")
            if len(self.floating) > self.sp.numforcesbodies:
                raise ValueError("%d floating bodies, but only %d bodies whose forces are computed (numforcesbodies)"
                                 % (len(self.floating), self.sp.numforcesbodies))
        self.part = SlabPartition(problem, world)
        arrs = problem.copy_to_array()
        mask = self.part.local_mask(rank, arrs["hash"]) if world > 1 else np.ones(len(arrs["hash"]), dtype=bool)
        n0 = int(mask.sum())
        self.alloc = int(allocated) if allocated is not None else int(n0 * margin) + 4096
        self.clobber_neibslist = clobber_neibslist
        if kernels is None:
            from .kernels import HipKernels
            kernels = HipKernels(problem, self.alloc, self.device)
        self.k = kernels
        # The EOS rows of the plain forces engine ride with the Euler step (include/sphx.h, sphx_eos_rows_follow_euler): this driver
        # owns the sequence of a step, so it can vouch for the velocity buffer between an Euler step and the forces pass that reads
        # it.  _rows_for = (the tensor the last Euler step wrote, its torch version counter): anything that rewrites it through
        # torch bumps the counter, the library's own rewrites (sort, filters, halo import) go to the other buffer or clear this
        self._rows_for = None
        self._surface_for = None      # the state (_state_key) whose FG_SURFACE flags are in INFO: wave_gages runs the detection otherwise
        # m_peakParticleSpeed / m_peakParticleSpeedTime (src/GPUSPH.cc:88-89): the largest speed any save_diagnostics saw, and when
        self.peak_particle_speed = np.float32(0.0)
        self.peak_particle_speed_time = 0.0
        self._rows_follow = (not self.sa and not self.grenier and not self.effvisc_on and hasattr(kernels, "eos_rows_follow_euler")
                             and problem.simparams.sph_formulation in (D.SPH_F1, D.SPH_F2))
        if self._rows_follow:
            kernels.eos_rows_follow_euler(True)
        # who moves the edge layers: torch.distributed by default, or a transport the caller built (halo.CapiTransport:
        # the library's own sphx_halo_* entry points; a callable gets the kernels of this rank and returns the transport)
        self.transport = None
        if world > 1:
            if callable(transport):
                transport = transport(self.k)
            if transport is None:
                import torch.distributed as dist
                from .halo import TorchTransport
                transport = TorchTransport(dist, self.is_cuda)
            self.transport = transport
        dev, A = self.device, self.alloc
        f32, i32, i16 = torch.float32, torch.int32, torch.int16
        # SA_BOUNDARY: dynamic gamma (no ENABLE_GAMMA_QUADRATURE) or gamma by quadrature, density summation or continuity equation
        self.sa_dynamic_gamma = self.sa and not (self.sp.simflags & D.ENABLE_GAMMA_QUADRATURE)
        self.sa_density_sum = self.sa and bool(self.sp.simflags & D.ENABLE_DENSITY_SUM)
        # SA open boundaries (ENABLE_INLET_OUTLET): the particle count grows inside the allocation.  The density summation form, a
        # rebuild in every iteration (the reference's open-boundary problems set buildneibsfreq = 1: a released particle exists for
        # the lists from the next rebuild on).  See _sa_post_euler_io.
        self.io = self.sa and bool(self.sp.simflags & D.ENABLE_INLET_OUTLET)
        # SA bodies with prescribed motion: BUFFER_BOUNDELEMENTS is a state buffer (BUFFERS)
        self.sa_moving = self.sa and bool(self.sp.simflags & D.ENABLE_MOVING_BODIES)
        if self.sa_moving and self.keps:
            raise NotImplementedError("SA bodies with prescribed motion: not together with k-epsilon")
        if self.io:
            if not self.sa_density_sum or self.keps or self.sp.buildneibsfreq != 1:
                raise NotImplementedError("open boundaries are built for the density summation form without k-epsilon, buildneibsfreq = 1")
            if not hasattr(problem, "impose_open_boundaries"):
                raise ValueError("a problem with ENABLE_INLET_OUTLET needs impose_open_boundaries (its imposeBoundaryConditionHost)")
        # GRANULAR: BUFFER_EFFPRES is solved at initialisation, after the predictor and after the corrector (_solve_effpres); single
        # domain: the exchange of the pressure per Jacobi iteration is not built
        self.granular = self.sp.rheologytype == D.GRANULAR
        if self.granular and world > 1:
            raise NotImplementedError("the GRANULAR rheology is built for a single domain")
        self.energy_on = bool(self.sp.simflags & D.ENABLE_INTERNAL_ENERGY)
        self._bufs = tuple(b for b in BUFFERS if b.has(self))
        self._resorted = tuple(b.name for b in self._bufs if b.resort)
        self._stepped = tuple(b.name for b in self._bufs if b.stepped(self))

        def up(a, dtype, shape):
            t = torch.zeros(shape, dtype=dtype, device=dev)
            t[:n0] = torch.from_numpy(a[mask]).to(dev)
            return t

        self.n_local = n0
        for b in self._bufs:         # both copies of every state buffer, at their fill value
            def full(row):
                return torch.full((A,) + row, b.fill, dtype=b.dtype, device=dev)
            for name in (b.name, b.name + "2"):
                setattr(self, name, {k: full(r) for k, r in b.row.items()} if isinstance(b.row, dict) else full(b.row))
            if b.init == ARRAY:
                a = arrs[b.name]
                getattr(self, b.name)[:n0] = torch.from_numpy((a.view(b.view) if b.view else a)[mask]).to(dev)
        self.info = up(arrs["info"].view(np.int16), i16, (A, 4))
        self.hash = up(arrs["hash"].view(np.int32), i32, (A,))
        self.partindex = torch.zeros(A, dtype=i32, device=dev)
        self.ncells = problem.grid_cells
        self.cellStart = torch.empty(self.ncells, dtype=i32, device=dev)
        self.cellEnd = torch.empty(self.ncells, dtype=i32, device=dev)
        self.neibslist = torch.empty(int(self.sp.neiblistsize) * A, dtype=i16, device=dev)
        self.forces = torch.zeros((A, 4), dtype=f32, device=dev)
        # what every forces pass starts from zero -- the CFL maxima and, with bodies, the RB_FORCES / RB_TORQUES rows -- lies in
        # one allocation, so that it is one memset per pass (three fill kernels of a few microseconds each otherwise)
        ncfl = (self.k.fmax_elements(A) + 8 + 3) // 4 * 4
        nrb = max(getattr(problem, "num_obstacle", 0), 1)
        self._zeroed = torch.zeros(ncfl + 8 * nrb, dtype=f32, device=dev)
        self.cfl = self._zeroed[:ncfl]
        self.cfl_temp = torch.zeros(max(self.k.fmax_temp_elements(self.cfl.numel()), 4), dtype=f32, device=dev)
        self.new_num = torch.zeros(1, dtype=i32, device=dev)
        self.segment_start = torch.zeros(4, dtype=i32, device=dev)
        self.has_rb = bool(getattr(problem, "num_obstacle", 0))      # BUFFER_RB_FORCES / RB_TORQUES rows of body particles
        self.rbforces = self._zeroed[ncfl:ncfl + 4 * nrb].view(nrb, 4)
        self.rbtorques = self._zeroed[ncfl + 4 * nrb:].view(nrb, 4)
        self.devmap = (torch.from_numpy(self.part.compact_device_map(rank).view(np.int32)).to(dev)
                       if world > 1 else None)
        dt0 = float(np.float32(self.sp.dt))
        self.d_dt = torch.full((1,), dt0, dtype=f32, device=dev)
        self.d_dt_next = torch.full((1,), dt0, dtype=f32, device=dev)
        self.d_t = torch.zeros(1, dtype=torch.float64, device=dev)      # simulated time, summed on the device like dt
        self.iterations = 0
        self.n_int = n0
        self.edge_start = n0
        self.send_l = self.send_r = self.recv_l = self.recv_r = (0, 0)
        self.overlap = overlap and self.is_cuda and world > 1
        self.comm_stream = torch.cuda.Stream(device=dev) if self.overlap else None
        # The tiled forces kernel is a persistent grid of one workgroup per CU that owns almost all of the CU's LDS, so the
        # RCCL send/recv kernels of the overlapped exchange would queue behind the inner stripe.  Leave a few CUs (one per
        # XCD by default) out of that grid when the exchange is overlapped (SPHX_COMM_CUS overrides; 0 = none).
        self.comm_cus = int(os.environ.get("SPHX_COMM_CUS", "8")) if self.overlap else 0
        if self.comm_cus and hasattr(self.k, "reserve_comm_cus"):
            self.k.reserve_comm_cus(self.comm_cus)
        # exchange accounting (bench.py --gpus N): bytes sent + received per call, stall of the compute stream on the exchange
        self.halo_bytes = 0
        self.exchange_events = None      # list of (before, after) events on the compute stream around the wait, when enabled
        self.profile_forces = None
        self.track_particle_count = track_particle_count
        # SPS: BUFFER_TAU as three float2 arrays, computed for the internal particles before each forces pass and imported
        # for the halo (CALC_VISC + UPDATE_EXTERNAL, src/integrators/PredictorCorrectorIntegrator.cc:460-480)
        self.sps = self.sp.turbmodel == D.SPS
        self.tau = [torch.zeros((A, 2), dtype=f32, device=dev) for _ in range(3)] if self.sps else None
        self.turbvisc = torch.zeros(A, dtype=f32, device=dev) if self.sps else None      # BUFFER_SPS_TURBVISC
        # ENABLE_XSPH: BUFFER_XSPH, written by every forces pass for the fluid particles, read by the Euler steps
        self.xsph = torch.zeros((A, 4), dtype=f32, device=dev) if (self.sp.simflags & D.ENABLE_XSPH) else None
        # what the option sets hold beside their state buffers
        if self.sa:      # BUFFER_VERTPOS (3 x float2) is written by the list build
            self.vertpos = [torch.zeros((A, 2), dtype=f32, device=dev) for _ in range(3)]
            # dynamic gamma: BUFFER_CFL_GAMMA, per particle and, behind round_up(n, 4), per block
            self.cfl_gamma = (torch.zeros(A + 4 + self.cfl.numel(), dtype=f32, device=dev) if self.sa_dynamic_gamma else None)
        if self.io:      # IOwaterdepth is one uint per open boundary
            self.water_depth_on = bool(self.sp.simflags & D.ENABLE_WATER_DEPTH)
            self.iowaterdepth = torch.zeros(max(int(problem.num_open_boundaries), 1), dtype=i32, device=dev) if self.water_depth_on else None
            self.io_count = torch.zeros(1, dtype=i32, device=dev)         # newNumParticles of the vertex pass
            self.io_created = self.io_removed = 0
        if self.keps:    # BUFFER_DKDE and BUFFER_CFL_KEPS are outputs of the forces passes
            self.dkde = torch.zeros((A, 3), dtype=f32, device=dev)
            self.cfl_keps = torch.zeros_like(self.cfl)
        self.effvisc = torch.zeros(A, dtype=f32, device=dev) if self.effvisc_on else None      # BUFFER_EFFVISC
        if self.granular:
            self.jacobi_iterations = {}      # phase ("init", "predictor", "corrector") -> h_jacobiCounter of its last solve
            self.jacobi_last = {}            # ... -> (backward error, residual) its stop test saw
            self.jacobi_max_iterations = 0   # the largest counter of any solve so far
        if self.energy_on:
            self.dedt = torch.zeros(A, dtype=f32, device=dev)      # the rate of BUFFER_INTERNAL_ENERGY
        if self.grenier:
            self.sigma = torch.zeros(A, dtype=f32, device=dev)     # BUFFER_SIGMA
        for b in self._bufs:         # the buffers that a call sets up
            if b.init not in (ARRAY, FILL):
                getattr(self, b.init)(arrs, mask, n0)
        self.filters = []            # [(FilterType, frequency)]
        # bodies with prescribed motion: every rank runs the same host kinematics (the callback is a pure function of time)
        self.bodies = None
        if getattr(problem, "moving_bodies_callback", None) is not None and getattr(problem, "num_obstacle", 0):
            from .bodies import MovingBodies
            self.bodies = MovingBodies(problem, problem.rb_cg_global, first=len(self.floating))
        self.t_host = 0.0
        if self.floating:            # the device takes over their slots of the rigid-body table; rows of RB_FORCES per body
            rowstart = np.asarray(problem.rb_rowstart, dtype=np.uint32)
            if len(rowstart) != len(self.floating) + 1 or int(rowstart[-1]) > self.rbforces.shape[0]:
                raise ValueError("rb_rowstart: one entry per floating body and one behind, inside the %d RB_FORCES rows" % self.rbforces.shape[0])
            self.k.floating_setup(self.floating, rowstart)
        self.floating_exact = bool(self.floating) and bool(getattr(problem, "floating_exact_sums", False))
        if self.floating_exact:      # [bodies, 6 components, limbs and counts], integer-valued doubles (include/sphx.h)
            from .capi import SPHX_FLOATING_LIMBS
            self.floating_limbs = torch.zeros((len(self.floating), 6, SPHX_FLOATING_LIMBS), dtype=torch.float64, device=dev)

    # ------------------------------------------------------------------ state buffers (BUFFERS)
    def _init_next_ids(self, arrs, mask, n0):
        """initializeNextIDs (src/GPUSPH.cc:1256-1302): the vertices of open boundaries get totParticles, totParticles + 1, ... in
        particle order; nobody else has one"""
        flags = arrs["info"][:, 0]
        openv = ((flags & 7) == D.PT_VERTEX) & ((flags & (D.FG_INLET | D.FG_OUTLET)) != 0)
        nid = np.full(len(flags), 0xFFFFFFFF, dtype=np.uint32)
        nid[openv] = len(flags) + np.arange(int(openv.sum()), dtype=np.uint32)
        self.num_open_vertices = int(openv.sum())
        self.next_ids[:n0] = torch.from_numpy(nid.view(np.int32)[mask]).to(self.device)

    def _init_keps(self, arrs, mask, n0):
        """ProblemCore::init_keps and init_turbvisc (src/ProblemCore.cc:1623-1659): the uniform initial state"""
        for t, v in zip(_tensors(self.ke), self.problem.init_keps()):      # k, epsilon, nu_t; the Eulerian velocity stays zero
            t.fill_(v)

    def _init_volume(self, arrs, mask, n0):
        self.k.init_volume(self.vol, self.pos, self.vel, self.info, n0)      # GPUSPH.cc:495-496

    @property
    def _lists(self):
        """what nearly every pass over the neighbours reads beside the state, to splat into the call; read when the call is made (a
        re-sort renames info and hash)"""
        return self.info, self.hash, self.cellStart, self.neibslist

    def _swap(self, *names):
        """rename <name> <-> <name>2"""
        for name in names:
            cur, other = getattr(self, name), getattr(self, name + "2")
            setattr(self, name, other); setattr(self, name + "2", cur)

    def _state_of(self, pos):
        """The state buffers that go with `pos`: those of the current state for self.pos, for anything else (self.pos2: n* and
        n+1 while a step is under way) the copy that the step writes, where it writes one."""
        new = pos is not self.pos
        return SimpleNamespace(**{b.name: getattr(self, b.name + "2" if new and b.name in self._stepped else b.name) for b in self._bufs})

    def halo_state(self):
        """what _update_segments_and_halo exchanges after a re-sort, in the order both ranks share"""
        state = [t for b in self._bufs if b.halo for t in _tensors(getattr(self, b.name))]
        return state[:2] + [self.info, self.hash] + state[2:]

    def _hot_rows(self):
        """(HotFile key, device tensor, dtype of the host array or None) of the option-dependent buffers a HotFile stores"""
        return [(k, t, b.view) for b in self._bufs if b.hot for k, t in _items(b.name, getattr(self, b.name))]

    # ------------------------------------------------------------------ exchange
    def _neighbours(self):
        if self.world > 1 and self.part.ring:
            return (self.rank - 1) % self.world, (self.rank + 1) % self.world
        left = self.rank - 1 if self.rank > 0 else None
        right = self.rank + 1 if self.rank < self.world - 1 else None
        return left, right

    def _exchange(self, tensors):
        """UPDATE_EXTERNAL of what a pass over the internal particles wrote: send my edge layers / receive the halo layers of
        every tensor in `tensors` (dim-0 ranges).  A single domain has no halo and no transport."""
        if self.transport is None:
            return
        left, right = self._neighbours()
        self.halo_bytes += self.transport.exchange(tensors, left, right, self.send_l, self.recv_l, self.send_r, self.recv_r)

    # ------------------------------------------------------------------ neighbour phase
    def build_neibs(self):
        K = self.k
        n = self.n_local
        self._rows_for = None
        if self.iterations == 0:
            K.fix_hash(self.hash, self.partindex, self.info, self.devmap, n)
        else:
            K.calc_hash(self.pos, self.hash, self.partindex, self.info, self.devmap, n)
        K.sort(self.hash, self.info, self.partindex, n)
        K.memset(self.cellStart, 0xFF)
        K.memset(self.cellEnd, 0xFF)
        K.reorder(self.segment_start if self.world > 1 else None, self.cellStart, self.cellEnd, self.pos2, self.vel2,
                  self.pos, self.vel, self.info, self.hash, self.partindex, n, self.new_num)
        for b in self._bufs:         # the arrays that reorderDataAndFindCellStart does not take along
            if b.resort == GATHER:
                for dst, src in zip(_tensors(getattr(self, b.name + "2")), _tensors(getattr(self, b.name))):
                    K.gather_rows(dst, src, self.partindex, n)
        self._swap(*self._resorted)
        if self.world == 1:
            if self.track_particle_count:
                before = self.n_local
                self.n_local = int(self.new_num.item()) & 0xFFFFFFFF
                if self.io:
                    self.io_removed += before - self.n_local
            self.n_int = self.n_local
            self.edge_start = self.n_int
        else:
            self._update_segments_and_halo()
        if self.clobber_neibslist:
            K.memset(self.neibslist, 0xFF)
        if self.sa:
            K.build_neibs_sa(self.neibslist, self.vertpos, self.pos, self.info, self.vertices, self.boundelements, self.hash,
                             self.cellStart, self.cellEnd, self.n_local, self.n_int)
            self._exchange(self.vertpos)      # the vertex offsets of the halo segments (UPDATE_EXTERNAL of BUFFER_VERTPOS after BUILDNEIBS)
        else:
            K.build_neibs(self.neibslist, self.pos, self.info, self.hash, self.cellStart, self.cellEnd, self.n_local, self.n_int)

    def _dt_op(self, step):
        """dt of the substep on the host, as the reference's commands carry it: half a step and a whole step are exact in float"""
        return float(np.float32(self.d_dt.item()) * np.float32(0.5 if step == 1 else 1.0))

    def _sa_bc(self, st, step, run_mode=D.SIMULATE):
        """SA_CALC_SEGMENT_BOUNDARY_CONDITIONS and SA_CALC_VERTEX_BOUNDARY_CONDITIONS on the state `st` (_state_of), in place, each
        over the internal particles and followed by the UPDATE_EXTERNAL of what it wrote; with k-epsilon the passes that also set
        k, epsilon and the Eulerian velocity of the wall"""
        K, n, ni = self.k, self.n_local, self.n_int
        if self.keps and run_mode == D.SIMULATE:
            ke = st.ke
            walls = [ke["tke"], ke["eps"], ke["eulervel"]]
            K.sa_segment_bc_keps(st.vel, st.gradgamma, ke, st.pos, self.vertices, self.boundelements, *self._lists, n, ni, step)
            self._exchange([st.vel, st.gradgamma] + walls)
            K.sa_vertex_bc_keps(st.vel, st.gradgamma, ke, self.vertices, self.boundelements, st.pos, *self._lists, n, ni, step)
            self._exchange([st.vel] + walls)
            return
        K.sa_segment_bc(st.vel, st.gradgamma, st.pos, self.vertices, st.boundelements, *self._lists, n, ni, step, run_mode)
        self._exchange([st.vel, st.gradgamma])
        K.sa_vertex_bc(st.vel, st.gradgamma, st.pos, *self._lists, n, ni, step, run_mode)
        self._exchange([st.vel])

    def _sa_bc_io(self, st, dt, step):
        """The same pair with open boundaries, on the state `st`: IMPOSE_OPEN_BOUNDARY_CONDITION (the problem's values; it consumes
        and clears the water depth, the maximum over the devices), the segment conditions, in the last step FIND_OUTGOING_SEGMENT,
        the vertex conditions (vertex masses; in the last step the take-over of outgoing particles and the release of new ones: the
        particle count grows), in the last step DISABLE_OUTGOING_PARTS"""
        K, n, ni = self.k, self.n_local, self.n_int
        self._io_impose(st.pos, st.vel, st.eulervel)
        K.sa_segment_bc_io(st.vel, st.gradgamma, st.eulervel, st.pos, self.vertices, st.boundelements, *self._lists, n, ni, step)
        self._exchange([st.vel, st.gradgamma, st.eulervel])
        if step == 2:
            K.sa_find_outgoing_segment(st.pos, st.vel, self.vertices, st.gradgamma, self.vertpos, st.boundelements, *self._lists, n, ni)
            self._exchange([self.vertices, st.gradgamma])      # the marks: a vertex takes over from the halo's particles too
        self._io_vertex_bc(st.pos, st.vel, st.gradgamma, st.eulervel, dt, step, st.boundelements)
        if step == 2:
            K.sa_disable_outgoing_parts(st.pos, self.vertices, self.info, self.n_local)

    def _sa_post_euler(self, step):
        """INTEGRATE_GAMMA on the new positions (always from the gamma of step n), then the boundary conditions of the new
        state (PredictorCorrectorIntegrator.cc:661-684 and the post-step phases); every pass covers the internal particles and is
        followed by the UPDATE_EXTERNAL of what it wrote"""
        K, n, ni = self.k, self.n_local, self.n_int
        new = self._state_of(self.pos2)      # (its elements are those of the new state)
        if self.sa_density_sum:
            # DENSITY_SUM [+ CALC_DENSITY_DIFFUSION + APPLY_DENSITY_DIFFUSION] (PredictorCorrectorIntegrator.cc:607-659): density and
            # gamma of the new state from the positions of step n and of the new state; BUFFER_FORCES is their scratch
            if self.sa_moving:       # ... and from the elements where they were and where they are; gamma of the vertices too
                K.sa_density_sum_moving(self.vel2, self.gradgamma2, self.forces, self.pos, self.pos2, self.vel, self.gradgamma,
                                        self.boundelements, new.boundelements, self.vertpos, *self._lists, n, ni)
            else:
                K.sa_density_sum(self.vel2, self.gradgamma2, self.forces, self.pos, self.pos2, self.vel, self.gradgamma, self.boundelements,
                                 self.vertpos, *self._lists, n, ni)
            self._exchange([self.vel2, self.gradgamma2])
            if self.sp.densitydiffusiontype == D.BREZZI:
                K.sa_density_diffusion(self.forces, self.pos2, self.vel2, self.gradgamma2, *self._lists, n, ni, self._dt_op(step))
                self._exchange([self.vel2])
        else:
            K.sa_integrate_gamma(self.gradgamma2, self.gradgamma, self.pos2, new.boundelements, self.vertpos, *self._lists, n, ni)
            self._exchange([self.gradgamma2])
        self._sa_bc(new, step)

    def _sa_post_euler_io(self, step):
        """The post-Euler commands of a step with ENABLE_INLET_OUTLET (src/integrators/PredictorCorrectorIntegrator.cc:127-300,
        607-684): DENSITY_SUM [+ density diffusion] with the open boundaries' terms from the state of step n, then the boundary
        conditions of the new state (_sa_bc_io).  Every pass covers the internal particles and is followed by the UPDATE_EXTERNAL
        of what it wrote."""
        K, n, ni = self.k, self.n_local, self.n_int
        dt = self._dt_op(step)
        # with bodies that move as well (the option set of CompleteSaExample.cu:46): the elements of step n and of the new state in
        # the density summation, those of the new state in everything that follows (as without open boundaries, _sa_post_euler)
        new = self._state_of(self.pos2)
        if self.sa_moving:
            K.sa_density_sum_io_moving(self.vel2, self.gradgamma2, self.forces, self.pos, self.pos2, self.vel, self.eulervel, self.gradgamma,
                                       self.boundelements, new.boundelements, self.vertpos, *self._lists, n, ni, dt)
        else:
            K.sa_density_sum_io(self.vel2, self.gradgamma2, self.forces, self.pos, self.pos2, self.vel, self.eulervel, self.gradgamma,
                                self.boundelements, self.vertpos, *self._lists, n, ni, dt)
        self._exchange([self.vel2, self.gradgamma2])
        if self.sp.densitydiffusiontype == D.BREZZI:
            K.sa_density_diffusion_io(self.forces, self.pos2, self.vel2, self.gradgamma2, new.boundelements, self.vertpos, *self._lists,
                                      n, ni, dt)
            self._exchange([self.vel2])
        self.eulervel2[:n] = self.eulervel[:n]
        self._sa_bc_io(new, dt, step)

    def _io_impose(self, pos, vel, eulervel):
        """IMPOSE_OPEN_BOUNDARY_CONDITION on every particle this device holds (the values are a function of position, time and
        the water level); over several devices the level is the maximum of theirs first (DOWNLOAD_IOWATERDEPTH,
        FIND_MAX_IOWATERDEPTH, UPLOAD_IOWATERDEPTH: src/integrators/PredictorCorrectorIntegrator.cc:214-222, GPUSPH.cc:2206-2226)"""
        if self.world > 1 and self.iowaterdepth is not None:
            mine = (self.iowaterdepth.to(torch.int64) & 0xFFFFFFFF).cpu().tolist()
            best = [max(v for v, _ in self.transport.allgather_pair(m, 0, self.device)) for m in mine]
            self.iowaterdepth.copy_(torch.tensor(best, dtype=torch.int64).to(torch.int32).to(self.device)
                                    if max(best) < 2 ** 31 else
                                    torch.from_numpy(np.array(best, dtype=np.uint32).view(np.int32)).to(self.device))
        self.problem.impose_open_boundaries(pos, vel, eulervel, self.info, self.hash, self.iowaterdepth, self.time(), self.n_local)

    def _io_vertex_bc(self, pos, vel, ggam, eulervel, dt, step, boundelements):
        """SA_CALC_VERTEX_BOUNDARY_CONDITIONS with open boundaries: the pass writes the vertex masses (and the rows of released
        particles) into `pos`, in place as the reference has it; the new particle count comes back in a device word.  Released
        particles are appended behind everything this device holds (its halo included); they belong to it (the hash of the vertex
        that released them) and are sorted in at the next rebuild"""
        K, n, ni = self.k, self.n_local, self.n_int
        self.io_count[0] = n
        K.sa_vertex_bc_io(vel, pos, pos, ggam, eulervel, self.forces, self.vertices, boundelements, self.vertpos,
                          self.info, self.hash, self.next_ids, self.io_count, self.cellStart, self.neibslist, n, ni, self.alloc,
                          dt, step, self.num_open_vertices)      # (the rows of released particles are written to `boundelements` too)
        n2 = int(self.io_count.item()) & 0xFFFFFFFF
        if n2 > self.alloc:
            raise RuntimeError("open boundaries released more particles than the allocation holds (%d > %d)" % (n2, self.alloc))
        self._exchange([pos, vel, eulervel])      # vertex masses, densities and Eulerian velocities of the halo's vertices
        self.io_created += n2 - n
        self.n_local = n2
        if self.world == 1:
            self.n_int = self.edge_start = n2

    def calc_private(self):
        """CALC_PRIVATE of the post-processing engine (src/cuda/post_process.cu:575-640: Problem::calcPrivate fills BUFFER_PRIVATE
        with whatever the problem defines, from positions, velocities, info, the hash and the neighbour list): the problem's
        `calc_private(engine)` gets the engine (its tensors live on the device) and returns one row per particle"""
        fn = getattr(self.problem, "calc_private", None)
        if fn is None:
            raise NotImplementedError("CALC_PRIVATE: the problem defines no calc_private (the reference's default throws as well)")
        out = fn(self)
        if out.shape[0] != self.n_local:
            raise ValueError("calc_private: one row per particle held by this device expected")
        return out

    def open_boundary_flux(self):
        """FLUX_COMPUTATION of the post-processing engine (src/cuda/post_process.cu:485-570) on the current state: per open boundary
        the volume flux sum A_s (u_E . n_s) through its segments, positive into the domain.  -> float32 tensor [num_open_boundaries]"""
        if not self.io:
            raise ValueError("the flux through open boundaries needs ENABLE_INLET_OUTLET")
        nob = int(self.problem.num_open_boundaries)
        flux = torch.zeros(max(nob, 1), dtype=torch.float32, device=self.device)
        self.k.flux_computation(flux, self.info, self.eulervel, self.boundelements, self.n_local, nob)
        return flux[:nob]

    def sa_boundary_conditions(self, step, run_mode=D.SIMULATE):
        """initializeBoundaryConditionsSequence<SA_BOUNDARY> (src/integrators/PredictorCorrectorIntegrator.cc:117-290): at
        initialisation (step 0) the vertex normals and gamma, then in every step the segment and the vertex boundary conditions,
        in place on the current state (_sa_bc; with open boundaries the initialisation sequence only, _sa_bc_io); internal
        particles, then UPDATE_EXTERNAL."""
        if not self.sa:
            raise ValueError("boundary conditions sequence of a problem without SA_BOUNDARY")
        K, n, ni = self.k, self.n_local, self.n_int
        if step == 0:
            K.sa_compute_vertex_normal(self.boundelements, self.vertices, *self._lists, n, ni)
            self._exchange([self.boundelements])
            K.sa_init_gamma(self.gradgamma2, self.gradgamma, self.pos, self.boundelements, self.vertpos, *self._lists, n, ni)
            self._swap("gradgamma")
            self._exchange([self.gradgamma])
        if not self.io:
            return self._sa_bc(self._state_of(self.pos), step, run_mode)
        # with open boundaries (:150-290): corner vertices, the initial masses of the open vertices, then the imposed values and
        # the two condition passes of step 0
        if step != 0 or run_mode != D.SIMULATE:
            raise NotImplementedError("open boundaries: only the initialisation sequence goes through sa_boundary_conditions")
        K.sa_identify_corner_vertices(self.pos, self.info, self.hash, self.vertices, self.cellStart, self.neibslist, n, ni)
        self._exchange([self.info])
        K.sa_init_io_mass_vertex_count(self.forces, self.pos, self.vertices, self.hash, self.info, self.cellStart, self.neibslist, n, ni)
        self._exchange([self.forces])      # a vertex divides by the counts of the vertices it shares segments with, the halo's among them
        K.sa_init_io_mass(self.pos2, self.pos, self.forces, self.vertices, self.hash, self.info, self.cellStart, self.neibslist, n, ni)
        self.pos2[ni:n] = self.pos[ni:n]      # (the pass writes the internal rows)
        self._swap("pos")
        self._exchange([self.pos])
        self._sa_bc_io(self._state_of(self.pos), 0.0, 0)

    def _update_segments_and_halo(self):
        """UPDATE_SEGMENTS + CROP + APPEND_EXTERNAL (src/Integrator.cc:170-230)"""
        K = self.k
        seg = [int(v) & 0xFFFFFFFF for v in self.segment_start.cpu().tolist()]       # DOWNLOAD (sync)
        newn = int(self.new_num.item()) & 0xFFFFFFFF
        starts = list(seg) + [newn]
        for i in range(3, -1, -1):                 # EMPTY_SEGMENT -> start of the next non-empty one
            if starts[i] == D.EMPTY_SEGMENT:
                starts[i] = starts[i + 1]
        edge_start, n_int = starts[1], starts[2]   # internal = inner + inner edge; the rest is cropped
        self.edge_start, self.n_int = edge_start, n_int
        left, right = self._neighbours()
        # my inner-edge segment is sorted by hash: the plane facing the left neighbour comes first
        if left is not None and right is not None:
            key = (D.CELLTYPE_INNER_EDGE_CELL << 30) | ((self.part.hi[self.rank] - 1) * self.part.plane)
            h = self.hash[edge_start:n_int].to(torch.int64) & 0xFFFFFFFF
            split = edge_start + int(torch.searchsorted(h, torch.tensor([key], dtype=torch.int64, device=h.device)).item())
        elif left is not None:
            split = n_int
        else:
            split = edge_start
        self.send_l = (edge_start, split) if left is not None else (0, 0)
        self.send_r = (split, n_int) if right is not None else (0, 0)
        # counts of the layers my neighbours send me
        allc = self.transport.allgather_pair(self.send_l[1] - self.send_l[0], self.send_r[1] - self.send_r[0], self.device)
        rl = allc[left][1] if left is not None else 0      # left neighbour's right layer
        rr = allc[right][0] if right is not None else 0    # right neighbour's left layer
        if n_int + rl + rr > self.alloc:
            raise RuntimeError("rank %d: %d internal + %d halo particles exceed the %d allocated"
                               % (self.rank, n_int, rl + rr, self.alloc))
        self.recv_l = (n_int, n_int + rl)
        self.recv_r = (n_int + rl, n_int + rl + rr)
        self.n_local = n_int + rl + rr
        self._exchange(self.halo_state())
        # imported cells are OUTER_EDGE cells here whatever they are at home
        if self.n_local > n_int:
            hs = self.hash[n_int:self.n_local]
            hs.bitwise_and_(D.CELLTYPE_BITMASK).bitwise_or_(-2147483648)          # CELLTYPE_OUTER_EDGE_CELL << 30
        # cell ranges: forget everything outside my own planes, then index the fresh halo
        lo, hi, plane = self.part.lo[self.rank] * self.part.plane, self.part.hi[self.rank] * self.part.plane, self.part.plane
        for t in (self.cellStart, self.cellEnd):
            if lo > 0:
                K.memset(t[:lo], 0xFF)
            if hi < self.ncells:
                K.memset(t[hi:], 0xFF)
        K.find_cell_start(self.cellStart, self.cellEnd, self.hash, n_int, self.n_local)

    # ------------------------------------------------------------------ forces / euler
    def _solve_effpres(self, phase, pos, vel):
        """INIT_ / POSTPRED_ / POSTCORR_EFFPRES_PREP and the Jacobi loop behind it (PredictorCorrectorIntegrator.cc:962-1008,
        1046-1182) on the given state, as one call; the surface and interface flags are those the last
        postprocess(INTERFACE_DETECTION) left in INFO.  Synchronises (the iteration count comes back)."""
        it, err, res = self.k.jacobi_solve(self.effpres, pos, vel, *self._lists, self.n_local, self.n_int)
        self.jacobi_iterations[phase] = it
        self.jacobi_last[phase] = (err, res)
        self.jacobi_max_iterations = max(self.jacobi_max_iterations, it)

    # The forces entry of each option set.  _forces_<set>(pos, vel, step, run_mode) first computes what its entry reads beside the
    # state, over the internal particles and with the UPDATE_EXTERNAL of it, and returns (launch, outputs): launch(from, to, offset
    # into the CFL array) runs the entry on a range of particles and returns its blocks; `outputs` is what the entry writes beside
    # BUFFER_FORCES that the halo copies integrate from.
    def _forces_sa(self, pos, vel, step, run_mode):
        """forces engine of SA_BOUNDARY: the state's gamma, the boundary elements, the vertex offsets of the segments, its k-epsilon
        fields, its Eulerian velocities"""
        K, st = self.k, self._state_of(pos)
        ke = st.ke if (self.keps and run_mode == D.SIMULATE) else None
        if ke is not None:
            K.memset(self.cfl_keps, 0)
        # bodies that feel the fluid (FG_COMPUTE_FORCE segments): the pressure force on their elements rides with the pass
        # (compute_boundary_pressure_force inside finalizeforcesDevice, src/cuda/forces_kernel.def:4115-4145)
        body_forces = self.has_rb and self.sp.numforcesbodies > 0 and run_mode == D.SIMULATE

        def launch(frm, to, off):
            if ke is not None:
                nb = K.forces_sa_keps(self.forces, self.cfl, self.cfl_keps, self.dkde, pos, vel, *self._lists, st.gradgamma,
                                      self.boundelements, self.vertpos, ke, self.n_local, frm, to, off, cfl_gamma=self.cfl_gamma)
            elif self.io:    # the Eulerian velocity of the open boundaries in the viscous terms and in the gamma CFL condition
                nb = K.forces_sa_io(self.forces, self.cfl, pos, vel, st.eulervel, *self._lists, st.gradgamma, st.boundelements,
                                    self.vertpos, self.n_local, frm, to, off, cfl_gamma=self.cfl_gamma)
            else:
                nb = K.forces_sa(self.forces, self.cfl, pos, vel, *self._lists, st.gradgamma, st.boundelements, self.vertpos,
                                 self.n_local, frm, to, off, cfl_gamma=self.cfl_gamma, run_mode=run_mode)
            if body_forces:
                K.sa_body_pressure_forces(self.forces, self.rbforces, self.rbtorques, pos, vel, self.info, self.hash, st.boundelements, frm, to)
            return nb
        # BUFFER_DKDE is a POST_FORCES_UPDATE_BUFFER: the halo copies integrate k and epsilon from the exchanged rates
        return launch, ([] if ke is None else [self.dkde])

    def _forces_effvisc(self, pos, vel, step, run_mode):
        """generalized Newtonian rheology: CALC_VISC on the state the forces read; its largest kinematic viscosity is the viscous
        limit of this pass's dt on this device (the dt of the step is the minimum over the devices)"""
        K = self.k
        if self.granular:      # the yield stress of the sediment comes from BUFFER_EFFPRES
            K.calc_effvisc_granular(self.effvisc, self.effpres, pos, vel, *self._lists, self.n_local, self.n_int)
        else:
            K.calc_effvisc(self.effvisc, pos, vel, *self._lists, self.n_local, self.n_int)
        self._exchange([self.effvisc])
        return (lambda frm, to, off: K.forces_effvisc(self.forces, self.cfl, pos, vel, *self._lists, self.effvisc, self.n_local,
                                                      frm, to, off)), []

    def _forces_grenier(self, pos, vel, step, run_mode):
        """SPH_GRENIER: COMPUTE_DENSITY on the state the forces read, UPDATE_EXTERNAL of sigma and of the rewritten velocity buffer
        (PredictorCorrectorIntegrator.cc:443-458), then the Grenier forces"""
        K = self.k
        K.compute_density(self.sigma, vel, pos, self.info, self.hash, self._state_of(pos).vol, self.cellStart, self.neibslist, self.n_int)
        self._exchange([self.sigma, vel])
        return (lambda frm, to, off: K.forces_grenier(self.forces, self.cfl, pos, vel, *self._lists, self.sigma, self.n_local,
                                                      frm, to, off)), []

    def _forces_plain(self, pos, vel, step, run_mode):
        """the plain forces engine (and every engine's REPACK pass but SA's): SPS stresses, XSPH, the rows of the bodies"""
        K = self.k
        args = (self.forces, self.cfl, self.rbforces if self.has_rb else None, self.rbtorques if self.has_rb else None, pos, vel,
                *self._lists, self.n_local)
        kw = dict(tau=self.tau) if self.sps and run_mode == D.SIMULATE else {}
        if self.xsph is not None:
            kw["xsph"] = self.xsph
        if run_mode != D.SIMULATE or step != 1:
            kw.update(run_mode=run_mode, step=step)
        follow = self._rows_follow and run_mode == D.SIMULATE
        vouch = [follow and self._rows_for is not None and self._rows_for[0] is vel and vel._version == self._rows_for[1]]

        def launch(frm, to, off):
            if vouch[0]:
                K.eos_rows_current(vel, self.n_local)
            vouch[0] = follow      # a second stripe of this pass reads the buffer the first one read
            return K.forces(*args, frm, to, off, **kw)
        return launch, []

    def _launch_stripes(self, launch, outputs, e0):
        """`launch` over the internal particles, then the UPDATE_EXTERNAL of `outputs`; returns the blocks launched.  With a halo the
        edge stripe goes first and its forces travel, on the exchange stream when overlapped, while the inner stripe computes.
        `e0`: the event that opened an interval of profile_forces, or None."""
        def profiled():
            if e0 is not None:
                e1 = torch.cuda.Event(enable_timing=True)
                e1.record(); self.profile_forces.append((e0, e1))
        if self.world > 1 and self.n_int > self.edge_start:
            # edge stripe first, then the inner stripe while the edge forces travel
            nb1 = launch(self.edge_start, self.n_int, 0)
            if self.overlap:
                ev = torch.cuda.Event(); ev.record()
            nb2 = launch(0, self.edge_start, nb1)
            profiled()
            if self.overlap:
                with torch.cuda.stream(self.comm_stream):
                    self.comm_stream.wait_event(ev)
                    self._exchange(outputs)
                if self.exchange_events is not None:     # how long the compute stream sits waiting for the halo forces
                    b = torch.cuda.Event(enable_timing=True); a_ = torch.cuda.Event(enable_timing=True)
                    b.record()
                torch.cuda.current_stream(self.device).wait_stream(self.comm_stream)
                if self.exchange_events is not None:
                    a_.record(); self.exchange_events.append((b, a_))
            else:
                self._exchange(outputs)
            return nb1 + nb2
        nb = launch(0, self.n_int, 0)
        profiled()
        self._exchange(outputs)
        return nb

    def _forces(self, pos, vel, step, combine_min, run_mode=D.SIMULATE):
        """One forces pass on the given state: CALC_VISC and what else the option set's entry reads (_forces_sa, _forces_effvisc,
        _forces_grenier, _forces_plain), the entry over one stripe or two (_launch_stripes), then the reductions of this pass's dt
        into d_dt_next (`combine_min`: the minimum with what the predictor's pass left there)."""
        K, simulate = self.k, run_mode == D.SIMULATE
        # (with bodies: rows of body particles owned by other ranks must read zero in the reduction)
        K.memset(self._zeroed if self.has_rb else self.cfl, 0)
        e0 = None
        if self.profile_forces is not None and self.is_cuda:
            e0 = torch.cuda.Event(enable_timing=True)
            e0.record()
        if self.sps and simulate:   # CALC_VISC on the state the forces read (PredictorCorrectorIntegrator.cc:460-480)
            K.calc_visc(self.tau, pos, vel, *self._lists, self.n_local, self.n_int, turbvisc=self.turbvisc)
            self._exchange(self.tau)
        entry = (self._forces_sa if self.sa else self._forces_effvisc if self.effvisc_on and simulate else
                 self._forces_grenier if self.grenier and simulate else self._forces_plain)
        launch, more = entry(pos, vel, step, run_mode)
        outputs = [self.forces]
        if self.energy_on and simulate:      # the BUFFER_INTERNAL_ENERGY_UPD output of the pass travels with the forces
            K.forces_internal_energy(self.dedt, pos, vel, *self._lists, self.n_local, 0, self.n_int)
            outputs.append(self.dedt)
        if self.xsph is not None and simulate:      # BUFFER_XSPH is a POST_FORCES_UPDATE_BUFFER: the halo copies are moved with it
            outputs.append(self.xsph)
        nb = self._launch_stripes(launch, outputs + more, e0)
        K.dtreduce(self.cfl, self.cfl_temp, nb, self.d_dt_next, combine_min)
        if self.keps and simulate:         # viscous limit with the largest eddy viscosity (src/cuda/forces.cu:585-598)
            K.dtreduce_keps(self.cfl_keps, nb, self.d_dt_next)
        if self.sa and self.sa_dynamic_gamma and simulate:     # the CFL condition of the gamma transport (src/cuda/forces.cu:576-585)
            K.dtreduce_gamma(self.cfl_gamma, self.n_local, nb, self.d_dt_next)
        if self.io and self.water_depth_on:      # the vertex pass of the forces (vertex_forces, src/cuda/forces.cu:676-686)
            K.sa_io_water_depth(self.iowaterdepth, pos, *self._lists, self.n_local, 0, self.n_int)

    def _euler(self, step, dt_scale, run_mode=D.SIMULATE):
        """the EULER command of the plain integrator: the new positions and velocities from the state of step n and BUFFER_FORCES"""
        kw = dict(xsph=self.xsph) if self.xsph is not None else {}
        if run_mode != D.SIMULATE:
            kw["run_mode"] = run_mode
        self.k.euler(self.pos2, self.vel2, self.pos, self.vel, self.info, self.hash, self.forces, self.n_local, self.d_dt,
                     dt_scale, step, **kw)

    def apply_filter(self, filtertype):
        """FILTER_CALL phase (src/integrators/PredictorCorrectorIntegrator.cc:831-859): read the unfiltered velocities, write the
        filtered ones of the internal particles, UPDATE_EXTERNAL, swap the two VEL buffers."""
        self._rows_for = None      # the velocity buffer may be rewritten behind torch's back (_rows_for)
        self.k.filter(int(filtertype), self.vel2, self.pos, self.vel, *self._lists, self.n_local, self.n_int)
        self._exchange([self.vel2])
        self._swap("vel")

    def _substep(self, step, dt_host=None):
        """Predictor (step 1): forces(n) -> n* = n + dt/2 f.  Corrector (step 2): forces(n*) -> n+1 = n + dt f*, written over n*.
        Every update integrates from the state of step n into the second copy of its buffer.  `dt_host`: dt for the bodies'
        callback."""
        K, n, dt_scale = self.k, self.n_local, (0.5 if step == 1 else 1.0)
        pos, vel = (self.pos, self.vel) if step == 1 else (self.pos2, self.vel2)
        self._forces(pos, vel, step, combine_min=step - 1)
        if self.bodies is not None:                 # MOVE_BODIES + uploads (PredictorCorrectorIntegrator.cc:550-570)
            self._last_motion = self.bodies.timestep(step, dt_host, self.t_host)
            K.set_body_motion(self._last_motion, self.sp.numforcesbodies > 0)
        if self.floating:                           # ... of the floating bodies, on the device and behind the host's uploads
            if self.floating_exact:
                # a rank writes the rows of the body particles it owns and no others: the pass zeroes the buffer (_forces) and runs
                # over [0, n_int) alone, the row is id + rbstart, global; so the ranks' limbs add up to the limbs of all rows
                K.floating_limbs(self.rbforces, self.rbtorques, self.floating_limbs)
                if self.world > 1:
                    self.transport.allreduce_sum(self.floating_limbs)
                K.floating_move_limbs(self.floating_limbs, step, self.d_dt)
            else:
                K.floating_move(self.rbforces, self.rbtorques, step, self.d_dt)
        if self.grenier:             # with the volumes, which the corrector overwrites like pos and vel
            K.euler_grenier(self.pos2, self.vel2, self.vol2, self.pos, self.vel, self.vol, self.info, self.hash, self.forces, n, self.d_dt,
                            dt_scale, step)
        else:
            self._euler(step, dt_scale)
            self._rows_for = (self.vel2, self.vel2._version)
        if self.sa_moving:           # update_normals of the Euler step: BUFFER_BOUNDELEMENTS of n* / n+1 from that of n
            K.sa_update_normals(self.boundelements2, self.boundelements, self.info, n, n)
        if self.energy_on:
            K.euler_internal_energy(self.energy2, self.energy, self.dedt, self.pos, self.info, n, self.d_dt, dt_scale)
        if self.keps:
            K.euler_keps(self.ke2, self.ke, self.dkde, self.forces, self.pos, self.info, n, self.d_dt, dt_scale)
        if self.io:                  # (in the corrector the particle count grows by the released particles: n is stale behind it)
            self._sa_post_euler_io(step)
        elif self.sa:
            self._sa_post_euler(step)
        if self.granular:            # POSTPRED_EFFPRES on n* (its result is the field of the state n as well), POSTCORR_EFFPRES on n+1
            self._solve_effpres("predictor" if step == 1 else "corrector", self.pos2, self.vel2)

    def _finish_step(self, written):
        """TIME_STEP_EPILOGUE (GPUSPH.cc:650-657): the new state becomes the current one (`written`: the buffers that have a new copy),
        t += dt, dt = min(dt_pred, dt_corr) over all devices"""
        self._swap(*written)
        self.k.time_advance(self.d_t, self.d_dt)
        if self.world > 1:
            self.transport.allreduce_min(self.d_dt_next)
        self.d_dt, self.d_dt_next = self.d_dt_next, self.d_dt
        self.iterations += 1

    def step(self):
        if self.iterations % self.sp.buildneibsfreq == 0:
            self.build_neibs()
            if self.sa and self.iterations == 0:     # initialisation step of the boundary conditions (not after a resume)
                self.sa_boundary_conditions(0)
            if self.granular and self.iterations == 0:      # INIT_EFFPRES, after the first list build
                self._solve_effpres("init", self.pos, self.vel)
        if self.iterations > 0:
            for ftype, freq in self.filters:
                if self.iterations % freq == 0:
                    self.apply_filter(ftype)
        # (the callback of bodies with prescribed motion needs dt on the host: one synchronisation per step; floating bodies need none)
        dt_host = float(self.d_dt.item()) if self.bodies is not None else None
        self._substep(1, dt_host)
        self._substep(2, dt_host)
        if self.bodies is not None:                 # EULER_UPLOAD_OBJECTS_CG in the post-corrector phase (:331-332)
            self.k.set_body_cg_integration(self._last_motion)
            self.t_host += dt_host                  # the same double += float as on the device
        self._finish_step(self._stepped)            # every buffer the step wrote a new copy of (BUFFERS)

    def run(self, steps):
        for _ in range(steps):
            self.step()

    def time(self):
        return float(self.d_t.item())

    # ------------------------------------------------------------------ views
    @property
    def n(self):
        return self.n_int

    def internal_particles(self):
        return self.n_int

    def neibs_info(self):
        return self.k.neibs_info()

    def add_filter(self, filtertype, frequency):
        self.filters.append((int(filtertype), int(frequency)))

    def current_dt(self):
        return float(self.d_dt.item())

    def floating_state(self, slots=False):
        """The floating bodies as the device holds them: float64 [bodies, 19] -- centre of rotation (3), orientation (4: w, x, y, z),
        linear velocity (3), angular velocity (3, world frame), total force (3) and torque (3) of the last substep -- and, with
        slots=True, a dict of the bodies' rows of the rigid-body table as well.  Every rank of a run on several slabs holds the
        same.  Synchronises."""
        if not self.floating:
            raise ValueError("the problem has no floating bodies")
        return self.k.floating_state(slots)

    def reduce_rb_forces(self):
        """REDUCE_BODIES_FORCES + REDUCE_BODIES_FORCES_HOST (src/GPUSPH.cc): total force and torque on the feedback body,
        per device over the rows of its own particles, then summed over the devices (one all_reduce of 6 floats).
        The order of the float sum is implementation-defined in the reference too (thrust scan): tolerance-only."""
        if not self.has_rb:
            return None
        tot = torch.cat([self.rbforces[:, :3].double().sum(0), self.rbtorques[:, :3].double().sum(0)])
        if self.world > 1:
            self.transport.allreduce_sum(tot)
        tot = tot.cpu().numpy()
        return tot[:3].astype(np.float32), tot[3:].astype(np.float32)

    # ------------------------------------------------------------------ wave gages
    def _state_key(self):
        return (self.iterations, self.pos.data_ptr(), self.info.data_ptr(), self.n_int)

    def detect_surface(self, normals=None):
        """SURFACE_DETECTION of the rows this rank owns (their lists reach into the halo): FG_SURFACE in INFO, in place"""
        pp = self.problem.physparams
        self.k.postprocess(D.SURFACE_DETECTION, None, None, self.info, normals, self.pos, self.vel, *self._lists, self.n_int,
                           getattr(pp, "cosconeanglefluid", 0.86), getattr(pp, "cosconeanglenonfluid", 0.5))
        self._surface_for = self._state_key()

    def wave_gages(self, gages=None):
        """The water level at the problem's gages (Problem.add_gage), or at `gages` ((n, 4): x, y, unused, smoothing length): float64
        [n], computed on the device from the free-surface particles (GPUSPH::doWrite, src/GPUSPH.cc:1579-1697, without its host
        copy of the state).  The surface detection runs first if it has not run on this state (the reference force-enables it for
        a problem with gages, src/ProblemCore.cc:102).  Every rank counts the rows it owns, never its halo, and the ranks combine
        their partial sums (smoothing length > 0) or take the nearest particle of all (0; the lower rank among equals).
        NaN where a smoothed gage has no surface particle in reach, 0 where a nearest-mode gage has none at all.  Needs the neighbour
        list of the state (build_neibs, or a step).  Synchronises."""
        g = np.ascontiguousarray(self.problem.gages if gages is None else gages, dtype=np.float64).reshape(-1, 4)
        ng = len(g)
        if self._surface_for != self._state_key():
            self.detect_surface()
        dev = self.device
        d_g = torch.from_numpy(g).to(dev)
        part = torch.zeros((max(ng, 1), 4), dtype=torch.float64, device=dev)
        self.k.wave_gages(part, d_g, ng, self.pos, self.info, self.hash, self.n_int)
        if not ng:
            return np.zeros(0, dtype=np.float64)
        if self.world > 1:
            nearest = np.nonzero(~(g[:, 3] > 0))[0]
            mine = part.cpu().numpy()
            sums = part[:, :2].contiguous()
            self.transport.allreduce_sum(sums)
            part[:, :2] = sums
            for k in nearest:       # the smallest r of all ranks: (bits of r >= 0, bits of z), +inf where a rank has none
                r = mine[k, 1] if mine[k, 2] else np.inf
                got = self.transport.allgather_pair(int(np.float64(r).view(np.uint64)), int(np.float64(mine[k, 0]).view(np.uint64)), dev)
                rb, zb = min(got, key=lambda v: v[0])          # (min returns the first of equals: the lowest rank)
                rr = float(np.uint64(rb).view(np.float64))
                part[k] = torch.tensor([float(np.uint64(zb).view(np.float64)) if np.isfinite(rr) else 0.0, rr,
                                        1.0 if np.isfinite(rr) else 0.0, 0.0], dtype=torch.float64, device=dev)
        z = torch.empty(ng, dtype=torch.float64, device=dev)
        self.k.wave_gages_finish(z, part, d_g, ng)
        return z.cpu().numpy()

    def write_wave_gages(self, path, gages=None):
        """one line of WaveGage.txt (CommonWriter::write_WaveGage, src/writers/CommonWriter.cc:244-252) for the current state;
        the header (:72-80) goes first into a new file.  Every rank takes part in the reading, rank 0 writes.  Returns the levels."""
        from . import commonwriter
        z = self.wave_gages(gages)
        if self.rank != 0:
            return z
        new = not os.path.exists(path) or os.path.getsize(path) == 0
        with open(path, "a") as f:
            if new:
                f.write(commonwriter.wave_gage_header(len(z)))
            f.write(commonwriter.wave_gage_line(self.time(), z))
        return z

    # ------------------------------------------------------------------ save-time diagnostics
    def save_diagnostics(self):
        """What GPUSPH::doWrite takes from its host copy of the state besides the gages (src/GPUSPH.cc:1597-1647,1672-1684),
        computed on the device (diagnostics.hip): dict(energy = float64 [MAX_FLUID_TYPES + 1, 3], kinetic, potential and internal
        energy per fluid with the non-fluid class last; rows = the number of active rows per class; max_speed = the largest
        length(vel), float32; nan_row = (rank, row) of the first active particle without a finite position, or None).  Every rank
        counts the rows it owns, never its halo; the ranks add their sums in double in rank order, take the largest speed and
        the nan_row of the lowest rank.  Inactive rows count for nothing, and kinetic and potential energy are formed without
        ENABLE_INTERNAL_ENERGY too (internal = 0).  Keeps peak_particle_speed and its time up to date (a strict >, :1681-1684) and
        warns, naming the row, when nan_row is set.  Synchronises."""
        K, dev = self.k, self.device
        out = torch.empty(K.DIAG_DOUBLES, dtype=torch.float64, device=dev)
        K.save_diagnostics(out, self.pos, self.vel, self.info, self.hash, self.energy if self.energy_on else None, self.n_int)
        mine = out.cpu().numpy()
        sums, pairs = mine[:K.DIAG_MAXSQ], [(mine[K.DIAG_MAXSQ], mine[K.DIAG_NANROW])]
        if self.world > 1:
            d_sums = out[:K.DIAG_MAXSQ].contiguous()
            self.transport.allreduce_sum(d_sums)
            sums = d_sums.cpu().numpy()
            got = self.transport.allgather_pair(int(mine[K.DIAG_MAXSQ:K.DIAG_MAXSQ + 1].view(np.uint64)[0]),
                                                int(mine[K.DIAG_NANROW:K.DIAG_NANROW + 1].view(np.uint64)[0]), dev)
            pairs = [tuple(np.array(v, dtype=np.uint64).view(np.float64)) for v in got]
        sums = sums.reshape(D.MAX_FLUID_TYPES + 1, 4)
        max_speed = np.sqrt(np.float32(max(v[0] for v in pairs)))         # ONE correctly rounded float sqrt of the largest |v|^2
        nan_row = next(((r, int(v[1])) for r, v in enumerate(pairs) if v[1] < K.DIAG_NO_ROW), None)
        if max_speed > self.peak_particle_speed:
            self.peak_particle_speed = max_speed
            self.peak_particle_speed_time = self.time()
        if nan_row is not None:
            import warnings
            warnings.warn("particle %d of rank %d has a NaN position at iteration %d, time %g"
                          % (nan_row[1], nan_row[0], self.iterations, self.time()), RuntimeWarning, stacklevel=2)
        return {"energy": sums[:, :3].copy(), "rows": sums[:, 3].astype(np.int64), "max_speed": max_speed, "nan_row": nan_row}

    def peak_speed_line(self):
        """the line GPUSPH prints at the end of a run (src/GPUSPH.cc:775-776) from the peak over the save_diagnostics calls so far"""
        v = float(self.peak_particle_speed)
        return ("Peak particle speed was ~%g m/s at %g s -> can set maximum vel %.2g for this problem\n"
                % (v, self.peak_particle_speed_time, v*1.1))

    def write_energy(self, path):
        """one line of energy.txt (CommonWriter::write_energy, src/writers/CommonWriter.cc:226-241) for the current state; the header
        (:53-70) goes first into a new file.  Every rank takes part in the reading, rank 0 writes.  Returns save_diagnostics()."""
        from . import commonwriter
        d = self.save_diagnostics()
        if self.rank != 0:
            return d
        nf = self.problem.physparams.numFluids()
        new = not os.path.exists(path) or os.path.getsize(path) == 0
        with open(path, "a") as f:
            if new:
                f.write(commonwriter.energy_header(nf))
            f.write(commonwriter.energy_line(self.time(), d["energy"], nf))
        return d

    def download_internal(self):
        n = self.n_int
        out = {k: t[:n].cpu().numpy() for b in self._bufs if b.download for k, t in _items(b.name, getattr(self, b.name))}
        out.update(info=self.info[:n].cpu().numpy().view(np.uint16), hash=self.hash[:n].cpu().numpy().view(np.uint32),
                   forces=self.forces[:n].cpu().numpy())
        return out
