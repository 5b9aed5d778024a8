"""Velocity-Verlet / Langevin integrator on HIP kernels.

Mirror of the reference module (`torchmd/integrator.py`): same constants, helper functions,
`Integrator(systems, forces, timestep, device, gamma=None, T=None, batch=None)` constructor and
`step(niter) -> (Ekin, pot, T)` contract, plus an opt-in `constraints` keyword ("water": rigid waters by SETTLE;
"hbonds": also every X-H bond by SHAKE/RATTLE) and an opt-in `barostat` keyword (a
`barostat.MonteCarloBarostat`, or a `crescale.CRescaleBarostat` driven by the virial: constant pressure, DESIGN §11 and
§20) and an opt-in `thermostat` keyword (a
`thermostat.VelocityRescale`: stochastic velocity rescaling between batches of steps, one target temperature per replica,
DESIGN §14) and an opt-in `exchange` keyword (an `exchange.ReplicaExchange`: temperature replica exchange on the thermostat's
ladder, DESIGN §16, or an `hrex.HamiltonianExchange`: replicas trade alchemical couplings and restraint windows)
that this package adds.  Each iteration is

    tmdhip_first_vv  ->  forces.compute  ->  tmdhip_langevin_second_vv | tmdhip_second_vv

(integrator.py:115-120).  With this package's `Forces` the loop enqueues everything asynchronously
and only reads energies back after the last iteration (the reference returns the energies of the last
`compute()` only, integrator.py:125); any other object with a `.compute(pos, box, forces)` method
(the duck type shown by tests/test_integrator.py:155-158) is called as in the reference.
"""

from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib as L
from .controls import draw_seed
from .forces import active_side_terms

TIMEFACTOR = 48.88821
BOLTZMAN = 0.001987191
PICOSEC2TIMEU = 1000.0 / TIMEFACTOR


def kinetic_energy(masses, vel, batch=None):
    """Kinetic energy per replica (nreplicas, 1), or per replica and atom group (nreplicas, nbatches)
    when `batch` (natoms,) assigns atoms to groups — reference integrator.py:8-43.  Analysis helper
    on torch tensors (any device); `Integrator.step` uses the fused HIP reduction instead."""
    if vel.dim() != 3:
        raise ValueError(f"vel must be 3D (nreplicas, natoms, 3), got {vel.dim()}D")
    per_atom = 0.5 * masses * torch.sum(vel * vel, dim=2, keepdim=True)
    if batch is None:
        return torch.sum(per_atom, dim=1)
    nbatch = int(torch.max(batch).item() + 1)
    out = torch.zeros(vel.shape[0], nbatch, device=vel.device, dtype=vel.dtype)
    out.index_add_(1, batch, per_atom[:, :, 0])
    return out


def maxwell_boltzmann(masses, T, replicas=1):
    """Velocities ~ N(0, sqrt(kB T / m)) per replica (reference integrator.py:46-54)."""
    natoms = len(masses)
    scale = torch.sqrt(T * BOLTZMAN / masses)
    return torch.stack([scale * torch.randn((natoms, 3)).type_as(masses) for _ in range(replicas)], dim=0)


def kinetic_to_temp(Ekin, natoms):
    return 2.0 / (3.0 * natoms * BOLTZMAN) * Ekin


def _stream(device):
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def _first_VV(pos, vel, force, mass, dt):
    """pos += vel*dt + 0.5*(F/m)*dt^2 ; vel += 0.5*dt*(F/m)   (integrator.py:61-64), one kernel."""
    lib = L.load()
    for name, t in (("pos", pos), ("vel", vel), ("force", force), ("mass", mass)):
        L.require_device_tensor(t, name)
    R, N = pos.shape[0], pos.shape[1]
    with torch.cuda.device(pos.device):
        L.check(
            lib.tmdhip_first_vv(
                L.dtype_code(pos.dtype), R, N, pos.data_ptr(), vel.data_ptr(), force.data_ptr(), mass.data_ptr(),
                float(dt), _stream(pos.device),
            ),
            "tmdhip_first_vv",
        )


def _second_VV(vel, force, mass, dt):
    """vel += 0.5*dt*(F/m)   (integrator.py:67-69)."""
    lib = L.load()
    for name, t in (("vel", vel), ("force", force), ("mass", mass)):
        L.require_device_tensor(t, name)
    R, N = vel.shape[0], vel.shape[1]
    with torch.cuda.device(vel.device):
        L.check(
            lib.tmdhip_second_vv(
                L.dtype_code(vel.dtype), R, N, vel.data_ptr(), force.data_ptr(), mass.data_ptr(), float(dt),
                _stream(vel.device),
            ),
            "tmdhip_second_vv",
        )


_REPLAY_FAILED = ("Integrator.step(): the batch of steps was rewound and repeated once and failed again; the trajectory "
                  "since the previous step() call is invalid (restart from the last saved state).  The library says: ")
# (the step-by-step loop over a duck-typed / external force has no saved entry state: nothing was rewound)
_LIST_INVALID = ("Integrator.step(): a neighbour list overflowed or outlived its skin during this call; the trajectory since "
                 "the previous step() call is invalid (restart from the last saved state; the list capacity has been grown)")


def cut_segments(nstep, niter, frequency):
    """How `step(niter)` is cut when something has to happen every `frequency` steps counted over the integrator's life:
    [(n, attempt), ...] with sum(n) == niter; a segment ends where `nstep` + the steps so far reaches a multiple of
    `frequency` (attempt = True) or where the call ends."""
    out, done = [], 0
    while done < niter:
        n = min(frequency - (nstep + done) % frequency, niter - done)
        done += n
        out.append((n, (nstep + done) % frequency == 0))
    return out


def cut_schedules(nstep, niter, frequencies):
    """`cut_segments` for several things with a frequency each: [(n, (hit, ...)), ...] with sum(n) == niter, cut at the union
    of the schedules; hit[k] says that the segment ends on a multiple of frequencies[k]."""
    ends = {}
    for k, f in enumerate(frequencies):
        done = 0
        for n, hit in cut_segments(nstep, niter, f):
            done += n
            ends.setdefault(done, [False] * len(frequencies))[k] = hit
    out, prev = [], 0
    for end in sorted(ends):
        out.append((end - prev, tuple(ends[end])))
        prev = end
    return out


class Integrator:
    def __init__(self, systems, forces, timestep, device, gamma=None, T=None, batch=None, constraints=None, barostat=None,
                 thermostat=None, exchange=None):
        self.dt = timestep / TIMEFACTOR
        self.systems = systems
        self.forces = forces
        self.device = device
        if gamma is not None:
            gamma = gamma / PICOSEC2TIMEU
        self.gamma = gamma
        self.T = T
        if torch.any(systems.masses != 0):
            self.masses = systems.masses
        else:
            self.masses = torch.as_tensor(self.forces.par.masses).detach().clone()
            self.masses = self.masses.to(device=device, dtype=systems.pos.dtype).view(-1, 1)
        self.masses = self.masses.contiguous()
        if T:
            if gamma is None:
                raise RuntimeError("Langevin temperature T requires a friction gamma")
            self.vcoeff = torch.sqrt(2.0 * gamma / self.masses * BOLTZMAN * T * self.dt).to(device).contiguous()
            self.vcoeff[self.masses == 0] = 0.0  # (massless virtual sites: no noise, and no division by their mass)
        self.batch = batch
        if batch is not None:
            self.natoms = torch.bincount(batch).cpu().numpy()
        else:
            self.natoms = len(self.masses)
        self._seed = draw_seed()  # (the noise stream)
        self._nstep = 0
        self._ke = None
        self.constraints = None  # constraints.ConstraintSet
        self.virtual_sites = getattr(forces, "virtual_sites", None)
        if self.virtual_sites is not None and not self.virtual_sites.nsites:
            self.virtual_sites = None
        if self.virtual_sites is not None and constraints is None:
            raise ValueError("a Forces with virtual_sites is integrated with constraints='water' or 'hbonds' only: a site is "
                             "stepped as part of its rigid water (sites on flexible molecules: Forces.compute only)")
        if constraints is not None:
            self._init_constraints(constraints)
        # the scheduled controls (controls.Control): thermostat.VelocityRescale; barostat.MonteCarloBarostat or
        # crescale.CRescaleBarostat; exchange.ReplicaExchange or hrex.HamiltonianExchange.  `forces.metadynamics` is the fourth.
        self.thermostat, self.barostat, self.exchange = thermostat, barostat, None
        self._virial_barostat = bool(getattr(barostat, "virial_driven", False))  # (a plain attribute: nothing dispatches on it)
        self.kinetic_source = None  # the control whose `kinetic()` holds the kinetic energies left (`Control.after_segment`)
        self._check_side_terms()  # (before the exchange is known, so that the controls' own refusals come first)
        self.replays = 0  # batches that were rewound and repeated (list validity failure / step-block time-out)
        self.exchange = exchange
        for c in (thermostat, barostat, exchange):  # (rank order)
            if c is not None:
                c.attach(self)
        self._check_side_terms()

    def _check_side_terms(self):
        """What is refused with a side term of the forces (ValueError, the term's own message: `SideTerm.refusals`): atom groups,
        whose replicas share one row of positions; a barostat (distance restraints alone are allowed: they scale with the box);
        for metadynamics, replica exchange and a bias made for another number of replicas.  Looked at when the integrator is
        made and again at every `step`: entries may be added to a `Restraints` at any time."""
        for t in active_side_terms(self.forces):
            for what, on in (("batch", self.batch), ("barostat", self.barostat), ("exchange", getattr(self, "exchange", None))):
                if on is not None and t.refusal(what):
                    raise ValueError(t.refusal(what))
        md = getattr(self.forces, "metadynamics", None)
        if md is not None and md.nreplicas != self.systems.pos.shape[0]:
            raise ValueError(f"the metadynamics bias was made for {md.nreplicas} replicas, the systems have {self.systems.pos.shape[0]}")

    def _init_constraints(self, mode):
        from .constraints import find_constraints
        from .forces import Forces

        if not isinstance(self.forces, Forces) or self.forces.external:
            raise ValueError("constraints need this package's Forces without an `external` term (the tmdhip_md_run path); "
                             "duck-typed force objects and external forces are not supported")
        par = self.forces.par
        self.constraints = find_constraints(self.masses.detach().cpu().double().reshape(-1).numpy(), par.bond_params,
                                            getattr(par, "angle_params", None), mode, virtual_sites=self.virtual_sites)
        self._ndof = self.constraints.ndof(self.batch)
        self._projected = False

    def _temperature(self, Ekin):
        if self.constraints is None:
            return kinetic_to_temp(Ekin, self.natoms)
        return 2.0 / (np.asarray(self._ndof, dtype=np.float64) * BOLTZMAN) * Ekin

    def _run_precision(self, Ekin):
        """A host array of kinetic energies in the precision of the run, as `step` returns it."""
        return Ekin.astype(np.dtype("float32") if self.systems.pos.dtype == torch.float32 else np.float64)

    def _project_start(self):
        """OpenMM's applyConstraints at the first step: SHAKE the positions onto the constraints (the current positions as
        reference), remove the velocity components along them, and evaluate the forces of the projected positions."""
        s, cs = self.systems, self.constraints
        pos = s.pos.detach().cpu().double().numpy()
        vel = s.vel.detach().cpu().double().numpy()
        for r in range(pos.shape[0]):
            ref = pos[r].copy()
            cs.shake_positions(pos[r], ref)
            cs.project_velocities(pos[r], vel[r])
            if self.virtual_sites is not None:  # sites on the projected parents, at rest (maxwell_boltzmann gave them inf)
                self.virtual_sites.construct(pos[r])
                vel[r][self.virtual_sites.sites] = 0.0
        s.pos.copy_(torch.as_tensor(pos).to(s.pos.dtype))
        s.vel.copy_(torch.as_tensor(vel).to(s.vel.dtype))
        self.forces.compute(s.pos, s.box, s.forces)
        self._projected = True

    def _check_layout(self):
        s = self.systems
        for name in ("pos", "vel", "forces"):
            t = getattr(s, name)
            L.require_device_tensor(t, f"systems.{name}")
            if not t.is_contiguous():
                raise RuntimeError(f"systems.{name} must be contiguous (it is updated in place by the HIP kernels)")
            if t.dtype != s.pos.dtype:
                raise RuntimeError("systems.pos/vel/forces must share one dtype")
        if self.masses.device != s.pos.device or self.masses.dtype != s.pos.dtype:
            self.masses = self.masses.to(device=s.pos.device, dtype=s.pos.dtype).contiguous()
            if self.T:
                self.vcoeff = self.vcoeff.to(device=s.pos.device, dtype=s.pos.dtype).contiguous()

    def step(self, niter=1):
        L.load()
        self._check_layout()
        self._check_side_terms()
        with torch.cuda.device(self.systems.pos.device):
            if self.constraints is not None and not self._projected:
                self._project_start()
            found = (self.thermostat, self.barostat, self.exchange, getattr(self.forces, "metadynamics", None))
            return self.run_schedule(niter, [c for c in found if c is not None], self._step_body)

    def run_schedule(self, niter, controls, run):
        """`step(niter)` under scheduled controls (`controls.Control`): the call is cut into segments that end on
        the multiples of the controls' frequencies, counted over the integrator's life; `run(n)` runs a segment as `step` runs
        a call (rewind and replay included) and returns its (Ekin, pot, T); the controls whose multiple the segment ends on
        then act in rank order.  The kinetic energy returned is that of the velocities as they are left: of whatever rescaled
        them last after the last segment (`kinetic_source.kinetic()`, the only record read back).  `run` is `_step_body`; a host test
        hands in a fake."""
        controls = sorted(controls, key=lambda c: c.rank)
        if not controls or niter <= 0:
            return run(niter)
        for n, hit in cut_schedules(self._nstep, niter, [c.frequency for c in controls]):
            out, self.kinetic_source = run(n), None
            for c, on in zip(controls, hit):
                if on:
                    out = c.after_segment(self, out)
        if self.kinetic_source is not None:
            Ekin = self._run_precision(self.kinetic_source.kinetic().cpu().numpy())
            out, self.kinetic_source = (Ekin, out[1], self._temperature(Ekin)), None
        return out

    def _pressure_terms(self):
        from .forces import Forces

        if not isinstance(self.forces, Forces):
            raise ValueError("the pressure needs this package's Forces (duck-typed force objects are not supported)")
        if self.batch is not None:
            raise ValueError("the pressure does not support atom groups (batch=): its molecules are per replica")
        self._check_layout()
        s = self.systems
        return self.forces._pressure_terms(s.pos, s.box, vel=s.vel, masses=self.masses)

    def pressure_tensor(self):
        """The diagonal (P_xx, P_yy, P_zz) of the instantaneous pressure of every replica, [R, 3] float64 in bar, from the
        molecular virial: P_aa V = sum_I M_I V_I,a^2 + W_aa with `Forces.virial`'s W and the velocities of the
        molecules' centres of mass as they are now (after `step()`: both half kicks made).  The pressure of the force
        field: no `external`, restraint or metadynamics contribution, no dispersion correction.  Separate launches between
        two `step()` calls; a run `step(); pressure(); step()` equals the run that calls `forces.compute()` there."""
        from .barostat import BAR_TO_KCAL_MOL_A3

        t = self._pressure_terms()
        return (t[:, 0:3] + t[:, 3:6]) / t[:, 6:7] / BAR_TO_KCAL_MOL_A3

    def pressure(self):
        """The instantaneous pressure (P_xx + P_yy + P_zz) / 3 of every replica, [R] float64 in bar (`pressure_tensor`)."""
        from .barostat import BAR_TO_KCAL_MOL_A3

        return self._pressure_terms()[:, 7] / BAR_TO_KCAL_MOL_A3

    def _step_body(self, niter, replay=False):
        from .forces import Forces

        lib, s = L.load(), self.systems
        dev, code = s.pos.device, L.dtype_code(s.pos.dtype)
        R, N = s.pos.shape[0], s.pos.shape[1]
        fast = isinstance(self.forces, Forces)
        fused = fast and not self.forces.external and niter > 0
        pot = None
        ebuf = ext = None
        if fused:
            # whole loop enqueued from C (tmdhip_md_run): fused half-kick/drift/displacement-test
            # kernels, no Python or ctypes work per step
            step0 = self._nstep - niter if replay else self._nstep
            ebuf = self.forces._md_run(
                s, self.masses, self.vcoeff if self.T else None, self.dt,
                float(self.gamma) if self.T else 0.0, self._seed, step0, niter, restore=replay,
                constraints=self.constraints,
            )
            if not replay:
                self._nstep += niter
        for it in range(0 if not fused else niter, niter):
            st = _stream(dev)
            L.check(
                lib.tmdhip_first_vv(code, R, N, s.pos.data_ptr(), s.vel.data_ptr(), s.forces.data_ptr(),
                                    self.masses.data_ptr(), self.dt, st),
                "tmdhip_first_vv",
            )
            if fast:
                ebuf, ext = self.forces._compute_async(s.pos, s.box, s.forces, want_energy=(it == niter - 1))
            else:
                pot = self.forces.compute(s.pos, s.box, s.forces)
            if self.T:
                L.check(
                    lib.tmdhip_langevin_second_vv(code, R, N, s.vel.data_ptr(), s.forces.data_ptr(),
                                                  self.masses.data_ptr(), self.vcoeff.data_ptr(), self.dt,
                                                  float(self.gamma), self._seed, self._nstep, st),
                    "tmdhip_langevin_second_vv",
                )
            else:
                L.check(
                    lib.tmdhip_second_vv(code, R, N, s.vel.data_ptr(), s.forces.data_ptr(),
                                         self.masses.data_ptr(), self.dt, st),
                    "tmdhip_second_vv",
                )
            self._nstep += 1

        eng = self.forces._engine(s.pos) if (fast and niter > 0) else None
        if fused and self.batch is None:
            # kinetic energy + energies of the last step + neighbour-list validity: ONE C call, ONE read-back,
            # ONE host synchronisation (tmdhip_md_observe)
            obs = np.empty((R, L.NENERGY + 1), dtype=np.float64)
            rc = L.check(
                # (AFTER_RUN: nothing has touched the velocities since the tmdhip_md_run a few lines up returned)
                lib.tmdhip_md_observe(eng.ctx, s.vel.data_ptr(), self.masses.data_ptr(), ebuf.data_ptr(),
                                      obs.ctypes.data_as(C.POINTER(C.c_double)), L.OBSERVE_AFTER_RUN, _stream(dev)),
                "tmdhip_md_observe",
            )
            if rc != 0:
                # a neighbour list was truncated or outlived its skin between two scheduled rebuilds, or a step block
                # of a fused pair + step launch timed out: rewind to the entry state (saved by tmdhip_md_run) and
                # repeat the batch with the rebuild chain on every step (and, after a time-out, the separate
                # integrator kernel); the noise stream is counter based, so it is the same trajectory
                if not replay:
                    self.replays += 1
                    return self._step_body(niter, replay=True)
                raise RuntimeError(_REPLAY_FAILED + L.last_error())
            cols = self.forces.energy_columns()
            tot = obs[:, cols].sum(axis=1) if cols else np.zeros(R)
            for t in active_side_terms(self.forces):  # the run's finishing launch has summed them: one small copy each
                row = np.empty((R, t.side_width), dtype=np.float64)
                L.check(getattr(lib, t.side_energy)(eng.ctx, row.ctypes.data_as(C.POINTER(C.c_double)), _stream(dev)), t.side_energy)
                t.store(row)
                tot = tot + t.potential(row)
            pot = [float(v) for v in tot]
            Ekin = self._run_precision(obs[:, L.NENERGY].copy())
            return Ekin, pot, self._temperature(Ekin)
        if self.batch is None:
            if eng is not None:
                kebuf = eng.kebuf  # shares one buffer with the energies: a single read-back below
            else:
                if self._ke is None or self._ke.shape[0] != R or self._ke.device != dev:
                    self._ke = torch.zeros(R, dtype=torch.float64, device=dev)
                kebuf = self._ke
            L.check(
                lib.tmdhip_kinetic_energy(code, R, N, s.vel.data_ptr(), self.masses.data_ptr(),
                                          kebuf.data_ptr(), _stream(dev)),
                "tmdhip_kinetic_energy",
            )
            ke = kebuf
        else:
            ke = kinetic_energy(self.masses, s.vel, self.batch).flatten().to(torch.float64)
        if eng is not None:
            if self.batch is None and ebuf is eng.ebuf:
                host = eng.comb.cpu().numpy()  # the only synchronising call of step()
                e = host[: R * L.NENERGY].reshape(R, L.NENERGY)
                Ekin = host[R * L.NENERGY:].copy()
                cols = self.forces.energy_columns()
                tot = e[:, cols].sum(axis=1) if cols else np.zeros(R)
                if ext is not None:
                    tot = tot + ext.cpu().numpy()
                pot = [float(v) for v in tot]
            else:
                tot = self.forces.total_energy_from(ebuf, ext)
                host = torch.cat([ke.flatten(), tot]).cpu().numpy()
                Ekin, pot = host[: ke.numel()], [float(v) for v in host[ke.numel():]]
            if not self.forces._verify(eng, s.pos):
                why = L.last_error()  # (tmdhip_check's verdict, set by judge_flags a moment ago)
                if fused and not replay:  # (batch mode of the fused loop: same rewind as above)
                    self.replays += 1
                    return self._step_body(niter, replay=True)
                raise RuntimeError((_REPLAY_FAILED + why) if (fused and replay) else (_LIST_INVALID + ": " + why))
            if ebuf is not None:
                # (the step-by-step loop: the side terms' energies of its last evaluation, as the fused path leaves them)
                for t in active_side_terms(self.forces):
                    t.store(eng.side_row(t).cpu().numpy())
        else:
            Ekin = ke.flatten().cpu().numpy()
        Ekin = self._run_precision(Ekin)
        return Ekin, pot, self._temperature(Ekin)
