"""Constant pressure from the virial: the stochastic cell-rescaling barostat for orthorhombic periodic boxes.

`CRescaleBarostat(pressure_bar, temperature, tau=1.0, compressibility=4.5e-5, frequency=10, stochastic=True, seed=None)`,
handed to `Integrator(..., barostat=...)`, rescales the box every `frequency` steps (Bernetti & Bussi, J. Chem. Phys. 153,
114107, 2020; GROMACS' `pcoupl = C-rescale`).  One application, for every replica r independently, with eps = ln V,
dt_p = frequency dt, kT_r = k_B T_r, beta_r the isothermal compressibility and tau_p the relaxation time:

    d eps = -(beta_r dt_p / tau_p) (P0_r - P_int) + sqrt(2 kT_r beta_r dt_p / (V tau_p)) xi        mu = exp(d eps / 3)

1. P_int and V come from `Forces._pressure_terms`: the molecular pressure, with the kinetic term of the
   molecules' centres of mass, of the state `step()` left (both half kicks made);
2. xi is one standard normal of the replica's generator; it is drawn also when `stochastic=False`, which drops the noise
   term (the Berendsen limit: the box relaxes deterministically, the ensemble is not NPT; for equilibration);
3. the three box edges are multiplied by mu and rounded to the box tensor's precision; the per-axis factors applied to the
   molecules are new_edge / old_edge (as `MonteCarloBarostat.attempt` forms them), so box and positions stay consistent in
   fp32;
4. every molecule (§19's: connected components of the bond graph, virtual sites with their parents) moves rigidly
   (`tmdhip_rescale_molecules`, crescale.hip): each atom by (s_a - 1) R_I,a, each velocity by (1 / s_a - 1) V_I,a, with R_I /
   V_I the mass-weighted centre and its velocity.  Distances and relative velocities inside a molecule do not change:
   constrained states survive to storage rounding;
5. `forces.compute` at the new state refreshes `systems.forces` and gives U'.

Every move is made — none is rejected — and the barostat takes one target pressure, temperature and compressibility per
replica.  `work()` accumulates the change of E_kin + E_pot + P0 V over all applications, so that E_kin + E_pot + P0 V - heat -
work is the conserved quantity of a run (heat: the thermostat's).

Units: `pressure_bar` in bar, `compressibility` in 1/bar (4.5e-5: water), `tau` in ps, `temperature` in K.  Random numbers:
every replica owns a `numpy.random.Generator(Philox(key=(seed, replica)))` and draws exactly one number per application, so a
replica's chain does not depend on how many replicas run beside it.  Molecules must be whole (what `Wrapper.wrap` leaves).
"""

from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib as L
from .barostat import BAR_TO_KCAL_MOL_A3
from .controls import Control, box_edges, forget_continuation, positive_edges, require_layout, scaled_box
from .integrator import BOLTZMAN, PICOSEC2TIMEU

_KEYS = ("V", "V_new", "P_int", "xi", "mu", "U", "U_new", "K_before", "K_after")


def delta_epsilon(p0, p_int, volume, kT, beta, dt_over_tau, xi, stochastic=True):
    """d eps of one application (module docstring); pressures in kcal/mol/A^3, beta in A^3 mol/kcal, float64 arrays.  The
    order of the operations is that of csrc/crescale_math.h."""
    drift = -(beta * dt_over_tau) * (p0 - p_int)
    if not stochastic:
        return drift
    return drift + np.sqrt(((2.0 * kT) * (beta * dt_over_tau)) / volume) * xi


def rescale_molecules(pos, vel, masses, scale, offsets, members, has_big, record, partials):
    """`tmdhip_rescale_molecules`: move every molecule of `pos` / `vel` [R,N,3] (device, in place) with a box whose edges are
    multiplied by `scale` (host array [R,3]); `masses`: device tensor [N] of the dtype of `pos`; `offsets` / `members`: the
    molecules' CSR as int32 device tensors; `record` (device float64 [R,2]) receives (K_before, K_after); `partials`: scratch
    sized by `tmdhip_rescale_molecules_workspace`."""
    L.require_device_tensor(vel, "vel")
    R, N = require_layout(pos, "pos", masses)
    if vel.shape != pos.shape or vel.dtype != pos.dtype or vel.device != pos.device or not vel.is_contiguous():
        raise RuntimeError("vel must be a contiguous tensor with the shape, dtype and device of pos")
    for name, t in (("offsets", offsets), ("members", members)):
        if t.dtype != torch.int32 or t.device != pos.device or not t.is_contiguous():
            raise RuntimeError(f"{name} must be a contiguous int32 tensor on the device of pos")
    if members.numel() != N:
        raise RuntimeError("the molecules must cover every atom exactly once")
    nmol = offsets.numel() - 1
    nrec, npart = C.c_int64(), C.c_int64()
    L.check(L.load().tmdhip_rescale_molecules_workspace(R, nmol, C.byref(nrec), C.byref(npart)), "tmdhip_rescale_molecules_workspace")
    for name, t, need in (("record", record, nrec.value), ("partials", partials, npart.value)):
        if t.dtype != torch.float64 or t.device != pos.device or not t.is_contiguous() or t.numel() < need:
            raise RuntimeError(f"{name} must be a contiguous float64 tensor of at least {need} entries on the device of pos")
    sc = np.ascontiguousarray(np.asarray(scale, dtype=np.float64).reshape(R, 3))
    with torch.cuda.device(pos.device):
        L.check(
            L.load().tmdhip_rescale_molecules(
                L.dtype_code(pos.dtype), R, N, pos.data_ptr(), vel.data_ptr(), masses.data_ptr(),
                sc.ctypes.data_as(C.POINTER(C.c_double)), nmol, offsets.data_ptr(), members.data_ptr(), 1 if has_big else 0,
                record.data_ptr(), partials.data_ptr(), C.c_void_p(torch.cuda.current_stream(pos.device).cuda_stream),
            ),
            "tmdhip_rescale_molecules",
        )


def _per_replica(value, name, positive):
    a = np.atleast_1d(np.asarray(value, dtype=np.float64))
    if a.ndim != 1 or a.size == 0 or not np.isfinite(a).all() or (positive and not (a > 0).all()):
        raise ValueError(f"{name} must be a finite{' positive' if positive else ''} number, or a sequence of them (one per replica)")
    return a, np.ndim(value) > 0


class CRescaleBarostat(Control):
    """Stochastic cell rescaling; see the module docstring.  `apply(system, forces, masses, dt, epot, ekin)` is what the
    integrator calls every `frequency` steps; it returns (and keeps as `.last`) a record with, per replica, `V`, `V_new`,
    `P_int` (kcal/mol/A^3), `xi`, `mu`, `U`, `U_new`, `K_before` and `K_after` (the kinetic energy of the atoms around the
    move).  `applications` counts them; `work()` is the energy bookkeeping; `rng` is the list of per-replica generators
    (anything with `.standard_normal()`)."""

    rank = 1
    virial_driven = True  # (moves every time, rescales velocities too and holds one target per replica; nothing dispatches on it)

    def __init__(self, pressure_bar, temperature, tau=1.0, compressibility=4.5e-5, frequency=10, stochastic=True, seed=None):
        self.pressures_bar, p_seq = _per_replica(pressure_bar, "pressure_bar", positive=False)
        self.temperatures, t_seq = _per_replica(temperature, "temperature", positive=True)
        self.compressibilities, c_seq = _per_replica(compressibility, "compressibility", positive=True)
        self._sequences = {"pressure_bar": (self.pressures_bar, p_seq), "temperature": (self.temperatures, t_seq),
                           "compressibility": (self.compressibilities, c_seq)}
        if not np.isfinite(tau) or not tau > 0:
            raise ValueError("tau must be a positive time in ps")
        super().__init__(frequency, seed)
        self.tau = float(tau)
        self.stochastic = bool(stochastic)
        self.last = None
        self.applications = 0
        self._work = None
        self._molecules = None

    # ------------------------------------------------------------------ set-up
    def targets(self, nreplicas):
        """(P0 [R] in kcal/mol/A^3, kT [R] in kcal/mol, beta [R] in A^3 mol/kcal); ValueError if a sequence was given and its
        length is not R."""
        out = []
        for name, (a, seq) in self._sequences.items():
            if seq and len(a) != nreplicas:
                raise ValueError(f"the barostat holds {len(a)} entries of {name} for {nreplicas} replicas")
            out.append(np.ascontiguousarray(np.broadcast_to(a, (nreplicas,)), dtype=np.float64))
        return out[0] * BAR_TO_KCAL_MOL_A3, BOLTZMAN * out[1], out[2] / BAR_TO_KCAL_MOL_A3

    def dt_over_tau(self, dt):
        """dt_p / tau_p for a time step `dt` in the integrator's time units."""
        return self.frequency * dt / (self.tau * PICOSEC2TIMEU)

    def check(self, integrator):
        """What is refused (ValueError) when the integrator is made: see `Integrator`'s `barostat` keyword."""
        from .domain import DomainSet
        from .forces import Forces

        it = integrator
        if isinstance(it.forces, DomainSet) or isinstance(it.systems, DomainSet):
            raise ValueError("the C-rescale barostat is not available under domain decomposition (a DomainSet)")
        if not isinstance(it.forces, Forces):
            raise ValueError("the barostat needs this package's Forces (the box it changes must reach the engine, and the "
                             "pressure comes from its virial); duck-typed force objects are not supported")
        if it.batch is not None:
            raise ValueError("the C-rescale barostat does not support atom groups (batch=): its molecules are per replica")
        R = it.systems.pos.shape[0]
        _, kT, _ = self.targets(R)
        th = it.thermostat
        # (a Langevin T with a friction of zero is no bath: nothing acts on the velocities)
        bath = th.targets(R) if th is not None else (np.full(R, float(it.T)) if it.T and it.gamma else None)
        if bath is None:
            if self.stochastic:
                raise ValueError("the stochastic C-rescale barostat needs a thermostat (Langevin T / gamma, or thermostat=): its "
                                 "noise is that of the bath; stochastic=False (Berendsen) runs without one")
        elif not np.array_equal(BOLTZMAN * np.asarray(bath, dtype=np.float64), kT):
            raise ValueError("the barostat's temperatures must equal the thermostat's, replica by replica")
        positive_edges(box_edges(it.systems.box))
        it.forces._molecules()  # (pressure.check_molecules: every exclusion and every site's parents inside one molecule)

    attach = check

    def after_segment(self, integrator, out):
        """Every replica is rescaled, velocities included: all three entries are those of the rescaled state."""
        it = integrator
        rec = self.apply(it.systems, it.forces, it.masses, it.dt, out[1], out[0])
        Ekin, it.kinetic_source = it._run_precision(rec["K_after"]), None
        return (Ekin, [float(u) for u in rec["U_new"]], it._temperature(Ekin))

    def _setup(self, system, forces):
        R, dev = system.pos.shape[0], system.pos.device
        self._streams(R, "barostat")
        if self._work is None:
            self._work = np.zeros(R, dtype=np.float64)
        off, mem, _ = forces._molecules()
        if self._molecules is None or self._molecules[0] is not off or self._molecules[1].device != dev:
            self._molecules = (off, torch.as_tensor(off, device=dev), torch.as_tensor(mem, device=dev), bool(np.any(np.diff(off) > 64)))
            self._record = None
        self._workspace("tmdhip_rescale_molecules_workspace", R, dev, len(off) - 1)

    # ------------------------------------------------------------------ one application
    def apply(self, system, forces, masses, dt, epot, ekin=None):
        """One box rescaling per replica.  `masses`: device tensor [N] or [N,1] of the dtype of the positions; `dt`: the time
        step in the integrator's units (`Integrator.dt`); `epot`: the potential energy of the current state per replica (what
        `Integrator.step` returned for it).  `ekin` is accepted for symmetry with `step()`'s return value and not used: the
        kernel measures the kinetic energy on both sides of the move itself (the thermostat may have rescaled since).  Reads
        the record back: one host synchronisation besides those of the pressure and of `compute`."""
        from .forces import Forces, _is_batched

        if not isinstance(forces, Forces):
            raise ValueError("the barostat needs this package's Forces (the box it changes must reach the engine)")
        if _is_batched(system.pos) or _is_batched(system.box):
            raise ValueError("the barostat cannot run under torch.vmap (its molecule table and lists are per replica)")
        R = system.pos.shape[0]
        p0, kT, beta = self.targets(R)
        self._setup(system, forces)
        _, off, mem, has_big = self._molecules
        m = masses.reshape(-1)
        box0 = system.box.detach().clone()
        edges = positive_edges(box_edges(box0))
        terms = forces._pressure_terms(system.pos, system.box, vel=system.vel, masses=m)
        V, p_int = terms[:, 6].copy(), terms[:, 7].copy()
        U = np.asarray(epot, dtype=np.float64).reshape(R)
        xi = np.array([g.standard_normal() for g in self.rng], dtype=np.float64)  # always drawn
        mu = np.exp(delta_epsilon(p0, p_int, V, kT, beta, self.dt_over_tau(dt), xi, self.stochastic) / 3.0)
        if not (np.isfinite(mu).all() and (mu > 0).all()):
            raise RuntimeError("barostat: the box factor is not positive and finite (pressure or volume out of range)")
        new_box, new_edges, V_new = scaled_box(box0, edges, mu)

        rescale_molecules(system.pos, system.vel, m, new_edges / edges, off, mem, has_big, self._record, self._partials)
        system.box.copy_(new_box)  # through torch: Forces._host_box keys on the tensor's version counter
        U_new = np.asarray(forces.compute(system.pos, system.box, system.forces), dtype=np.float64).reshape(R)
        forget_continuation(forces, system.pos)
        K = self._record[:, :2].cpu().numpy()

        self._work += (K[:, 1] - K[:, 0]) + (U_new - U) + p0 * (V_new - V)
        self.applications += 1
        self.last = dict(zip(_KEYS, (V, V_new, p_int, xi, mu, U, U_new, K[:, 0].copy(), K[:, 1].copy())))
        return self.last

    def work(self):
        """The change of E_kin + E_pot + P0 V summed over all applications, host array [R] in kcal/mol (None before the
        first): E_kin + E_pot + P0 V - heat - work is the conserved quantity."""
        return None if self._work is None else self._work.copy()
