"""Constant temperature without friction on every atom: stochastic velocity rescaling with one target per replica, and
centre-of-mass motion removal.

`VelocityRescale(temperature, tau=0.1, frequency=10, remove_com=True, seed=None)`, handed to `Integrator(..., thermostat=...)`,
rescales the velocities of every replica every `frequency` steps (Bussi, Donadio & Parrinello, J. Chem. Phys. 126, 014101,
2007: "CSVR", GROMACS' `v-rescale`).  One application, for every replica r independently, over the atoms with mass > 0:

1. V_cm = sum m v / sum m when `remove_com` is on (else 0); K = (1/2) sum m v^2 - (1/2) (sum m) V_cm^2;
2. alpha^2 = c + (1 - c) Kbar (R1^2 + S) / (N_f K) + 2 R1 sqrt(c (1 - c) Kbar / (N_f K)) with the target
   Kbar = N_f k_B T_r / 2, c = exp(-frequency dt / tau), R1 a standard normal and S a chi-squared variate with N_f - 1
   degrees of freedom; alpha = +sqrt(max(alpha^2, 0)), and alpha = 1 when K = 0;
3. v <- alpha (v - V_cm).

The kinetic energy then samples the canonical distribution of the target temperature, with a relaxation time `tau`;
`tau=0` (c = 0) draws a fresh canonical K at every application.  Everything runs in two launches of
`tmdhip_thermostat_apply` (thermostat.hip), all sums in double; nothing is read back, so an application costs no host
synchronisation.  `temperature` may be a sequence with one entry per replica: a temperature ladder.

N_f is the number of degrees of freedom the integrator uses for its temperature (3 per massive atom, or
`ConstraintSet.ndof()` with constraints), minus 3 when `remove_com` is on: the centre-of-mass motion the thermostat takes
out carries no thermal energy.  `Integrator._temperature` keeps its own count, so the temperature `step()` returns is lower
than the target by the factor N_f / (N_f + 3) on average.

Random numbers: every replica owns a `numpy.random.Generator(Philox(key=(seed, replica)))` (as the barostat) and draws
exactly two numbers per application, R1 = standard_normal() first, then S = 2 standard_gamma((N_f - 1) / 2), so a replica's
chain does not depend on how many replicas run beside it.  The energy the thermostat has put into a replica is accumulated
on the device (`heat()`): E_kin + E_pot - heat is the conserved quantity of a thermostatted run.
"""

from __future__ import annotations

import ctypes as C
import math

import numpy as np
import torch

from . import _lib as L
from .controls import Control, require_layout
from .integrator import BOLTZMAN, PICOSEC2TIMEU

_DP = C.POINTER(C.c_double)


def _dp(a):
    return a.ctypes.data_as(_DP)


class VelocityRescale(Control):
    """Stochastic velocity rescaling; see the module docstring.  `apply(system, masses, dt, ndof)` is what the integrator calls
    every `frequency` steps.  `last`: the device record of the last application, double [R, 4] = {K_before, alpha, K_after,
    |V_cm|} per replica (K of the centre-of-mass-free velocities when `remove_com` is on); `heat()`: the sum of
    K_after - K_before over all applications, per replica; `draws`: the host array [R, 2] of the (R1, S) of the last
    application; `applications`: how many were made; `nf`: the N_f of the last application; `rng`: the list of per-replica
    generators (anything with `.standard_normal()` and `.standard_gamma(shape)`)."""

    rank = 0

    def __init__(self, temperature, tau=0.1, frequency=10, remove_com=True, seed=None):
        t = np.atleast_1d(np.asarray(temperature, dtype=np.float64))
        if t.ndim != 1 or t.size == 0 or not np.isfinite(t).all() or not (t > 0).all():
            raise ValueError("temperature must be a positive number, or a sequence of positive numbers (one per replica)")
        if not np.isfinite(tau) or tau < 0:
            raise ValueError("tau must be a non-negative time in ps (0: the kinetic energy is resampled at every application)")
        super().__init__(frequency, seed)
        self.temperatures = t
        self.ladder = np.ndim(temperature) > 0  # a sequence (even of length 1) must match the number of replicas
        self.tau = float(tau)
        self.remove_com = bool(remove_com)
        self.draws = None
        self.nf = None
        self.applications = 0

    # ------------------------------------------------------------------ set-up
    @property
    def temperature(self):
        """The common target temperature, or None for a ladder of different ones."""
        return float(self.temperatures[0]) if np.all(self.temperatures == self.temperatures[0]) else None

    def targets(self, nreplicas):
        """Target temperature per replica [R] (ValueError if a sequence was given and its length is not R)."""
        if self.ladder and len(self.temperatures) != nreplicas:
            raise ValueError(f"the thermostat holds {len(self.temperatures)} target temperatures for {nreplicas} replicas")
        return np.broadcast_to(self.temperatures, (nreplicas,)) if not self.ladder else self.temperatures

    def decay(self, dt):
        """c = exp(-frequency dt / tau) for a time step `dt` in the integrator's time units; 0 for tau = 0."""
        return math.exp(-self.frequency * dt / (self.tau * PICOSEC2TIMEU)) if self.tau > 0 else 0.0

    def degrees_of_freedom(self, ndof):
        """N_f: `ndof` (what the integrator divides by for its temperature), minus 3 with `remove_com`."""
        nf = int(ndof) - (3 if self.remove_com else 0)
        if nf < 2:
            raise ValueError(f"the thermostat needs at least 2 degrees of freedom, has {nf}")
        return nf

    def attach(self, integrator):
        """What is refused (ValueError): a second thermostat (Langevin), atom groups, a ladder of the wrong length, a ladder
        under a barostat that knows one temperature.  N_f is the integrator's count of degrees of freedom minus 3 when the
        centre-of-mass motion is removed; `Integrator._temperature` keeps dividing by the full count."""
        it = integrator
        if it.T or it.gamma is not None:
            raise ValueError("thermostat= and a Langevin T / gamma are two thermostats: give one of them")
        if it.batch is not None:
            raise ValueError("thermostat= does not support atom groups (batch=): its scale factor is per replica")
        self.targets(it.systems.pos.shape[0])
        if it.barostat is not None and self.temperature is None and not it.barostat.ladder_ok:
            raise ValueError("a temperature ladder cannot run under barostat=: the barostat holds one temperature")
        ndof = int(it._ndof) if it.constraints is not None else 3 * int((it.masses > 0).sum().item())
        self.degrees_of_freedom(ndof)
        it._thermostat_ndof = ndof

    def after_segment(self, integrator, out):
        it = integrator
        self.apply(it.systems, it.masses, it.dt, it._thermostat_ndof)
        it.kinetic_source = self
        return out

    def kinetic(self):
        return self.last[:, L.THERMOSTAT_K_AFTER]

    # ------------------------------------------------------------------ one application
    def apply(self, system, masses, dt, ndof, active=None):
        """Enqueue one application on the current stream (no host synchronisation).  `system.vel` [R, N, 3] is rescaled in
        place; `masses` [N] or [N, 1]: a device tensor of the dtype of the velocities, rows with mass 0 are left alone;
        `dt`: the time step in the integrator's time units (`Integrator.dt`), the time between two applications being
        `frequency * dt`; `ndof`: the degrees of freedom before the centre-of-mass motion is taken off (3 per massive atom,
        or `ConstraintSet.ndof()`); `active` (optional, [R]): replicas with a 0 are skipped — their velocities and
        records stay, their random numbers are drawn all the same."""
        vel = system.vel
        R, N = require_layout(vel, "system.vel", masses)
        T = np.ascontiguousarray(self.targets(R), dtype=np.float64)
        nf = self.degrees_of_freedom(ndof)
        self._streams(R, "thermostat")
        self._workspace("tmdhip_thermostat_workspace", R, vel.device)
        draws = np.array([[g.standard_normal(), 2.0 * g.standard_gamma(0.5 * (nf - 1))] for g in self.rng], dtype=np.float64)
        kbar = np.ascontiguousarray(0.5 * nf * BOLTZMAN * T)
        nfs = np.full(R, float(nf))
        c = np.full(R, self.decay(dt))
        r1, s = np.ascontiguousarray(draws[:, 0]), np.ascontiguousarray(draws[:, 1])
        act = None
        if active is not None:
            act = np.ascontiguousarray(np.asarray(active).reshape(R) != 0, dtype=np.int32)
        with torch.cuda.device(vel.device):
            L.check(
                L.load().tmdhip_thermostat_apply(
                    L.dtype_code(vel.dtype), R, N, vel.data_ptr(), masses.data_ptr(), _dp(kbar), _dp(nfs), _dp(c), _dp(r1), _dp(s),
                    act.ctypes.data_as(C.POINTER(C.c_int32)) if act is not None else None, 1 if self.remove_com else 0,
                    self._record.data_ptr(), self._partials.data_ptr(),
                    C.c_void_p(torch.cuda.current_stream(vel.device).cuda_stream),
                ),
                "tmdhip_thermostat_apply",
            )
        self.draws = draws
        self.nf = nf
        self.applications += 1

    @property
    def last(self):
        """Device record of the last application, double [R, 4]: K_before, alpha, K_after, |V_cm| (None before the first)."""
        return None if self._record is None else self._record[:, : L.THERMOSTAT_VCM + 1]

    def heat(self):
        """Energy the thermostat has put into each replica so far (sum of K_after - K_before), host array [R]; synchronises."""
        if self._record is None:
            return None
        return self._record[:, L.THERMOSTAT_HEAT].cpu().numpy().copy()
