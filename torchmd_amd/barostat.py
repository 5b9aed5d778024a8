"""Constant pressure: an isotropic Monte Carlo barostat for orthorhombic periodic boxes.

`MonteCarloBarostat(pressure_bar, temperature, frequency=25, seed=None)`, handed to `Integrator(..., barostat=...)`,
attempts a volume change every `frequency` steps (Chow & Ferguson 1995; Aqvist et al. 2004; the scheme of OpenMM's
`MonteCarloBarostat`).  One attempt, for every replica independently:

1. V = Lx Ly Lz; dV uniform in [-dVmax, +dVmax]; the three edges are multiplied by s = ((V + dV) / V)^(1/3) and V' is
   the product of the new edges;
2. every molecule (connected component of the bond graph, `wrapper.calculate_molecule_groups`; atoms without bonds are
   molecules of one) is moved rigidly so that its centre — the unweighted mean of its atoms — follows the box
   (`tmdhip_scale_groups`, one launch for all replicas, which also keeps a copy of the old positions);
3. U' = `forces.compute` at the new positions and box, with the forces written to a scratch tensor;
4. w = (U' - U) + P (V' - V) - N_mol k_B T ln(V'/V); the move is accepted if w <= 0 or u < exp(-w / k_B T);
5. an accepted replica takes the scratch forces; a rejected one gets its positions and box back bit for bit (a copy,
   not a scaling by 1/s) and keeps its forces.  Velocities are never touched;
6. dVmax starts at 1 % of V; after every 10 attempts of a replica it is divided by 1.1 if fewer than 25 % of them were
   accepted and multiplied by 1.1 (at most 0.3 V) if more than 75 % were.

Only energies are needed — no virial —, and because molecules move rigidly every constrained bond length is
untouched, so the barostat composes with `pme=True` and with `constraints=`.  Molecules must be whole (not split across
the periodic boundary): true of what `Wrapper.wrap` leaves and of unwrapped trajectories.

Random numbers: every replica owns a `numpy.random.Generator(Philox(key=(seed, replica)))` and draws exactly two numbers
per attempt (dV first, then u), so a replica's stream does not depend on how many replicas run beside it.
"""

from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib as L
from .controls import Control, box_edges, forget_continuation, positive_edges, require_layout, scaled_box
from .integrator import BOLTZMAN
from .wrapper import calculate_molecule_groups

AVOGADRO = 6.02214076e23
# 1 bar = 1e5 J/m^3 = 1e-25 J/A^3; times N_A / 4184 J/kcal: 1.4393e-5 kcal/mol/A^3
BAR_TO_KCAL_MOL_A3 = AVOGADRO * 1e-25 / 4184.0

ADAPT_EVERY = 10
ADAPT_FACTOR = 1.1
MAX_DV_FRACTION = 0.3
START_DV_FRACTION = 0.01


def acceptance_weight(U, U_new, V, V_new, ngroups, pressure_bar, temperature):
    """w = (U' - U) + P (V' - V) - N_groups k_B T ln(V'/V) in kcal/mol (U in kcal/mol, V in A^3, P in bar, T in K).
    The move is accepted when w <= 0 or u < exp(-w / k_B T)."""
    kT = BOLTZMAN * temperature
    return (U_new - U) + pressure_bar * BAR_TO_KCAL_MOL_A3 * (V_new - V) - ngroups * kT * np.log(V_new / V)


def scale_groups(pos, scale, offsets, members, has_big, saved=None):
    """`tmdhip_scale_groups`: translate every group of `pos` [R,N,3] (device, in place) by (scale[r] - 1) * its centre;
    `scale` is a host array [R,3]; `offsets` / `members`: the groups' CSR as int32 device tensors; `saved` (like `pos`,
    or None) receives the positions as they were."""
    R, N = require_layout(pos, "pos")
    sc = np.ascontiguousarray(np.asarray(scale, dtype=np.float64).reshape(R, 3))
    if saved is not None and (saved.shape != pos.shape or saved.dtype != pos.dtype or saved.device != pos.device
                              or not saved.is_contiguous()):
        raise RuntimeError("saved must be a contiguous tensor with the shape, dtype and device of pos")
    for name, t in (("offsets", offsets), ("members", members)):
        if t.dtype != torch.int32 or t.device != pos.device or not t.is_contiguous():
            raise RuntimeError(f"{name} must be a contiguous int32 tensor on the device of pos")
    ngroups = offsets.numel() - 1
    if members.numel() != N:
        raise RuntimeError("the groups must cover every atom exactly once")
    with torch.cuda.device(pos.device):
        L.check(
            L.load().tmdhip_scale_groups(
                L.dtype_code(pos.dtype), R, N, pos.data_ptr(), saved.data_ptr() if saved is not None else None,
                sc.ctypes.data_as(C.POINTER(C.c_double)), ngroups, offsets.data_ptr(), members.data_ptr(),
                1 if has_big else 0, C.c_void_p(torch.cuda.current_stream(pos.device).cuda_stream),
            ),
            "tmdhip_scale_groups",
        )


class MonteCarloBarostat(Control):
    """Isotropic Monte Carlo pressure coupling; see the module docstring.  `attempt(system, forces, epot)` is what the
    integrator calls every `frequency` steps; it returns (and keeps as `.last`) a record with, per replica, `V`, `V_new`,
    `U`, `U_new`, `u_volume`, `u_accept`, `w` and `accepted`.  `attempts` / `accepted` count per replica; `max_dv` holds
    the current dVmax per replica.  `rng` is the list of per-replica generators (anything with `.random()`)."""

    rank, ladder_ok = 1, False

    def __init__(self, pressure_bar, temperature, frequency=25, seed=None):
        if not np.isfinite(pressure_bar):
            raise ValueError("pressure_bar must be finite")
        if not temperature or not temperature > 0:
            raise ValueError("the barostat needs a positive temperature (that of the thermostat)")
        super().__init__(frequency, seed)
        self.pressure_bar = float(pressure_bar)
        self.temperature = float(temperature)
        self.max_dv = None
        self.attempts = self.accepted = None
        self.last = None
        self._window = None  # [R,2]: attempts and acceptances since the last look at the step size
        self._groups = None
        self._saved = self._scratch = None

    # ------------------------------------------------------------------ set-up
    def check(self, system, forces, temperature=None):
        """What is refused (ValueError): non-periodic boxes, a missing temperature, foreign force objects."""
        from .forces import Forces

        if not isinstance(forces, Forces):
            raise ValueError("the barostat needs this package's Forces (the box it changes must reach the engine); "
                             "duck-typed force objects are not supported")
        if temperature is not None and not temperature:
            raise ValueError("the barostat needs a thermostat: set T (and gamma) on the integrator")
        positive_edges(box_edges(system.box))

    def attach(self, integrator):
        it, th = integrator, integrator.thermostat
        self.check(it.systems, it.forces, temperature=(th.temperature if th is not None else it.T) or 0)

    def after_segment(self, integrator, out):
        """The potential energy of the replicas whose move was accepted changes; velocities are never touched."""
        rec = self.attempt(integrator.systems, integrator.forces, out[1])
        pot = [float(un if ok else u) for u, un, ok in zip(rec["U"], rec["U_new"], rec["accepted"])]
        return (out[0], pot, out[2])

    def _setup(self, system, forces):
        R, N = system.pos.shape[0], system.pos.shape[1]
        self._streams(R, "barostat")
        if self.attempts is None:
            self.attempts = np.zeros(R, dtype=np.int64)
            self.accepted = np.zeros(R, dtype=np.int64)
            self._window = np.zeros((R, 2), dtype=np.int64)
        if self._groups is None or self._groups[0] != N or self._groups[1].device != system.pos.device:
            bp = getattr(forces.par, "bond_params", None)
            bonds = bp["idx"].detach().cpu().numpy() if bp is not None and len(bp["idx"]) else None
            off, mem = calculate_molecule_groups(N, bonds)
            dev = system.pos.device
            self._groups = (N, torch.as_tensor(off, device=dev), torch.as_tensor(mem, device=dev), bool(np.any(np.diff(off) > 64)),
                            len(off) - 1)
        if self._saved is None or self._saved.shape != system.pos.shape or self._saved.dtype != system.pos.dtype \
                or self._saved.device != system.pos.device:
            self._saved = torch.empty_like(system.pos)
            self._scratch = torch.empty_like(system.pos)

    @property
    def ngroups(self):
        return None if self._groups is None else self._groups[4]

    # ------------------------------------------------------------------ one attempt
    def attempt(self, system, forces, epot):
        """One trial volume change per replica.  `epot`: the potential energy of the current state per replica (what
        `Integrator.step` or `forces.compute` returned for it); `system.forces` must hold the forces of that state."""
        from .forces import Forces

        if not isinstance(forces, Forces):
            raise ValueError("the barostat needs this package's Forces (the box it changes must reach the engine)")
        self._setup(system, forces)
        R = system.pos.shape[0]
        _, off, mem, has_big, ngroups = self._groups
        kT = BOLTZMAN * self.temperature
        box0 = system.box.detach().clone()
        edges = positive_edges(box_edges(box0))
        V =edges[:, 0] * edges[:, 1] * edges[:, 2]
        if self.max_dv is None:
            self.max_dv = START_DV_FRACTION * V
        U = np.asarray(epot, dtype=np.float64).reshape(R)
        u = np.array([[g.random(), g.random()] for g in self.rng], dtype=np.float64)  # dV, then acceptance: always both
        dV = self.max_dv * 2.0 * (u[:, 0] - 0.5)
        s = ((V + dV) / V) ** (1.0 / 3.0)
        if not (np.isfinite(s).all() and (s > 0).all()):
            raise RuntimeError("barostat: the trial volume is not positive")
        trial, new_edges, V_new = scaled_box(box0, edges, s)
        scale = np.where((dV == 0.0)[:, None], 1.0, new_edges / edges)

        scale_groups(system.pos, scale, off, mem, has_big, saved=self._saved)
        system.box.copy_(trial)  # through torch: Forces._host_box keys on the tensor's version counter
        U_new = np.asarray(forces.compute(system.pos, system.box, self._scratch), dtype=np.float64).reshape(R)

        w = acceptance_weight(U, U_new, V, V_new, ngroups, self.pressure_bar, self.temperature)
        with np.errstate(over="ignore", invalid="ignore"):
            ok = (w <= 0) | (u[:, 1] < np.exp(-w / kT))
        ok &= np.isfinite(U_new)
        for r in range(R):
            if ok[r]:
                system.forces[r].copy_(self._scratch[r])
            else:
                system.pos[r].copy_(self._saved[r])
        if not ok.all():
            final = trial
            for r in np.flatnonzero(~ok):
                final[r].copy_(box0[r])
            system.box.copy_(final)
        forget_continuation(forces, system.pos)

        self.attempts += 1
        self.accepted += ok
        self._window[:, 0] += 1
        self._window[:, 1] += ok
        V_now = np.where(ok, V_new, V)
        for r in range(R):
            n, a = self._window[r]
            if n >= ADAPT_EVERY:
                if a < 0.25 * n:
                    self.max_dv[r] /= ADAPT_FACTOR
                elif a > 0.75 * n:
                    self.max_dv[r] = min(self.max_dv[r] * ADAPT_FACTOR, MAX_DV_FRACTION * V_now[r])
                self._window[r] = 0
        self.last = {"V": V, "V_new": V_new, "U": U, "U_new": U_new, "u_volume": u[:, 0].copy(), "u_accept": u[:, 1].copy(),
                     "w": w, "accepted": ok.copy()}
        return self.last
