"""Energy minimisers driving `Forces.compute` (mirror of the reference module `torchmd/minimizers.py`:
same function names, arguments and effect on `system.pos`).  They are callers of the hot path, not part
of it: every energy/force evaluation is one `forces.compute(pos, box, forces)` on the device; the
optimisation logic runs on the host (scipy L-BFGS-B), in torch (LBFGS on the differentiable potential)
or as a few tensor operations per line-search point (conjugate gradient).

`minimize_fire` has no counterpart in the reference and is built differently: FIRE needs forces only, so an
iteration is the integrator's force-only evaluation plus two HIP launches (`tmdhip_fire_step`), the state of every replica
stays on the device, and the host reads it back once per `check_every` iterations.
"""

from __future__ import annotations

import ctypes as C
import logging
from dataclasses import dataclass

import numpy as np
import torch

from . import _lib as L

logger = logging.getLogger(__name__)

_GOLDEN = 0.618033988749895  # (sqrt(5) - 1) / 2


def minimize_bfgs(system, forces, fmax=0.5, steps=1000):
    """scipy L-BFGS-B on the potential of the single replica (reference minimizers.py:8-51):
    `gtol = fmax`, `maxiter = steps`; the minimum is written to `system.pos`."""
    from scipy.optimize import minimize

    if steps == 0:
        return None
    if system.pos.shape[0] != 1:
        raise RuntimeError("System minimization currently doesn't support replicas")
    n = system.pos.shape[1]
    count = [0]

    def fun(x):
        system.pos[:] = torch.as_tensor(x.reshape(1, n, 3), dtype=system.pos.dtype, device=system.pos.device)
        e = forces.compute(system.pos, system.box, system.forces)[0]
        g = -system.forces.detach().cpu().numpy().astype(np.float64)[0]
        logger.info("%4d   % 3.6f   % 3.6f", count[0], e, np.max(np.linalg.norm(g, axis=1)))
        count[0] += 1
        return float(e), g.reshape(-1)

    x0 = system.pos.detach().cpu().numpy().astype(np.float64).reshape(-1)
    res = minimize(fun, x0, method="L-BFGS-B", jac=True, options={"gtol": fmax, "maxiter": steps, "disp": False})
    system.pos[:] = torch.as_tensor(res.x.reshape(1, n, 3), dtype=system.pos.dtype, device=system.pos.device)
    return res


def minimize_pytorch_bfgs(system, calculator, steps=10, max_iter=20, tolerance_change=1e-9):
    """`torch.optim.LBFGS` on the summed potential of all replicas, through the differentiable
    `compute(..., toNumpy=False)` (reference minimizers.py:54-96).  Returns the energies seen, shape
    [nreplicas, evaluations]."""
    if steps == 0:
        return None
    x = system.pos.detach().clone().requires_grad_(True)
    opt = torch.optim.LBFGS([x], max_iter=max_iter, tolerance_change=tolerance_change)
    seen = []

    def closure():
        opt.zero_grad()
        pots = calculator.compute(x, system.box, system.forces, explicit_forces=False, toNumpy=False)
        pots = torch.stack([p.reshape(()) for p in pots]) if isinstance(pots, (list, tuple)) else pots.reshape(-1)
        seen.append(pots.detach().cpu().numpy())
        total = pots.sum()
        if x.grad is None and total.requires_grad:
            total.backward()
        elif not total.requires_grad:  # calculator without autograd support: use its explicit forces
            x.grad = -system.forces.detach().clone()
        return total

    for _ in range(steps):
        opt.step(closure)
    with torch.no_grad():
        system.pos[:] = x.detach()
    return np.stack(seen, axis=1)


def _energy_forces(forces, system, pos):
    e = forces.compute(pos, system.box, system.forces)[0]
    return float(e), system.forces.detach()[0].clone()


def _line_minimum(forces, system, start, direction, u0, max_disp=1.0, tol=1e-2):
    """Golden-section search for the minimum of U(start + a * direction), a in [0, max_disp / max |d_i|]
    (no atom moves further than `max_disp` Angstrom per line search; reference minimizers.py:108-262)."""
    dmax = float(torch.sqrt((direction**2).sum(dim=1).max()))
    if dmax == 0.0:
        return start, u0
    lo, hi = 0.0, max_disp / dmax
    width0 = hi - lo

    def energy(a):
        return _energy_forces(forces, system, (start + a * direction)[None])[0]

    a1, a2 = hi - _GOLDEN * (hi - lo), lo + _GOLDEN * (hi - lo)
    u1, u2 = energy(a1), energy(a2)
    best_a, best_u = 0.0, u0
    while (hi - lo) > tol * width0:
        if u1 < u2:
            hi, a2, u2 = a2, a1, u1
            a1 = hi - _GOLDEN * (hi - lo)
            u1 = energy(a1)
        else:
            lo, a1, u1 = a1, a2, u2
            a2 = lo + _GOLDEN * (hi - lo)
            u2 = energy(a2)
        for a, u in ((a1, u1), (a2, u2)):
            if u < best_u:
                best_a, best_u = a, u
    return start + best_a * direction, best_u


def minimize_cg(system, forces, steps=1000, start_step: int = 0, threshold=None):
    """Fletcher-Reeves conjugate gradient with a golden-section line search (reference
    minimizers.py:264-310).  Returns the index of the last step taken; stops early when the largest force
    component drops below `threshold`."""
    if system.pos.shape[0] != 1:
        raise RuntimeError("System minimization currently doesn't support replicas")
    pos = system.pos.detach()[0].clone()
    u, frc = _energy_forces(forces, system, pos[None])
    direction = frc.clone()
    fdf = float((frc**2).sum())
    last = start_step
    for step in range(start_step, steps):
        last = step
        pos, u = _line_minimum(forces, system, pos, direction, u)
        u, frc = _energy_forces(forces, system, pos[None])
        new_fdf = float((frc**2).sum())
        beta = new_fdf / fdf if fdf > 0 else 0.0
        fdf = new_fdf
        direction = frc + beta * direction
        fmax = float(frc.abs().max())
        logger.info("%12d %14.4f %16.4f", step, u, fmax)
        if threshold is not None and fmax < threshold:
            break
    with torch.no_grad():
        system.pos[0] = pos
    forces.compute(system.pos, system.box, system.forces)
    return last


@dataclass
class FireResult:
    """What `minimize_fire` did, one entry per replica: `converged` (bool; the largest atom force fell below `fmax`),
    `iterations` (moves made), `fmax` (largest atom force norm at the returned positions, kcal/mol/A) and `nuphill` (how often
    the power F.v was not positive and the velocities were dropped)."""

    converged: np.ndarray
    iterations: np.ndarray
    fmax: np.ndarray
    nuphill: np.ndarray


_SEGMENT_FAILED = ("minimize_fire(): a stretch of iterations was rewound to its check point and repeated once with fresh "
                   "neighbour lists and failed again; system.pos holds the check point.  The library says: ")


def _fire_segments(ops, steps, check_every):
    """The host side of `minimize_fire`: enqueue `check_every` iterations at a time, then look once.  `ops` supplies
    `save()` (snapshot of positions, velocities and state: the check point), `advance(first, n)` (enqueue iterations first ..
    first + n - 1), `verify()` (False: a neighbour list overflowed or outlived its skin during the stretch), `restore()`,
    `invalidate()`, `all_done()` (one read-back of the state) and `error()` (the library's message).  A stretch that fails is
    rewound to its check point and repeated once with fresh lists; a second failure raises.  Returns the number of iterations
    enqueued (a replica that converged earlier was frozen on the device from then on)."""
    first = 0
    ops.save()
    while first < steps:
        n = min(check_every, steps - first)
        ops.advance(first, n)
        if not ops.verify():
            ops.restore()
            ops.invalidate()
            ops.advance(first, n)
            if not ops.verify():
                why = ops.error()
                ops.restore()
                raise RuntimeError(_SEGMENT_FAILED + why)
        first += n
        if ops.all_done():
            break
        if first < steps:
            ops.save()
    return first


class _FireOps:
    """`_fire_segments` on the device: this package's `Forces` and `tmdhip_fire_step`."""

    def __init__(self, system, forces, masses, prm):
        pos = system.pos
        self.system, self.forces, self.masses, self.prm = system, forces, masses, prm
        self.lib = L.load()
        self.code = L.dtype_code(pos.dtype)
        R = pos.shape[0]
        self.vel = torch.zeros_like(pos)  # FIRE's own velocities: system.vel is not touched
        self.state = torch.zeros((R, 2, L.FIRE_STATE_DOUBLES), dtype=torch.float64, device=pos.device)
        self.partials = torch.zeros((R, L.FIRE_MAX_BLOCKS, 4), dtype=torch.float64, device=pos.device)
        self.saved = (torch.empty_like(pos), torch.empty_like(pos), torch.empty_like(self.state))
        self.eng = forces._engine(pos.detach())
        self.done = 0  # iterations enqueued: the live state slot is `done & 1`
        L.check(self.lib.tmdhip_fire_init(R, self.state.data_ptr(), C.byref(prm), self._stream()), "tmdhip_fire_init")

    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.system.pos.device).cuda_stream)

    def save(self):
        for dst, src in zip(self.saved, (self.system.pos, self.vel, self.state)):
            dst.copy_(src.detach())

    def restore(self):
        for dst, src in zip((self.system.pos, self.vel, self.state), self.saved):
            dst.detach().copy_(src)

    def invalidate(self):
        self.forces.invalidate_lists(self.system.pos)

    def advance(self, first, n):
        s, lib = self.system, self.lib
        pos = s.pos.detach()
        R, N = pos.shape[0], pos.shape[1]
        args = (self.code, R, N, pos.data_ptr(), self.vel.data_ptr(), s.forces.data_ptr(), self.masses.data_ptr(),
                self.state.data_ptr(), self.partials.data_ptr(), C.byref(self.prm))
        for it in range(first, first + n):
            self.forces._compute_async(pos, s.box, s.forces, want_energy=False)
            L.check(lib.tmdhip_fire_step(*args, it, self._stream()), "tmdhip_fire_step")
        self.done = first + n

    def verify(self):
        return self.forces._verify(self.eng, self.system.pos)

    def error(self):
        return L.last_error()

    def live_state(self):
        return self.state[:, self.done & 1].cpu().numpy()

    def all_done(self):
        return bool((self.live_state()[:, L.FIRE_DONE] != 0).all())


def minimize_fire(system, forces, fmax=0.5, steps=1000, timestep=1.0, dt_max=None, max_step=0.1, n_min=5, f_inc=1.1,
                  f_dec=0.5, alpha_start=0.1, f_alpha=0.99, check_every=50):
    """FIRE (Bitzek et al., PRL 97, 170201, 2006) on every replica of `system.pos` at once, independently and in place, until
    the largest atom force of a replica is below `fmax` (kcal/mol/A) or `steps` iterations were made.  `timestep` (fs, converted
    as `Integrator` does) is the first time step of the damped dynamics, `dt_max` its ceiling (default 10 x `timestep`),
    `max_step` (A) the largest move of one atom in one iteration; the other arguments are the constants of the paper.

    One iteration is `forces._compute_async(..., want_energy=False)` (forces only: virtual-site placement and spreading, PME,
    the bonded terms and `external` included; no host synchronisation) and one `tmdhip_fire_step` (two HIP launches, DESIGN
    §13).  The state of every replica (time step, mixing factor, counters, the `done` flag) lives on the device; a replica that
    has converged is frozen there, bit for bit, however many iterations are still enqueued.  The host looks once per
    `check_every` iterations: it reads the state, checks the neighbour lists (`forces._verify`) and stops when every replica is
    done.  If a list overflowed or outlived its skin, positions, velocities and state go back to the previous check point, the
    lists are dropped and the stretch is repeated once; a second failure raises `RuntimeError`.

    Masses as in `Integrator`: `system.masses`, else `forces.par.masses`.  Rows with mass 0 (virtual sites) are no degrees of
    freedom: they enter no sum and are moved only by the site placement of the force evaluation.  The velocities of the damped
    dynamics are private, `system.vel` is not touched; `system.forces` holds the forces of the returned positions.

    Rigid units are not handled: this minimises the flexible model, whose bond and angle minima are the rigid geometry the
    constraint finder reads, and leaves the projection onto the constraints to `Integrator._project_start`.

    Returns a `FireResult`, or None for `steps == 0`.  `ValueError` for a force object that is not this package's `Forces`
    (the loop needs `_compute_async` and `_verify`), a non-contiguous `pos`, a `pos` whose dtype differs from that of `system.forces`,
    and `fmax <= 0`."""
    from .forces import Forces
    from .integrator import TIMEFACTOR

    if steps == 0:
        return None
    if not isinstance(forces, Forces):
        raise ValueError("minimize_fire needs this package's Forces (its force-only evaluation `_compute_async` and its list "
                         "check `_verify`); a duck-typed force object is not supported")
    if not fmax > 0:
        raise ValueError(f"fmax must be positive, got {fmax}")
    if steps < 0 or check_every < 1:
        raise ValueError("steps must not be negative and check_every must be at least 1")
    pos = system.pos
    L.require_device_tensor(pos, "system.pos")
    if not pos.is_contiguous():
        raise ValueError("system.pos must be contiguous (it is updated in place by the HIP kernels)")
    if pos.dtype != system.forces.dtype or not system.forces.is_contiguous() or system.forces.shape != pos.shape:
        raise ValueError("system.forces must be contiguous and have the dtype and shape of system.pos")
    if torch.any(system.masses != 0):
        masses = system.masses
    else:
        masses = torch.as_tensor(forces.par.masses).detach().clone()
    masses = masses.to(device=pos.device, dtype=pos.dtype).reshape(-1).contiguous()
    if masses.numel() != pos.shape[1]:
        raise ValueError("one mass per atom is needed")
    prm = L.FireParams()
    prm.struct_size = C.sizeof(L.FireParams)
    prm.n_min = int(n_min)
    prm.f_tol = float(fmax)
    prm.dt_start = float(timestep) / TIMEFACTOR
    prm.dt_max = (10.0 * float(timestep) if dt_max is None else float(dt_max)) / TIMEFACTOR
    prm.max_step = float(max_step)
    prm.f_inc, prm.f_dec, prm.alpha_start, prm.f_alpha = float(f_inc), float(f_dec), float(alpha_start), float(f_alpha)
    with torch.cuda.device(pos.device):
        ops = _FireOps(system, forces, masses, prm)
        _fire_segments(ops, int(steps), int(check_every))
        # the forces of the returned positions, and their largest norm over the real atoms (once per call, not per iteration)
        forces._compute_async(pos.detach(), system.box, system.forces, want_energy=False)
        norm = torch.linalg.vector_norm(system.forces.detach().to(torch.float64), dim=2)
        norm = torch.where(masses.reshape(1, -1) > 0, norm, torch.zeros_like(norm)).max(dim=1).values.cpu().numpy()
        state = ops.live_state()
        if not forces._verify(ops.eng, pos):
            raise RuntimeError("minimize_fire(): a neighbour list failed in the evaluation of the returned positions: " + L.last_error())
    res = FireResult(converged=state[:, L.FIRE_DONE] != 0, iterations=state[:, L.FIRE_ITERATIONS].astype(np.int64), fmax=norm,
                     nuphill=state[:, L.FIRE_NUPHILL].astype(np.int64))
    logger.info("minimize_fire: iterations %s, fmax %s, converged %s", res.iterations, res.fmax, res.converged)
    return res
