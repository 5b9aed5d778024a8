"""What acts between batches of steps — thermostat, barostats, replica exchange, the metadynamics deposition — as one
protocol, and the helpers those classes share ("Adding a scheduled control").  Imports none of them."""

from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib as L


def draw_seed(seed=None):
    """`seed`, or one drawn from torch's global generator so torch.manual_seed() reproduces runs."""
    return int(seed) if seed is not None else int(torch.randint(0, 2**62, (1,), dtype=torch.int64).item())


def philox_stream(seed, r):
    return np.random.Generator(np.random.Philox(key=np.array([seed, r], dtype=np.uint64)))


def whole_frequency(frequency, message="frequency must be a positive number of steps"):
    if int(frequency) != frequency or frequency < 1:
        raise ValueError(message)
    return int(frequency)


def require_layout(t, name, masses=None):
    """(R, N) of `t`, a contiguous device tensor [R, N, 3]; `masses`: N entries with its dtype and device."""
    L.require_device_tensor(t, name)
    if masses is not None:
        L.require_device_tensor(masses, "masses")
    if t.dim() != 3 or t.shape[2] != 3 or not t.is_contiguous():
        raise RuntimeError(f"{name} must be a contiguous (nreplicas, natoms, 3) tensor")
    if masses is not None and (masses.numel() != t.shape[1] or masses.dtype != t.dtype or masses.device != t.device
                               or not masses.is_contiguous()):
        raise RuntimeError(f"masses must be a contiguous tensor of natoms entries with the dtype and device of {name}")
    return t.shape[0], t.shape[1]


def box_edges(box):
    """The edges [R, 3] of orthorhombic boxes [R, 3, 3], host float64."""
    return torch.diagonal(box.detach(), dim1=-2, dim2=-1).to("cpu", torch.float64).numpy().reshape(-1, 3)


def positive_edges(edges):
    if not (np.asarray(edges) > 0).all():
        raise ValueError("the barostat needs a periodic box: every box edge must be positive")
    return edges


def scaled_box(box0, edges, factor):
    """(box, new_edges, V_new) for `edges` times `factor` [R]: the box the engine will see holds the scaled edges rounded to
    the box tensor's precision; V' and the factors the molecules' centres are scaled by (new_edges / edges) are taken from
    those, so box and positions stay consistent in fp32."""
    new = box0.clone()
    torch.diagonal(new, dim1=-2, dim2=-1).copy_(torch.as_tensor(factor[:, None] * edges).to(new))
    new_edges = box_edges(new)
    return new, new_edges, new_edges[:, 0] * new_edges[:, 1] * new_edges[:, 2]


def forget_continuation(forces, pos):
    """Positions (or velocities) were written behind torch's back and the box is another one: the next tmdhip_md_run must
    not be told that it continues the previous one."""
    forces._engine(pos)._md_key = None


class Control:
    """Something that acts every `frequency` steps, counted over the integrator's life.  `Integrator.step` cuts a call at
    the union of the controls' multiples and, after a segment that ends on some of them, calls those in `rank` order."""

    rank = None  # thermostat 0, barostat 1, exchange 2, metadynamics deposition 3
    ladder_ok = True  # (False: holds one temperature, so a thermostat with different targets per replica is refused)
    frequency = rng = _record = _partials = None

    def __init__(self, frequency, seed=None, message="frequency must be a positive number of steps"):
        self.frequency = whole_frequency(frequency, message)
        self.seed = draw_seed(seed)

    def attach(self, integrator):
        """What is refused (ValueError) when the integrator is made; called in rank order."""

    def after_segment(self, integrator, out):
        """Act on the state a segment left; `out` = (Ekin, pot, T) as `step` would return it.  Returns `out`, with what the
        action changed.  After rescaling velocities, set `integrator.kinetic_source` to self (`kinetic()` is then read back
        once, after the call's last segment and not before), or to None when `out[0]` already holds the kinetic energies."""
        return out

    def kinetic(self):
        """Device tensor [R]: the kinetic energies the last action left, for a control that names itself the kinetic source."""
        raise NotImplementedError

    def _streams(self, R, who):
        """One Philox stream per replica, so a replica's chain does not depend on how many run beside it."""
        if self.rng is None:
            self.rng = [philox_stream(self.seed, r) for r in range(R)]
        if len(self.rng) != R:
            raise RuntimeError(f"the {who} holds {len(self.rng)} random streams for {R} replicas")

    def _workspace(self, sizes, R, dev, *extra):
        """`_record` [R, ...] (zeroed) and `_partials`, sized by the library's `sizes` function, for R replicas on `dev`."""
        if self._record is None or self._record.shape[0] != R or self._record.device != dev:
            nrec, npart = C.c_int64(), C.c_int64()
            L.check(getattr(L.load(), sizes)(R, *extra, C.byref(nrec), C.byref(npart)), sizes)
            self._record = torch.zeros(R, nrec.value // R, dtype=torch.float64, device=dev)
            self._partials = torch.empty(npart.value, dtype=torch.float64, device=dev)
