"""A numpy model of one FIRE iteration as include/tmdhip.h states it for `tmdhip_fire_step` (Bitzek et al., PRL 97, 170201,
2006): float64 throughout, the same order of operations per atom as the kernel.  The three dot products are summed exactly
(math.fsum), so the model's figures do not depend on a summation order (numpy's changes with the host's SIMD width); the kernel
sums them over lanes, waves and blocks, and that is all a comparison has to allow for.

`store` is the dtype positions and velocities are rounded to when they are stored (np.float32 models the fp32 kernels, which
compute in double and round once on the store)."""

import math
from dataclasses import dataclass

import numpy as np


@dataclass
class Params:
    f_tol: float
    dt_start: float
    dt_max: float
    max_step: float = 0.1
    n_min: int = 5
    f_inc: float = 1.1
    f_dec: float = 0.5
    alpha_start: float = 0.1
    f_alpha: float = 0.99


@dataclass
class State:
    dt: float
    alpha: float
    npos: int = 0
    done: int = 0
    iterations: int = 0
    fmax: float = 0.0
    nuphill: int = 0

    def as_row(self):
        """The layout of a state slot of `tmdhip_fire_step`."""
        return np.array([self.dt, self.alpha, self.npos, self.done, self.iterations, self.fmax, self.nuphill, 0.0])


def init(prm):
    return State(dt=prm.dt_start, alpha=prm.alpha_start)


def _total(a):
    return math.fsum(a.tolist())


def step(pos, vel, frc, mass, st, prm, store=np.float64):
    """One iteration of one replica, in place: `pos`, `vel` [N,3] arrays of dtype `store`, `frc` [N,3], `mass` [N]; rows with
    mass == 0 are neither read into a sum nor written.  Returns the branch taken: "done", "converged", "downhill", "uphill"."""
    if st.done:
        return "done"
    real = np.asarray(mass, dtype=np.float64) > 0
    f = np.asarray(frc, dtype=np.float64)[real]
    v = np.asarray(vel, dtype=np.float64)[real]
    m = np.asarray(mass, dtype=np.float64)[real][:, None]
    f2 = f[:, 0] * f[:, 0] + f[:, 1] * f[:, 1] + f[:, 2] * f[:, 2]
    st.fmax = float(np.sqrt(f2.max())) if len(f2) else 0.0
    if st.fmax < prm.f_tol:
        st.done = 1
        return "converged"
    p = _total(f[:, 0] * v[:, 0] + f[:, 1] * v[:, 1] + f[:, 2] * v[:, 2])
    vv = _total(v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1] + v[:, 2] * v[:, 2])
    ff = _total(f2)
    if p > 0.0:
        keep, mix = 1.0 - st.alpha, st.alpha * np.sqrt(vv / ff)
        st.npos += 1
        if st.npos > prm.n_min:
            st.dt = min(st.dt * prm.f_inc, prm.dt_max)
            st.alpha = st.alpha * prm.f_alpha
        branch = "downhill"
    else:
        keep, mix = 0.0, 0.0
        st.dt = st.dt * prm.f_dec
        st.alpha = prm.alpha_start
        st.npos = 0
        st.nuphill += 1
        branch = "uphill"
    st.iterations += 1
    v = keep * v + mix * f
    v = v + (st.dt * f) / m
    vn = np.sqrt(v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1] + v[:, 2] * v[:, 2])
    capped = vn * st.dt > prm.max_step
    c = np.ones_like(vn)
    c[capped] = (prm.max_step / st.dt) / vn[capped]
    v[capped] = v[capped] * c[capped][:, None]
    pos[real] = (np.asarray(pos, dtype=np.float64)[real] + st.dt * v).astype(store)
    vel[real] = v.astype(store)
    return branch
