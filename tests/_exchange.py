"""Numpy models for replica exchange: of one application of tmdhip_velocity_rescale (torchmd_amd/csrc/exchange.hip)
— the kernel's per-atom order of operations, the sum by math.fsum (exact, so the only expected difference to the device is the
order of its additions), the stored velocities rounded to the run's precision — and of the Metropolis decision, written
independently of torchmd_amd/exchange.py, pair by pair."""

import math

import numpy as np

BOLTZMAN = 0.001987191
TIMEFACTOR = 48.88821


def rescale(vel, mass, factor, dtype=np.float64):
    """One application to one replica: vel [N, 3] (float64 array holding the stored values; changed in place), mass [N],
    `dtype` the precision of the stored velocities.  Returns (K_before, factor, K_after)."""
    on = mass > 0
    m, v = mass[on].astype(np.float64), vel[on].astype(np.float64)
    K = 0.5 * math.fsum(m * (v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1] + v[:, 2] * v[:, 2]))
    if factor != 1.0:
        vel[on] = (factor * v).astype(dtype).astype(np.float64)
    return K, factor, (factor * factor) * K


def pairs_of(parity, R):
    return [(a, a + 1) for a in range(parity, R - 1, 2)]


def decide(U, T, rungs, parity, u):
    """The swaps of one attempt: (new rungs, accepted, delta), one entry of `u` per tried pair in rung order."""
    rungs = list(rungs)
    acc, delta = [], []
    for k, (a, b) in enumerate(pairs_of(parity, len(rungs))):
        i, j = rungs.index(a), rungs.index(b)
        d = (1.0 / (BOLTZMAN * T[a]) - 1.0 / (BOLTZMAN * T[b])) * (U[i] - U[j])
        ok = d >= 0.0 or u[k] < math.exp(d)
        if ok:
            rungs[i], rungs[j] = b, a
        acc.append(ok), delta.append(d)
    return np.array(rungs), np.array(acc, dtype=bool), np.array(delta)


class Counting:
    """A stand-in for the generator: counts its draws and returns a constant (or the next of a list)."""

    def __init__(self, value=0.0):
        self.value, self.count = value, 0

    def random(self):
        self.count += 1
        return self.value[self.count - 1] if isinstance(self.value, (list, tuple)) else self.value


def block_statistics(x, nblocks=20):
    """(mean, its block standard error, variance, its block standard error) of a series, from `nblocks` block averages."""
    x = np.asarray(x, dtype=np.float64)
    x = x[: len(x) // nblocks * nblocks]
    mean = x.mean()
    blocks = x.reshape(nblocks, -1)
    bm = blocks.mean(axis=1)
    bv = ((blocks - mean) ** 2).mean(axis=1)
    return mean, bm.std(ddof=1) / math.sqrt(nblocks), bv.mean(), bv.std(ddof=1) / math.sqrt(nblocks)
