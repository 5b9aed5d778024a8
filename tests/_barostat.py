"""Host model of the Monte Carlo barostat's volume chain (numpy only; no torch, no package import): the rule of
`torchmd_amd/barostat.py` restated for a system whose potential energy is identically zero, where positions do not enter.
The volume density of that chain is exactly Gamma(N + 1, k_B T / P): <V> = (N + 1) k_B T / P, sigma_V / <V> = 1 / sqrt(N + 1).
It is what tests/test_gpu_barostat.py compares the GPU run with, volume for volume."""

import numpy as np

BOLTZMAN = 0.001987191  # kcal/mol/K
BAR = 6.02214076e23 * 1e-25 / 4184.0  # kcal/mol/A^3 per bar


class ListStream:
    """A random stream with prescribed values (`.random()` pops them in order): forces a barostat's decisions."""

    def __init__(self, values):
        self.values = list(values)

    def random(self):
        return float(self.values.pop(0))


def philox_stream(seed, replica=0):
    """The generator the barostat gives replica `replica` for `seed`."""
    return np.random.Generator(np.random.Philox(key=np.array([seed, replica], dtype=np.uint64)))


def volume_chain(edges, ngroups, pressure_bar, temperature, nattempts, rng):
    """`nattempts` moves with U = 0 from a box with the three `edges`: every attempt draws two numbers (volume change, then
    acceptance), scales the three edges by ((V + dV) / V)^(1/3), takes V' as the product of the new edges, accepts when
    w = P (V' - V) - N k_B T ln(V'/V) <= 0 or u < exp(-w / k_B T), and adapts dVmax every 10 attempts.  Returns the
    volume after every attempt and the accept flags."""
    e = np.array(edges, dtype=np.float64)
    kT = BOLTZMAN * temperature
    P = pressure_bar * BAR
    V = e[0] * e[1] * e[2]
    dmax = 0.01 * V
    att = acc = 0
    vols, flags = np.empty(nattempts), np.zeros(nattempts, dtype=bool)
    for i in range(nattempts):
        u1, u2 = rng.random(), rng.random()
        dV = dmax * 2.0 * (u1 - 0.5)
        s = ((V + dV) / V) ** (1.0 / 3.0)
        en = s * e
        Vn = en[0] * en[1] * en[2]
        w = (0.0 - 0.0) + P * (Vn - V) - ngroups * kT * np.log(Vn / V)
        if w <= 0 or u2 < np.exp(-w / kT):
            e, V = en, Vn
            acc += 1
            flags[i] = True
        att += 1
        if att >= 10:
            if acc < 0.25 * att:
                dmax /= 1.1
            elif acc > 0.75 * att:
                dmax = min(dmax * 1.1, 0.3 * V)
            att = acc = 0
        vols[i] = V
    return vols, flags


def block_stats(vols, discard=0.2, nblocks=20):
    """Mean, standard error from `nblocks` block averages, and sigma / mean of the series after its first fifth."""
    v = np.asarray(vols)[int(len(vols) * discard):]
    b = v[: len(v) // nblocks * nblocks].reshape(nblocks, -1).mean(axis=1)
    return v.mean(), b.std(ddof=1) / np.sqrt(nblocks), v.std() / v.mean()
