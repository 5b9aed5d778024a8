"""Numpy model of the stochastic cell-rescaling barostat, float64 throughout, written from the formulas of Bernetti &
Bussi (J. Chem. Phys. 153, 114107, 2020): the step of eps = ln V, the rigid move of the molecules with their mass-weighted centres, and
the Euler chain of an ideal gas under Langevin dynamics.  It imports nothing from torchmd_amd.  The move of the molecules is
written another way than the kernel (vectorised sums per molecule) and is an independent reference for it.  The three lines of
`delta_eps` are necessarily those of `torchmd_amd.crescale.delta_epsilon`, operation for operation, because the integrator test
compares runs for equal bits; what holds mu to something outside both is the compiled header (within 4 eps64), the hand
numbers of the units test and the volume distribution of the ideal gas."""

import numpy as np

AVOGADRO = 6.02214076e23
BAR_TO_KCAL_MOL_A3 = AVOGADRO * 1e-25 / 4184.0  # 1 bar = 1e-25 J/A^3
BOLTZMAN = 0.001987191
TIMEFACTOR = 48.88821  # fs per time unit of the integrator
PICOSEC2TIMEU = 1000.0 / TIMEFACTOR


def delta_eps(p0, p_int, volume, kT, beta, dt_over_tau, xi, stochastic=True):
    """d eps = -(beta dt_p / tau_p) (P0 - P_int) + sqrt(2 kT beta dt_p / (V tau_p)) xi."""
    drift = -(beta * dt_over_tau) * (p0 - p_int)
    if not stochastic:
        return drift
    return drift + np.sqrt(((2.0 * kT) * (beta * dt_over_tau)) / volume) * xi


def mu_of(de):
    return np.exp(de / 3.0)


def mu(pressure_bar, p_int, volume, temperature, compressibility, tau_ps, frequency, dt, xi, stochastic=True):
    """The box-edge factor from the public units: bar, K, 1/bar, ps; `dt` in the integrator's time units; `p_int` in
    kcal/mol/A^3 (entry 7 of the pressure terms)."""
    return mu_of(delta_eps(np.asarray(pressure_bar, dtype=np.float64) * BAR_TO_KCAL_MOL_A3, p_int, volume,
                           BOLTZMAN * np.asarray(temperature, dtype=np.float64),
                           np.asarray(compressibility, dtype=np.float64) / BAR_TO_KCAL_MOL_A3,
                           frequency * dt / (tau_ps * PICOSEC2TIMEU), xi, stochastic))


def new_edges(edges, mu, dtype):
    """The edges of the rescaled box, rounded to the box tensor's precision, as float64; the per-axis factors are new / old."""
    return (np.asarray(mu, dtype=np.float64)[..., None] * np.asarray(edges, dtype=np.float64)).astype(dtype).astype(np.float64)


def rescale_molecules(pos, vel, mass, scale, off, mem):
    """One replica.  pos, vel [N,3] and mass [N] (the values the device holds, as float64), scale [3].  Returns the float64
    positions and velocities (not rounded).  A member of mass 0 moves with its molecule, keeps its velocity and enters no sum."""
    pos, vel, mass = (np.asarray(a, dtype=np.float64) for a in (pos, vel, mass))
    scale = np.asarray(scale, dtype=np.float64)
    new_pos, new_vel = pos.copy(), vel.copy()
    massive = mass > 0
    for g in range(len(off) - 1):
        a = np.asarray(mem[off[g]:off[g + 1]])
        w = a[massive[a]]
        M = mass[w].sum()
        if not M > 0:
            continue
        centre = (mass[w, None] * pos[w]).sum(axis=0) / M
        vcm = (mass[w, None] * vel[w]).sum(axis=0) / M
        new_pos[a] = pos[a] + (scale - 1.0) * centre
        new_vel[w] = vel[w] + (1.0 / scale - 1.0) * vcm
    return new_pos, new_vel


def kinetic(mass, vel):
    """sum m v^2 / 2 over the massive atoms, and sum |m v^2| (the scale of its rounding error)."""
    mass, vel = np.asarray(mass, dtype=np.float64), np.asarray(vel, dtype=np.float64)
    w = mass > 0
    mv2 = mass[w] * (vel[w] ** 2).sum(axis=1)
    return 0.5 * mv2.sum(), np.abs(mv2).sum()


def ideal_gas_chain(napplications, natoms=64, mean_volume=27000.0, dt_over_tau=0.1, gamma_dt=1.0, kT=BOLTZMAN * 300.0, seed=0):
    """The Euler chain of the barostat for an ideal gas of `natoms` atoms (molecules of one) under Langevin dynamics: between two
    applications the velocities relax as an Ornstein-Uhlenbeck process over gamma dt_p = `gamma_dt` (exact propagator), P_int =
    sum m v^2 / (3 V); P0 is chosen so that (N + 1) kT / P0 = `mean_volume`, beta = 1 / P0.  The stationary distribution of the
    continuous process is P(V) ~ V^N exp(-P0 V / kT).  Returns the volumes after every application."""
    rng = np.random.default_rng(seed)
    p0 = (natoms + 1) * kT / mean_volume
    beta = 1.0 / p0
    c = np.exp(-gamma_dt)
    s = np.sqrt(1.0 - c * c)
    # unit masses: v in units of sqrt(kT / m), m v^2 = kT u^2
    u = rng.standard_normal((natoms, 3))
    V = mean_volume
    out = np.empty(napplications)
    for k in range(napplications):
        u = c * u + s * rng.standard_normal((natoms, 3))
        p_int = kT * (u * u).sum() / (3.0 * V)
        m = mu_of(delta_eps(p0, p_int, V, kT, beta, dt_over_tau, rng.standard_normal()))
        V = V * m**3
        u = u / m
        out[k] = V
    return out


def block_stats(x, nblocks=10):
    """Mean of x and the standard error of the mean from `nblocks` block means; sigma / mean and its block standard error."""
    x = np.asarray(x, dtype=np.float64)
    blocks = x[: len(x) // nblocks * nblocks].reshape(nblocks, -1)
    means = blocks.mean(axis=1)
    rel = blocks.std(axis=1) / means
    return x.mean(), means.std(ddof=1) / np.sqrt(nblocks), x.std() / x.mean(), rel.std(ddof=1) / np.sqrt(nblocks)
