"""A numpy model of one application of the velocity-rescaling thermostat (torchmd_amd/csrc/thermostat.hip), in double:
the kernel's per-atom order of operations, the sums by math.fsum (exact, so the only expected difference to the device is
the order of its additions), optionally the stored velocities rounded to float32."""

import math

import numpy as np

BOLTZMAN = 0.001987191
TIMEFACTOR = 48.88821
PICOSEC2TIMEU = 1000.0 / TIMEFACTOR


def alpha(K, kbar, nf, c, r1, s):
    """csvr_alpha of thermostat_math.h, operation for operation."""
    if not K > 0.0:
        return 1.0
    nk = nf * K
    a2 = c + ((1.0 - c) * kbar * (r1 * r1 + s)) / nk + 2.0 * r1 * math.sqrt((c * (1.0 - c) * kbar) / nk)
    return math.sqrt(a2 if a2 > 0.0 else 0.0)


def kinetic(sm, p, mv2, remove_com):
    """csvr_kinetic of thermostat_math.h: (K, vcm[3])."""
    vcm = [0.0, 0.0, 0.0]
    K = 0.5 * mv2
    if remove_com and sm > 0.0:
        vcm = [p[0] / sm, p[1] / sm, p[2] / sm]
        K = K - 0.5 * sm * (vcm[0] * vcm[0] + vcm[1] * vcm[1] + vcm[2] * vcm[2])
    return (K if K > 0.0 else 0.0), vcm


def apply(vel, mass, kbar, nf, c, r1, s, remove_com=True, fp32=False):
    """One application to one replica: vel [N, 3] (float64 array holding the stored values; changed in place), mass [N].
    Returns the record (K_before, alpha, K_after, |V_cm|)."""
    on = mass > 0
    m, v = mass[on].astype(np.float64), vel[on].astype(np.float64)
    sm = math.fsum(m)
    p = [math.fsum(m * v[:, k]) for k in range(3)]
    mv2 = math.fsum(m * (v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1] + v[:, 2] * v[:, 2]))
    K, vcm = kinetic(sm, p, mv2, remove_com)
    a = alpha(K, kbar, nf, c, r1, s)
    if remove_com or c != 1.0:
        new = a * (v - np.array(vcm))
        vel[on] = new.astype(np.float32).astype(np.float64) if fp32 else new
    return K, a, (a * a) * K, math.sqrt(vcm[0] * vcm[0] + vcm[1] * vcm[1] + vcm[2] * vcm[2])


def generators(seed, nreplicas):
    return [np.random.Generator(np.random.Philox(key=np.array([seed, r], dtype=np.uint64))) for r in range(nreplicas)]


def draw(gen, nf):
    """(R1, S) of one application: a standard normal, then a chi-squared variate with nf - 1 degrees of freedom."""
    r1 = gen.standard_normal()
    return r1, 2.0 * gen.standard_gamma(0.5 * (nf - 1))


# ------------------------------------------------------------------ the free-particle chain of the host and the GPU test
CHAIN_NATOMS = 22  # massive atoms; N_f = 3 * 22 - 3 = 63 with the centre-of-mass motion removed
CHAIN_NF = 63
CHAIN_T = (250.0, 300.0, 350.0, 400.0)
CHAIN_LENGTH = 8000
CHAIN_C = 0.9
CHAIN_SEED = 2007


def chain_start(dtype=np.float64):
    """Masses [N] and start velocities [R, N, 3] of the chain (with a net drift), already rounded to `dtype`."""
    rng = np.random.default_rng(63)
    mass = rng.choice([1.008, 12.011, 15.999], CHAIN_NATOMS)
    vel = rng.standard_normal((len(CHAIN_T), CHAIN_NATOMS, 3)) * np.sqrt(BOLTZMAN * 300.0 / mass)[None, :, None] + 0.01
    return mass.astype(dtype).astype(np.float64), vel.astype(dtype).astype(np.float64)


def model_chain(fp32=False, length=CHAIN_LENGTH):
    """The K_after chain [R, length] of the model with the chain's seed."""
    mass, vel = chain_start(np.float32 if fp32 else np.float64)
    out = np.zeros((len(CHAIN_T), length))
    for r, (T, g) in enumerate(zip(CHAIN_T, generators(CHAIN_SEED, len(CHAIN_T)))):
        kbar = 0.5 * CHAIN_NF * BOLTZMAN * T
        for k in range(length):
            r1, s = draw(g, CHAIN_NF)
            out[r, k] = apply(vel[r], mass, kbar, float(CHAIN_NF), CHAIN_C, r1, s, True, fp32)[2]
    return out


def chain_statistics(K, T, nf=CHAIN_NF, drop=0.2, nblocks=20):
    """(mean, its block standard error, variance, its block standard error, expected mean, expected variance) of a K chain
    with the first `drop` of it left out; the errors from `nblocks` block averages."""
    k = np.asarray(K, dtype=np.float64)[int(drop * len(K)):]
    k = k[: len(k) // nblocks * nblocks]
    mean = k.mean()
    blocks = k.reshape(nblocks, -1)
    bm = blocks.mean(axis=1)
    bv = ((blocks - mean) ** 2).mean(axis=1)
    kT = BOLTZMAN * T
    return mean, bm.std(ddof=1) / math.sqrt(nblocks), bv.mean(), bv.std(ddof=1) / math.sqrt(nblocks), 0.5 * nf * kT, 0.5 * nf * kT * kT
