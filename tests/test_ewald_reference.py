"""The host Ewald references (tests/_ewald.py) against known answers: the NaCl Madelung constant, beta independence of a
converged Ewald sum, forces against a finite-difference gradient, smooth PME converging to Ewald, exclusions."""

import math

import numpy as np
import pytest

import _ewald as E


def test_nacl_madelung_constant():
    r0 = 2.8
    pos, q, box = E.nacl_lattice(r0, cells=2)
    e, f = E.ewald(pos, q, box, 1.6 / r0, nimg=2, kmax=14)
    per_pair = e / (len(q) / 2)
    assert abs(per_pair / (-E.KE / r0) - E.NACL_MADELUNG) < 1e-10 * E.NACL_MADELUNG
    assert np.abs(f).max() < 1e-10  # every ion sits at a centre of symmetry


@pytest.mark.parametrize("net", [0, 2])
def test_ewald_does_not_depend_on_beta(net):
    box = np.array([18.0, 19.0, 20.0])
    pos, q = E.random_ions(40, box, seed=1, net=net)
    excl = [(0, 1), (2, 3), (5, 9)]
    es = [E.ewald(pos, q, box, b, excl=excl, nimg=2, kmax=16) for b in (0.25, 0.3, 0.35)]
    for e, f in es[1:]:
        assert abs(e - es[0][0]) <= 1e-10 * abs(es[0][0])
        assert np.abs(f - es[0][1]).max() <= 1e-8 * np.abs(es[0][1]).max()


def test_ewald_forces_are_the_gradient():
    box = np.array([14.0, 15.0, 16.0])
    pos, q = E.random_ions(13, box, seed=3, net=1)
    excl = [(0, 1)]
    _, f = E.ewald(pos, q, box, 0.35, excl=excl, nimg=2, kmax=12)
    h = 1e-5
    for i in (0, 1, 7):
        for d in range(3):
            p1, p2 = pos.copy(), pos.copy()
            p1[i, d] += h
            p2[i, d] -= h
            g = (E.ewald(p1, q, box, 0.35, excl=excl, nimg=2, kmax=12)[0] - E.ewald(p2, q, box, 0.35, excl=excl, nimg=2, kmax=12)[0]) / (2 * h)
            assert abs(-g - f[i, d]) < 1e-6 * max(1.0, abs(f[i, d]))


def test_host_pme_forces_are_the_gradient_of_its_energy():
    box = np.array([14.0, 15.0, 16.0])
    pos, q = E.random_ions(12, box, seed=4)
    args = (box, 0.4, 6.9, (16, 15, 18), 5)
    _, f = E.pme(pos, q, *args, excl=[(2, 3)])
    h = 1e-5
    for i, d in ((0, 0), (2, 1), (3, 2)):
        p1, p2 = pos.copy(), pos.copy()
        p1[i, d] += h
        p2[i, d] -= h
        g = (E.pme(p1, q, *args, excl=[(2, 3)])[0] - E.pme(p2, q, *args, excl=[(2, 3)])[0]) / (2 * h)
        assert abs(-g - f[i, d]) < 1e-6 * max(1.0, abs(f[i, d]))


def test_host_pme_converges_to_ewald():
    """Energy and forces within 1e-8 relative.  The floor is the grid: real space is converged (erfc(beta rc) ~ 1e-15)
    and so is the Ewald reference (kmax 16 -> 22 moves it by 1.6e-10); the order-6 error falls about as K^-6 —
    6.8e-8 at K = 96, 1.9e-8 at 128, 6.3e-9 at 160."""
    box = np.array([38.0, 39.0, 40.0])
    pos, q = E.random_ions(40, box, seed=1)
    eE, fE = E.ewald(pos, q, box, 0.3, nimg=2, kmax=22)
    errs = []
    for K, p in ((32, 4), (48, 5), (64, 6), (160, 6)):
        e, f = E.pme(pos, q, box, 0.3, 18.9, (K, K, K), p)
        errs.append(max(abs(e - eE) / abs(eE), np.abs(f - fE).max() / np.abs(fE).max()))
    assert all(b < a for a, b in zip(errs, errs[1:])), errs
    assert errs[-1] <= 1e-8, errs


def test_excluded_pair_removes_its_minimum_image_coulomb_term():
    box = np.array([18.0, 19.0, 20.0])
    pos, q = E.random_ions(20, box, seed=5)
    i, j = 3, 11
    e0, f0 = E.ewald(pos, q, box, 0.3, nimg=2, kmax=16)
    e1, f1 = E.ewald(pos, q, box, 0.3, excl=[(i, j)], nimg=2, kmax=16)
    d = pos[i] - pos[j]
    d = d - box * np.round(d / box)
    r = np.linalg.norm(d)
    assert abs((e0 - e1) - E.KE * q[i] * q[j] / r) < 1e-9 * abs(e0)
    fc = E.KE * q[i] * q[j] / r**3 * d  # Coulomb force on i from j
    assert np.abs((f0 - f1)[i] - fc).max() < 1e-8
    assert np.abs((f0 - f1)[j] + fc).max() < 1e-8
    others = [k for k in range(len(q)) if k not in (i, j)]
    assert np.abs((f0 - f1)[others]).max() < 1e-8


def test_grid_rule_matches_openmm_sizes():
    from torchmd_amd.forces import _fft_size, pme_grid_size

    assert [_fft_size(n) for n in (1, 11, 13, 17, 88, 97)] == [1, 12, 14, 18, 90, 98]
    beta = E.ewald_beta(9.0, 5e-4)
    assert abs(beta - math.sqrt(-math.log(1e-3)) / 9.0) < 1e-15
    assert pme_grid_size(beta, 98.6, 5e-4) == _fft_size(math.ceil(2 * beta * 98.6 / (3 * 5e-4 ** 0.2)))


@pytest.mark.parametrize("case", ["ions", "ions_unwrapped", "water_like", "tiny_box"])
def test_kdtree_real_space_equals_dense(case):
    """The k-d tree pair search of real_space (for systems of 10^5 atoms) against the O(N^2) path: the same pairs, the same
    exclusions, energy and forces equal to rounding — on wrapped positions, on positions shifted by up to +-3 boxes, and
    with a cutoff close to half the box."""
    rng = np.random.default_rng(11)
    box = np.array([18.0, 19.0, 20.0])
    cutoff, excl = 8.0, [(0, 1), (2, 3), (5, 9), (9, 5)]
    if case.startswith("ions"):
        pos, q = E.random_ions(120, box, seed=2, net=2)
        if case == "ions_unwrapped":
            pos = pos + rng.integers(-3, 4, size=pos.shape) * box
    elif case == "water_like":  # bonded triples straddling the faces, each moved as a whole by whole boxes
        o = rng.uniform(0, 1, (60, 3)) * box
        pos = np.concatenate([o, o + [0.96, 0, 0], o + [-0.24, 0.93, 0]], axis=1).reshape(-1, 3)
        pos = (pos.reshape(-1, 3, 3) + rng.integers(-3, 4, size=(60, 1, 3)) * box).reshape(-1, 3)
        pos[0] = [0.0, box[1], -1e-7 * box[2]]
        q = np.tile([-0.834, 0.417, 0.417], 60)
        excl = [(3 * m + a, 3 * m + b) for m in range(60) for a, b in ((0, 1), (0, 2), (1, 2))]
    else:
        box = np.array([12.0, 12.5, 13.0])
        pos, q = E.random_ions(30, box, seed=3, min_dist=1.5)
        cutoff = 5.99
    e0, f0 = E.real_space(pos, q, box, 0.33, cutoff, excl)
    e1, f1 = E.real_space(pos, q, box, 0.33, cutoff, excl, pairs="kdtree")
    assert abs(e1 - e0) <= 1e-12 * max(1.0, abs(e0)), (e0, e1)
    assert np.abs(f1 - f0).max() <= 1e-11 * max(1.0, np.abs(f0).max())
    # the total of pme() is unchanged by the pair search
    ep0, fp0 = E.pme(pos, q, box, 0.33, cutoff, (16, 18, 20), 4, excl)
    ep1, fp1 = E.pme(pos, q, box, 0.33, cutoff, (16, 18, 20), 4, excl, pairs="kdtree")
    assert abs(ep1 - ep0) <= 1e-12 * max(1.0, abs(ep0))
    assert np.abs(fp1 - fp0).max() <= 1e-11 * max(1.0, np.abs(fp0).max())
