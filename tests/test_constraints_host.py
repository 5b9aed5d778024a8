"""Constraints on the host (no GPU): the topology analysis of torchmd_amd/constraints.py on the fixtures, the degrees of
freedom, the refused configurations, and the host reference step of tests/_constraints.py."""

import numpy as np
import pytest
import torch

import _constraints as H
from _golden import GoldenParameters, load


def _fixture(name):
    par = GoldenParameters(load(name))
    return par


def _tip3p(nside):
    from torchmd_amd.builders import tip3p_box, water_forcefield
    from torchmd_amd.parameters import Parameters

    mol, pos, box = tip3p_box(nside, seed=0)
    return Parameters(water_forcefield(mol), mol, ["lj", "electrostatics", "bonds", "angles"], precision=torch.float64), pos


@pytest.mark.parametrize("name,nw", [("water291", 97), ("ala2", 222), ("tip3p4", 64)])
def test_waters_found(name, nw):
    from torchmd_amd.constraints import find_constraints

    par = _tip3p(4)[0] if name == "tip3p4" else _fixture(name)
    cs = find_constraints(par.masses, par.bond_params, par.angle_params, "water")
    assert cs.nwaters == nw and cs.nclusters == 0
    m = par.masses.reshape(-1).numpy()
    assert np.all(m[cs.waters[:, 0]] > 1.5) and np.all(m[cs.waters[:, 1:]] < 1.5)
    assert np.allclose(cs.water_dist[:, 0], 0.9572, atol=1e-6)
    assert np.allclose(cs.water_dist[:, 1], 1.5139 if name != "ala2" else 1.5136, atol=1e-4)
    assert cs.ndof() == 3 * len(m) - 3 * nw


def test_ala2_hbonds_clusters():
    from torchmd_amd.constraints import find_constraints

    par = _fixture("ala2")
    cs = find_constraints(par.masses, par.bond_params, par.angle_params, "hbonds")
    assert cs.nwaters == 222
    m = par.masses.reshape(-1).numpy()
    cl = cs.clusters()
    assert sum(len(c) - 1 for c in cl) == 12  # the peptide's X-H bonds
    assert sorted(len(c) - 1 for c in cl) == [1, 1, 1, 3, 3, 3]  # N-H, N-H, CA-HA and three methyls
    bonds = {tuple(sorted(b)) for b in par.bond_params["idx"].numpy().tolist()}
    for c in cl:
        assert m[c[0]] > 1.5 and np.all(m[c[1:]] < 1.5)
        for h in c[1:]:
            assert tuple(sorted((int(c[0]), int(h)))) in bonds
    assert cs.ndof() == 3 * 688 - 3 * 222 - 12
    batch = torch.zeros(688, dtype=torch.long)
    batch[22:] = 1  # the peptide, then the water
    assert list(cs.ndof(batch)) == [3 * 22 - 12, 3 * 666 - 3 * 222]


def _toy(bonds, masses, req=1.0):
    idx = torch.tensor(bonds, dtype=torch.long)
    tab = {"idx": idx, "map": torch.stack([torch.arange(len(bonds)), torch.zeros(len(bonds), dtype=torch.long)], 1),
           "params": torch.tensor([[100.0, req]])}
    return torch.tensor(masses, dtype=torch.float64), tab


def test_refused():
    from torchmd_amd.constraints import find_constraints

    m, tab = _toy([[0, 1], [1, 2]], [12.0, 1.0, 12.0])  # a hydrogen between two heavy atoms
    with pytest.raises(ValueError, match="two constraints"):
        find_constraints(m, tab, None, "hbonds")
    m, tab = _toy([[0, k] for k in range(1, 6)], [12.0] + [1.0] * 5)  # five hydrogens around one carbon
    with pytest.raises(ValueError, match="more than|at most"):
        find_constraints(m, tab, None, "hbonds")
    with pytest.raises(ValueError, match="constraints must be"):
        find_constraints(m, tab, None, "allbonds")


def test_integrator_refuses_other_force_objects():
    from torchmd_amd.integrator import Integrator
    from torchmd_amd.systems import System

    class Duck:
        par = type("P", (), {"masses": torch.ones(3)})()

        def compute(self, pos, box, forces):
            return [0.0]

    s = System(3, 1, torch.float64, "cpu")
    with pytest.raises(ValueError, match="constraints need"):
        Integrator(s, Duck(), 2.0, "cpu", constraints="water")


def test_water_without_hh_bond_uses_the_angle():
    from torchmd_amd.constraints import find_constraints

    m, tab = _toy([[0, 1], [0, 2]], [16.0, 1.008, 1.008], req=0.9572)
    ang = {"idx": torch.tensor([[1, 0, 2]]), "map": torch.tensor([[0, 0]]), "params": torch.tensor([[55.0, np.deg2rad(104.52)]])}
    cs = find_constraints(m, tab, ang, "water")
    assert cs.nwaters == 1 and abs(cs.water_dist[0, 1] - 2 * 0.9572 * np.sin(np.deg2rad(104.52) / 2)) < 1e-6


@pytest.mark.parametrize("mode", ["water", "hbonds"])
def test_host_step_holds_its_constraints(mode):
    from torchmd_amd.constraints import find_constraints

    par = _fixture("ala2")
    cs = find_constraints(par.masses, par.bond_params, par.angle_params, mode)
    us = H.units(cs)
    m = par.masses.reshape(-1).double().numpy()
    rng = np.random.default_rng(0)
    x0 = np.asarray(load("ala2")["pos"], dtype=np.float64)
    H.shake(x0, x0.copy(), m, us)
    v = H.project(x0, rng.normal(size=x0.shape) * np.sqrt(0.6 / m)[:, None] * 0.05, m, us)
    f = rng.normal(size=x0.shape) * 20
    dt = 2.0 / 48.88821
    x1, vh = H.first_half(x0, v, f, m, dt, us)
    v1 = H.second_half(x1, vh, f, m, dt, us)
    pairs, d = cs.pairs()
    dr, dv = H.residuals(x1, v1, pairs, d)
    assert dr < 1e-13 and dv < 1e-12, (dr, dv)
    # the vectorised start-up projection of the package agrees with the per-unit reference
    xp = x0 + rng.normal(size=x0.shape) * 0.05
    xa, xb = xp.copy(), xp.copy()
    cs.shake_positions(xa, xp.copy())
    H.shake(xb, xp.copy(), m, us)
    assert np.abs(xa - xb).max() < 1e-10
    va = cs.project_velocities(xa, rng.normal(size=x0.shape))
    assert H.residuals(xa, va, pairs, d)[1] < 1e-12


@pytest.mark.parametrize("size", ["small", "large"])
def test_synthetic_system_holds_every_unit_kind(size):
    """tests/_constraint_systems.py: free ions, two kinds of rigid three-atom units, clusters of 1 .. 4 hydrogens, numbered at
    random — what `find_constraints` makes of it."""
    import _constraint_systems as S
    from torchmd_amd.constraints import find_constraints

    s = S.build(size)
    par = s.par()
    m = par.masses.reshape(-1).numpy()
    n = s.natoms
    assert n == (S.CELLLIST_MIN_ATOMS if size == "large" else 260)
    cs = find_constraints(par.masses, par.bond_params, par.angle_params, "hbonds")
    c = s.meta["counts"]
    assert cs.nwaters == c["tip3p"] + c["h2s"] == s.meta["nwaters"]
    heavy = np.round(m[cs.waters[:, 0]], 2)
    assert (heavy == 16.0).sum() == c["tip3p"] and (heavy == 32.06).sum() == c["h2s"]
    for w, (doh, dhh) in zip(cs.waters, cs.water_dist):
        want = (0.9572, 2 * 0.9572 * np.sin(np.deg2rad(104.52) / 2)) if m[w[0]] < 20 else (1.34, 2 * 1.34 * np.sin(np.deg2rad(92.0) / 2))
        assert abs(doh - want[0]) < 1e-12 and abs(dhh - want[1]) < 1e-12
    cl = cs.clusters()
    sizes = sorted(len(a) - 1 for a in cl)
    assert sizes == s.meta["cluster_sizes"] and set(sizes) == {1, 2, 3, 4}
    for k in (1, 2, 3, 4):  # at least two of every size, around heavy atoms of different masses
        mk = [m[a[0]] for a in cl if len(a) - 1 == k]
        assert len(mk) >= 2 and len(set(np.round(mk, 2))) >= 2, (k, mk)
    assert cs.nconstraints == s.meta["nconstraints"] and cs.ndof() == 3 * n - s.meta["nconstraints"]
    # every unit's first entry is the heavy atom, the others are its hydrogens
    for u in list(cs.waters) + cl:
        assert m[u[0]] > 1.5 and np.all(m[u[1:]] < 1.5), u
    # free atoms: the ions, and the heavy atoms without a hydrogen would be too (there are none)
    in_unit = np.zeros(n, dtype=bool)
    in_unit[np.concatenate([cs.waters.reshape(-1), cs.atoms])] = True
    assert (~in_unit).sum() == s.meta["nions"] and np.all(s.meta["kind"][~in_unit] == "ion")
    # scrambled numbering: units interleave (hydrogens do not follow their heavy atom) and span 64-atom blocks
    units = [np.asarray(u) for u in list(cs.waters) + cl]
    assert sum(1 for u in units if np.any(np.diff(u) != 1)) > 0.9 * len(units)
    assert sum(1 for u in units if len(set(u // 64)) > 1) > 0.5 * len(units)
    # heavy atoms bonded to each other
    b = par.bond_params["idx"].numpy()
    assert (np.all(m[b] > 1.5, axis=1)).sum() >= c["methanol"] + c["methylamine"] + c["methanethiol"] + 2 * c["ethanol"]
    # in "water" mode only the three-atom units remain
    cw = find_constraints(par.masses, par.bond_params, par.angle_params, "water")
    assert cw.nwaters == cs.nwaters and cw.nclusters == 0
