"""CPU tests (no GPU) of virtual interaction sites: the site model of torchmd_amd/vsites.py, its refusals, the constraint
search with sites in the topology, the degrees of freedom, the builder and the driver's configuration key."""

import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TERMS = ["lj", "electrostatics", "bonds", "angles"]


def _tip4p(nside=2, seed=1, dtype=torch.float64):
    from torchmd_amd.builders import tip4p_box, tip4pew_forcefield
    from torchmd_amd.parameters import Parameters

    mol, pos, box, vs = tip4p_box(nside, seed=seed)
    par = Parameters(tip4pew_forcefield(mol), mol, TERMS, precision=dtype)
    return mol, pos, box, vs, par


def test_abi_symbols_and_constant():
    from torchmd_amd import _lib

    header = open(os.path.join(ROOT, "include", "tmdhip.h")).read()
    declared = set(re.findall(r"\b(tmdhip_[a-z0-9_]+)\s*\(", header))
    for name in ("tmdhip_vsite_construct", "tmdhip_vsite_spread", "tmdhip_set_vsites"):
        assert name in declared and name in _lib.SIGNATURES
    assert int(re.search(r"#define\s+TMDHIP_ABI_VERSION\s+(\d+)", header).group(1)) == _lib.ABI_VERSION
    assert "#define TMDHIP_NENERGY 8" in header  # a site needs no energy slot
    lib = _lib.load()
    # argument validation happens before any HIP call
    assert lib.tmdhip_vsite_construct(7, 1, 4, None, 1, None, None, None, None) < 0 and "dtype" in _lib.last_error()
    assert lib.tmdhip_vsite_spread(_lib.F32, 1, 4, None, 1, None, None, None, None) < 0 and "null" in _lib.last_error()
    assert lib.tmdhip_vsite_construct(_lib.F64, 0, 4, None, 1, None, None, None, None) < 0


def test_tip4p_weights():
    from torchmd_amd.vsites import VirtualSites

    vs = VirtualSites.tip4p(5, 0.125, 0.9572, 104.52)
    assert vs.nsites == 5 and vs.sites.tolist() == [3, 7, 11, 15, 19] and vs.parents[1].tolist() == [4, 5, 6]
    assert np.abs(vs.weights - np.array([0.786646558, 0.106676721, 0.106676721])).max() < 1e-9
    assert abs(vs.weights[0, 1] - 0.1066767) < 1e-7


def test_construct_puts_m_on_the_bisector():
    mol, pos, box, vs, par = _tip4p(3)
    x = pos.copy()
    x[vs.sites] = 99.0  # misplaced
    vs.construct(x)
    o, h1, h2, m = (x[k::4] for k in range(4))
    assert np.abs(np.linalg.norm(m - o, axis=1) - 0.125).max() < 1e-12
    bis = (h1 - o) + (h2 - o)
    bis /= np.linalg.norm(bis, axis=1, keepdims=True)
    assert np.abs((m - o) / 0.125 - bis).max() < 1e-12
    assert np.array_equal(x[~vs.site_mask(len(x))], pos[~vs.site_mask(len(x))])
    # float32 positions: summed in float64, rounded once
    x32 = pos.astype(np.float32)
    want = (vs.weights[:, :, None] * x32[vs.parents].astype(np.float64)).sum(axis=1)
    vs.construct(x32)
    assert x32.dtype == np.float32 and np.abs(x32[vs.sites] - want).max() <= np.spacing(np.float32(np.abs(want).max()))


@pytest.mark.parametrize("nparents", [2, 3])
def test_spread_preserves_force_and_torque(nparents):
    from torchmd_amd.vsites import VirtualSites

    rng = np.random.default_rng(nparents)
    n, ns = 40, 8
    perm = rng.permutation(n)
    sites, parents = perm[:ns], perm[ns:ns + ns * nparents].reshape(ns, nparents)
    w = rng.uniform(-0.5, 1.0, size=(ns, nparents))
    w[:, -1] = 1.0 - w[:, :-1].sum(axis=1)
    vs = VirtualSites(sites, parents, w)
    r = rng.normal(size=(n, 3)) * 10.0
    vs.construct(r)
    f = rng.normal(size=(n, 3)) * 50.0
    f0 = f.copy()
    vs.spread(f)
    assert np.all(f[sites] == 0.0)
    assert np.abs(f.sum(axis=0) - f0.sum(axis=0)).max() <= 1e-13 * np.abs(f0).sum()
    t0, t1 = np.cross(r, f0).sum(axis=0), np.cross(r, f).sum(axis=0)
    assert np.abs(t1 - t0).max() <= 1e-13 * (np.linalg.norm(r, axis=1) * np.linalg.norm(f0, axis=1)).sum()
    # batched [R, N, 3] input
    fb = np.stack([f0, 2 * f0])
    vs.spread(fb)
    assert np.array_equal(fb[0], f) and np.all(fb[1][sites] == 0.0)


def test_refusals_of_the_site_model():
    from torchmd_amd.vsites import VirtualSites

    ok = dict(sites=[3], parents=[[0, 1, 2]], weights=[[0.5, 0.25, 0.25]])
    VirtualSites(**ok)
    VirtualSites([3], [[0, 1]], [[0.4, 0.6]])
    with pytest.raises(ValueError, match="sum to 1"):
        VirtualSites([3], [[0, 1, 2]], [[0.5, 0.25, 0.25 + 1e-9]])
    with pytest.raises(ValueError, match="parent"):
        VirtualSites([3], [[3, 1, 2]], [[0.5, 0.25, 0.25]])  # its own parent
    with pytest.raises(ValueError, match="parent"):
        VirtualSites([3, 7], [[0, 1, 2], [4, 5, 3]], [[0.5, 0.25, 0.25]] * 2)  # a parent of another site
    with pytest.raises(ValueError, match="share a parent"):
        VirtualSites([3, 7], [[0, 1, 2], [4, 5, 2]], [[0.5, 0.25, 0.25]] * 2)
    m = np.array([16.0, 1.0, 1.0, 0.0])
    VirtualSites(masses=m, **ok)
    with pytest.raises(ValueError, match="mass 0"):
        VirtualSites(masses=np.array([16.0, 1.0, 1.0, 0.5]), **ok)
    with pytest.raises(ValueError, match="parent must have a mass"):
        VirtualSites(masses=np.array([16.0, 0.0, 1.0, 0.0]), **ok)
    with pytest.raises(ValueError):
        VirtualSites([3], [[0, 1, 2, 4]], [[0.25] * 4])


def test_refusals_of_forces_and_integrator():
    from torchmd_amd.builders import tip3p_box, water_forcefield
    from torchmd_amd.domain import DomainSet
    from torchmd_amd.forces import Forces
    from torchmd_amd.integrator import Integrator
    from torchmd_amd.parameters import Parameters
    from torchmd_amd.systems import System
    from torchmd_amd.vsites import VirtualSites

    mol, pos, box, vs, par = _tip4p(2)
    f = Forces(par, terms=TERMS, cutoff=9.0, rfa=True, virtual_sites=vs)
    p = torch.zeros(1, mol.numAtoms, 3, dtype=torch.float64)
    b = torch.zeros(1, 3, 3, dtype=torch.float64)
    with pytest.raises(ValueError, match="explicit_forces"):
        f.compute(p.requires_grad_(True), b, torch.zeros_like(p), explicit_forces=False)
    with pytest.raises(ValueError, match="vmap"):
        torch.vmap(lambda q: f.compute(q, b, None, toNumpy=False))(torch.zeros(2, 1, mol.numAtoms, 3, dtype=torch.float64))
    with pytest.raises(ValueError, match="update_atoms"):
        f.update_atoms(par)
    with pytest.raises(ValueError, match="virtual sites"):
        DomainSet(box, 2, torch.device("cpu"), torch.float32, ["lj"], 9.0, dry=True, virtual_sites=vs)
    with pytest.raises(ValueError, match="VirtualSites"):
        Forces(par, terms=TERMS, virtual_sites=[3, 7])
    # a site with a mass / a massless parent, seen from the topology's masses
    with pytest.raises(ValueError, match="mass"):
        Forces(par, terms=TERMS, virtual_sites=VirtualSites([1], [[0, 2, 3]], [[0.5, 0.25, 0.25]]))
    # every (site, parent) pair is excluded, also when the topology does not say so
    f2 = Forces(par, terms=["lj", "electrostatics"], exclusions=(), virtual_sites=vs)
    off, idx = f2._excl_csr
    assert idx[off[3]:off[4]].tolist() == [0, 1, 2] and idx[off[0]:off[1]].tolist() == [3]
    off1, idx1 = f._excl_csr  # ... and a no-op when it does
    f0 = Forces(par, terms=TERMS, cutoff=9.0, rfa=True)
    assert np.array_equal(off1, f0._excl_csr[0]) and np.array_equal(idx1, f0._excl_csr[1])
    # the skin weights never divide by the zero mass: a site takes the weight of its first parent
    w = f._skin_weight_array()
    assert np.isfinite(w).all() and np.array_equal(w[3::4], w[0::4]) and w[1] == 1.0 and w[0] < 1.0

    s = System(mol.numAtoms, 1, torch.float64, "cpu")
    with pytest.raises(ValueError, match="constraints"):
        Integrator(s, f, 2.0, "cpu")  # flexible parents in MD are out of scope
    # the parents of a site must be one rigid water: here the site hangs on two molecules
    bad = VirtualSites(vs.sites, np.stack([vs.parents[:, 0], vs.parents[:, 1], np.roll(vs.parents[:, 2], 1)], axis=1), vs.weights)
    fb = Forces(par, terms=TERMS, cutoff=9.0, rfa=True, virtual_sites=bad)
    with pytest.raises(ValueError, match="rigid water"):
        Integrator(s, fb, 2.0, "cpu", constraints="water")
    integ = Integrator(s, f, 2.0, "cpu", gamma=1.0, T=300.0, constraints="water")
    assert integ._ndof == 6 * 8 and torch.all(integ.vcoeff.reshape(-1)[3::4] == 0) and torch.isfinite(integ.vcoeff).all()


def test_find_constraints_with_sites():
    from torchmd_amd.builders import tip3p_box, water_forcefield
    from torchmd_amd.constraints import find_constraints
    from torchmd_amd.parameters import Parameters
    from torchmd_amd.wrapper import calculate_molecule_groups

    mol, pos, box, vs, par = _tip4p(3)
    nmol = mol.numAtoms // 4
    for mode in ("water", "hbonds"):
        cs = find_constraints(par.masses, par.bond_params, par.angle_params, mode, virtual_sites=vs)
        assert cs.nwaters == nmol and cs.nclusters == 0
        assert cs.ndof() == 9 * nmol - 3 * nmol
        assert cs.waters.tolist() == vs.parents.tolist() and cs.water_sites.tolist() == vs.sites.tolist()
        assert np.abs(cs.water_dist - np.array([0.9572, 1.5139])).max() < 1e-6
    batch = torch.as_tensor(np.repeat([0, 1], [4 * 10, 4 * (nmol - 10)]))
    assert cs.ndof(batch).tolist() == [60, 6 * (nmol - 10)]
    # the start-up projection leaves the massless rows alone and produces no inf / nan
    x = pos + np.random.default_rng(0).normal(size=pos.shape) * 0.02
    with np.errstate(all="raise"):
        cs.shake_positions(x, x.copy())
    assert np.isfinite(x).all()
    # M stays with its water in the barostat's / wrapper's groups
    off, mem = calculate_molecule_groups(mol.numAtoms, mol.bonds)
    assert np.all(np.diff(off) == 4) and np.array_equal(mem.reshape(-1, 4), np.arange(mol.numAtoms).reshape(-1, 4))

    # the three-site box: what the function returns today, with and without the new argument
    mol3, pos3, _ = tip3p_box(3, seed=1)
    par3 = Parameters(water_forcefield(mol3), mol3, TERMS, precision=torch.float64)
    a = find_constraints(par3.masses, par3.bond_params, par3.angle_params, "water")
    b = find_constraints(par3.masses, par3.bond_params, par3.angle_params, "water", virtual_sites=None)
    base = 3 * np.arange(27)
    assert np.array_equal(a.waters, np.stack([base, base + 1, base + 2], axis=1)) and a.nclusters == 0
    assert np.abs(a.water_dist - np.array([0.9572, 1.5139])).max() < 1e-6 and a.ndof() == 6 * 27
    for name in ("waters", "water_dist", "offsets", "atoms", "dist"):
        assert np.array_equal(getattr(a, name), getattr(b, name))
    assert a.nsites == 0 and a.water_sites is None and a.ndof() == b.ndof()


def test_builder_and_force_field():
    from torchmd_amd.builders import TIP4PEW_FF

    mol, pos, box, vs, par = _tip4p(2)
    assert list(mol.atomtype[:4]) == ["OW", "HW", "HW", "MW"]
    assert np.allclose(mol.charge[:4], [0.0, 0.52422, 0.52422, -1.04844]) and abs(float(np.sum(mol.charge))) < 1e-5
    assert par.masses.reshape(-1)[:4].tolist() == pytest.approx([15.9994, 1.008, 1.008, 0.0])
    assert np.abs(np.linalg.norm(pos[1::4] - pos[0::4], axis=1) - 0.9572).max() < 1e-12
    assert np.abs(np.linalg.norm(pos[3::4] - pos[0::4], axis=1) - 0.125).max() < 1e-12
    # every intramolecular pair is excluded by the reference's rules (bonds and angle ends)
    ex = {tuple(sorted(e)) for e in par.get_exclusions()}
    assert {(i, j) for i in range(4) for j in range(i + 1, 4)} <= ex and len(ex) == 6 * 8
    # only the oxygen carries LJ
    A, B = par.get_AB()
    ot = int(par.mapped_atom_types[0])
    assert (A != 0).sum() == 1 and A[ot, ot] > 0 and B[ot, ot] > 0
    sig, eps = TIP4PEW_FF["lj"]["OW"]["sigma"], TIP4PEW_FF["lj"]["OW"]["epsilon"]
    assert abs(float(B[ot, ot]) - 4 * eps * sig**6) < 1e-3 * 4 * eps * sig**6


def test_run_py_configuration_key(tmp_path):
    import yaml

    from torchmd_amd import run as driver
    from torchmd_amd.builders import TIP4PEW_FF
    from torchmd_amd.forcefields import YamlForceField

    log = str(tmp_path / "log")  # (get_args echoes the configuration into log_dir)
    assert driver.get_args(["--log-dir", log]).virtual_sites is None
    conf = tmp_path / "c.yaml"
    conf.write_text(yaml.safe_dump({"virtual_sites": "tip4p", "constraints": "water", "log_dir": log}))
    assert driver.get_args(["--conf", str(conf)]).virtual_sites == "tip4p"
    conf.write_text(yaml.safe_dump({"virtual_sites": "tip5p", "log_dir": log}))
    with pytest.raises(ValueError, match="virtual_sites"):
        driver.get_args(["--conf", str(conf)])
    mol, pos, box, vs, par = _tip4p(2)
    ffp = tmp_path / "ff.yaml"
    ffp.write_text(yaml.safe_dump(TIP4PEW_FF))
    got = driver.tip4p_sites(YamlForceField(mol, str(ffp)), mol)
    assert np.array_equal(got.sites, vs.sites) and np.array_equal(got.parents, vs.parents) and np.array_equal(got.weights, vs.weights)
    bare = {k: v for k, v in TIP4PEW_FF.items() if k != "virtual_sites"}
    with pytest.raises(ValueError, match="virtual_sites"):
        driver.tip4p_sites(YamlForceField(mol, bare), mol)
