"""Charge products from the LJ class table in the lean fp32 list pair kernel (pair_fast_kernel.h: QTAB; run with `-m gpu`).

A context whose scaled fp32 charges are, bit for bit, a function of the LJ class (`Forces.stats(...)["charge_by_class"] == 1`)
gathers 12 bytes per neighbour and reads `q_i q_j` and `(q_i 2 krf) q_j` from the class table in LDS; the products are formed
with the operands and in the order of the per-pair code, so NOTHING may change by a bit against the kernel that gathers the
charge (`TMDHIP_CHARGE_TABLE=0`, read when a context is created).  Checked here on the smallest boxes that have these code
paths:

  - forces of a plain evaluation (with energies: `compute`; forces only: the hot variant) and positions, velocities and forces
    after 25 MD steps with device-side list rebuilds inside (Langevin and NVE; interior and final launches), `torch.equal`
    against a fresh context with the table off: the smallest TIP3P box on the cell-list path, the 3 993-atom box (its last
    pair wave holds one atom), a water box with eight monatomic ions (four LJ classes), the LJ switching function, and two
    replicas with different boxes in one launch (the replica-batched kernel);
  - the same evaluations against the CPU oracle, within `FTOL["f32"]` of test_gpu_parity.py, with the exact in-cutoff pair count;
  - contexts that do not qualify — one atom's charge moved by one ulp, the alanine dipeptide (many charges per class) — report
    `charge_by_class == 0` and are bit-identical to `TMDHIP_CHARGE_TABLE=0` (the dipeptide on the list path, in a 32 A box;
    in its own box it takes the all-pairs kernel, whose fp32 atomics are not bit-reproducible from run to run: compared to
    rounding there); `update_atoms` re-decides, both ways."""

import functools

import numpy as np
import pytest
import torch

from _golden import GoldenParameters, box_tensor, load, pos_tensor
from test_gpu_parity import FTOL

pytestmark = pytest.mark.gpu

TERMS = ["lj", "electrostatics", "bonds", "angles"]
KW = dict(cutoff=9.0, rfa=True)
NSTEPS = 25


def _dev():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    return torch.device("cuda:0")


def _algorithm(par, pos, box):
    from torchmd_amd.forces import Forces

    f = Forces(par, terms=TERMS, **KW)
    p, b = pos_tensor(pos, 1, torch.float32, _dev()), box_tensor(box, 1, torch.float32, _dev())
    f.compute(p, b, torch.zeros_like(p))
    algo = f.stats(p)["algorithm"]
    f.close()
    return algo


@functools.lru_cache(maxsize=None)
def _smallest_celllist_nside():
    """The smallest tip3p_box the engine puts on the cell-list path by itself (2 048 atoms and three cells per box edge)."""
    from torchmd_amd.builders import tip3p_box, water_forcefield
    from torchmd_amd.parameters import Parameters

    for nside in range(8, 13):
        mol, pos, box = tip3p_box(nside, seed=3)
        if _algorithm(Parameters(water_forcefield(mol), mol, TERMS, precision=torch.float32), pos, box) == "celllist":
            return nside
    raise AssertionError("no tip3p_box up to nside = 12 (5 184 atoms) reaches the cell-list path")


def _ion_water(nside, seed):
    """tip3p_box with eight waters replaced by monatomic ions (4 Na+, 4 Cl-; CHARMM-style LJ parameters): four LJ classes,
    one charge each."""
    from torchmd_amd.builders import TIP3P_FF, tip3p_box
    from torchmd_amd.forcefields import YamlForceField
    from torchmd_amd.io import Topology

    mol, pos, box = tip3p_box(nside, seed=seed)
    nmol = mol.numAtoms // 3
    ions = np.arange(5, nmol, nmol // 8)[:8]
    keep = np.ones(mol.numAtoms, dtype=bool)
    atomtype, charge, masses = mol.atomtype.copy(), mol.charge.copy(), mol.masses.copy()
    for k, m in enumerate(ions):
        keep[3 * m + 1 : 3 * m + 3] = False
        atomtype[3 * m], charge[3 * m], masses[3 * m] = ("SOD", 1.0, 22.98977) if k % 2 == 0 else ("CLA", -1.0, 35.45)
    new_index = np.cumsum(keep) - 1
    bonds = new_index[mol.bonds[keep[mol.bonds].all(axis=1)]]
    angles = new_index[mol.angles[keep[mol.angles].all(axis=1)]]
    ff = {k: (dict(v) if isinstance(v, dict) else list(v)) for k, v in TIP3P_FF.items()}
    ff["atomtypes"] += ["SOD", "CLA"]
    ff["lj"].update({"SOD": {"sigma": 2.42993, "epsilon": -0.0469}, "CLA": {"sigma": 4.04468, "epsilon": -0.15}})
    ff["electrostatics"].update({"SOD": {"charge": 1.0}, "CLA": {"charge": -1.0}})
    ff["masses"].update({"SOD": 22.98977, "CLA": 35.45})
    ion_mol = Topology(atomtype=atomtype[keep], charge=charge[keep], masses=masses[keep], bonds=bonds, angles=angles)
    return ion_mol, pos[keep], box, YamlForceField(ion_mol, ff)


@functools.lru_cache(maxsize=None)
def _system(name):
    """(par, pos [N, 3], box [3], LJ classes) of a test system, fp32"""
    from torchmd_amd.builders import tip3p_box, water_forcefield
    from torchmd_amd.parameters import Parameters

    if name == "ions":
        mol, pos, box, ff = _ion_water(_smallest_celllist_nside(), seed=4)
        nclass = 4
    else:
        nside = {"smallest": _smallest_celllist_nside(), "water11": 11}[name.split("-")[0]]
        mol, pos, box = tip3p_box(nside, seed=3)
        if name.endswith("-ulp"):  # ONE charge (a hydrogen's, in the middle of the box's atoms) moved by one ulp of fp32
            k = 3 * (mol.numAtoms // 6) + 1
            mol.charge = mol.charge.astype(np.float32)
            mol.charge[k] = np.nextafter(mol.charge[k], np.float32(1.0))
        ff, nclass = water_forcefield(mol), 2
    par = Parameters(ff, mol, TERMS, precision=torch.float32)
    assert len(np.unique(par.mapped_atom_types.numpy())) == nclass
    return par, pos, box, nclass


def _evaluate(name, table, monkeypatch, **kw):
    """Forces of `compute` (with energies) and of a forces-only evaluation in a fresh context, its stats and pair count."""
    from torchmd_amd.forces import Forces

    monkeypatch.setenv("TMDHIP_CHARGE_TABLE", "1" if table else "0")
    par, pos, box, _ = _system(name)
    dev = _dev()
    p, b = pos_tensor(pos, 1, torch.float32, dev), box_tensor(box, 1, torch.float32, dev)
    f = Forces(par, terms=TERMS, **{**KW, **kw})
    Fe = torch.full_like(p, 7.0)
    pots = f.compute(p, b, Fe, returnDetails=True)
    Fo = torch.full_like(p, 7.0)
    f._evaluate(p, b, Fo, False, True)  # forces only: the hot variant of the pair kernel
    st = f.stats(p)
    npairs = f.count_pairs(p, b)
    f.close()
    return Fe, Fo, pots, st, npairs


def _md(name, table, langevin, monkeypatch, scales=(1.0,), **kw):
    """len(scales) replicas of the system (boxes and coordinates scaled), NSTEPS MD steps from hot velocities."""
    from torchmd_amd.forces import Forces
    from torchmd_amd.integrator import Integrator, maxwell_boltzmann
    from torchmd_amd.systems import System

    monkeypatch.setenv("TMDHIP_CHARGE_TABLE", "1" if table else "0")
    par, pos, box, _ = _system(name)
    dev, R = _dev(), len(scales)
    s = System(pos.shape[0], R, torch.float32, dev)
    s.set_positions(np.stack([pos * sc for sc in scales], axis=2))
    s.set_box(np.stack([box * sc for sc in scales], axis=1))
    torch.manual_seed(11)
    s.set_velocities(maxwell_boltzmann(par.masses, 1500.0, R))  # (hot: the fastest hydrogens use up the skin in ~5 steps)
    f = Forces(par, terms=TERMS, **{**KW, **kw})
    f.compute(s.pos, s.box, s.forces)
    r0 = f.stats(s.pos)["n_rebuilds"]
    torch.manual_seed(5)
    integ = Integrator(s, f, 1.0, dev, **(dict(gamma=0.5, T=300.0) if langevin else {}))
    out = integ.step(NSTEPS)
    st = f.stats(s.pos)
    res = (s.pos.clone(), s.vel.clone(), s.forces.clone(), out, st, st["n_rebuilds"] - r0)
    f.close()
    return res


def _same_md(a, b):
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])
    assert torch.isfinite(a[0]).all() and torch.isfinite(a[1]).all() and torch.isfinite(a[2]).all()
    for x, y in zip(a[3], b[3]):  # kinetic energy, potential energy, temperature: sums of the same terms (fp64 atomics: another order)
        assert np.allclose(x, y, rtol=2e-7)
    assert a[5] == b[5] >= 2, (a[5], b[5])  # two or more device-side rebuilds inside


def test_the_boxes_are_the_ones_these_code_paths_need():
    nside = _smallest_celllist_nside()
    assert 3 * nside**3 >= 2048 and 3 * (nside - 1) ** 3 < 5184
    par, pos, box, _ = _system("water11")
    assert pos.shape[0] == 3993 and _algorithm(par, pos, box) == "celllist"  # 3 993 = 499 x 8 + 1
    par, pos, box, _ = _system("ions")
    assert pos.shape[0] == 3 * nside**3 - 16 and _algorithm(par, pos, box) == "celllist"


@pytest.mark.parametrize("kw", [{}, {"switch_dist": 7.5}], ids=["plain", "switch"])
@pytest.mark.parametrize("name", ["smallest", "water11", "ions"])
def test_forces_are_bit_identical_to_the_gathered_charge(name, kw, monkeypatch):
    Fe1, Fo1, pots1, st1, _ = _evaluate(name, True, monkeypatch, **kw)
    Fe0, Fo0, pots0, st0, _ = _evaluate(name, False, monkeypatch, **kw)
    assert st1["charge_by_class"] == 1 and st0["charge_by_class"] == 0
    assert st1["algorithm"] == st0["algorithm"] == "celllist"
    assert torch.equal(Fe1, Fe0) and torch.equal(Fo1, Fo0)
    assert torch.isfinite(Fe1).all() and Fe1.abs().max().item() > 1.0
    for t in TERMS:
        assert abs(pots1[0][t] - pots0[0][t]) <= 2e-7 * max(1.0, abs(pots0[0][t])), t


@pytest.mark.parametrize("langevin", [True, False], ids=["langevin", "nve"])
@pytest.mark.parametrize("name", ["smallest", "water11", "ions"])
def test_md_is_bit_identical_to_the_gathered_charge(name, langevin, monkeypatch):
    on = _md(name, True, langevin, monkeypatch)
    off = _md(name, False, langevin, monkeypatch)
    assert on[4]["charge_by_class"] == 1 and off[4]["charge_by_class"] == 0
    assert on[4]["steps_in_pair_launch"] >= NSTEPS // 2 and off[4]["steps_in_pair_launch"] == on[4]["steps_in_pair_launch"]
    _same_md(on, off)


@pytest.mark.parametrize("langevin", [True, False], ids=["langevin", "nve"])
def test_md_with_the_switching_function_is_bit_identical(langevin, monkeypatch):
    on = _md("smallest", True, langevin, monkeypatch, switch_dist=7.5)
    off = _md("smallest", False, langevin, monkeypatch, switch_dist=7.5)
    assert on[4]["charge_by_class"] == 1 and off[4]["charge_by_class"] == 0
    _same_md(on, off)


@pytest.mark.parametrize("langevin", [True, False], ids=["langevin", "nve"])
@pytest.mark.parametrize("name", ["smallest", "ions"])
def test_two_replicas_with_different_boxes_in_one_launch_are_bit_identical(name, langevin, monkeypatch):
    monkeypatch.setenv("TMDHIP_BATCH_REPLICAS", "1")
    on = _md(name, True, langevin, monkeypatch, scales=(1.0, 1.004))
    off = _md(name, False, langevin, monkeypatch, scales=(1.0, 1.004))
    assert on[4]["charge_by_class"] == 1 and off[4]["charge_by_class"] == 0
    assert on[4]["batched_launches"] >= NSTEPS // 2 and off[4]["batched_launches"] == on[4]["batched_launches"]
    _same_md(on, off)
    assert (on[0][0] * 1.004 - on[0][1]).abs().max().item() > 1e-3  # (the replicas went their own ways)


@functools.lru_cache(maxsize=None)
def _oracle(name):
    from oracle import torchmd_oracle as orc

    par, pos, box, _ = _system(name)
    p, b = pos_tensor(pos, 1, torch.float32), box_tensor(box, 1, torch.float32)
    pairs = orc.candidate_pairs(p[0].double().numpy(), box, 9.6, orc.exclusion_pairs(par))
    return orc.compute(par, p, b, TERMS, pairs=pairs, **KW)


@pytest.mark.parametrize("name", ["smallest", "water11", "ions"])
def test_forces_and_pair_count_against_the_oracle(name, monkeypatch):
    po, Fo, npairs = _oracle(name)
    Fe, Ff, pots, st, counted = _evaluate(name, True, monkeypatch)
    assert st["charge_by_class"] == 1
    err_e, err_f = (Fe.cpu() - Fo).abs().max().item(), (Ff.cpu() - Fo).abs().max().item()
    print(f"{name}: {Fo.shape[1]} atoms, max|dF| vs the oracle {err_e:.2e} (with energies) / {err_f:.2e} (forces only), "
          f"{int(npairs[0])} pairs in the cutoff")
    assert err_e <= FTOL["f32"] and err_f <= FTOL["f32"]
    assert counted == npairs


def test_one_ulp_in_one_charge_keeps_the_gathered_charge(monkeypatch):
    name = "smallest-ulp"
    Fe1, Fo1, _, st1, n1 = _evaluate(name, True, monkeypatch)
    Fe0, Fo0, _, st0, n0 = _evaluate(name, False, monkeypatch)
    assert st1["charge_by_class"] == 0 and st0["charge_by_class"] == 0 and st1["algorithm"] == "celllist"
    assert torch.equal(Fe1, Fe0) and torch.equal(Fo1, Fo0) and n1 == n0
    on, off = _md(name, True, True, monkeypatch), _md(name, False, True, monkeypatch)
    assert on[4]["charge_by_class"] == 0
    _same_md(on, off)
    # ... and the moved charge is really in the forces: they differ from the unmodified box's
    assert not torch.equal(Fe1, _evaluate("smallest", False, monkeypatch)[0])


def test_alanine_dipeptide_has_many_charges_per_class(monkeypatch):
    from torchmd_amd.forces import Forces

    g = load("ala2")
    par = GoldenParameters(g, torch.float32)
    dev = _dev()
    p = pos_tensor(g["pos"], 1, torch.float32, dev)
    # its own box: the all-pairs kernel; a 32 A box (three cells of cutoff + skin per edge): the list path, the lean kernel
    boxes = {"auto": box_tensor(g["box"], 1, torch.float32, dev), "celllist": box_tensor(np.full(3, 32.0), 1, torch.float32, dev)}
    out = {}
    for table in (True, False):
        monkeypatch.setenv("TMDHIP_CHARGE_TABLE", "1" if table else "0")
        for algo in ("auto", "celllist"):
            f = Forces(par, terms=["electrostatics", "lj"], cutoff=9.0, switch_dist=7.5, rfa=True,
                       **({} if algo == "auto" else {"algorithm": algo}))
            F = torch.full_like(p, 7.0)
            f.compute(p, boxes[algo], F)
            st = f.stats(p)
            assert st["charge_by_class"] == 0 and st["algorithm"] == ("allpairs" if algo == "auto" else "celllist")
            out[table, algo] = F.clone()
            f.close()
    assert torch.equal(out[True, "celllist"], out[False, "celllist"]) and torch.isfinite(out[True, "celllist"]).all()
    # (the all-pairs kernel, which the switch does not reach, sums a j range per block with fp32 atomics: two runs of ONE
    # library differ in the last bits, so there the comparison is to the rounding of a sum: 21 partners of each of the 22
    # atoms, pair forces below 100 kcal/mol/A, one ulp of fp32 each)
    assert (out[True, "auto"] - out[False, "auto"]).abs().max().item() <= 21 * 100 * 2.0**-23


def test_update_atoms_decides_again_both_ways(monkeypatch):
    """An atomic mixture whose types A1 / A2 share one LJ class: with opposite charges the class has two charges (no table),
    with A2's charge made A1's it has one.  `update_atoms` swaps the two atom sets into ONE context, there and back; every
    evaluation is bit-identical to a fresh context with the table off."""
    from _oracle_sample import mixed_system
    from torchmd_amd.domain import _local_parameters
    from torchmd_amd.forces import Forces

    dev, dt = _dev(), torch.float32
    _, pos, box, par, terms = mixed_system(18, dt, seed=9)  # 5 832 atoms
    A, B = par.get_AB()
    same = par.charges.clone()
    same[same < 0] = -same[same < 0]
    sets = {"one": _local_parameters(same, par.mapped_atom_types, par.masses.reshape(-1), A, B),
            "two": _local_parameters(par.charges, par.mapped_atom_types, par.masses.reshape(-1), A, B)}
    p, b = pos_tensor(pos, 1, dt, dev), box_tensor(box, 1, dt, dev)

    def forces_of(f):
        F = torch.full_like(p, float("nan"))
        f._evaluate(p, b, F, False, True)
        return F

    monkeypatch.setenv("TMDHIP_CHARGE_TABLE", "0")
    ref = {}
    for k, lp in sets.items():
        f0 = Forces(lp, terms=terms, skin_weights=None, **KW)
        ref[k] = forces_of(f0)
        assert f0.stats(p)["charge_by_class"] == 0 and f0.stats(p)["algorithm"] == "celllist"
        f0.close()
    assert not torch.equal(ref["one"], ref["two"]) and torch.isfinite(ref["one"]).all()
    monkeypatch.setenv("TMDHIP_CHARGE_TABLE", "1")
    f = Forces(sets["one"], terms=terms, skin_weights=None, **KW)
    for k, want in (("one", 1), ("two", 0), ("one", 1), ("two", 0)):
        if f._engines:
            f.update_atoms(sets[k])
        F = forces_of(f)
        assert f.stats(p)["charge_by_class"] == want, k
        assert torch.equal(F, ref[k]), k
    f.close()
