"""CPU checks of the synthetic bonded topologies (tests/_bonded_systems.py) that test_gpu_bonded.py runs on the GPU:
the builders are deterministic, land where they claim (record counts, wrap clearance, near-cutoff bond lengths), and
the oracle's explicit forces on them equal minus its autograd gradient — so that no case sits on a discontinuity."""

import numpy as np
import pytest
import torch

from oracle import torchmd_oracle as orc

import _bonded_systems as B

NAMES = ["light-full", "light-plus-one", "hub", "harmonic", "harmonic-dihedrals", "edges"]


@pytest.mark.parametrize("size", [B.SMALL, B.LARGE])
@pytest.mark.parametrize("name", NAMES)
def test_builders_are_deterministic_and_meet_their_claims(name, size):
    a, b = B.build(name, size), B.build(name, size)  # (each builder asserts its own record counts and clearances)
    assert a.natoms == b.natoms and np.array_equal(a.pos, b.pos) and np.array_equal(a.box, b.box)
    assert a.g.keys() == b.g.keys() and all(np.array_equal(a.g[k], b.g[k]) for k in a.g)
    assert a.natoms <= 2048 if size == B.SMALL else 4000 <= a.natoms <= 8000
    par = a.par()
    # molecules are spread over the 64-atom blocks; some atoms are a box length or more outside the box
    bonds = a.g["par_bond_idx"]
    assert (bonds[:, 0] // 64 != bonds[:, 1] // 64).mean() > 0.5
    assert ((a.pos < -a.box) | (a.pos >= 2 * a.box)).any() and ((a.pos < 0) | (a.pos >= a.box)).any(axis=1).mean() > 0.05
    assert len(np.unique(a.g["par_types"])) <= 5
    if par.dihedral_params is not None:  # map rows not grouped by torsion (forces.py's stable argsort has work to do)
        assert (np.diff(a.g["par_dihedral_map"][:, 0]) < 0).any()
        assert set(np.bincount(a.g["par_dihedral_map"][:, 0]).tolist()) == {1, 2, 3}


def test_record_counts_mirror_set_bonded_rules():
    s = B.light_full()
    par = s.par()
    full, bonded = B.records_per_atom(par, B.ALL_TERMS), B.records_per_atom(par, B.BONDED)
    n14 = np.bincount(s.g["par_nonbonded_14_idx"].reshape(-1), minlength=s.natoms)
    assert np.array_equal(full - bonded, n14)  # 1-4 records only with lj / electrostatics
    k0 = s.g["par_bond_params"][s.g["par_bond_map"][:, 1], 0]
    assert (k0 == 0).any()
    dead = s.g["par_bond_idx"][k0 == 0].reshape(-1)
    assert (bonded[dead] == 0).all()  # the k0 = 0 diatomics: no record at all


@pytest.mark.parametrize("name", ["harmonic", "harmonic-dihedrals"])
def test_harmonic_wrap_fires_and_keeps_clear_of_the_jump(name):
    s = B.build(name)
    for t in ["improper"] + (["dihedral"] if name == "harmonic-dihedrals" else []):
        raw, w = B.harmonic_offsets(s, t)
        assert (raw > np.pi).any() and (raw < -np.pi).any()
        assert np.abs(np.abs(w) - np.pi).min() >= B.WRAP_CLEARANCE
        # ... also for the fp32-rounded inputs the fp32 runs see
        raw32, w32 = B.harmonic_offsets(s.rounded(torch.float32), t)
        assert np.abs(np.abs(w32) - np.pi).min() >= B.WRAP_CLEARANCE / 2


@pytest.mark.parametrize("prec", ["f64", "f32"])
def test_near_cutoff_bonds_sit_ulps_either_side_of_the_cutoff(prec):
    dt = {"f64": torch.float64, "f32": torch.float32}[prec]
    s = B.edges(dt)
    rows, k = s.meta["near_cutoff_bonds"], s.meta["near_cutoff_offsets"]
    pos = torch.tensor(s.pos).to(dt)
    idx = torch.tensor(s.g["par_bond_idx"][rows])
    d = orc.pair_geometry(pos, idx, torch.tensor(s.box).to(dt))[0].numpy()
    npdt = np.float32 if prec == "f32" else np.float64
    c = npdt(9.0)
    assert np.array_equal(d, np.array([float(c) + j * float(np.spacing(c)) for j in k], dtype=npdt))
    assert ((d <= c) == (k <= 0)).all() and (k < 0).any() and (k > 0).any()
    long_d = orc.pair_geometry(pos, torch.tensor(s.g["par_bond_idx"][s.meta["long_bonds"]]), torch.tensor(s.box).to(dt))[0]
    assert (long_d > 9.0).all()
    # the angles at the edge: exactly linear (cos = -1 with no rounding) and within 1e-3 rad of it
    ang = torch.tensor(s.g["par_angle_idx"])
    for rows, lo, hi in ((s.meta["linear_angles"], 0.0, 0.0), (s.meta["near_linear_angles"], 4e-4, 1e-3)):
        _, _, r21 = orc.pair_geometry(pos, ang[rows][:, [0, 1]], torch.tensor(s.box).to(dt))
        _, _, r23 = orc.pair_geometry(pos, ang[rows][:, [2, 1]], torch.tensor(s.box).to(dt))
        cos = (r21 * r23).sum(1) / r21.norm(dim=1) / r23.norm(dim=1)
        if hi == 0.0:
            assert (cos == -1).all()
        else:
            dl = np.pi - np.arccos(cos.double().numpy())
            assert (dl > lo).all() and (dl < hi).all(), dl
    th0 = s.g["par_angle_params"][s.g["par_angle_map"][:, 1], 1]
    for rows in (s.meta["linear_angles"], s.meta["near_linear_angles"]):
        assert (th0[rows] == np.pi).any() and (th0[rows] != np.pi).any()


@pytest.mark.parametrize("name", NAMES)
def test_oracle_explicit_forces_equal_its_autograd_gradient(name):
    """Every system is smooth where it stands: the explicit forces (forces.py's formulas) equal minus the autograd
    gradient of the energy to 1e-9.  (The exactly linear angles of `edges` sit on the kink of k (theta - theta0)^2 at
    theta = pi by design — the reference's sin = 0 rule gives them zero force, test_gpu_bonded checks that — and are left
    out here.)"""
    s = B.build(name)
    if name == "edges":
        keep = np.ones(len(s.g["par_angle_idx"]), bool)
        keep[s.meta["linear_angles"]] = False
        s = s.with_tables(angle=keep)
    par = s.par()
    pos = torch.tensor(s.pos)[None]
    box = torch.diag(torch.tensor(s.box))[None]
    pairs = orc.candidate_pairs(s.pos, s.box, 9.5, orc.exclusion_pairs(par))
    E, F, _ = orc.compute(par, pos, box, B.ALL_TERMS, cutoff=9.0, rfa=True, pairs=pairs)
    p = pos.clone().requires_grad_(True)
    Ea, Fa, _ = orc.compute(par, p, box, B.ALL_TERMS, cutoff=9.0, rfa=True, pairs=pairs, explicit_forces=False)
    assert ((F - Fa).abs() / (1 + F.abs())).max().item() <= 1e-9
    for t in B.ALL_TERMS:
        assert abs(E[0][t] - Ea[0][t]) <= 1e-12 * max(1.0, abs(E[0][t]))
