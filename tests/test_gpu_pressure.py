"""The pressure observable on the device: `Forces.virial`, `Integrator.pressure` / `pressure_tensor` and
`tmdhip_pressure` against the numpy model of tests/_pressure.py, against each other, and — independently of the model —
against -3V dU/dV by central differences of `compute()`'s energy.

Bars.  Virial against model: (64 eps + M eps64) S per axis, eps that of the context's precision, S the model's condition scale
(_pressure.py: what one relative rounding error of every pair force moves W by at most), M the number of addends of the
double sums (two visits per pair).  64 eps S is the bar and derivation of DESIGN §15: the kernels call the same `pair_terms`
on the same d, the products f_a (d_a / 2 - delta_a) are formed in double from the force component as rounded in the context's
precision, so a pair's error is that of its force times |d_a / 2| + |delta_a|, which is what S sums.  Kinetic part: M eps64
sum |terms|, all in double from the stored velocities.  Finite differences: 10 |FD(eps) - FD(eps / 2)| + 64 eps64 S.
Observed multiples are printed by every test."""

import ctypes as C
import os

import numpy as np
import pytest
import torch

import _pressure as M
from _golden import PREC, GoldenParameters, box_tensor, load, pos_tensor
from _pair_reference import SWITCH_DIST

pytestmark = pytest.mark.gpu

EPS = {"f32": float(np.finfo(np.float32).eps), "f64": float(np.finfo(np.float64).eps)}
EPS64 = EPS["f64"]
WATER_TERMS = ["lj", "electrostatics", "bonds", "angles"]
# (id, nonbonded terms, Forces keywords): RF, plain Coulomb, LJ switched in both flavours, repulsion
TERM_SETS = {
    "lj_rf": (("lj", "electrostatics"), dict(rfa=True)),
    "coul": (("electrostatics",), dict()),
    "lj_sw_ref": (("lj",), dict(switch_dist=SWITCH_DIST, switch_mode="reference")),
    "lj_sw_exact": (("lj",), dict(switch_dist=SWITCH_DIST, switch_mode="exact")),
    "repulsion": (("repulsion",), dict()),
}
TERM_SETS_MORE = {"lj_pme": (("lj", "electrostatics"), dict())}


def _dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _bar(m, prec):
    return (64 * EPS[prec] + m.addends * EPS64) * m.S


_CASES = {}


def _water(kind, nside, seed, prec):
    """(mol, pos [N,3] float64, box [3], Parameters, VirtualSites or None) of a jittered water box, cached."""
    from torchmd_amd.builders import tip3p_box, tip4p_box, tip4pew_forcefield, water_forcefield
    from torchmd_amd.parameters import Parameters

    key = (kind, nside, seed, prec)
    if key not in _CASES:
        if kind == "tip4p":
            mol, pos, box, vs = tip4p_box(nside, seed=seed)
            par = Parameters(tip4pew_forcefield(mol), mol, WATER_TERMS, precision=PREC[prec])
        else:
            mol, pos, box = tip3p_box(nside, seed=seed)
            vs = None
            par = Parameters(water_forcefield(mol), mol, WATER_TERMS, precision=PREC[prec])
        _CASES[key] = (mol, np.asarray(pos, dtype=np.float64), np.asarray(box, dtype=np.float64), par, vs)
    return _CASES[key]


def _forces(par, tset, cutoff, vs=None, **kw):
    from torchmd_amd.forces import Forces

    terms, opts = {**TERM_SETS, **TERM_SETS_MORE}[tset]
    return Forces(par, terms=list(terms), cutoff=cutoff, virtual_sites=vs, **opts, **kw)


def _sys(f, par, tset, vs=None):
    return M.system_of(par, {**TERM_SETS, **TERM_SETS_MORE}[tset][0], f._excl_csr, vs)


def _model(sysm, pos, box, tset, cutoff, prec, **kw):
    terms, opts = {**TERM_SETS, **TERM_SETS_MORE}[tset]
    return M.nonbonded_model(pos, box, sysm, terms, cutoff, prec=prec, **opts, **kw)


def _stored(pos, prec):
    """The positions as the device stores them, float64."""
    return np.asarray(pos, dtype=np.float64).astype(M.NP_DTYPE[prec]).astype(np.float64)


def _check(tag, W, m, prec):
    bar = _bar(m, prec)
    mult = np.abs(W - m.W) / (EPS[prec] * m.S)
    print(f"{tag} {prec}: W = {W}, model {m.W}, |dW| = {np.abs(W - m.W)}, bar {bar}, multiples of eps S: {mult}, pairs {m.npairs}")
    assert np.isfinite(W).all() and (np.abs(W - m.W) <= bar).all(), (tag, W, m.W, bar)
    if prec == "f64":
        assert (np.abs(m.W) > 1e3 * bar).any()  # (the bar resolves the value)


def _translate_molecules(pos, box, sysm, seed):
    rng = np.random.default_rng(seed)
    k = rng.integers(-2, 3, size=(len(sysm.off) - 1, 3)).astype(np.float64)
    return pos + (k * box)[sysm.mol_of]


# ---------------------------------------------------------------- all-pairs kernel
@pytest.mark.parametrize("tset", list(TERM_SETS))
@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_allpairs_kernel_against_model(prec, tset):
    mol, pos, box, par, _ = _water("tip3p", 6, 3, prec)  # 648 atoms, L = 18.6: fewer than three cells per edge
    f = _forces(par, tset, 9.0)
    p, b = pos_tensor(pos, 1, PREC[prec], _dev()), box_tensor(box, 1, PREC[prec], _dev())
    W = f.virial(p, b)
    assert W.shape == (1, 3) and f.stats(p)["algorithm"] == "allpairs"
    sysm = _sys(f, par, tset)
    _check(f"648 all pairs {tset}", W[0], _model(sysm, _stored(pos, prec), box, tset, 9.0, prec), prec)
    # whole molecules moved by box multiples: the same virial, within the bar of either state
    moved = _translate_molecules(pos, box, sysm, 5)
    m2 = _model(sysm, _stored(moved, prec), box, tset, 9.0, prec)
    W2 = f.virial(pos_tensor(moved, 1, PREC[prec], _dev()), b)
    _check(f"648 all pairs {tset}, molecules translated", W2[0], m2, prec)


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_water291_two_replicas_virial_and_kinetic_part(prec):
    g = load("water291")
    par = GoldenParameters(g, PREC[prec])
    pos = np.stack([np.asarray(g["pos"], dtype=np.float64), np.asarray(g["f64_traj_pos"], dtype=np.float64)[1]])
    vel = np.asarray(g["traj_vel0"], dtype=np.float64) * np.array([1.0, 1.7])[:, None, None]
    box = np.asarray(g["box"], dtype=np.float64).reshape(-1)[:3]
    from torchmd_amd.forces import Forces

    f = Forces(par, terms=WATER_TERMS, cutoff=7.3, rfa=True)
    sysm = M.system_of(par, ("lj", "electrostatics"), f._excl_csr)
    # molecules are whole in both replicas (the contract): every bonded pair closer than 2 A without any image
    bonds = par.bond_params["idx"].numpy()
    assert all(np.linalg.norm(pos[r][bonds[:, 0]] - pos[r][bonds[:, 1]], axis=1).max() < 2.0 for r in range(2))
    p = torch.as_tensor(pos, dtype=PREC[prec]).to(_dev()).contiguous()
    v = torch.as_tensor(vel, dtype=PREC[prec]).to(_dev()).contiguous()
    b = box_tensor(box, 2, PREC[prec], _dev())
    t = f._pressure_terms(p, b, vel=v, masses=par.masses)
    assert t.shape == (2, 8) and f.stats(p)["algorithm"] == "allpairs"
    assert np.array_equal(f.virial(p, b), t[:, 3:6])
    for r in range(2):
        m = M.nonbonded_model(_stored(pos[r], prec), box, sysm, ("lj", "electrostatics"), 7.3, prec=prec, rfa=True)
        _check(f"water291 replica {r}", t[r, 3:6], m, prec)
        vs = v[r].cpu().double().numpy()
        kin = M.kinetic_model(vs, sysm.mass, sysm.off, sysm.mem)
        scale = (sysm.mass[:, None] * vs * vs).sum(axis=0)
        print(f"water291 {prec} replica {r}: kinetic {t[r, :3]} model {kin} |d| {np.abs(t[r, :3] - kin)} bar {len(vs) * EPS64 * scale}")
        assert (np.abs(t[r, :3] - kin) <= len(vs) * EPS64 * scale).all()
        V = float(np.prod(torch.diagonal(b[r]).cpu().double().numpy()))  # (the box as the tensor holds it)
        assert t[r, 6] == V
        assert abs(t[r, 7] - (t[r, :6].sum() / (3 * V))) <= 8 * EPS64 * np.abs(t[r, :6]).sum() / (3 * V)
    assert not np.array_equal(t[0], t[1])


# ---------------------------------------------------------------- list kernel
LIST_CUTOFF = 6.5  # 1 536 atoms, L = 24.84: three cells per edge of cutoff + the largest pair skin (1.44 with per-atom skins) = 7.94
_LIST_STATES = {}


def _list_states(prec):
    """Positions (float64, as stored) of the 1 536-atom box: fresh, after 30 MD steps, and the latter with whole molecules
    translated by box multiples — with the model of each, computed once."""
    if prec not in _LIST_STATES:
        from torchmd_amd.integrator import Integrator, maxwell_boltzmann
        from torchmd_amd.systems import System

        mol, pos, box, par, _ = _water("tip3p", 8, 4, prec)
        from torchmd_amd.forces import Forces

        f = Forces(par, terms=WATER_TERMS, cutoff=LIST_CUTOFF, rfa=True, algorithm="celllist")
        s = System(mol.numAtoms, 1, PREC[prec], _dev())
        s.set_positions(pos[:, :, None])
        s.set_box(box)
        torch.manual_seed(3)
        s.set_velocities(maxwell_boltzmann(par.masses.double(), 300, 1).to(PREC[prec]))
        f.compute(s.pos, s.box, s.forces)
        integ = Integrator(s, f, 1.0, _dev())
        integ.step(30)
        assert f.stats(s.pos)["algorithm"] == "celllist"
        aged = s.pos[0].cpu().double().numpy()
        sysm = M.system_of(par, ("lj", "electrostatics"), f._excl_csr)
        states = {"fresh": _stored(pos, prec), "aged": aged, "translated": _stored(_translate_molecules(aged, box, sysm, 9), prec)}
        models = {k: _model(sysm, v, box, "lj_rf", LIST_CUTOFF, prec) for k, v in states.items()}
        _LIST_STATES[prec] = (par, box, states, models, s.vel.clone(), sysm)
    return _LIST_STATES[prec]


@pytest.mark.parametrize("lpa", [1, 2, 4, 8, 16, 32, 64])
@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_list_kernel_against_model_and_allpairs_kernel(prec, lpa, monkeypatch):
    monkeypatch.setenv("TMDHIP_LPA", str(lpa))
    par, box, states, models, _, _ = _list_states(prec)
    f = _forces(par, "lj_rf", LIST_CUTOFF, algorithm="celllist")  # (AUTO takes the list from 2 048 atoms on)
    g = _forces(par, "lj_rf", LIST_CUTOFF, algorithm="allpairs")
    b = box_tensor(box, 1, PREC[prec], _dev())
    for name in ("fresh", "aged", "translated"):  # (aged: the list of the fresh positions, 30 steps on)
        p = torch.as_tensor(states[name], dtype=PREC[prec]).to(_dev())[None].contiguous()
        W = f.virial(p, b)[0]
        st = f.stats(p)
        assert st["algorithm"] == "celllist" and min(st["ncell"]) >= 3
        _check(f"1536 list lpa {lpa} {name} (rebuilds {st['n_rebuilds']})", W, models[name], prec)
        Wa = g.virial(p, b)[0]
        assert g.stats(p)["algorithm"] == "allpairs"
        assert (np.abs(W - Wa) <= 2 * _bar(models[name], prec)).all(), (name, W, Wa)
    # whole molecules moved by box multiples: the same virial
    assert (np.abs(models["aged"].W - models["translated"].W) <= 64 * EPS[prec] * models["aged"].S).all()


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_kinetic_part_of_the_list_box_and_pressure_in_bar(prec):
    from torchmd_amd.barostat import BAR_TO_KCAL_MOL_A3
    from torchmd_amd.integrator import Integrator
    from torchmd_amd.systems import System

    par, box, states, models, vel, sysm = _list_states(prec)
    f = _forces(par, "lj_rf", LIST_CUTOFF, algorithm="celllist")  # (AUTO takes the list from 2 048 atoms on)
    s = System(len(sysm.mass), 1, PREC[prec], _dev())
    s.set_positions(states["aged"][:, :, None])
    s.set_box(box)
    s.set_velocities(vel)
    integ = Integrator(s, f, 1.0, _dev())
    P3, P = integ.pressure_tensor(), integ.pressure()
    assert P3.shape == (1, 3) and P.shape == (1,)
    vs = s.vel[0].cpu().double().numpy()
    kin = M.kinetic_model(vs, sysm.mass, sysm.off, sysm.mem)
    V = float(np.prod(box))
    want = (kin + models["aged"].W) / V / BAR_TO_KCAL_MOL_A3
    bar = (_bar(models["aged"], prec) + len(vs) * EPS64 * (sysm.mass[:, None] * vs * vs).sum(axis=0)) / V / BAR_TO_KCAL_MOL_A3
    print(f"1536 {prec}: P_aa = {P3[0]} bar, model {want}, bar {bar}; P = {P[0]} bar")
    assert (np.abs(P3[0] - want) <= bar).all() and abs(P[0] - want.mean()) <= bar.max()
    assert 10 < kin.sum() / (3 * V) / BAR_TO_KCAL_MOL_A3 < 1e4  # (an ideal-gas term of water at ~300 K: ~1 400 bar)


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_bond_free_atoms_kinetic_part_is_two_thirds_of_the_kinetic_energy(prec):
    """64 atoms without bonds are 64 molecules of one: sum M V^2 = 2 E_kin of tmdhip_kinetic_energy, and delta = 0."""
    from torchmd_amd import _lib as L
    from torchmd_amd.builders import argon_forcefield, lj_box
    from torchmd_amd.forces import Forces
    from torchmd_amd.integrator import maxwell_boltzmann
    from torchmd_amd.parameters import Parameters

    mol, pos, box = lj_box(4, seed=2)
    par = Parameters(argon_forcefield(mol), mol, ["lj"], precision=PREC[prec])
    f = Forces(par, terms=["lj"], cutoff=7.0)
    p, b = pos_tensor(pos, 1, PREC[prec], _dev()), box_tensor(box, 1, PREC[prec], _dev())
    torch.manual_seed(1)
    v = maxwell_boltzmann(par.masses.double(), 120, 1).to(PREC[prec]).to(_dev()).contiguous()
    t = f._pressure_terms(p, b, vel=v, masses=par.masses)
    ke = torch.zeros(1, dtype=torch.float64, device=_dev())
    m = par.masses.to(_dev()).reshape(-1).contiguous()
    L.check(L.load().tmdhip_kinetic_energy(L.dtype_code(PREC[prec]), 1, 64, v.data_ptr(), m.data_ptr(), ke.data_ptr(),
                                           C.c_void_p(torch.cuda.current_stream(_dev()).cuda_stream)))
    ek = float(ke.cpu()[0])
    print(f"64 atoms {prec}: sum M V^2 = {t[0, :3].sum()}, 2 E_kin = {2 * ek}")
    assert abs(t[0, :3].sum() - 2 * ek) <= 64 * EPS64 * 2 * ek
    sysm = M.system_of(par, ("lj",), f._excl_csr)
    assert len(sysm.off) == 65
    mm = M.nonbonded_model(_stored(pos, prec), box, sysm, ("lj",), 7.0, prec=prec)
    _check("64 bond-free atoms", t[0, 3:6], mm, prec)


# ---------------------------------------------------------------- virtual sites
@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_tip4p_sites_placed_by_the_call(prec):
    mol, pos, box, par, vs = _water("tip4p", 6, 3, prec)
    f = _forces(par, "lj_rf", 9.0, vs=vs)
    raw = pos.copy()
    raw[vs.sites] = 0.0  # the call places them
    p, b = pos_tensor(raw, 1, PREC[prec], _dev()), box_tensor(box, 1, PREC[prec], _dev())
    W = f.virial(p, b)[0]
    placed = p[0].cpu().double().numpy()
    assert np.abs(placed[vs.sites]).max() > 1.0  # (written in place, as compute() does)
    sysm = _sys(f, par, "lj_rf", vs)
    assert len(sysm.off) - 1 == mol.numAtoms // 4 and np.all(np.diff(sysm.off) == 4)
    _check("tip4p 864", W, _model(sysm, placed, box, "lj_rf", 9.0, prec), prec)


# ---------------------------------------------------------------- PME
# tests/test_gpu_pme.py's bars (fp64 GPU against host PME: energy 1e-10 of its scale, forces 1e-8 kcal/mol/A; fp32 against fp64:
# 2e-5 and 5e-3), scaled: the energy bar by the sum of |e(m) factor| of the modes, the force bar by sum_i |delta_i,a|
PME_ETOL = {"f64": 1e-10, "f32": 2e-5}
PME_FTOL = {"f64": 1e-8, "f32": 5e-3}


def _charged(prec):
    """The 648-atom box with a net charge of +0.7 e (the neutralising background has a value)."""
    from torchmd_amd.builders import tip3p_box, water_forcefield
    from torchmd_amd.parameters import Parameters

    key = ("charged", prec)
    if key not in _CASES:
        mol, pos, box = tip3p_box(6, seed=3)
        par = Parameters(water_forcefield(mol), mol, WATER_TERMS, precision=PREC[prec])
        par.charges[0] += 0.7
        _CASES[key] = (mol, np.asarray(pos, dtype=np.float64), np.asarray(box, dtype=np.float64), par, None)
    return _CASES[key]


@pytest.mark.parametrize("order", [4, 5, 6])
@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_pme_virial_against_model(prec, order):
    mol, pos, box, par, _ = _charged(prec)
    grid = (21, 25, 27)  # odd
    f = _forces(par, "lj_pme", 9.0, pme=True, pme_order=order, pme_grid=grid)
    p, b = pos_tensor(pos, 1, PREC[prec], _dev()), box_tensor(box, 1, PREC[prec], _dev())
    W = f.virial(p, b)[0]
    assert f.stats(p)["algorithm"] == "allpairs"
    sysm = M.system_of(par, ("lj", "electrostatics"), f._excl_csr)
    stored = _stored(pos, prec)
    boxs = torch.diagonal(b[0]).cpu().double().numpy()
    real = M.nonbonded_model(stored, boxs, sysm, ("lj", "electrostatics"), 9.0, prec=prec, ewald_beta=f.ewald_beta)
    rec = M.reciprocal_model(stored, boxs, sysm, f.ewald_beta, grid, order)
    want = real.W + rec.W
    bar = _bar(real, prec) + PME_ETOL[prec] * rec.S_modes + PME_FTOL[prec] * rec.S_delta
    print(f"PME order {order} {prec}: W = {W}, model {want} (real {real.W}, modes {rec.modes}, -delta.F {rec.correction}, background "
          f"{rec.background}), |dW| = {np.abs(W - want)}, bar {bar}")
    assert abs(rec.background) > 0.1 and (np.abs(W - want) <= bar).all()
    if prec == "f64":  # every part is resolved by the bar
        for part in (rec.modes, rec.correction, np.full(3, rec.background)):
            assert (np.abs(part) > 1e3 * bar).all()


# ---------------------------------------------------------------- determinism, more than 16 replicas
@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_seventeen_replicas_twenty_repeats_bit_identical(prec):
    mol, pos, box, par, _ = _water("tip3p", 4, 6, prec)  # 192 atoms
    R = 17
    rng = np.random.default_rng(0)
    allpos = np.stack([pos + 0.02 * r * rng.standard_normal(pos.shape) for r in range(R)])
    vel = 0.01 * rng.standard_normal(allpos.shape)
    f = _forces(par, "lj_rf", 6.0)
    p = torch.as_tensor(allpos, dtype=PREC[prec]).to(_dev()).contiguous()
    v = torch.as_tensor(vel, dtype=PREC[prec]).to(_dev()).contiguous()
    b = box_tensor(box, R, PREC[prec], _dev())
    first = f._pressure_terms(p, b, vel=v, masses=par.masses)
    for _ in range(19):
        assert np.array_equal(first.view(np.int64), f._pressure_terms(p, b, vel=v, masses=par.masses).view(np.int64))
    sysm = _sys(f, par, "lj_rf")
    for r in (0, 16):
        _check(f"192 x 17 replica {r}", first[r, 3:6], _model(sysm, p[r].cpu().double().numpy(), box, "lj_rf", 6.0, prec), prec)
    assert len({first[r].tobytes() for r in range(R)}) == R


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_list_path_repeats_bit_identical_two_replicas(prec, monkeypatch):
    monkeypatch.setenv("TMDHIP_LPA", "8")
    par, box, states, models, _, _ = _list_states(prec)
    f = _forces(par, "lj_rf", LIST_CUTOFF, algorithm="celllist")  # (AUTO takes the list from 2 048 atoms on)
    p = torch.as_tensor(np.stack([states["fresh"], states["aged"]]), dtype=PREC[prec]).to(_dev()).contiguous()
    b = box_tensor(box, 2, PREC[prec], _dev())
    first = f.virial(p, b)
    assert f.stats(p, 1)["algorithm"] == "celllist"
    for _ in range(19):
        assert np.array_equal(first.view(np.int64), f.virial(p, b).view(np.int64))
    _check("1536 x 2 replica 0", first[0], models["fresh"], prec)
    _check("1536 x 2 replica 1", first[1], models["aged"], prec)


# ---------------------------------------------------------------- large
def test_large_box_fp32_nothing_overflows():
    """N = 98 304 once in fp32 on the list path, against the model over EVERY row (the kernels return sums, not rows): its pairs
    come from a periodic k-d tree with a margin, the decision stays the model's.  Not a timing."""
    mol, pos, box, par, _ = _water("tip3p", 32, 0, "f32")
    f = _forces(par, "lj_rf", 6.0)
    p, b = pos_tensor(pos, 1, torch.float32, _dev()), box_tensor(box, 1, torch.float32, _dev())
    W = f.virial(p, b)[0]
    st = f.stats(p)
    assert st["algorithm"] == "celllist" and st["overflow"] == 0
    sysm = _sys(f, par, "lj_rf")
    stored = _stored(pos, "f32")
    boxs = torch.diagonal(b[0]).cpu().double().numpy()
    m = _model(sysm, stored, boxs, "lj_rf", 6.0, "f32", pairs=list(M.tree_pairs(stored, boxs, 6.01)))
    assert m.npairs > 4_000_000
    _check("98304 list", W, m, "f32")
    assert (np.abs(W - m.W) <= 1e-6 * np.abs(m.W)).all()  # (and nothing wrapped: the sums agree to a part in a million)


# ---------------------------------------------------------------- refusals
def test_c_refusals():
    from torchmd_amd import _lib as L

    mol, pos, box, par, _ = _water("tip3p", 4, 6, "f64")
    f = _forces(par, "lj_rf", 6.0)
    p, b = pos_tensor(pos, 1, torch.float64, _dev()), box_tensor(box, 1, torch.float64, _dev())
    eng = f._engine(p)
    lib = eng.lib
    m = par.masses.to(_dev()).reshape(-1).contiguous()
    out = np.zeros((1, 8))
    hb = np.ascontiguousarray(box.reshape(1, 3))
    st = C.c_void_p(torch.cuda.current_stream(_dev()).cuda_stream)

    def call(ctx=eng.ctx, pos_=p, mass=m, hbox=hb, out_=out):
        return lib.tmdhip_pressure(ctx, C.c_void_p(pos_.data_ptr()) if pos_ is not None else C.c_void_p(), C.c_void_p(),
                                   C.c_void_p(mass.data_ptr()) if mass is not None else C.c_void_p(),
                                   hbox.ctypes.data_as(C.POINTER(C.c_double)) if hbox is not None else None,
                                   out_.ctypes.data_as(C.POINTER(C.c_double)) if out_ is not None else None, st)

    assert call() < 0 and "not set" in L.last_error()  # molecules not set
    off, mem, _ = f._molecules()
    md = L.MoleculeDesc()
    md.struct_size = C.sizeof(L.MoleculeDesc)
    md.nmol = len(off) - 1
    md.offsets_host, md.members_host = off.ctypes.data_as(C.c_void_p), mem.ctypes.data_as(C.c_void_p)
    assert lib.tmdhip_set_molecules(None, C.byref(md)) < 0 and lib.tmdhip_set_molecules(eng.ctx, None) < 0
    md.struct_size -= 4
    assert lib.tmdhip_set_molecules(eng.ctx, C.byref(md)) < 0 and "size" in L.last_error()
    md.struct_size += 4
    twice = mem.copy()
    twice[1] = twice[0]
    md.members_host = twice.ctypes.data_as(C.c_void_p)
    assert lib.tmdhip_set_molecules(eng.ctx, C.byref(md)) < 0 and "two molecules" in L.last_error()
    beyond = mem.copy()
    beyond[5] = len(mem)
    md.members_host = beyond.ctypes.data_as(C.c_void_p)
    assert lib.tmdhip_set_molecules(eng.ctx, C.byref(md)) < 0 and "out of range" in L.last_error()
    md.members_host = mem.ctypes.data_as(C.c_void_p)
    assert call() < 0  # (still not set: every refused table left the context as it was)
    assert lib.tmdhip_set_molecules(eng.ctx, C.byref(md)) == 0
    assert call() == 0 and np.isfinite(out).all()
    for kw in (dict(ctx=None), dict(pos_=None), dict(mass=None), dict(hbox=None), dict(out_=None)):
        assert call(**kw) < 0 and "null" in L.last_error()
    zero = hb.copy()
    zero[0, 1] = 0.0
    assert call(hbox=zero) < 0 and "box edge" in L.last_error()
    massless = m.clone()
    massless[3:6] = 0.0
    assert call(mass=massless) < 0 and "no mass" in L.last_error()
    assert call() == 0


def test_c_refusal_of_a_context_with_passive_atoms():
    from torchmd_amd import _lib as L
    from torchmd_amd.builders import argon_forcefield, lj_box
    from torchmd_amd.forces import Forces
    from torchmd_amd.parameters import Parameters

    mol, pos, box = lj_box(4, seed=2)
    par = Parameters(argon_forcefield(mol), mol, ["lj"], precision=torch.float64)
    f = Forces(par, terms=["lj"], cutoff=7.0)
    p, b = pos_tensor(pos, 1, torch.float64, _dev()), box_tensor(box, 1, torch.float64, _dev())
    assert np.isfinite(f.virial(p, b)).all()
    f.update_atoms(par, nactive=32)
    eng = f._engine(p)
    off, mem = np.arange(65, dtype=np.int32), np.arange(64, dtype=np.int32)
    md = L.MoleculeDesc()
    md.struct_size, md.nmol = C.sizeof(L.MoleculeDesc), 64
    md.offsets_host, md.members_host = off.ctypes.data_as(C.c_void_p), mem.ctypes.data_as(C.c_void_p)
    assert eng.lib.tmdhip_set_molecules(eng.ctx, C.byref(md)) < 0 and "passive" in L.last_error()
    out, hb = np.zeros((1, 8)), np.ascontiguousarray(box.reshape(1, 3))
    m = par.masses.to(_dev()).reshape(-1).contiguous()
    rc = eng.lib.tmdhip_pressure(eng.ctx, C.c_void_p(p.data_ptr()), C.c_void_p(), C.c_void_p(m.data_ptr()),
                                 hb.ctypes.data_as(C.POINTER(C.c_double)), out.ctypes.data_as(C.POINTER(C.c_double)), C.c_void_p())
    assert rc < 0 and "passive" in L.last_error()
    with pytest.raises(ValueError, match="domain decomposition"):
        f.virial(p, b)


def test_python_refusals():
    from torchmd_amd.forces import Forces
    from torchmd_amd.integrator import Integrator
    from torchmd_amd.systems import System

    mol, pos, box, par, _ = _water("tip3p", 4, 6, "f64")
    f = _forces(par, "lj_rf", 6.0)
    p, b = pos_tensor(pos, 2, torch.float64, _dev()), box_tensor(box, 2, torch.float64, _dev())
    with pytest.raises(ValueError, match="vmap"):
        torch.vmap(lambda x: torch.as_tensor(f.virial(x[None], b[:1])))(p)
    zero = b.clone()
    zero[1, 2, 2] = 0.0
    with pytest.raises(ValueError, match="box edge"):
        f.virial(p, zero)
    s = System(mol.numAtoms, 1, torch.float64, _dev())
    s.set_positions(pos[:, :, None])
    s.set_box(box)
    integ = Integrator(s, f, 1.0, _dev(), batch=torch.zeros(mol.numAtoms, dtype=torch.int64))
    with pytest.raises(ValueError, match="batch"):
        integ.pressure()
    with pytest.raises(ValueError, match="batch"):
        integ.pressure_tensor()
    # an exclusion between two molecules
    from torchmd_amd.forces import build_exclusion_csr

    g = Forces(par, terms=["lj", "electrostatics"], cutoff=6.0, rfa=True)
    g._excl_csr = build_exclusion_csr(mol.numAtoms, [list(map(int, e)) for e in par.get_exclusions(("bonds", "angles", "1-4"))] + [[0, 3]])
    with pytest.raises(ValueError, match="two molecules"):
        g.virial(p, b)


# ---------------------------------------------------------------- a run is not perturbed
def test_pressure_between_steps_equals_compute_between_steps_bit_for_bit(monkeypatch):
    """fp32, the fused pair + step launch, the smallest box the planner puts on the cell-list path: step(10); pressure();
    step(10) leaves the bits of the twin that calls forces.compute() in the same place."""
    from torchmd_amd.integrator import Integrator, maxwell_boltzmann
    from torchmd_amd.systems import System

    monkeypatch.setenv("TMDHIP_LPA", "8")
    mol, pos, box, par, _ = _water("tip3p", 9, 4, "f32")  # 2 187 atoms: AUTO takes the list from 2 048 atoms on; L = 27.9
    from torchmd_amd.forces import Forces

    def run(between):
        f = Forces(par, terms=WATER_TERMS, cutoff=7.0, rfa=True)
        s = System(mol.numAtoms, 1, torch.float32, _dev())
        s.set_positions(pos[:, :, None])
        s.set_box(box)
        torch.manual_seed(3)
        s.set_velocities(maxwell_boltzmann(par.masses.double(), 300, 1).float())
        f.compute(s.pos, s.box, s.forces)
        torch.manual_seed(11)
        integ = Integrator(s, f, 1.0, _dev(), gamma=0.1, T=300.0)
        integ.step(10)
        mid = between(integ, f, s)
        out = integ.step(10)
        st = f.stats(s.pos)
        assert st["algorithm"] == "celllist" and st["steps_in_pair_launch"] > 0  # (the fused launch made the steps)
        return s.pos.cpu().numpy().copy(), s.vel.cpu().numpy().copy(), s.forces.cpu().numpy().copy(), out, mid, integ.replays

    a = run(lambda integ, f, s: integ.pressure())
    b = run(lambda integ, f, s: f.compute(s.pos, s.box, torch.zeros_like(s.forces)))
    for k in range(3):
        assert np.array_equal(a[k].view(np.int32), b[k].view(np.int32)), k
    assert np.array_equal(a[3][0], b[3][0]) and a[3][1] == b[3][1] and a[5] == b[5] == 0
    assert np.isfinite(a[4]).all() and abs(a[4][0]) < 1e5


# ---------------------------------------------------------------- independent of the model: -3V dU/dV
def _fd_case(name):
    # the seeds: the first of 1 .. 15 at which the numpy model counts the same pairs at volumes 1 -+ 1e-5, 1 -+ 5e-6 and 1 (at a
    # larger eps the differences of U carry less of U's own rounding, 1 ulp(U) / eps)
    if name == "allpairs_rf":
        mol, pos, box, par, vs = _water("tip3p", 6, 1, "f64")
        return par, pos, box, vs, "lj_rf", 9.0, {}, "allpairs"
    if name == "list_rf":
        mol, pos, box, par, vs = _water("tip3p", 8, 6, "f64")
        return par, pos, box, vs, "lj_rf", LIST_CUTOFF, dict(algorithm="celllist"), "celllist"
    if name == "tip4p":
        mol, pos, box, par, vs = _water("tip4p", 6, 15, "f64")
        return par, pos, box, vs, "lj_rf", 9.0, {}, "allpairs"
    if name == "pme5":
        mol, pos, box, par, vs = _water("tip3p", 6, 1, "f64")
        return par, pos, box, vs, "lj_pme", 9.0, dict(pme=True, pme_order=5, pme_grid=(21, 25, 27)), "allpairs"
    mol, pos, box, par, vs = _water("tip3p", 6, 1, "f64")
    return par, pos, box, vs, "lj_sw_exact", 9.0, {}, "allpairs"


@pytest.mark.parametrize("name", ["allpairs_rf", "list_rf", "pme5", "tip4p", "lj_switched_autograd_flavour"])
def test_virial_is_minus_3V_dU_dV_of_computes_energy(name):
    """fp64.  The test scales the molecules' mass-weighted centres and the box by (1 +- eps)^(1/3) in float64 itself and
    differences compute()'s total energy; eps is halved from 1e-5 until the pair count is the same at 1 - eps, 1 - eps / 2, 1,
    1 + eps / 2 and 1 + eps (an unswitched cutoff makes U jump, a reaction field makes dU/dr jump)."""
    par, pos, box, vs, tset, cutoff, kw, algo = _fd_case(name)
    f = _forces(par, tset, cutoff, vs=vs, **kw)
    sysm = _sys(f, par, tset, vs)
    if vs is not None:
        pos = pos.copy()
        vs.construct(pos)

    def state(lam):
        pp, bb = M.scale_molecules(pos, box, sysm, lam ** (1.0 / 3.0))
        return pos_tensor(pp, 1, torch.float64, _dev()), box_tensor(bb, 1, torch.float64, _dev())

    def energy(lam):
        p, b = state(lam)
        return float(f.compute(p, b, torch.zeros_like(p))[0]), f.count_pairs(p, b)[0]

    p0, b0 = state(1.0)
    W = f.virial(p0, b0)[0]
    assert f.stats(p0)["algorithm"] == algo
    n0 = f.count_pairs(p0, b0)[0]
    eps = 1e-5
    for _ in range(12):
        vals = {s: energy(1.0 + s * eps) for s in (-1.0, -0.5, 0.5, 1.0)}
        if all(v[1] == n0 for v in vals.values()):
            break
        eps /= 2
    else:
        pytest.fail("no eps with a constant pair count")
    fd1 = -3.0 * (vals[1.0][0] - vals[-1.0][0]) / (2 * eps)
    fd2 = -3.0 * (vals[0.5][0] - vals[-0.5][0]) / eps
    m = _model(sysm, pos, box, tset, cutoff, "f64", **(dict(ewald_beta=f.ewald_beta) if f.pme else {}))
    bar = 10 * abs(fd1 - fd2) + 64 * EPS64 * m.S.sum()
    print(f"{name}: eps {eps:.3g}, pairs {n0}, trace W = {W.sum()!r}, FD(eps) = {fd1!r}, FD(eps/2) = {fd2!r}, |d| = {abs(W.sum() - fd1):.3e}, bar {bar:.3e}")
    assert abs(W.sum() - fd1) <= bar
    assert abs(W.sum()) > 100 * bar  # (the bar resolves the value)


# ---------------------------------------------------------------- run.py
@pytest.mark.parametrize("with_pressure", [False, True])
def test_run_py_pressure_column(tmp_path, with_pressure):
    """The water example of tests/test_gpu_driver.py (its input files regenerated from tests/golden/water291.npz), 2 replicas."""
    import csv

    import yaml

    from test_gpu_driver import _write_pdb, _write_psf
    from torchmd_amd import run
    from torchmd_amd.builders import TIP3P_FF

    g = load("water291")
    psf, pdb, ff = tmp_path / "structure.psf", tmp_path / "structure.pdb", tmp_path / "water_forcefield.yaml"
    _write_psf(psf, g)
    _write_pdb(pdb, g)
    ff.write_text(yaml.safe_dump(TIP3P_FF))
    conf = {"structure": [str(psf), str(pdb)], "forcefield": str(ff), "forceterms": ["LJ", "Bonds", "Angles", "Electrostatics"],
            "cutoff": 7.3, "rfa": True, "replicas": 2, "precision": "double", "device": "cuda", "timestep": 1, "temperature": 300,
            "langevin_gamma": 0.1, "langevin_temperature": 300, "seed": 1, "steps": 20, "output_period": 10, "save_period": 20,
            "log_dir": str(tmp_path / "log"), "output": "output"}
    if with_pressure:
        conf["pressure"] = True
    cpath = tmp_path / "conf.yaml"
    cpath.write_text(yaml.safe_dump(conf))
    args = run.get_args(["--conf", str(cpath)])
    mol, system, forces = run.setup(args)
    captured, real = {}, run.Integrator

    class Spy(real):
        def __init__(self, *a, **k):
            super().__init__(*a, **k)
            captured["integ"] = self

    run.Integrator = Spy
    try:
        run.dynamics(args, mol, system, forces)
    finally:
        run.Integrator = real
    for k in range(2):
        with open(tmp_path / "log" / f"monitor_{k}.csv") as fh:
            rows = list(csv.DictReader(line for line in fh if not line.startswith("#")))
        assert len(rows) == 2
        if not with_pressure:
            assert list(rows[0]) == ["iter", "ns", "epot", "ekin", "etot", "T", "t"]
            continue
        assert list(rows[0]) == ["iter", "ns", "epot", "ekin", "etot", "T", "pressure", "t"]
        col = [float(r["pressure"]) for r in rows]
        again = captured["integ"].pressure()[k]  # the state of the last row
        print(f"run.py replica {k}: pressure column {col} bar, Integrator.pressure() at the last row {again}")
        assert np.isfinite(col).all() and col[-1] == again and col[0] != col[1]
