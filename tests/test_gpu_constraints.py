"""Constrained MD on the GPU (run with `-m gpu` on an MI355X): rigid waters (SETTLE) and X-H bonds (SHAKE / RATTLE) through
`Integrator(..., constraints=...)` and tmdhip_md_run's constrained kernel, against the fp64 host reference of
tests/_constraints.py, the oracle, and the invariants of constrained dynamics."""

import ctypes as C
import os

import numpy as np
import pytest
import torch
import yaml

import _constraints as H
import _philox as P
from _golden import GoldenParameters, load
from oracle import torchmd_oracle as orc

pytestmark = pytest.mark.gpu

ALL_TERMS = ["bonds", "angles", "dihedrals", "impropers", "1-4", "electrostatics", "lj"]
WATER_TERMS = ["lj", "electrostatics", "bonds", "angles"]
FTOL = {"f64": 1e-8, "f32": 3e-4}  # the suite's force bars against the oracle (test_gpu_parity.py)
CONS_TOL = {"f32": (3e-5, 1e-5), "f64": (1e-10, 1e-10)}  # bond length (relative), velocity along the bond / rms


def _dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _golden(name):
    g = load(name)
    if name == "water291":
        return g, WATER_TERMS, dict(cutoff=7.3, rfa=True)
    return g, ALL_TERMS, dict(cutoff=9.0, switch_dist=7.5, rfa=True)


def _constrained_start(cs, m, x, T=300.0, seed=0):
    """Positions SHAKEn onto the constraints, Maxwell-Boltzmann velocities projected onto them (host, fp64)."""
    us = H.units(cs)
    x = H.shake(np.array(x, dtype=np.float64), np.array(x, dtype=np.float64), m, us)
    rng = np.random.default_rng(seed)
    v = rng.normal(size=x.shape) * np.sqrt(T * 0.001987191 / m)[:, None]
    return x, H.project(x, v, m, us)


def _golden_system(name, mode, prec, R=1, langevin=False, seed=0):
    from torchmd_amd.constraints import find_constraints
    from torchmd_amd.forces import Forces
    from torchmd_amd.integrator import Integrator
    from torchmd_amd.systems import System

    g, terms, kw = _golden(name)
    dt = torch.float64 if prec == "f64" else torch.float32
    par = GoldenParameters(g, dt)
    m = par.masses.reshape(-1).double().numpy()
    cs = find_constraints(m, par.bond_params, par.angle_params, mode)
    x, v = _constrained_start(cs, m, g["pos"], seed=seed)
    n = len(m)
    s = System(n, R, dt, _dev())
    s.set_positions(np.repeat(x[:, :, None], 1, axis=2))
    if R > 1:
        s.pos[:] = torch.as_tensor(x).to(dt)
    s.set_box(g["box"])
    s.set_velocities(torch.as_tensor(np.repeat(v[None], R, axis=0)))
    f = Forces(par, terms=terms, **kw)
    f.compute(s.pos, s.box, s.forces)
    integ = Integrator(s, f, 2.0, _dev(), gamma=5.0 if langevin else None, T=300.0 if langevin else None, constraints=mode)
    return g, par, terms, kw, cs, m, s, f, integ


def _oracle_forces(par, x, box, terms, kw):
    ex = orc.exclusion_pairs(par)
    pairs = orc.candidate_pairs(x, np.asarray(box, dtype=np.float64), kw["cutoff"] + 2.0, ex)
    bt = torch.diag(torch.as_tensor(np.asarray(box, dtype=np.float64)))[None]
    _, F, _ = orc.compute(par, torch.as_tensor(x)[None], bt, terms, pairs=pairs, **kw)
    return F[0].double().numpy()


def _noise(integ, step, n):
    """The thermostat's noise of global step `step`, rows 0 .. n-1: the device's own fp32 variates (tmdhip_normal_fill, held
    to tests/_philox.py's host Philox by test_gpu_langevin.py) — the host's float64 Box-Muller differs by ~1e-7."""
    from torchmd_amd import _lib as L

    out = torch.empty(3 * n, dtype=torch.float64, device=_dev())
    L.check(L.load().tmdhip_normal_fill(L.dtype_code(torch.float64), 3 * n, out.data_ptr(), C.c_uint64(integ._seed),
                                        C.c_uint64(step), C.c_void_p(torch.cuda.current_stream().cuda_stream)), "tmdhip_normal_fill")
    g = out.cpu().numpy().reshape(n, 3)
    h = np.stack(P.normal3(integ._seed, step, np.arange(n, dtype=np.uint64)), axis=1)
    assert np.abs(g - h).max() < 2e-5 * (1 + np.abs(h).max())
    return g


# ----------------------------------------------------------------------------- 1. one step, five steps against the host
@pytest.mark.parametrize("langevin", [False, True])
@pytest.mark.parametrize("name,mode", [("water291", "water"), ("ala2", "hbonds")])
def test_one_step_equals_the_host(name, mode, langevin):
    g, par, terms, kw, cs, m, s, f, integ = _golden_system(name, mode, "f64", langevin=langevin)
    us = H.units(cs)
    x0, v0, f0 = (t[0].cpu().double().numpy() for t in (s.pos, s.vel, s.forces))
    integ.step(1)
    dt = integ.dt
    x1, vh = H.first_half(x0, v0, f0, m, dt, us)
    xg = s.pos[0].cpu().numpy()
    assert np.abs(xg - x1).max() < 1e-9, np.abs(xg - x1).max()
    extra = {}
    if langevin:
        extra = dict(gamma=integ.gamma, vcoeff=integ.vcoeff.reshape(-1).cpu().double().numpy(), noise=_noise(integ, 0, len(m)))
    v1 = H.second_half(x1, vh, s.forces[0].cpu().double().numpy(), m, dt, us, **extra)
    vg = s.vel[0].cpu().numpy()
    assert np.abs(vg - v1).max() < 1e-9 * np.abs(v1).max(), np.abs(vg - v1).max()

    # five steps in one call (the interior kernel: second kick and first half step fused), oracle forces in between
    g, par, terms, kw, cs, m, s, f, integ = _golden_system(name, mode, "f64", langevin=langevin)
    x, v, fx = (t[0].cpu().double().numpy() for t in (s.pos, s.vel, s.forces))
    integ.step(5)
    for k in range(5):
        x, vh = H.first_half(x, v, fx, m, dt, us)
        fx = _oracle_forces(par, x, g["box"], terms, kw)
        if langevin:
            extra["noise"] = _noise(integ, k, len(m))
        v = H.second_half(x, vh, fx, m, dt, us, **extra)
    ex, ev = np.abs(s.pos[0].cpu().numpy() - x).max(), np.abs(s.vel[0].cpu().numpy() - v).max() / np.abs(v).max()
    print(f"{name} {mode} langevin={langevin}: 5 steps, max|dx| = {ex:.2e} A, max|dv|/max|v| = {ev:.2e}")
    assert ex < 1e-9 and ev < 1e-9


# ----------------------------------------------------------------------------- 2. invariants at scale
def _water_box(nside, prec, seed=0, pme=False, R=1, T=300.0, gamma=1.0, mode="water"):
    from torchmd_amd.builders import tip3p_box, water_forcefield
    from torchmd_amd.constraints import find_constraints
    from torchmd_amd.forces import Forces
    from torchmd_amd.integrator import Integrator, maxwell_boltzmann
    from torchmd_amd.parameters import Parameters
    from torchmd_amd.systems import System

    dt = torch.float64 if prec == "f64" else torch.float32
    mol, pos, box = tip3p_box(nside, seed=seed)
    par = Parameters(water_forcefield(mol), mol, WATER_TERMS, precision=dt)
    s = System(mol.numAtoms, R, dt, _dev())
    s.set_positions(pos[:, :, None])
    if R > 1:
        s.pos[:] = torch.as_tensor(pos).to(dt)
    s.set_box(box)
    torch.manual_seed(seed)
    s.set_velocities(maxwell_boltzmann(par.masses, T, R))
    kw = dict(cutoff=9.0, pme=True) if pme else dict(cutoff=9.0, rfa=True)
    f = Forces(par, terms=WATER_TERMS, **kw)
    f.compute(s.pos, s.box, s.forces)
    integ = Integrator(s, f, 2.0, _dev(), gamma=gamma, T=T if gamma else None, constraints=mode)
    cs = find_constraints(par.masses, par.bond_params, par.angle_params, mode)
    return mol, par, box, s, f, integ, cs


def _check_constraints(s, cs, prec, what):
    pairs, d = cs.pairs()
    worst = (0.0, 0.0)
    for r in range(s.pos.shape[0]):
        dr, dv = H.residuals(s.pos[r].cpu().double().numpy(), s.vel[r].cpu().double().numpy(), pairs, d)
        worst = (max(worst[0], dr), max(worst[1], dv))
    lim = CONS_TOL[prec]
    assert worst[0] <= lim[0] and worst[1] <= lim[1], (what, worst)
    return worst


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_invariants_at_scale(prec):
    from _oracle_sample import periodic_count, periodic_tree, sample_pairs

    mol, par, box, s, f, integ, cs = _water_box(16, prec)
    worst = (0.0, 0.0)
    for call in range(20):
        _, pot, T = integ.step(100)
        w = _check_constraints(s, cs, prec, f"call {call}")
        worst = (max(worst[0], w[0]), max(worst[1], w[1]))
        assert np.isfinite(pot).all()
    st = f.stats(s.pos)
    assert st["algorithm"] == "celllist" and st["n_rebuilds"] > 1, st
    print(f"tip3p_box(16) {prec}: 2000 steps at 2 fs, worst bond error {worst[0]:.2e}, velocity along bonds {worst[1]:.2e}, "
          f"{st['n_rebuilds']} rebuilds, T = {T[0]:.1f} K")
    p = s.pos.detach().cpu()
    tree = periodic_tree(p[0].double().numpy(), box)
    n = p.shape[1]
    pick, pairs = sample_pairs(tree, n, 2000, 3, 9.5)
    ex = orc.exclusion_pairs(par)  # (the oracle takes the candidate pairs as given: the bonded pairs go)
    exk = np.minimum(ex[:, 0], ex[:, 1]) * n + np.maximum(ex[:, 0], ex[:, 1])
    keep = ~np.isin(pairs[:, 0] * n + pairs[:, 1], exk)
    _, F, _ = orc.compute(par, p, s.box.cpu(), WATER_TERMS, pairs=pairs[keep], cutoff=9.0, rfa=True)
    err = (s.forces[0].cpu()[pick] - F[0, pick]).abs().max().item()
    assert err < FTOL[prec], err
    # (the GPU counts non-excluded pairs; every excluded pair — within a water — is inside the cutoff)
    assert f.count_pairs(s.pos, s.box)[0] + len(np.unique(exk)) == periodic_count(p[0], box, 9.0, tree=tree)


# ----------------------------------------------------------------------------- 3. temperature with the ndof correction
def test_langevin_temperature_counts_constrained_dof():
    mol, par, box, s, f, integ, cs = _water_box(12, "f32", seed=2, R=2, gamma=1.0)
    Ts = []
    for call in range(200):
        _, _, T = integ.step(100)
        if call >= 50:
            Ts.append(T)
    mean = np.mean(np.asarray(Ts), axis=0)
    print(f"tip3p_box(12) rigid, Langevin 300 K, 2 fs: mean T over steps 5000-20000 = {mean}")
    assert np.all(np.abs(mean - 300.0) < 9.0), mean


# ----------------------------------------------------------------------------- 4. second-order energy conservation
def _cluster_drift(dt_fs, nsteps, every):
    from torchmd_amd.builders import tip3p_box, water_forcefield
    from torchmd_amd.constraints import find_constraints
    from torchmd_amd.forces import Forces
    from torchmd_amd.integrator import Integrator
    from torchmd_amd.parameters import Parameters
    from torchmd_amd.systems import System

    mol, pos, _ = tip3p_box(4, seed=1)
    par = Parameters(water_forcefield(mol), mol, WATER_TERMS, precision=torch.float64)
    m = par.masses.reshape(-1).double().numpy()
    cs = find_constraints(m, par.bond_params, par.angle_params, "water")
    x, v = _constrained_start(cs, m, pos, T=300.0, seed=3)
    s = System(mol.numAtoms, 1, torch.float64, _dev())
    s.set_positions(x[:, :, None])
    s.set_box(np.zeros(3))
    s.set_velocities(torch.as_tensor(v[None]))
    f = Forces(par, terms=WATER_TERMS, algorithm="allpairs")
    e0 = f.compute(s.pos, s.box, s.forces)[0] + 0.5 * float(np.sum(m[:, None] * v * v))
    integ = Integrator(s, f, dt_fs, _dev(), constraints="water")
    dev = 0.0
    for _ in range(nsteps // every):
        ek, pot, _ = integ.step(every)
        dev = max(dev, abs(float(ek[0]) + pot[0] - e0))
    return dev


def test_energy_conservation_is_second_order():
    d2 = _cluster_drift(2.0, 200, 5)
    d1 = _cluster_drift(1.0, 400, 10)
    print(f"64 rigid waters, NVE fp64, 400 fs: max|E - E0| = {d2:.3e} at 2 fs, {d1:.3e} at 1 fs, ratio {d2 / d1:.2f}")
    assert 3.0 <= d2 / d1 <= 5.5, (d2, d1)


# ----------------------------------------------------------------------------- 5. replicas
def test_replicas_allpairs():
    _, _, _, _, cs, m, s3, f3, i3 = _golden_system("ala2", "hbonds", "f64", R=3)
    _, _, _, _, _, _, s1, f1, i1 = _golden_system("ala2", "hbonds", "f64", R=1)
    for _ in range(2):
        i3.step(10)
        i1.step(10)
    p = s3.pos.cpu().numpy()
    # (the all-pairs kernel adds its forces with atomics: its replicas agree to rounding, not bit for bit, with or without
    # constraints; the cell-list path below is bit-identical)
    assert np.abs(p[0] - p[1]).max() < 1e-10 and np.abs(p[0] - p[2]).max() < 1e-10
    assert np.abs(p[0] - s1.pos[0].cpu().numpy()).max() < 1e-9


def test_replicas_celllist():
    from torchmd_amd.integrator import Integrator

    _, _, _, s3, f3, _, cs = _water_box(12, "f64", seed=4, R=3, gamma=None)
    _, _, _, s1, f1, _, _ = _water_box(12, "f64", seed=4, R=1, gamma=None)
    s3.vel[:] = s1.vel[0]
    f3.compute(s3.pos, s3.box, s3.forces)
    i3 = Integrator(s3, f3, 2.0, _dev(), constraints="water")
    i1 = Integrator(s1, f1, 2.0, _dev(), constraints="water")
    for _ in range(2):
        i3.step(10)
        i1.step(10)
    p = s3.pos.cpu().numpy()
    assert np.array_equal(p[0], p[1]) and np.array_equal(p[0], p[2])
    assert np.abs(p[0] - s1.pos[0].cpu().numpy()).max() < 1e-9
    assert f3.stats(s3.pos)["algorithm"] == "celllist"


# ----------------------------------------------------------------------------- 6. PME with rigid water
def test_pme_with_rigid_water():
    mol, par, box, s, f, integ, cs = _water_box(12, "f32", seed=5, pme=True)
    for call in range(5):
        ek, pot, T = integ.step(100)
        assert np.isfinite(ek).all() and np.isfinite(pot).all()
        _check_constraints(s, cs, "f32", f"PME call {call}")
    assert f.stats(s.pos)["pme_evaluations"] > 0


# ----------------------------------------------------------------------------- 7. start-up projection
def test_startup_projection():
    from torchmd_amd.integrator import maxwell_boltzmann

    mol, par, box, s, f, integ, cs = _water_box(8, "f64", seed=6, gamma=None)
    g = torch.Generator().manual_seed(7)
    s.pos.add_((0.05 * torch.randn(s.pos.shape, generator=g, dtype=torch.float64)).to(s.pos))
    torch.manual_seed(8)
    s.set_velocities(maxwell_boltzmann(par.masses, 300, 1))
    integ.step(1)
    _check_constraints(s, cs, "f64", "after the start-up projection")
    fresh = torch.zeros_like(s.forces)
    f.compute(s.pos, s.box, fresh)
    assert (fresh - s.forces).abs().max().item() < 1e-8


# ----------------------------------------------------------------------------- 8. run.py
def test_run_py_rigid_water(tmp_path):
    import test_gpu_driver as D
    from torchmd_amd import run as driver
    from torchmd_amd.builders import TIP3P_FF

    g = load("water291")
    psf, pdb, ff = tmp_path / "structure.psf", tmp_path / "structure.pdb", tmp_path / "water_forcefield.yaml"
    D._write_psf(psf, g)
    D._write_pdb(pdb, g)
    ff.write_text(yaml.safe_dump(TIP3P_FF))
    conf = {
        "structure": [str(psf), str(pdb)], "forcefield": str(ff), "forceterms": ["LJ", "Bonds", "Angles", "Electrostatics"],
        "cutoff": 7.3, "rfa": True, "replicas": 1, "precision": "single", "device": "cuda", "timestep": 2,
        "temperature": 300, "langevin_gamma": 5.0, "langevin_temperature": 300, "seed": 1, "steps": 2000,
        "output_period": 100, "save_period": 0, "log_dir": str(tmp_path / "log"), "output": "output", "constraints": "water",
    }
    cpath = tmp_path / "conf.yaml"
    cpath.write_text(yaml.safe_dump(conf))
    driver.main(["--conf", str(cpath)])
    rows = (tmp_path / "log" / "monitor_0.csv").read_text().strip().splitlines()
    head = rows[0].split(",")
    T = np.array([float(dict(zip(head, r.split(",")))["T"]) for r in rows[1:]])
    print(f"run.py, rigid water291 at 2 fs: mean T over the second half {T[len(T) // 2:].mean():.1f} K")
    assert len(T) == 20 and np.isfinite(T).all() and abs(T[len(T) // 2:].mean() - 300.0) < 45.0
    assert os.path.exists(tmp_path / "log" / "input.yaml")
