"""Smooth PME on the GPU (Forces(..., pme=True)) against the host references of tests/_ewald.py.

fp64 GPU against host PME with the same beta, grid and order: the discretised algorithm reproduced to rounding.  fp32
against fp64 GPU on the same inputs.  Classic Ewald and the NaCl Madelung constant pin the physics.  The remaining tests
cover every entry point (compute, the MD loop, autograd), determinism, replicas, box changes and the argument checks.
"""

import math

import numpy as np
import pytest
import torch

import _ewald as E
import _golden as G

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
EXCL = ("bonds", "angles", "1-4")


def _atomic_par(q, dtype=torch.float64):
    n = len(q)
    g = {"par_charges": np.asarray(q, np.float64), "par_masses": np.full(n, 22.99), "par_types": np.zeros(n, np.int64)}
    return G.GoldenParameters(g, precision=dtype, device=DEV)


def _box_t(box, R, dtype):
    return G.box_tensor(box, R, dtype, DEV)


def _gpu(par, pos, box, terms, dtype, R=1, **kw):
    from torchmd_amd.forces import Forces

    fo = Forces(par, terms=terms, **kw)
    p = G.pos_tensor(pos, R, dtype, DEV)
    f = torch.zeros_like(p)
    e = fo.compute(p, _box_t(box, R, dtype), f, returnDetails=True)
    return fo, e, f.double().cpu().numpy()


def _host_excl(par, natoms):
    return [tuple(x) for x in par.get_exclusions(EXCL)] if natoms else []


def _host_cutoff_coulomb(pos, q, box, cutoff, excl):
    return E.real_space(pos, q, box, 0.0, cutoff, excl)


# ---- systems -------------------------------------------------------------------------------------------------------------
def _ions(dtype=torch.float64, n=200, seed=0, net=0):
    box = np.array([30.0, 31.0, 32.0])
    pos, q = E.random_ions(n, box, seed=seed, net=net, min_dist=2.2)
    return _atomic_par(q, dtype), pos, q, box, ["electrostatics"], 9.0, []


def _water(dtype=torch.float64):
    g = G.load("water291")
    par = G.GoldenParameters(g, precision=dtype, device=DEV)
    return par, g["pos"], g["par_charges"], g["box"], ["electrostatics"], 7.3, _host_excl(par, 1)


def _ala2(dtype=torch.float64):
    g = G.load("ala2")
    par = G.GoldenParameters(g, precision=dtype, device=DEV)
    return par, g["pos"], g["par_charges"], g["box"], ["electrostatics"], 9.0, _host_excl(par, 1)


def _tip3p(dtype=torch.float64, nside=16):
    from torchmd_amd.builders import tip3p_box, water_forcefield
    from torchmd_amd.parameters import Parameters

    mol, pos, box = tip3p_box(nside, seed=0)
    par = Parameters(water_forcefield(mol), mol, ["lj", "electrostatics", "bonds", "angles"], precision=dtype, device=DEV)
    q = par.charges.double().cpu().numpy()
    excl = [tuple(x) for x in par.get_exclusions(EXCL)]
    return par, np.asarray(pos, np.float64), q, np.asarray(box, np.float64), ["electrostatics"], 9.0, excl


SYSTEMS = {"ions": _ions, "water": _water, "ala2": _ala2, "tip3p16": _tip3p}
_HOST = {}


def _host_pme(name, beta, grid, order):
    key = (name, beta, grid, order)
    if key not in _HOST:
        par, pos, q, box, terms, rc, excl = SYSTEMS[name]()
        _HOST[key] = E.pme(pos, q, box, beta, rc, grid, order, excl)
    return _HOST[key]


# ---- fp64 GPU == host PME ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(SYSTEMS))
def test_fp64_gpu_pme_matches_host_pme(name):
    par, pos, q, box, terms, rc, excl = SYSTEMS[name]()
    fo, e, f = _gpu(par, pos, box, terms, torch.float64, cutoff=rc, pme=True)
    beta, grid = fo.ewald_beta, fo.pme_grid
    assert abs(beta - E.ewald_beta(rc, 5e-4)) < 1e-15
    eh, fh = _host_pme(name, beta, grid, 5)
    # 1e-10 of the total.  tip3p_box(16) is a lattice of randomly oriented molecules: its total (126 kcal/mol) is what is left
    # of parts of 2.3e5 (the self term) and 1e-10 of it lies below the fp64 rounding of those parts (~1e-13 of 2.3e5 = 2e-8,
    # observed 1.6e-8); there the bound is 1e-12 of the largest part instead, about 15x the observed difference
    eself = abs(E.self_and_background(q, box, beta))
    bound = 1e-10 * abs(eh) if abs(eh) > 1e-2 * eself else 1e-12 * eself
    print(f"energy [{name}]: |dE| = {abs(e[0]['electrostatics'] - eh):.2e}, total {eh:.6e}, self term {eself:.3e}")
    assert abs(e[0]["electrostatics"] - eh) <= bound, (e[0]["electrostatics"], eh)
    assert np.abs(f[0] - fh).max() <= 1e-8, np.abs(f[0] - fh).max()
    if name == "tip3p16":
        assert fo.stats(G.pos_tensor(pos, 1, torch.float64, DEV))["algorithm"] == "celllist"


def test_fp64_all_terms_alanine_dipeptide():
    """All seven terms with 1-4 pairs: PME changes the electrostatics term by exactly host (PME - cutoff Coulomb)."""
    par, pos, q, box, _, rc, excl = _ala2()
    terms = ["bonds", "angles", "dihedrals", "impropers", "1-4", "electrostatics", "lj"]
    fo, e1, f1 = _gpu(par, pos, box, terms, torch.float64, cutoff=rc, pme=True)
    _, e0, f0 = _gpu(par, pos, box, terms, torch.float64, cutoff=rc)
    eh, fh = _host_pme("ala2", fo.ewald_beta, fo.pme_grid, 5)
    ec, fc = _host_cutoff_coulomb(pos, q, box, rc, excl)
    for t in terms:
        if t != "electrostatics":
            assert abs(e1[0][t] - e0[0][t]) <= 1e-10 * max(1.0, abs(e0[0][t])), t
    assert abs((e1[0]["electrostatics"] - e0[0]["electrostatics"]) - (eh - ec)) <= 1e-10 * abs(eh)
    assert np.abs((f1[0] - f0[0]) - (fh - fc)).max() <= 1e-8


# fp32 against fp64 GPU PME.  Observed on an MI355X: forces <= 6.5e-5 kcal/mol/A (ions, water291, alanine dipeptide) and
# 2.5e-4 (tip3p_box(16)); energies <= 1.5e-7 of the self term (the largest part of the sum).  Bounds: the fp32 energy to
# 2e-5 relative and forces to 5e-3 kcal/mol/A, the tolerances the project holds fp32 pair forces to elsewhere, about 20x the
# observation.
@pytest.mark.parametrize("name", list(SYSTEMS))
def test_fp32_against_fp64(name):
    par64, pos, q, box, terms, rc, excl = SYSTEMS[name]()
    par32 = SYSTEMS[name](torch.float32)[0]
    _, e64, f64 = _gpu(par64, pos, box, terms, torch.float64, cutoff=rc, pme=True)
    _, e32, f32 = _gpu(par32, pos, box, terms, torch.float32, cutoff=rc, pme=True)
    scale = max(abs(e64[0]["electrostatics"]), abs(E.self_and_background(q, box, E.ewald_beta(rc, 5e-4))))
    de, df = abs(e32[0]["electrostatics"] - e64[0]["electrostatics"]) / scale, np.abs(f32 - f64).max()
    print(f"fp32 vs fp64 [{name}]: energy {de:.2e} of the self term, forces {df:.2e} kcal/mol/A")
    assert de <= 2e-5
    assert df <= 5e-3


# ---- the physics --------------------------------------------------------------------------------------------------------
def test_gpu_reproduces_the_madelung_constant():
    r0 = 2.82
    pos, q, box = E.nacl_lattice(r0, cells=4)  # 512 ions, L = 22.56 A
    fo, e, f = _gpu(_atomic_par(q), pos, box, ["electrostatics"], torch.float64, cutoff=11.0, pme=True, ewald_tolerance=1e-8,
                    pme_order=6, pme_grid=(64, 64, 64))
    m = -e[0]["electrostatics"] / (len(q) / 2) * r0 / E.KE
    assert abs(m - E.NACL_MADELUNG) <= 1e-6 * E.NACL_MADELUNG, m


def test_rms_force_error_against_ewald():
    """delta = 5e-4: RMS force error against converged Ewald <= 5e-4 of the RMS force; delta = 1e-6: at least 10x smaller."""
    par, pos, q, box, terms, rc, _ = _ions(n=120, seed=2)
    _, fE = E.ewald(pos, q, box, 0.3, nimg=2, kmax=16)
    rms = np.sqrt(np.mean(fE**2))
    err = {}
    for tol in (5e-4, 1e-6):
        _, _, f = _gpu(par, pos, box, terms, torch.float64, cutoff=rc, pme=True, ewald_tolerance=tol)
        err[tol] = np.sqrt(np.mean((f[0] - fE) ** 2)) / rms
    print(f"RMS force error / RMS force: {err}")
    assert err[5e-4] <= 5e-4, err
    assert err[1e-6] * 10 <= err[5e-4], err


def test_net_charged_box_matches_host():
    """One Na+ in water: the neutralising background term."""
    par, pos, q, box, terms, rc, excl = _water()
    q2 = np.concatenate([q, [1.0]])
    pos2 = np.concatenate([pos, [[0.5, 0.5, 0.5]]])
    par2 = _atomic_par(q2)
    par2.get_exclusions = lambda types=EXCL: [list(e) for e in excl]  # the water molecules' exclusions, the ion has none
    from torchmd_amd.forces import Forces

    fo = Forces(par2, terms=["electrostatics"], cutoff=rc, pme=True)
    p = G.pos_tensor(pos2, 1, torch.float64, DEV)
    f = torch.zeros_like(p)
    e = fo.compute(p, _box_t(box, 1, torch.float64), f, returnDetails=True)
    eh, fh = E.pme(pos2, q2, box, fo.ewald_beta, rc, fo.pme_grid, 5, excl)
    assert abs(e[0]["electrostatics"] - eh) <= 1e-10 * abs(eh)
    assert np.abs(f[0].double().cpu().numpy() - fh).max() <= 1e-8


# ---- paths ---------------------------------------------------------------------------------------------------------------
def test_celllist_and_allpairs_agree():
    par, pos, q, box, _, rc, _ = _tip3p(nside=16)
    terms = ["lj", "electrostatics", "bonds", "angles"]
    fa, ea, Fa = _gpu(par, pos, box, terms, torch.float64, cutoff=rc, pme=True, algorithm="allpairs")
    fc, ec, Fc = _gpu(par, pos, box, terms, torch.float64, cutoff=rc, pme=True, algorithm="celllist")
    for t in terms:
        assert abs(ea[0][t] - ec[0][t]) <= 1e-10 * max(1.0, abs(ec[0][t])), t
    assert np.abs(Fa - Fc).max() <= 1e-10 * max(1.0, np.abs(Fc).max())


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_deterministic_and_replicas_identical(dtype):
    from torchmd_amd.forces import Forces

    par, pos, q, box, _, rc, _ = _tip3p(dtype, nside=16)
    terms = ["lj", "electrostatics", "bonds", "angles"]
    fo = Forces(par, terms=terms, cutoff=rc, pme=True)
    p = G.pos_tensor(pos, 1, dtype, DEV)
    b = _box_t(box, 1, dtype)
    f1, f2 = torch.zeros_like(p), torch.zeros_like(p)
    e1 = fo.compute(p, b, f1, returnDetails=True)
    e2 = fo.compute(p, b, f2, returnDetails=True)
    assert torch.equal(f1, f2)
    # (the pair kernels' energy rows are filled with atomics, so the real-space energy may differ in its last bits)
    assert abs(e1[0]["electrostatics"] - e2[0]["electrostatics"]) <= 1e-12 * abs(e1[0]["lj"])
    p3 = G.pos_tensor(pos, 3, dtype, DEV)
    f3 = torch.zeros_like(p3)
    e3 = fo.compute(p3, _box_t(box, 3, dtype), f3, returnDetails=True)
    for r in range(3):
        # (a context of three replicas may pick other lanes per atom for its pair kernel than a context of one: rows of the
        # same context are compared)
        assert torch.equal(f3[r], f3[0])
        assert abs(e3[r]["electrostatics"] - e3[0]["electrostatics"]) <= 1e-12 * abs(e3[0]["lj"])
        assert fo.stats(p3, r)["pme_evaluations"] == 1


def test_two_boxes_each_match_host():
    from torchmd_amd.forces import Forces

    par, pos, q, box, terms, rc, excl = _ions(n=150, seed=4)
    fo = Forces(par, terms=terms, cutoff=rc, pme=True)
    p = G.pos_tensor(pos, 1, torch.float64, DEV)
    for scale in (1.0, 1.03, 1.0):
        bx = box * scale
        f = torch.zeros_like(p)
        e = fo.compute(p, _box_t(bx, 1, torch.float64), f, returnDetails=True)
        eh, fh = E.pme(pos, q, bx, fo.ewald_beta, rc, fo.pme_grid, 5, excl)
        assert abs(e[0]["electrostatics"] - eh) <= 1e-10 * abs(eh), scale
        assert np.abs(f[0].cpu().numpy() - fh).max() <= 1e-8, scale


def test_autograd_equals_explicit_forces():
    from torchmd_amd.forces import Forces

    par, pos, q, box, _, rc, _ = _water()
    terms = ["lj", "electrostatics", "bonds", "angles"]
    fo = Forces(par, terms=terms, cutoff=rc, pme=True)
    b = _box_t(box, 1, torch.float64)
    p = G.pos_tensor(pos, 1, torch.float64, DEV)
    f = torch.zeros_like(p)
    fo.compute(p, b, f)
    pg = p.clone().requires_grad_(True)
    ef = torch.zeros_like(p)
    fo.compute(pg, b, ef, explicit_forces=False)
    assert torch.allclose(ef, f, rtol=0, atol=1e-10)
    pv = p.clone().requires_grad_(True)
    tot = fo.compute(pv, b, None, toNumpy=False)
    (g,) = torch.autograd.grad(tot.sum(), pv)
    assert torch.allclose(-g, f, rtol=0, atol=1e-10)
    # torch.vmap over replicas
    v = torch.vmap(lambda x: fo.compute(x, b, None, toNumpy=False))(p[None].repeat(2, 1, 1, 1))
    assert abs(float(v[0, 0].detach()) - float(tot[0].detach())) <= 1e-9 * abs(float(tot[0].detach()))


def _python_nve(fo, par, pos, vel, box, niter, dt_fs):
    """`compute` + host velocity Verlet (reference integrator.py:61-74); returns positions, velocities, forces and the
    potential energy of the last positions per replica."""
    from torchmd_amd.integrator import TIMEFACTOR

    dt = dt_fs / TIMEFACTOR
    m = par.masses.double().to(DEV).reshape(1, -1, 1)
    x = pos.clone()
    v = vel.clone()
    f = torch.zeros_like(x)
    fo.compute(x, box, f)
    for _ in range(niter):
        x = x + v * dt + 0.5 * f / m * dt * dt
        v = v + 0.5 * dt * f / m
        f = torch.zeros_like(x)
        pot = fo.compute(x, box, f)
        v = v + 0.5 * dt * f / m
    return x, v, f, np.asarray(pot)


def _integrator_against_loop(par, pos, box, rc, R, dt_fs, **kw):
    """Integrator.step (tmdhip_md_run) with PME in fp64 NVE, in calls of 1, 7 and 50 steps, against a Python loop of
    `compute` + host velocity Verlet on a Forces object of its own: positions, velocities and forces to 1e-9 (forces
    1e-8), the potential energy of the last step to 1e-10 of the self term.  R > 1: replicas with their own velocities."""
    from torchmd_amd.forces import Forces
    from torchmd_amd.integrator import Integrator, maxwell_boltzmann
    from torchmd_amd.systems import System

    terms = ["lj", "electrostatics", "bonds", "angles"]
    fo = Forces(par, terms=terms, cutoff=rc, pme=True, **kw)
    n = len(pos)
    system = System(n, R, torch.float64, DEV)
    system.set_positions(np.asarray(pos)[:, :, None])
    system.set_box(np.asarray(box))
    torch.manual_seed(3)
    system.set_velocities(maxwell_boltzmann(par.masses.double().cpu().reshape(-1, 1), 300, R))
    v0, x0 = system.vel.clone(), system.pos.clone()
    fo.compute(system.pos, system.box, system.forces)
    integ = Integrator(system, fo, timestep=dt_fs, device=DEV)
    ref = Forces(par, terms=terms, cutoff=rc, pme=True, **kw)
    q = par.charges.double().cpu().numpy().reshape(-1)
    escale = abs(E.self_and_background(q, np.asarray(box, np.float64), fo.ewald_beta))
    done = 0
    for k in (1, 7, 50):
        _, pot, _ = integ.step(niter=k)
        done += k
        x, v, f, epot = _python_nve(ref, par, x0, v0, system.box, done, dt_fs)
        assert (system.pos - x).abs().max().item() <= 1e-9, k
        assert (system.vel - v).abs().max().item() <= 1e-9, k
        assert (system.forces - f).abs().max().item() <= 1e-8, k
        assert np.abs(np.asarray(pot).reshape(-1) - epot.reshape(-1)).max() <= 1e-10 * escale, (k, pot, epot)
    assert fo.stats(system.pos)["steps_in_pair_launch"] == 0
    for r in range(R):
        assert fo.stats(system.pos, r)["pme_evaluations"] > 0
    return fo, system


def test_integrator_equals_python_loop_celllist():
    """The cell-list branch of md_run, across list rebuilds."""
    par, pos, q, box, _, rc, _ = _tip3p(nside=16)
    fo, system = _integrator_against_loop(par, pos, box, rc, 1, 1.0)
    assert fo.stats(system.pos)["algorithm"] == "celllist"
    assert fo.stats(system.pos)["n_rebuilds"] > 1


@pytest.mark.parametrize("R", [1, 2])
def test_integrator_equals_python_loop_allpairs(R):
    """The all-pairs branches of md_run: one replica (the replica loop) and two (one launch for all replicas)."""
    g = G.load("water291")
    par = G.GoldenParameters(g, precision=torch.float64, device=DEV)
    fo, system = _integrator_against_loop(par, g["pos"], g["box"], 7.3, R, 0.5, algorithm="allpairs")
    assert fo.stats(system.pos)["algorithm"] == "allpairs"


def test_two_replicas_allpairs_match_host():
    """tmdhip_compute_nonbonded serves the replicas of an all-pairs context with one launch: each replica's PME part."""
    par, pos, q, box, terms, rc, excl = _water()
    rng = np.random.default_rng(7)
    pos2 = np.stack([pos, pos + rng.normal(scale=0.05, size=pos.shape)])
    from torchmd_amd.forces import Forces

    fo = Forces(par, terms=terms, cutoff=rc, pme=True, algorithm="allpairs")
    p = torch.as_tensor(pos2, dtype=torch.float64, device=DEV).contiguous()
    f = torch.zeros_like(p)
    e = fo.compute(p, _box_t(box, 2, torch.float64), f, returnDetails=True)
    assert fo.stats(p)["algorithm"] == "allpairs"
    for r in range(2):
        eh, fh = E.pme(pos2[r], q, box, fo.ewald_beta, rc, fo.pme_grid, 5, excl)
        assert abs(e[r]["electrostatics"] - eh) <= 1e-10 * abs(eh), r
        assert np.abs(f[r].cpu().numpy() - fh).max() <= 1e-8, r


def test_langevin_and_nve_drift_on_water():
    from torchmd_amd.forces import Forces
    from torchmd_amd.integrator import Integrator, maxwell_boltzmann
    from torchmd_amd.systems import System

    g = G.load("water291")
    par = G.GoldenParameters(g, precision=torch.float64, device=DEV)
    terms = ["lj", "electrostatics", "bonds", "angles"]
    for gamma, T in ((1.0, 300.0), (None, None)):
        fo = Forces(par, terms=terms, cutoff=7.3, pme=True, ewald_tolerance=1e-6)
        system = System(len(g["pos"]), 1, torch.float64, DEV)
        system.set_positions(g["pos"][:, :, None])
        system.set_box(g["box"])
        torch.manual_seed(5)
        system.set_velocities(maxwell_boltzmann(par.masses, 300, 1))
        integ = Integrator(system, fo, timestep=0.5, device=DEV, gamma=gamma, T=T)
        fo.compute(system.pos, system.box, system.forces)
        ek, pot, temp = integ.step(niter=10)
        assert np.isfinite(ek).all() and np.isfinite(pot).all()
        if gamma is None:
            e0 = ek[0] + pot[0]
            drift = []
            for _ in range(20):
                ek, pot, temp = integ.step(niter=10)
                drift.append(ek[0] + pot[0] - e0)
            # flexible water at 0.5 fs: the total energy stays within 0.5 kcal/mol of its start over 200 steps
            assert max(abs(d) for d in drift) < 0.5, drift


# ---- interface -----------------------------------------------------------------------------------------------------------
def test_value_errors():
    from torchmd_amd.domain import DomainSet
    from torchmd_amd.forces import Forces

    par, pos, q, box, terms, rc, _ = _ions(n=20)
    with pytest.raises(ValueError):
        Forces(par, terms=terms, cutoff=rc, rfa=True, pme=True)
    with pytest.raises(ValueError):
        Forces(par, terms=terms, pme=True)
    with pytest.raises(ValueError):
        Forces(par, terms=["lj"], cutoff=rc, pme=True)
    for order in (3, 7):
        with pytest.raises(ValueError):
            Forces(par, terms=terms, cutoff=rc, pme=True, pme_order=order)
    fo = Forces(par, terms=terms, cutoff=rc, pme=True)
    p = G.pos_tensor(pos, 1, torch.float64, DEV)
    with pytest.raises(ValueError):
        fo.compute(p, _box_t(np.zeros(3), 1, torch.float64), torch.zeros_like(p))
    with pytest.raises(ValueError):
        DomainSet(box, 2, DEV, torch.float64, ["lj"], 9.0, pme=True)


def test_pme_off_allocates_and_launches_nothing():
    from torchmd_amd.forces import Forces

    par, pos, q, box, _, rc, _ = _tip3p(torch.float32, nside=16)
    terms = ["lj", "electrostatics", "bonds", "angles"]
    p = G.pos_tensor(pos, 1, torch.float32, DEV)
    b = _box_t(box, 1, torch.float32)
    off = Forces(par, terms=terms, cutoff=rc, rfa=True)
    off.compute(p, b, torch.zeros_like(p))
    st = off.stats(p)
    assert st["pme_evaluations"] == 0 and st["pme_bytes"] == 0
    on = Forces(par, terms=terms, cutoff=rc, pme=True, pme_grid=(48, 50, 52))
    on.compute(p, b, torch.zeros_like(p))
    st = on.stats(p)
    assert on.pme_grid == (48, 50, 52)
    assert st["pme_evaluations"] == 1 and st["pme_bytes"] > 48 * 50 * 52 * 4
