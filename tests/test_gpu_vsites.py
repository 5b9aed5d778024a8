"""Virtual interaction sites on the GPU (run with `-m gpu` on an MI355X): the stateless kernels against the numpy methods of
torchmd_amd/vsites.py, `Forces(..., virtual_sites=...)` against the oracle, and four-site rigid water (TIP4P-Ew) through the
constrained MD step: geometry, idempotence of the in-kernel site, energy conservation, rewind, NPT, and that nothing leaks
into runs without sites."""

import ctypes as C

import numpy as np
import pytest
import torch

import _barostat as B
import _constraints as H
import _ewald as E
from oracle import torchmd_oracle as orc

pytestmark = pytest.mark.gpu

TERMS = ["lj", "electrostatics", "bonds", "angles"]
PREC = {"f32": torch.float32, "f64": torch.float64}
# the suite's bars for the same dtype and path: tests/test_gpu_parity.py (forces, energies against the oracle),
# tests/test_gpu_pme.py (fp64 against the host PME, fp32 against fp64), tests/test_gpu_constraints.py (constraints)
FTOL = {"f64": 1e-8, "f32": 3e-4}
ERTOL = {"f64": 1e-10, "f32": 2e-5}
EFAC = 3
CONS_TOL = {"f32": (3e-5, 1e-5), "f64": (1e-10, 1e-10)}
ULPS = {"f32": 1, "f64": 4}


def _dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _tables(vs):
    return tuple(torch.as_tensor(a, device=_dev()) for a in (vs.sites, vs.parents, vs.weights))


def _construct(x, vs, tabs=None):
    from torchmd_amd import _lib as L

    s, p, w = tabs or _tables(vs)
    L.check(L.load().tmdhip_vsite_construct(L.dtype_code(x.dtype), x.shape[0], x.shape[1], x.data_ptr(), vs.nsites, s.data_ptr(),
                                            p.data_ptr(), w.data_ptr(), _stream()), "tmdhip_vsite_construct")


def _spread(f, vs, tabs=None):
    from torchmd_amd import _lib as L

    s, p, w = tabs or _tables(vs)
    L.check(L.load().tmdhip_vsite_spread(L.dtype_code(f.dtype), f.shape[0], f.shape[1], f.data_ptr(), vs.nsites, s.data_ptr(),
                                         p.data_ptr(), w.data_ptr(), _stream()), "tmdhip_vsite_spread")


# ----------------------------------------------------------------------------- 1. the stateless kernels
def _random_sites(natoms, nsites, seed):
    """2- and 3-parent sites alternating, scattered over the atoms."""
    from torchmd_amd.vsites import VirtualSites

    rng = np.random.default_rng(seed)
    perm = rng.permutation(natoms)
    sites, rest = perm[:nsites], perm[nsites:]
    parents = -np.ones((nsites, 3), dtype=np.int64)
    w = np.zeros((nsites, 3))
    k = 0
    for s in range(nsites):
        npar = 2 + (s % 2)
        parents[s, :npar] = rest[k:k + npar]
        k += npar
        w[s, :npar] = rng.uniform(-0.4, 0.9, size=npar)
        w[s, npar - 1] = 1.0 - w[s, :npar - 1].sum()
    return VirtualSites(sites, parents, w)


@pytest.mark.parametrize("prec", ["f32", "f64"])
@pytest.mark.parametrize("R", [1, 3])
@pytest.mark.parametrize("natoms,nsites", [(23, 5), (1300, 300)])
def test_stateless_kernels_against_numpy(prec, R, natoms, nsites):
    vs = _random_sites(natoms, nsites, seed=natoms + R)
    assert (vs.parents[:, 2] < 0).any() and (vs.parents[:, 2] >= 0).any()
    rng = np.random.default_rng(7)
    dt = PREC[prec]
    x0 = torch.as_tensor(rng.normal(size=(R, natoms, 3)) * 30.0).to(dt)
    x = x0.to(_dev())
    _construct(x, vs)
    got = x.cpu().numpy()
    mask = vs.site_mask(natoms)
    assert np.array_equal(got[:, ~mask], x0.numpy()[:, ~mask])  # non-site rows: not a bit changed
    want = vs.construct(x0.double().numpy().copy())[:, vs.sites]  # float64 recomputation from the stored parents
    err = np.abs(got[:, vs.sites].astype(np.float64) - want)
    assert np.all(err <= ULPS[prec] * np.spacing(np.abs(want).astype(got.dtype)).astype(np.float64)), err.max()

    f0 = torch.as_tensor(rng.normal(size=(R, natoms, 3)) * 80.0).to(dt)
    f = f0.to(_dev())
    _spread(f, vs)
    gf = f.cpu().numpy()
    assert np.all(gf[:, vs.sites] == 0.0)
    wf = vs.spread(f0.double().numpy().copy())
    fmax = np.abs(f0.numpy()).max()
    assert np.abs(gf.astype(np.float64) - wf).max() <= ULPS[prec] * float(np.spacing(np.asarray(fmax, dtype=gf.dtype)))
    untouched = ~mask
    untouched[vs.parents[vs.parents >= 0]] = False
    assert np.array_equal(gf[:, untouched], f0.numpy()[:, untouched])
    f2 = f0.to(_dev())
    _spread(f2, vs)
    assert torch.equal(f, f2)  # no atomics: the same bits


# ----------------------------------------------------------------------------- 2. Forces.compute against the oracle
def _tip4p(nside, prec, seed=3):
    from torchmd_amd.builders import tip4p_box, tip4pew_forcefield
    from torchmd_amd.parameters import Parameters

    mol, pos, box, vs = tip4p_box(nside, seed=seed)
    par = Parameters(tip4pew_forcefield(mol), mol, TERMS, precision=PREC[prec])
    return mol, pos, box, vs, par


def _misplaced(pos, vs, prec, box=None):
    p = np.array(pos)
    p[vs.sites] += np.random.default_rng(5).normal(size=(vs.nsites, 3)) * 3.0
    return torch.as_tensor(p[None]).to(PREC[prec]).to(_dev())


def _box_t(box, prec):
    return torch.diag(torch.as_tensor(np.asarray(box, dtype=np.float64))).to(PREC[prec])[None].to(_dev())


def _check_placed(p, pos, vs, prec):
    """`pos` came back with the sites placed: within the kernel's bound of the float64 recomputation, other rows untouched."""
    got = p[0].cpu().numpy()
    src = torch.as_tensor(pos).to(PREC[prec]).numpy()
    mask = vs.site_mask(len(src))
    assert np.array_equal(got[~mask], src[~mask])
    want = vs.construct(got.astype(np.float64))[vs.sites]
    assert np.all(np.abs(got[vs.sites] - want) <= ULPS[prec] * np.spacing(np.abs(want).astype(got.dtype)))


@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("case", ["allpairs64", "celllist1728"])
def test_compute_against_the_oracle(prec, case):
    from torchmd_amd.forces import Forces

    nside, kw = (4, {}) if case == "allpairs64" else (12, dict(cutoff=9.0, rfa=True))
    mol, pos, box, vs, par = _tip4p(nside, prec)
    hbox = np.zeros(3) if case == "allpairs64" else box
    f = Forces(par, terms=TERMS, virtual_sites=vs, **kw)
    p, b = _misplaced(pos, vs, prec), _box_t(hbox, prec)
    F = torch.full_like(p, 7.0)
    pots = f.compute(p, b, F, returnDetails=True)
    assert f.stats(p)["algorithm"] == ("allpairs" if case == "allpairs64" else "celllist")
    _check_placed(p, pos, vs, prec)
    # The oracle at the constructed positions, its forces spread by the numpy method.  The oracle runs in float64 on the
    # positions the GPU holds (for fp32: the float32 values, exactly representable): with q_O = 0 the Coulomb energy of a
    # TIP4P-Ew box is what is left of terms a hundred times larger, and a float32 oracle sums them with an error of its own
    # (64 molecules, no cutoff: 4.8e-4 of a total of -4.92 kcal/mol, eight times the bar) that a reference must not have.
    # The float32 oracle's figures are printed beside.
    pc = p.cpu()
    pairs = None if case == "allpairs64" else orc.candidate_pairs(pc[0].double().numpy(), box, 9.6, orc.exclusion_pairs(par))
    par64 = par if prec == "f64" else _tip4p(nside, "f64")[4]
    po, Fo, npairs = orc.compute(par64, pc.double(), b.cpu().double(), TERMS, pairs=pairs, **kw)
    Fo = vs.spread(Fo.numpy().copy())
    got = F.cpu().numpy()
    assert np.all(got[0, vs.sites] == 0.0)
    err = np.abs(got - Fo).max()
    print(f"{case} {prec}: max|dF| = {err:.2e}; energies GPU / oracle: " + ", ".join(f"{t} {pots[0][t]:.6f} / {po[0][t]:.6f}" for t in TERMS))
    if prec == "f32":
        p32, F32, _ = orc.compute(par, pc, b.cpu(), TERMS, pairs=pairs, **kw)
        print(f"  float32 oracle: max|dF| = {np.abs(got - vs.spread(F32.numpy().copy())).max():.2e}; " +
              ", ".join(f"{t} {p32[0][t]:.6f}" for t in TERMS))
    assert err < FTOL[prec], err
    for t in TERMS:
        assert abs(pots[0][t] - po[0][t]) <= ERTOL[prec] * EFAC * max(1, abs(po[0][t])), (t, pots[0][t], po[0][t])
    if case != "allpairs64":
        assert f.count_pairs(p, b) == npairs


_PME64 = {}


def test_compute_with_pme():
    """fp64 against the host PME of tests/_ewald.py (electrostatics; sites are ordinary charges there), fp32 against fp64: the
    bars of tests/test_gpu_pme.py."""
    from torchmd_amd.forces import Forces

    res = {}
    for prec in ("f64", "f32"):
        mol, pos, box, vs, par = _tip4p(12, prec)
        f = Forces(par, terms=["electrostatics"], cutoff=9.0, pme=True, virtual_sites=vs)
        p, b = _misplaced(pos, vs, prec), _box_t(box, prec)
        F = torch.zeros_like(p)
        e = f.compute(p, b, F, returnDetails=True)[0]["electrostatics"]
        _check_placed(p, pos, vs, prec)
        assert f.stats(p)["pme_evaluations"] > 0 and torch.all(F[0, torch.as_tensor(vs.sites.astype(np.int64))] == 0)
        res[prec] = (e, F.double().cpu().numpy(), p.double().cpu().numpy()[0], f, par)
    e64, f64, x64, fo, par = res["f64"]
    q = par.charges.double().cpu().numpy()
    excl = [tuple(x) for x in par.get_exclusions(("bonds", "angles", "1-4"))]
    eh, fh = E.pme(x64, q, np.asarray(box, np.float64), fo.ewald_beta, 9.0, fo.pme_grid, 5, excl)
    fh = vs.spread(fh.copy())
    eself = abs(E.self_and_background(q, box, fo.ewald_beta))
    bound = 1e-10 * abs(eh) if abs(eh) > 1e-2 * eself else 1e-12 * eself
    print(f"PME fp64: |dE| = {abs(e64 - eh):.2e} (bound {bound:.2e}), max|dF| = {np.abs(f64[0] - fh).max():.2e}")
    assert abs(e64 - eh) <= bound and np.abs(f64[0] - fh).max() <= 1e-8
    e32, f32 = res["f32"][0], res["f32"][1]
    scale = max(abs(e64), eself)
    assert abs(e32 - e64) / scale <= 2e-5 and np.abs(f32 - f64).max() <= 5e-3


# ----------------------------------------------------------------------------- 3. MD: geometry and idempotence
def _md_box(nside, prec, seed=0, pme=False, barostat=None, gamma=1.0, T=300.0, dt_fs=2.0):
    from torchmd_amd.constraints import find_constraints
    from torchmd_amd.forces import Forces
    from torchmd_amd.integrator import Integrator, maxwell_boltzmann
    from torchmd_amd.systems import System

    mol, pos, box, vs, par = _tip4p(nside, prec, seed=seed)
    s = System(mol.numAtoms, 1, PREC[prec], _dev())
    s.set_positions(pos[:, :, None])
    s.set_box(box)
    torch.manual_seed(seed)
    vel = maxwell_boltzmann(par.masses, T, 1)
    vel[:, torch.as_tensor(vs.sites.astype(np.int64))] = 0.0
    s.set_velocities(vel)
    kw = dict(cutoff=9.0, pme=True) if pme else dict(cutoff=9.0, rfa=True)
    f = Forces(par, terms=TERMS, virtual_sites=vs, **kw)
    f.compute(s.pos, s.box, s.forces)
    extra = {} if barostat is None else {"barostat": barostat}
    integ = Integrator(s, f, dt_fs, _dev(), gamma=gamma, T=T if gamma else None, constraints="water", **extra)
    cs = find_constraints(par.masses, par.bond_params, par.angle_params, "water", virtual_sites=vs)
    return mol, par, box, vs, s, f, integ, cs


def _check_geometry(s, vs, cs, prec, what, tabs):
    again = s.pos.clone()
    _construct(again, vs, tabs)
    assert torch.equal(again, s.pos), what  # the in-kernel site and the stateless kernel: not a bit apart
    pairs, d = cs.pairs()
    dr, dv = H.residuals(s.pos[0].cpu().double().numpy(), s.vel[0].cpu().double().numpy(), pairs, d)
    assert dr <= CONS_TOL[prec][0] and dv <= CONS_TOL[prec][1], (what, dr, dv)
    assert torch.all(s.vel[0, torch.as_tensor(vs.sites.astype(np.int64))] == 0), what
    assert torch.all(s.forces[0, torch.as_tensor(vs.sites.astype(np.int64))] == 0), what
    return dr, dv


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_md_geometry_and_idempotence(prec):
    mol, par, box, vs, s, f, integ, cs = _md_box(12, prec)
    tabs = _tables(vs)
    nmol = mol.numAtoms // 4
    assert integ._ndof == 6 * nmol
    for call in range(4):
        ek, pot, T = integ.step(50)
        _check_geometry(s, vs, cs, prec, f"call {call}", tabs)
        assert np.isfinite(ek).all() and np.isfinite(pot).all() and np.isfinite(T).all()
        assert abs(T[0] - 2.0 * float(ek[0]) / (6 * nmol * 0.001987191)) <= 1e-5 * T[0]  # the new ndof
    st = f.stats(s.pos)
    assert st["algorithm"] == "celllist" and st["n_rebuilds"] > 0, st
    print(f"tip4p_box(12) {prec}: 200 steps at 2 fs, T = {T[0]:.1f} K, {st['n_rebuilds']} rebuilds, {integ.replays} replays")
    # the list never missed a site pair: the run's pair count equals a fresh count on the same positions
    from torchmd_amd.forces import Forces

    run_count = f.count_pairs(s.pos, s.box)[0]
    fresh = Forces(par, terms=TERMS, virtual_sites=vs, cutoff=9.0, rfa=True)
    assert run_count == fresh.count_pairs(s.pos.clone(), s.box)[0]
    # ... and the forces of the run's last step are those of a fresh evaluation (a missed site pair would show)
    F = torch.zeros_like(s.forces)
    fresh.compute(s.pos.clone(), s.box, F)
    assert (F - s.forces).abs().max().item() < FTOL[prec]


# ----------------------------------------------------------------------------- 4. energy conservation is second order
def _drift(dt_fs, nsteps, every):
    from torchmd_amd.constraints import find_constraints
    from torchmd_amd.forces import Forces
    from torchmd_amd.integrator import Integrator
    from torchmd_amd.systems import System

    mol, pos, box, vs, par = _tip4p(4, "f64", seed=1)
    m = par.masses.reshape(-1).double().numpy()
    cs = find_constraints(m, par.bond_params, par.angle_params, "water", virtual_sites=vs)
    real = ~vs.site_mask(len(m))
    us = H.units(cs)
    x = H.shake(np.array(pos), np.array(pos), m, us)
    vs.construct(x)
    rng = np.random.default_rng(3)
    v = np.zeros_like(x)
    v[real] = rng.normal(size=(real.sum(), 3)) * np.sqrt(300.0 * 0.001987191 / m[real])[:, None]
    H.project(x, v, m, us)
    s = System(mol.numAtoms, 1, torch.float64, _dev())
    s.set_positions(x[:, :, None])
    s.set_box(np.zeros(3))
    s.set_velocities(torch.as_tensor(v[None]))
    f = Forces(par, terms=TERMS, algorithm="allpairs", virtual_sites=vs)
    e0 = f.compute(s.pos, s.box, s.forces)[0] + 0.5 * float(np.sum(m[:, None] * v * v))
    integ = Integrator(s, f, dt_fs, _dev(), constraints="water")
    dev = 0.0
    for _ in range(nsteps // every):
        ek, pot, _ = integ.step(every)
        dev = max(dev, abs(float(ek[0]) + pot[0] - e0))
    return dev


def test_energy_conservation_is_second_order():
    d2 = _drift(2.0, 200, 5)
    d1 = _drift(1.0, 400, 10)
    print(f"64 rigid TIP4P-Ew waters, NVE fp64, 400 fs: max|E - E0| = {d2:.3e} at 2 fs, {d1:.3e} at 1 fs, ratio {d2 / d1:.2f}")
    assert 3.0 <= d2 / d1 <= 5.0, (d2, d1)


# ----------------------------------------------------------------------------- 5. rewind
@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_restore_returns_the_entry_state(prec):
    from torchmd_amd import _lib as L

    mol, par, box, vs, s, f, integ, cs = _md_box(12, prec, seed=2)
    integ.step(10)  # (past the start-up projection; the list exists: the next call's first kernel takes the snapshot itself)
    entry = [t.clone() for t in (s.pos, s.vel, s.forces)]
    integ.step(20)
    assert not torch.equal(entry[0], s.pos)
    eng = f._engine(s.pos)
    d = eng._md_cache[3]
    L.check(eng.lib.tmdhip_md_restore(eng.ctx, C.byref(d), _stream()), "tmdhip_md_restore")
    torch.cuda.synchronize()
    for name, a, b in zip(("pos", "vel", "forces"), entry, (s.pos, s.vel, s.forces)):
        assert torch.equal(a, b), name  # bit for bit, site rows included


# ----------------------------------------------------------------------------- 6. composition: rigid TIP4P-Ew + PME + NPT
def _seed_with_both(nmol, edges):
    """A barostat seed whose host chain (tests/_barostat.py, U = 0) accepts and rejects within the run's 10 attempts."""
    for seed in range(1, 200):
        _, flags = B.volume_chain(edges, nmol, 1.0, 300.0, 10, B.philox_stream(seed))
        if 2 <= flags.sum() <= 8:
            return seed
    raise AssertionError("no seed found")


def test_npt_pme_rigid_tip4p():
    from torchmd_amd.barostat import MonteCarloBarostat

    nmol = 12**3
    edge = (nmol / 0.0334) ** (1.0 / 3.0)
    bar = MonteCarloBarostat(1.0, 300.0, frequency=10, seed=_seed_with_both(nmol, [edge] * 3))
    mol, par, box, vs, s, f, integ, cs = _md_box(12, "f32", seed=5, pme=True, barostat=bar)
    tabs = _tables(vs)
    for call in range(2):
        ek, pot, T = integ.step(50)
        assert np.isfinite(ek).all() and np.isfinite(pot).all()
        _check_geometry(s, vs, cs, "f32", f"NPT call {call}", tabs)
    print(f"tip4p_box(12) f32, rigid, PME, 1 bar, 100 steps at 2 fs: {bar.accepted[0]} of {bar.attempts[0]} moves accepted")
    assert bar.ngroups == nmol and bar.attempts[0] == 10
    assert 1 <= bar.accepted[0] <= 9, (bar.accepted, bar.attempts)  # at least one accepted and one rejected
    assert f.stats(s.pos)["pme_evaluations"] > 0


# ----------------------------------------------------------------------------- 7. off means off
def test_three_site_run_is_untouched_by_a_four_site_context():
    import test_gpu_constraints as TC

    def three_site():
        mol, par, box, s, f, integ, cs = TC._water_box(16, "f32", seed=9)
        assert getattr(f, "virtual_sites", None) is None
        integ.step(100)
        out = s.pos.clone()
        f.close()
        return out

    before = three_site()
    mol, par, box, vs, s, f, integ, cs = _md_box(6, "f32", seed=1)
    integ.step(20)
    f.close()
    after = three_site()
    assert torch.equal(before, after)
