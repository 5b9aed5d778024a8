"""The velocity-rescaling thermostat on the device: tmdhip_thermostat_apply against the numpy model of
tests/_thermostat.py, its edge cases, the free-particle chain of tests/test_thermostat_host.py, and the thermostat inside
`Integrator.step` on the cell-list path, with constraints, with the barostat and from run.py.

Bars against the model (the only expected difference is the order of the device's sums, which the model takes exactly, by
math.fsum): ten times what was measured on one MI355X (DESIGN §14 has the measured values), relative for K_before, alpha and
K_after, relative to the largest component for the velocities."""

import json
import math
import os
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

import _reduce as RM
import _thermostat as M
from _golden import PREC

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WATER_TERMS = ["lj", "electrostatics", "bonds", "angles"]
NP = {"f32": np.float32, "f64": np.float64}
EPS64 = np.finfo(np.float64).eps
# 10 x measured (MEASURED_* below: worst over every application of tests 1, 2 and 4 on one MI355X).  K_before is a sum of N
# terms in another order; alpha and K_after follow from it.  In fp32 the model rounds every stored velocity to float32 as the
# kernel does, and the velocities came out equal bit for bit: ten times zero is equality.
MEASURED_REL = {"f64": 1.07e-15, "f32": 8.6e-16}
MEASURED_VEL = {"f64": 7.4e-16, "f32": 0.0}
REL_BAR = {p: 10 * v for p, v in MEASURED_REL.items()}
VEL_BAR = {p: 10 * v for p, v in MEASURED_VEL.items()}
CONS_TOL = {"f32": 3e-5, "f64": 1e-10}  # bond length (relative) of constrained dynamics (tests/test_gpu_constraints.py)


def _dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _thermostat(*a, **kw):
    from torchmd_amd.thermostat import VelocityRescale

    return VelocityRescale(*a, **kw)


def _sys(vel, prec):
    return types.SimpleNamespace(vel=torch.as_tensor(np.ascontiguousarray(vel), dtype=PREC[prec]).to(_dev()).contiguous())


def _mass_t(mass, prec):
    return torch.as_tensor(mass, dtype=PREC[prec]).to(_dev()).contiguous()


def _start(R, N, prec, seed, nan_rows=True):
    """Masses {1.008, 15.999, 0} in turn and velocities with a net drift, both already rounded to the precision; the massless
    rows hold arbitrary bits, some of them NaN."""
    rng = np.random.default_rng(seed)
    mass = np.array([1.008, 15.999, 0.0])[np.arange(N) % 3].astype(NP[prec]).astype(np.float64)
    vel = 0.05 * rng.standard_normal((R, N, 3)) + np.array([0.01, -0.02, 0.005])
    if nan_rows:
        vel[:, 2::6] = np.nan
    return mass, vel.astype(NP[prec]).astype(np.float64)


def _check(name, prec, got, want, worst):
    """Relative difference of two record columns against REL_BAR (after printing it)."""
    rel = float(np.max(np.abs(got - want) / np.abs(want)))
    worst[name] = max(worst.get(name, 0.0), rel)
    return rel


def _report(what, prec, worst, vel_err):
    print(f"{what} {prec}: device vs model, worst relative difference {', '.join(f'{k} {v:.2e}' for k, v in worst.items())}; "
          f"velocities {vel_err:.2e} of the largest component (bars {REL_BAR[prec]:.1e}, {VEL_BAR[prec]:.1e})")
    assert max(worst.values()) <= REL_BAR[prec], worst
    assert vel_err <= VEL_BAR[prec], vel_err


def _run_chain(th, s, mass_t, dt, ndof, napply):
    recs = []
    for _ in range(napply):
        th.apply(s, mass_t, dt, ndof)
        recs.append(th.last.clone())
    return torch.stack(recs).cpu().numpy()  # [napply, R, 4]


# ----------------------------------------------------------------------------- 1. the kernel against the model
@pytest.mark.parametrize("prec", ["f64", "f32"])
def test_kernel_against_the_model(prec):
    R, N, napply = 3, 1000, 300
    T = (280.0, 300.0, 320.0)
    mass, vel0 = _start(R, N, prec, 1)
    on = mass > 0
    ndof = 3 * int(on.sum())
    dt = 1.0 / M.TIMEFACTOR
    tau = 0.01 / -np.log(0.9)  # ten steps of 1 fs: c = 0.9
    mass_t = _mass_t(mass, prec)

    def device():
        th = _thermostat(T, tau=tau, frequency=10, seed=11)
        s = _sys(vel0, prec)
        rec = _run_chain(th, s, mass_t, dt, ndof, napply)
        return th, s, rec

    th, s, rec = device()
    c, nf = th.decay(dt), th.nf
    assert abs(c - 0.9) < 1e-12 and nf == ndof - 3
    # the model, with the same draws
    vel = vel0.copy()
    want = np.zeros((napply, R, 4))
    for r, g in enumerate(M.generators(11, R)):
        for k in range(napply):
            r1, sdraw = M.draw(g, nf)
            want[k, r] = M.apply(vel[r], mass, 0.5 * nf * M.BOLTZMAN * T[r], float(nf), c, r1, sdraw, True, prec == "f32")
    worst = {}
    for col, name in enumerate(("K_before", "alpha", "K_after")):
        _check(name, prec, rec[:, :, col], want[:, :, col], worst)
    got = s.vel.cpu().double().numpy()
    vel_err = float(np.abs(got[:, on] - vel[:, on]).max() / np.abs(vel[:, on]).max())
    # |V_cm| of the first application is the drift that was put in; afterwards it is zero to rounding
    assert np.allclose(rec[0, :, 3], want[0, :, 3], rtol=1e-9) and (rec[0, :, 3] > 0.01).all()
    _report("kernel, R = 3, N = 1000, 300 applications", prec, worst, vel_err)

    # massless rows keep their bit pattern, NaNs included
    bits = lambda t: t.cpu().contiguous().view(torch.int32 if prec == "f32" else torch.int64)  # noqa: E731
    start_bits = bits(_sys(vel0, prec).vel)
    assert torch.equal(bits(s.vel)[:, ~on], start_bits[:, ~on]) and np.isnan(vel0[:, ~on]).any()
    assert np.isfinite(got[:, on]).all()
    # two runs give the same bits
    th2, s2, rec2 = device()
    assert torch.equal(bits(s2.vel), bits(s.vel)) and np.array_equal(rec2, rec)
    assert np.array_equal(th2.heat(), th.heat()) and np.array_equal(th2.draws, th.draws)
    # heat is the sum of K_after - K_before, added in the order of the applications
    heat = np.zeros(R)
    for k in range(napply):
        heat = heat + (rec[k, :, 2] - rec[k, :, 0])
    assert np.array_equal(th.heat(), heat)

    # the centre-of-mass momentum after an application is zero to the rounding of the store.  Per component
    # sum m v' = alpha (sum m v - (sum m) V_cm) is zero but for: the store of each v' (half a step of the precision; none in
    # fp64), the two roundings of alpha (v - V_cm) in double (eps64 |v'| per atom), the rounding of the sums behind V_cm
    # (their depth — atoms per thread, shuffles, LDS fold, blocks per lane, shuffles — is below 24 additions of half an eps64
    # each: 12 eps64 N max|m v|), the division (eps64 / 2), and this test's own m * v products (eps64 / 2 each):
    # |P| <= N max|m v| (eps_store / 2 + 16 eps64), N the number of massive atoms.
    mv = mass[on][None, :, None] * got[:, on]
    P = np.array([[abs(math.fsum(mv[r, :, k])) for k in range(3)] for r in range(R)])
    bound = on.sum() * np.abs(mv).max() * ((np.finfo(np.float32).eps / 2 if prec == "f32" else 0.0) + 16 * EPS64)
    print(f"centre-of-mass momentum after 300 applications {prec}: max |P| = {P.max():.2e}, bound {bound:.2e}")
    assert P.max() <= bound, (P, bound)

    # a replica with active = 0 is never written: neither its velocities nor its record
    s3 = _sys(vel0, prec)
    th3 = _thermostat(T, tau=tau, frequency=10, seed=11)
    th3.apply(s3, mass_t, dt, ndof)
    before_v, before_r = bits(s3.vel).clone(), th3._record.clone()
    th3.apply(s3, mass_t, dt, ndof, active=[1, 0, 1])
    assert torch.equal(bits(s3.vel)[1], before_v[1]) and torch.equal(th3._record[1], before_r[1])
    assert not torch.equal(bits(s3.vel)[0], before_v[0]) and not torch.equal(bits(s3.vel)[2], before_v[2])
    assert th3._record[0, 5].item() == 2.0 and th3._record[1, 5].item() == 1.0


# ----------------------------------------------------------------------------- 2. the stride loop
@pytest.mark.parametrize("prec", ["f64", "f32"])
def test_stride_loop(prec):
    """70 001 atoms: more than 256 blocks x 256 threads, so every reduction block takes more than one atom per thread, and the
    update grid (274 blocks) is larger than the reduction grid."""
    N = 70001
    mass, vel0 = _start(1, N, prec, 2)
    on = mass > 0
    ndof = 3 * int(on.sum())
    th = _thermostat(310.0, tau=0.05, frequency=10, seed=12)
    s = _sys(vel0, prec)
    dt = 1.0 / M.TIMEFACTOR
    th.apply(s, _mass_t(mass, prec), dt, ndof)
    rec = th.last.cpu().numpy()
    vel = vel0.copy()
    r1, sdraw = M.draw(M.generators(12, 1)[0], th.nf)
    assert th.draws[0, 0] == r1 and th.draws[0, 1] == sdraw
    want = M.apply(vel[0], mass, 0.5 * th.nf * M.BOLTZMAN * 310.0, float(th.nf), th.decay(dt), r1, sdraw, True, prec == "f32")
    worst = {}
    for col, name in enumerate(("K_before", "alpha", "K_after")):
        _check(name, prec, rec[:, col], np.array([want[col]]), worst)
    got = s.vel.cpu().double().numpy()
    vel_err = float(np.abs(got[:, on] - vel[:, on]).max() / np.abs(vel[:, on]).max())
    assert not np.array_equal(got[0, on][-1], vel0[0, on][-1])  # (the last atom was reached)
    _report("stride loop, N = 70 001", prec, worst, vel_err)


@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("N", RM.SHAPES)
def test_partial_rows_and_record_bit_for_bit(N, prec):
    """The order of the fixed-order sum (tests/_reduce.py): every partial row thermostat_reduce_kernel writes (five columns) and
    the record's K_before against the model, addition by addition.  The four wave sums meet in sequence here.  The centre of
    mass stays in, so that K_before is half the folded sum of m v^2 and nothing else (what csvr_kinetic of thermostat_math.h
    subtracts for it is arithmetic behind the sum, which the compiler may contract)."""
    mass, vel = RM.velocities(2, N, prec, 7)
    on = mass > 0
    th = _thermostat((300.0, 310.0), tau=0.05, frequency=10, remove_com=False, seed=12)
    th.apply(_sys(vel, prec), _mass_t(mass, prec), 1.0 / M.TIMEFACTOR, 3 * int(on.sum()))
    rows = th._partials.cpu().numpy().reshape(2, -1, 5)
    rec = th._record.cpu().numpy()
    nb = RM.nblocks_of(N)
    for r in range(2):
        want = np.stack([RM.partial_rows(c, on, RM.SEQUENTIAL) for c in RM.thermostat_columns(mass, vel[r])], axis=1)
        differ = int((rows[r, :nb].view(np.int64) != want.view(np.int64)).any(axis=1).sum())
        K = 0.5 * RM.fold(want[:, 4])
        print(f"N = {N} {prec} replica {r}: {differ} of {nb} partial rows differ from the model; K_before {rec[r, 0]!r}, model {K!r}")
        assert differ == 0 and rec[r, 0] == K and rec[r, 3] == 0.0


# ----------------------------------------------------------------------------- 3. edges
@pytest.mark.parametrize("prec", ["f64", "f32"])
def test_edges(prec):
    R, N = 3, 1000
    T = np.array([280.0, 300.0, 320.0])
    mass, vel0 = _start(R, N, prec, 3)
    on = mass > 0
    ndof = 3 * int(on.sum())
    mass_t = _mass_t(mass, prec)
    dt = 1.0 / M.TIMEFACTOR
    # tau = 0: K_after = (k_B T_r / 2) (R1^2 + S) whatever K was — four roundings in double (tests/test_thermostat_host.py);
    # and the kinetic energy of the stored velocities is that to the rounding of the store — each m v'^2 is off by at most one
    # step of the precision, so the sum by at most eps_store K (nothing in fp64) — and to the rounding in double of the K the
    # scale factor was derived from: the device's sums (depth below 24 additions of half an eps64: 12 eps64), the two roundings
    # of alpha (v - V_cm), squared (2 eps64), and this test's own products and pairwise sum (below 8 eps64): 32 eps64 covers them
    for remove in (True, False):
        th = _thermostat(T, tau=0, frequency=10, remove_com=remove, seed=13)
        s = _sys(vel0, prec)
        th.apply(s, mass_t, dt, ndof)
        rec = th.last.cpu().numpy()
        want = 0.5 * M.BOLTZMAN * T * (th.draws[:, 0] ** 2 + th.draws[:, 1])
        assert th.nf == ndof - (3 if remove else 0)
        assert np.abs(rec[:, 2] - want).max() <= 8 * EPS64 * want.max(), (rec[:, 2], want)
        v = s.vel.cpu().double().numpy()[:, on]
        K = 0.5 * (mass[on][None, :, None] * v * v).sum(axis=(1, 2))
        err = np.abs(K - want) / want
        print(f"tau = 0 {prec} remove_com = {remove}: K of the stored velocities vs (kT/2)(R1^2 + S): {err.max():.2e}")
        assert err.max() <= (np.finfo(np.float32).eps if prec == "f32" else 0.0) + 32 * EPS64
    # c = 1 without centre-of-mass removal: not written, bit for bit (tau so long that exp(-dt / tau) rounds to 1)
    th = _thermostat(T, tau=1e30, frequency=10, remove_com=False, seed=13)
    assert th.decay(dt) == 1.0
    s = _sys(vel0, prec)
    ref = _sys(vel0, prec)
    th.apply(s, mass_t, dt, ndof)
    view = torch.int32 if prec == "f32" else torch.int64
    assert torch.equal(s.vel.view(view), ref.vel.view(view))
    rec = th.last.cpu().numpy()
    assert (rec[:, 1] == 1.0).all() and np.array_equal(rec[:, 0], rec[:, 2]) and (rec[:, 3] == 0).all() and (th.heat() == 0).all()
    # all-zero velocities: unchanged, no NaN
    for remove in (True, False):
        th = _thermostat(T, tau=0.1, frequency=10, remove_com=remove, seed=13)
        z = _sys(np.zeros((R, N, 3)), prec)
        th.apply(z, mass_t, dt, ndof)
        assert torch.equal(z.vel.view(view), torch.zeros_like(z.vel).view(view))
        rec = th.last.cpu().numpy()
        assert (rec[:, 0] == 0).all() and (rec[:, 1] == 1.0).all() and (rec[:, 2] == 0).all() and np.isfinite(rec).all()


# ----------------------------------------------------------------------------- 4. the free-particle chain
@pytest.mark.parametrize("prec", ["f64", "f32"])
def test_free_particle_chain_equals_the_model(prec):
    """The chain of tests/test_thermostat_host.py on the device: the same K, application for application, hence the same mean
    and variance (held there to four block standard errors of the canonical values)."""
    mass, vel0 = M.chain_start(NP[prec])
    want = M.model_chain(fp32=prec == "f32")
    th = _thermostat(M.CHAIN_T, tau=0.01 / -np.log(M.CHAIN_C), frequency=10, seed=M.CHAIN_SEED)
    s = _sys(vel0, prec)
    dt = 1.0 / M.TIMEFACTOR
    rec = _run_chain(th, s, _mass_t(mass, prec), dt, 3 * M.CHAIN_NATOMS, M.CHAIN_LENGTH)
    assert th.nf == M.CHAIN_NF and abs(th.decay(dt) - M.CHAIN_C) < 1e-12
    K = rec[:, :, 2].T
    rel = float(np.max(np.abs(K - want) / want))
    print(f"free-particle chain {prec}: K_after device vs model over 4 x 8000 applications: {rel:.2e} (bar {REL_BAR[prec]:.1e})")
    assert rel <= REL_BAR[prec]
    for r, T in enumerate(M.CHAIN_T):
        mean, emean, var, evar, wmean, wvar = M.chain_statistics(K[r], T)
        assert abs(mean - wmean) <= 4 * emean and abs(var - wvar) <= 4 * evar, (T, mean, wmean, emean, var, wvar, evar)


# ----------------------------------------------------------------------------- 5. inside the integrator
def _box(prec, R=1, temps=(300.0,), constraints=None, timestep=1.0, seed=0, **integ_kw):
    from torchmd_amd.builders import tip3p_box, water_forcefield
    from torchmd_amd.forces import Forces
    from torchmd_amd.integrator import Integrator, maxwell_boltzmann
    from torchmd_amd.parameters import Parameters
    from torchmd_amd.systems import System

    dt = PREC[prec]
    mol, pos, box = tip3p_box(12, seed=seed)
    terms = ["lj", "electrostatics"] if constraints else WATER_TERMS
    par = Parameters(water_forcefield(mol), mol, WATER_TERMS, precision=dt)
    s = System(mol.numAtoms, R, dt, _dev())
    s.set_positions(np.repeat(pos[:, :, None], R, axis=2))
    s.set_box(box)
    torch.manual_seed(seed)
    v = torch.cat([maxwell_boltzmann(par.masses, T, 1) for T in temps]).double()
    m = par.masses.double().reshape(1, -1, 1)
    v = v - (m * v).sum(dim=1, keepdim=True) / m.sum()  # (no net momentum: the total kinetic energy is the thermostat's K)
    s.set_velocities(v.to(dt))
    f = Forces(par, terms=terms, cutoff=9.0, rfa=True)
    f.compute(s.pos, s.box, s.forces)
    integ = Integrator(s, f, timestep, _dev(), constraints=constraints, **integ_kw)
    return mol, par, s, f, integ


def _kinetic(s, masses):
    from torchmd_amd import _lib as L
    from torchmd_amd.integrator import _stream

    out = torch.zeros(s.vel.shape[0], dtype=torch.float64, device=s.vel.device)
    L.check(L.load().tmdhip_kinetic_energy(L.dtype_code(s.vel.dtype), s.vel.shape[0], s.vel.shape[1], s.vel.data_ptr(),
                                           masses.data_ptr(), out.data_ptr(), _stream(s.vel.device)), "tmdhip_kinetic_energy")
    return out.cpu().numpy()


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_integrator_equals_manual_rounds(prec, monkeypatch):
    monkeypatch.setenv("TMDHIP_LPA", "16")  # (a context picks its lanes per atom from the atoms that share a launch: pin it)
    th = _thermostat(300, tau=0.1, frequency=10, seed=21)
    mol, par, s, f, integ = _box(prec, thermostat=th)
    ek, pot, T = integ.step(50)
    assert f.stats(s.pos)["algorithm"] == "celllist" and th.applications == 5 and th.nf == 3 * mol.numAtoms - 3
    # the twin: five rounds of plain step(10) and an application by hand
    th2 = _thermostat(300, tau=0.1, frequency=10, seed=21)
    _, _, s2, f2, plain = _box(prec)
    recs, around = [], []
    for _ in range(5):
        ek2, pot2, _ = plain.step(10)
        k0 = _kinetic(s2, plain.masses)
        th2.apply(s2, plain.masses, plain.dt, 3 * mol.numAtoms)
        around.append((k0, _kinetic(s2, plain.masses)))
        recs.append(th2.last.cpu().numpy())
    assert torch.equal(s.pos, s2.pos) and torch.equal(s.vel, s2.vel)
    assert pot == pot2
    want_ek = recs[-1][:, 2].astype(NP[prec])
    assert np.array_equal(ek, want_ek) and ek.dtype == want_ek.dtype and np.array_equal(T, plain._temperature(want_ek))
    assert not np.array_equal(ek, ek2)  # (the kinetic energy returned is the one after the application)
    # heat: the records' sum, in their order; and the same from tmdhip_kinetic_energy around every application.  That kernel
    # sums in another order (64 eps64 K covers both sums), and it sees the velocities as stored: every m v'^2 within one step of
    # the precision of its exact value, so K_after within eps K (zero in fp64, where the store does not round)
    heat = np.zeros(1)
    for r in recs:
        heat = heat + (r[:, 2] - r[:, 0])
    assert np.array_equal(th.heat(), heat) and np.array_equal(th2.heat(), heat)
    outside = sum(a - b for b, a in around)
    Kmax = max(a.max() for _, a in around)
    bound = 5 * Kmax * (64 * EPS64 + (np.finfo(np.float32).eps if prec == "f32" else 0.0))
    print(f"integrator {prec}: heat {heat[0]:.6f}, from tmdhip_kinetic_energy {outside[0]:.6f}, difference {abs(heat[0] - outside[0]):.2e} "
          f"(bound {bound:.2e}); E_kin {ek[0]:.3f}")
    assert abs(heat[0] - outside[0]) <= bound
    assert abs(heat[0]) > 1e-3  # (the thermostat did something)


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_temperature_ladder_replicas_equal_their_runs_alone(prec, monkeypatch):
    monkeypatch.setenv("TMDHIP_LPA", "16")
    temps, seed = (280.0, 300.0, 320.0), 22
    th = _thermostat(temps, tau=0, frequency=10, seed=seed)
    mol, par, s, f, integ = _box(prec, R=3, temps=temps, thermostat=th)
    for _ in range(3):
        ek, pot, T = integ.step(10)
        want = 0.5 * M.BOLTZMAN * np.array(temps) * (th.draws[:, 0] ** 2 + th.draws[:, 1])
        # (the record holds it to four roundings in double; step() returns it in the precision of the run)
        assert np.abs(th.last[:, 2].cpu().numpy() - want).max() <= 8 * EPS64 * want.max()
        assert np.array_equal(ek, th.last[:, 2].cpu().numpy().astype(NP[prec]))
        assert np.abs(ek - want).max() <= (np.finfo(np.float32).eps if prec == "f32" else 8 * EPS64) * want.max()
    assert f.stats(s.pos)["algorithm"] == "celllist"
    for r in range(3):
        alone = _thermostat(temps[r], tau=0, frequency=10, seed=seed)
        alone.rng = M.generators(seed, 3)[r:r + 1]  # the key (seed, r)
        _, _, s1, f1, i1 = _box(prec, R=3, temps=temps)  # (the same start velocities, then replica r only)
        _, _, sa, fa, ia = _box(prec, R=1, temps=temps[:1], thermostat=alone)
        sa.pos.copy_(s1.pos[r:r + 1]), sa.vel.copy_(s1.vel[r:r + 1])
        fa.compute(sa.pos, sa.box, sa.forces)
        for _ in range(3):
            ek1, pot1, _ = ia.step(10)
        assert torch.equal(sa.pos[0], s.pos[r]) and torch.equal(sa.vel[0], s.vel[r]), r
        assert ek1[0] == ek[r] and np.array_equal(alone.draws[0], th.draws[r])
        f1.close(), fa.close()


# ----------------------------------------------------------------------------- 6. composition
@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_composes_with_constraints(prec):
    import _constraints as H
    from torchmd_amd.constraints import find_constraints

    worst = {}
    for name in ("thermostat", "plain"):
        th = _thermostat(300.0, tau=0.1, frequency=10, seed=23) if name == "thermostat" else None
        mol, par, s, f, integ = _box(prec, constraints="water", timestep=2.0, **({"thermostat": th} if th else {}))
        ek, pot, T = integ.step(100)
        assert np.isfinite(ek).all() and np.isfinite(pot).all()
        cs = find_constraints(par.masses, par.bond_params, par.angle_params, "water")
        pairs, d = cs.pairs()
        worst[name] = H.residuals(s.pos[0].cpu().double().numpy(), s.vel[0].cpu().double().numpy(), pairs, d)
        if th is not None:
            assert th.applications == 10 and th.nf == cs.ndof() - 3 == integ.constraints.ndof() - 3
    print(f"rigid tip3p_box(12) {prec}, 100 steps at 2 fs: worst bond error / velocity along a bond: with the thermostat "
          f"{worst['thermostat'][0]:.3e} / {worst['thermostat'][1]:.3e}, without {worst['plain'][0]:.3e} / {worst['plain'][1]:.3e}")
    assert worst["thermostat"][0] <= CONS_TOL[prec]
    assert worst["thermostat"][0] <= worst["plain"][0], worst


def test_composes_with_the_barostat():
    from torchmd_amd.barostat import MonteCarloBarostat

    th = _thermostat(300.0, tau=0.1, frequency=10, seed=24)
    bar = MonteCarloBarostat(1.0, 300.0, frequency=25, seed=24)
    mol, par, s, f, integ = _box("f32", thermostat=th, barostat=bar)
    for n in (20, 30):  # (a call that ends between two multiples of 25, and one that ends on a common multiple)
        ek, pot, T = integ.step(n)
        assert np.isfinite(ek).all() and np.isfinite(pot).all()
    assert th.applications == 5 and bar.attempts[0] == 2 and integ._nstep == 50
    assert np.array_equal(ek, th.last[:, 2].cpu().numpy().astype(np.float32))


def test_with_the_barostat_equals_the_composition_by_hand(monkeypatch):
    """Thermostat every 10 and Monte Carlo barostat every 25 steps, calls of 20 and 30: bit for bit plain `step` over the
    segments 10, 10 | 5, 5, 10, 10 with the application and then the attempt by hand where their multiples fall."""
    from torchmd_amd.barostat import MonteCarloBarostat

    monkeypatch.setenv("TMDHIP_LPA", "16")
    th = _thermostat(300.0, tau=0.1, frequency=10, seed=24)
    bar = MonteCarloBarostat(1.0, 300.0, frequency=25, seed=24)
    mol, par, s, f, integ = _box("f32", thermostat=th, barostat=bar)
    returned = [integ.step(n) for n in (20, 30)]

    th2 = _thermostat(300.0, tau=0.1, frequency=10, seed=24)
    bar2 = MonteCarloBarostat(1.0, 300.0, frequency=25, seed=24)
    _, _, s2, f2, plain = _box("f32")
    pots, recs, done = {}, [], 0
    for n in (10, 10, 5, 5, 10, 10):
        _, pot, _ = plain.step(n)
        done += n
        if done % 10 == 0:
            th2.apply(s2, plain.masses, plain.dt, 3 * mol.numAtoms)
        if done % 25 == 0:
            rec = bar2.attempt(s2, f2, pot)
            recs.append(rec)
            pot = [float(un if ok else u) for u, un, ok in zip(rec["U"], rec["U_new"], rec["accepted"])]
        pots[done] = pot
    assert plain._nstep == integ._nstep == 50 and th.applications == th2.applications == 5 and len(recs) == 2
    assert torch.equal(s.pos, s2.pos) and torch.equal(s.vel, s2.vel) and torch.equal(s.box, s2.box)
    assert returned[0][1] == pots[20] and returned[1][1] == pots[50]
    for ek, _, T in returned:
        assert ek.dtype == np.float32 and np.array_equal(T, integ._temperature(ek))
    assert np.array_equal(returned[1][0], th.last[:, 2].cpu().numpy().astype(np.float32))
    assert torch.equal(th.last, th2.last) and np.array_equal(th.heat(), th2.heat())
    assert bar.last.keys() == bar2.last.keys() == recs[-1].keys()
    for k in bar.last:
        assert np.array_equal(bar.last[k], bar2.last[k]), k
    assert np.array_equal(bar.max_dv, bar2.max_dv) and np.array_equal(bar.accepted, bar2.accepted)
    print(f"thermostat + barostat by hand: accepted {bar.accepted[0]} of {bar.attempts[0]}, heat {th.heat()[0]:.6f}, "
          f"E_pot {returned[1][1][0]:.4f}, E_kin {returned[1][0][0]:.4f}")


_CHILD = r"""
import json, os, sys
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
import numpy as np, torch, yaml
import test_gpu_driver as D
from _golden import load
from torchmd_amd import run as driver
from torchmd_amd.builders import TIP3P_FF
g = load("water291")
psf, pdb, ff = (os.path.join(TMP, n) for n in ("structure.psf", "structure.pdb", "water_forcefield.yaml"))
D._write_psf(psf, g); D._write_pdb(pdb, g)
open(ff, "w").write(yaml.safe_dump(TIP3P_FF))
conf = {"structure": [psf, pdb], "forcefield": ff, "forceterms": ["LJ", "Bonds", "Angles", "Electrostatics"], "cutoff": 7.3, "rfa": True,
        "replicas": 1, "precision": "single", "device": "cuda", "timestep": 1, "temperature": 300, "langevin_gamma": 1.0,
        "langevin_temperature": 300, "seed": 1, "steps": 100, "output_period": 50, "save_period": 0, "log_dir": os.path.join(TMP, "log"),
        "output": "output"}
out = {}
def go(name, **kw):
    c = dict(conf, log_dir=os.path.join(TMP, name), **kw)
    open(os.path.join(TMP, name + ".yaml"), "w").write(yaml.safe_dump(c))
    driver.main(["--conf", os.path.join(TMP, name + ".yaml")])
    log = os.path.join(TMP, name)
    out[name] = {"files": sorted(os.listdir(log)), "rows": open(os.path.join(log, "monitor_0.csv")).read().splitlines()}
go("log")
out["module_after_off"] = "torchmd_amd.thermostat" in sys.modules
go("log_csvr", thermostat="csvr", thermostat_tau=0.05, thermostat_frequency=10, langevin_temperature=0, replicas=2,
   thermostat_temperature=[280, 320])
print("RESULT " + json.dumps(out))
"""


def test_run_py_with_and_without_the_key(tmp_path):
    code = f"ROOT = {ROOT!r}\nTMP = {str(tmp_path)!r}\n" + _CHILD
    res = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-4000:]
    out = json.loads(next(ln for ln in res.stdout.splitlines() if ln.startswith("RESULT "))[7:])
    # without the key: the thermostat module is never imported and the files are what they were
    assert out["module_after_off"] is False
    assert out["log"]["files"] == ["input.yaml", "monitor_0.csv", "output_0.npy"]
    assert out["log"]["rows"][0] == "iter,ns,epot,ekin,etot,T,t" and len(out["log"]["rows"]) == 3
    # with it: a ladder of two replicas, monitor rows for both
    assert out["log_csvr"]["files"] == ["input.yaml", "monitor_0.csv", "monitor_1.csv", "output_0.npy", "output_1.npy"]
    rows = out["log_csvr"]["rows"]
    assert rows[0] == "iter,ns,epot,ekin,etot,T,t" and len(rows) == 3
    assert all(np.isfinite([float(x) for x in r.split(",")]).all() for r in rows[1:])


# ----------------------------------------------------------------------------- 7. what is refused on the device
def test_refusals_on_the_device():
    mol, par, s, f, integ = _box("f32", R=1)
    from torchmd_amd.integrator import Integrator

    with pytest.raises(ValueError, match="replicas"):
        Integrator(s, f, 1.0, _dev(), thermostat=_thermostat([280.0, 300.0]))
    with pytest.raises(ValueError, match="Langevin"):
        Integrator(s, f, 1.0, _dev(), gamma=0.1, T=300.0, thermostat=_thermostat(300.0))
    th = _thermostat([280.0, 300.0])
    with pytest.raises(ValueError, match="replicas"):  # a ladder of two applied to one replica
        th.apply(s, integ.masses, integ.dt, 3 * mol.numAtoms)
    th = _thermostat(300.0)
    with pytest.raises(RuntimeError, match="masses"):
        th.apply(s, integ.masses.double(), integ.dt, 3 * mol.numAtoms)
    with pytest.raises(RuntimeError, match="device"):
        th.apply(types.SimpleNamespace(vel=s.vel.cpu()), integ.masses, integ.dt, 3 * mol.numAtoms)
    v0 = s.vel.clone()
    assert th.applications == 0 and torch.equal(s.vel, v0)
