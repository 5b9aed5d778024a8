"""Temperature replica exchange on the device: tmdhip_velocity_rescale against the numpy model of
tests/_exchange.py, its stride and chunk edges, the exchange inside `Integrator.step` on the cell-list path against the manual
composition of its parts, with one replica, with constraints, and from run.py.

Bars against the model: the new velocity is one IEEE product in double and one rounding to the run's precision, which the
model takes in the same way, so velocities are equal bit for bit.  K_before is a sum of N positive terms the device takes in
another order than the model (math.fsum: exact): any order of summation stays within N eps64 of it, relatively."""

import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import _exchange as M
import _reduce as RM
from _golden import PREC

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WATER_TERMS = ["lj", "electrostatics", "bonds", "angles"]
NP = {"f32": np.float32, "f64": np.float64}
EPS64 = np.finfo(np.float64).eps
EPS32 = np.finfo(np.float32).eps
CONS_TOL = {"f32": 3e-5, "f64": 1e-10}  # bond length (relative) of constrained dynamics (tests/test_gpu_constraints.py)
LADDER = (300.0, 302.0, 304.0, 306.0)


def _dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _bits(t):
    return t.cpu().contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int64)


def _start(R, N, prec, seed):
    """Masses {1.008, 15.999, 0} in turn and velocities, both already rounded to the precision; every massless row holds
    NaNs."""
    rng = np.random.default_rng(seed)
    mass = np.array([1.008, 15.999, 0.0])[np.arange(N) % 3].astype(NP[prec]).astype(np.float64)
    vel = 0.05 * rng.standard_normal((R, N, 3)) + np.array([0.01, -0.02, 0.005])
    vel[:, mass == 0] = np.nan
    return mass, vel.astype(NP[prec]).astype(np.float64)


class _Rescaler:
    """tmdhip_velocity_rescale by hand: its own record and scratch."""

    def __init__(self, R):
        import ctypes as C

        from torchmd_amd import _lib as L

        nrec, npart = C.c_int64(), C.c_int64()
        L.check(L.load().tmdhip_velocity_rescale_workspace(R, C.byref(nrec), C.byref(npart)), "tmdhip_velocity_rescale_workspace")
        assert nrec.value == R * L.EXCHANGE_RECORD_DOUBLES and npart.value == R * L.EXCHANGE_MAX_BLOCKS
        self.record = torch.zeros(R, 5, dtype=torch.float64, device=_dev())
        self.partials = torch.empty(npart.value, dtype=torch.float64, device=_dev())

    def __call__(self, vel, mass, factors, check=True):
        import ctypes as C

        from torchmd_amd import _lib as L
        from torchmd_amd.integrator import _stream

        f = np.ascontiguousarray(factors, dtype=np.float64)
        assert len(f) == vel.shape[0]
        rc = L.load().tmdhip_velocity_rescale(L.dtype_code(vel.dtype), vel.shape[0], vel.shape[1], vel.data_ptr(), mass.data_ptr(),
                                              f.ctypes.data_as(C.POINTER(C.c_double)), self.record.data_ptr(),
                                              self.partials.data_ptr(), _stream(vel.device))
        return L.check(rc, "tmdhip_velocity_rescale") if check else rc


def _tensor(a, prec):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=PREC[prec]).to(_dev()).contiguous()


def _against_model(what, prec, R, N, factors, ncalls, seed):
    """`ncalls` applications on the device and in the model: velocities bit for bit, records within N eps64."""
    mass, vel0 = _start(R, N, prec, seed)
    on = mass > 0
    mass_t = _tensor(mass, prec)

    def device():
        resc, v = _Rescaler(R), _tensor(vel0, prec)
        recs = []
        for _ in range(ncalls):
            resc(v, mass_t, factors)
            recs.append(resc.record.clone())
        return v, torch.stack(recs).cpu().numpy()

    v, rec = device()
    vel = vel0.copy()
    want = np.array([[M.rescale(vel[r], mass, float(factors[r]), NP[prec]) for r in range(R)] for _ in range(ncalls)])
    got = v.cpu().double().numpy()
    assert np.isfinite(got[:, on]).all() and np.isfinite(rec).all()
    assert np.array_equal(got[:, on], vel[:, on]), np.abs(got[:, on] - vel[:, on]).max()
    start_bits = _bits(_tensor(vel0, prec))
    assert torch.equal(_bits(v)[:, ~on], start_bits[:, ~on]) and np.isnan(vel0[:, ~on]).all()  # massless rows: untouched
    for r in range(R):
        if factors[r] == 1.0:
            assert torch.equal(_bits(v)[r], start_bits[r])  # never written
            assert np.array_equal(rec[:, r, 0], rec[:, r, 2]) and (rec[:, r, 3] == 0).all()
        else:
            assert not torch.equal(_bits(v)[r], start_bits[r]) and not np.array_equal(got[r, on][-1], vel0[r, on][-1])
    bar = N * EPS64
    relb = float(np.max(np.abs(rec[:, :, 0] - want[:, :, 0]) / want[:, :, 0]))
    rela = float(np.max(np.abs(rec[:, :, 2] - want[:, :, 2]) / want[:, :, 2]))
    assert np.array_equal(rec[:, :, 1], np.broadcast_to(np.asarray(factors, dtype=np.float64), (ncalls, R)))
    assert np.array_equal(rec[:, :, 4], np.broadcast_to(np.arange(1, ncalls + 1)[:, None], (ncalls, R)))
    # work: the device adds K_after - K_before call by call; each K within N eps64 of the model's, so each difference within
    # N eps64 (K_before + K_after), and the roundings of the ncalls additions are far below that
    work = np.cumsum(want[:, :, 2] - want[:, :, 0], axis=0)
    wbar = bar * np.cumsum(want[:, :, 2] + want[:, :, 0], axis=0)
    werr = np.abs(rec[:, :, 3] - work)
    print(f"{what} {prec}: velocities equal bit for bit; device vs model, worst relative difference K_before {relb:.2e}, "
          f"K_after {rela:.2e} (bar {bar:.1e}); work {float((werr / wbar).max()):.2e} of its bar")
    assert relb <= bar and rela <= bar and (werr <= wbar).all()
    # work is the sum of K_after - K_before of the records, added in the order of the applications
    acc = np.zeros(R)
    for k in range(ncalls):
        acc = acc + (rec[k, :, 2] - rec[k, :, 0])
    assert np.array_equal(rec[-1, :, 3], acc)
    v2, rec2 = device()  # two runs give the same bits
    assert torch.equal(_bits(v2), _bits(v)) and np.array_equal(rec2, rec)


# ----------------------------------------------------------------------------- 1. the kernel against the model
@pytest.mark.parametrize("prec", ["f64", "f32"])
def test_kernel_against_the_model(prec):
    _against_model("kernel, R = 3, N = 1000, 20 calls", prec, 3, 1000, [np.sqrt(320.0 / 280.0), 1.0, np.sqrt(280.0 / 320.0)], 20, 1)


# ----------------------------------------------------------------------------- 2. stride and chunk edges
@pytest.mark.parametrize("prec", ["f64", "f32"])
def test_stride_loop(prec):
    """70 001 atoms: more than 256 blocks x 256 threads, so every reduction block takes more than one atom per thread, and the
    update grid (274 blocks) is larger than the reduction grid."""
    _against_model("stride loop, N = 70 001", prec, 1, 70001, [np.sqrt(310.0 / 300.0)], 1, 2)


@pytest.mark.parametrize("prec", ["f64", "f32"])
def test_chunk_edge(prec):
    """17 replicas: two pairs of launches, the second for one replica; distinct factors, one of them 1."""
    factors = np.sqrt((300.0 + 5.0 * np.arange(17)) / 340.0)
    assert factors[8] == 1.0 and len(set(factors)) == 17
    _against_model("chunk edge, R = 17, N = 300", prec, 17, 300, factors, 2, 3)


@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("N", RM.SHAPES)
def test_partial_rows_and_record_bit_for_bit(N, prec):
    """The order of the fixed-order sum (tests/_reduce.py): every partial row exchange_reduce_kernel writes and the record's
    K_before against the model, addition by addition.  The four wave sums meet in sequence here."""
    mass, vel = RM.velocities(2, N, prec, 7)
    on = mass > 0
    factors = [1.0, np.sqrt(310.0 / 300.0)]
    resc = _Rescaler(2)
    resc.partials.fill_(float("nan"))
    resc(_tensor(vel, prec), _tensor(mass, prec), factors)
    rows = resc.partials.cpu().numpy().reshape(2, -1)
    rec = resc.record.cpu().numpy()
    nb = RM.nblocks_of(N)
    for r in range(2):
        want = RM.partial_rows(RM.mv2(mass, vel[r]), on, RM.SEQUENTIAL)
        differ = int((rows[r, :nb].view(np.int64) != want.view(np.int64)).sum())
        K = 0.5 * RM.fold(want)
        print(f"N = {N} {prec} replica {r}: {differ} of {nb} partial rows differ from the model; K_before {rec[r, 0]!r}, model {K!r}")
        assert differ == 0 and np.isnan(rows[r, nb:]).all()  # (rows past the grid are never written)
        assert rec[r, 0] == K and rec[r, 2] == (factors[r] * factors[r]) * K


def test_refusals_of_the_c_interface():
    from torchmd_amd import _lib as L

    mass, vel0 = _start(2, 30, "f32", 4)
    v, m = _tensor(vel0, "f32"), _tensor(mass, "f32")
    resc = _Rescaler(2)
    before = _bits(v).clone()
    for bad in ([1.0, 0.0], [-1.0, 1.0], [np.nan, 1.0], [1.0, np.inf]):
        assert resc(v, m, bad, check=False) < 0 and "factor" in L.last_error()
    lib = L.load()
    f = np.ones(2)
    fp = f.ctypes.data_as(L.C.POINTER(L.C.c_double))
    st = L.C.c_void_p(torch.cuda.current_stream(_dev()).cuda_stream)
    args = lambda **kw: [kw.get("dtype", L.F32), kw.get("R", 2), kw.get("N", 30), kw.get("vel", v.data_ptr()), m.data_ptr(),  # noqa: E731
                         kw.get("f", fp), kw.get("rec", resc.record.data_ptr()), resc.partials.data_ptr(), st]
    for kw, word in ((dict(dtype=7), "dtype"), (dict(R=0), "nreplicas"), (dict(R=65536), "nreplicas"), (dict(N=0), "natoms"),
                     (dict(vel=None), "null"), (dict(f=None), "null"), (dict(rec=None), "null")):
        assert lib.tmdhip_velocity_rescale(*args(**kw)) < 0 and word in L.last_error(), kw
    assert lib.tmdhip_velocity_rescale_workspace(0, None, None) < 0
    torch.cuda.synchronize()
    assert torch.equal(_bits(v), before) and (resc.record == 0).all()  # nothing was launched


# ----------------------------------------------------------------------------- 3. inside the integrator
def _box(prec, R=1, temps=(300.0,), constraints=None, timestep=1.0, seed=0, **integ_kw):
    """The 5 184-atom water box of tests/test_gpu_thermostat.py."""
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


def _parts(temps=LADDER, seed=31, frequency=20):
    from torchmd_amd.exchange import ReplicaExchange
    from torchmd_amd.thermostat import VelocityRescale

    return VelocityRescale(list(temps), tau=0.1, frequency=10, seed=seed), ReplicaExchange(frequency=frequency, seed=seed)


def _watch(ex, around):
    """Have `ex.attempt` take tmdhip_kinetic_energy of the velocities before and after itself."""
    inner = ex.attempt

    def attempt(system, masses, thermostat, epot):
        k0 = _kinetic(system, masses)
        rec = inner(system, masses, thermostat, epot)
        around.append((k0, _kinetic(system, masses)))
        return rec

    ex.attempt = attempt


def _check_work(what, prec, ex, around, ek):
    """work() against tmdhip_kinetic_energy around every attempt.  That kernel sums in another order (64 eps64 K covers both
    sums), and it sees the velocities as stored: every m v'^2 within one step of the precision of its exact value, so K_after
    within eps K (zero in fp64, where the record's factor^2 K and the stored factor v differ by roundings in double only):
    the bound of tests/test_gpu_thermostat.py::test_integrator_equals_manual_rounds, per attempt."""
    outside = sum(a - b for b, a in around)
    Kmax = max(a.max() for _, a in around)
    bound = len(around) * Kmax * (64 * EPS64 + (EPS32 if prec == "f32" else 0.0))
    work = ex.work()
    print(f"{what} {prec}: work {work}, from tmdhip_kinetic_energy {outside}, difference {np.abs(work - outside).max():.2e} "
          f"(bound {bound:.2e})")
    assert np.abs(work - outside).max() <= bound
    want = ex.last[:, 2].cpu().numpy().astype(NP[prec])
    assert np.array_equal(ek, want) and ek.dtype == want.dtype


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_every_pair_accepted_walks_the_ladder(prec, monkeypatch):
    monkeypatch.setenv("TMDHIP_LPA", "16")  # (a context picks its lanes per atom from the atoms that share a launch: pin it)
    th, ex = _parts()
    ex.rng = M.Counting(0.0)  # u = 0 < exp(Delta): every tried pair is accepted
    around = []
    _watch(ex, around)
    mol, par, s, f, integ = _box(prec, R=4, temps=LADDER, thermostat=th, exchange=ex)
    ek, pot, T = integ.step(80)
    assert f.stats(s.pos)["algorithm"] == "celllist" and th.applications == 8 and ex.nattempts == 4 and len(around) == 4
    # odd-even transposition: four rounds reverse four rungs
    assert [h.tolist() for h in ex.history] == [[1, 0, 3, 2], [2, 0, 3, 1], [3, 1, 2, 0], [3, 2, 1, 0]]
    assert ex.rungs.tolist() == [3, 2, 1, 0] and ex.rng.count == 6
    assert ex.attempts.tolist() == [2, 2, 2] and np.array_equal(ex.accepted, ex.attempts)
    assert th.temperatures.tolist() == [306.0, 304.0, 302.0, 300.0] and ex.ladder.tolist() == list(LADDER)
    assert np.isfinite(ex.record["delta"]).all() and ex.record["accepted"].all() and ex.record["pairs"].tolist() == [[1, 2]]
    assert ex.record["factors"].tolist() == [1.0, np.sqrt(304.0 / 302.0), np.sqrt(302.0 / 304.0), 1.0]
    assert np.array_equal(ex.last[:, 1].cpu().numpy(), ex.record["factors"]) and (ex.last[:, 4] == 4).all()
    assert np.array_equal(T, integ._temperature(ek)) and np.isfinite(pot).all()
    _check_work("all accepted", prec, ex, around, ek)
    assert np.abs(ex.work()).min() > 1e-3  # (every slot was rescaled)


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_integrator_equals_manual_composition(prec, monkeypatch):
    from torchmd_amd.exchange import exchange_decisions

    monkeypatch.setenv("TMDHIP_LPA", "16")
    th, ex = _parts()
    around = []
    _watch(ex, around)
    mol, par, s, f, integ = _box(prec, R=4, temps=LADDER, thermostat=th, exchange=ex)
    records = []
    for n in (30, 50):  # (a call that ends on an application only, and one that ends on an attempt)
        ek, pot, T = integ.step(n)
        records.append((ek, ex.nattempts))
    assert f.stats(s.pos)["algorithm"] == "celllist" and th.applications == 8 and ex.nattempts == 4
    # the twin: plain step(10) segments, the thermostat and the exchange by hand
    th2, _ = _parts()
    _, _, s2, f2, plain = _box(prec, R=4, temps=LADDER)
    resc = _Rescaler(4)
    g = np.random.Generator(np.random.Philox(key=np.array([31, 0], dtype=np.uint64)))
    ladder, rungs, history, ek30 = np.array(LADDER), np.arange(4), [], None
    for seg in range(8):
        ek2, pot2, _ = plain.step(10)
        th2.apply(s2, plain.masses, plain.dt, 3 * mol.numAtoms)
        if seg == 2:
            ek30 = th2.last[:, 2].cpu().numpy().astype(NP[prec])
        if seg % 2 == 1:
            parity = (seg // 2) % 2
            u = [g.random() for _ in M.pairs_of(parity, 4)]
            new, acc, delta, pairs = exchange_decisions(pot2, ladder, rungs, parity, u)
            mr, ma, md = M.decide(pot2, ladder, rungs, parity, u)
            assert np.array_equal(new, mr) and np.array_equal(acc, ma) and np.array_equal(delta, md)
            factors = np.where(new != rungs, np.sqrt(ladder[new] / ladder[rungs]), 1.0)
            resc(s2.vel, plain.masses, factors)
            th2.temperatures[:] = ladder[new]
            rungs = new
            history.append(new.copy())
            assert np.array_equal(ex.history[seg // 2], new)
    assert torch.equal(s.pos, s2.pos) and torch.equal(s.vel, s2.vel)
    assert pot == pot2 and np.array_equal(records[0][0], ek30) and records[0][1] == 1
    assert np.array_equal(ex.rungs, rungs) and [h.tolist() for h in ex.history] == [h.tolist() for h in history]
    assert np.array_equal(ex.record["U"], np.array(pot2)) and np.array_equal(ex.record["u"], np.array(u))
    assert np.array_equal(ex.record["delta"], delta) and np.array_equal(ex.record["accepted"], acc)
    assert np.array_equal(ex.record["pairs"], pairs) and np.array_equal(ex.record["factors"], factors)
    assert torch.equal(ex.last, resc.record) and np.array_equal(ex.work(), resc.record[:, 3].cpu().numpy())
    assert np.array_equal(th.temperatures, th2.temperatures) and np.array_equal(th.temperatures, ladder[rungs])
    assert np.array_equal(th.heat(), th2.heat()) and np.array_equal(th.draws, th2.draws)
    assert ex.attempts.tolist() == [2, 2, 2] and (ex.accepted <= ex.attempts).all()
    print(f"manual composition {prec}: rungs {[h.tolist() for h in history]}, accepted {ex.accepted.tolist()} of {ex.attempts.tolist()}")
    _check_work("real generator", prec, ex, around, ek)


# ----------------------------------------------------------------------------- 4. edges
@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_one_replica_is_the_run_without_exchange(prec, monkeypatch):
    monkeypatch.setenv("TMDHIP_LPA", "16")
    th, ex = _parts(temps=(300.0,))
    mol, par, s, f, integ = _box(prec, thermostat=th, exchange=ex)
    ek, pot, T = integ.step(40)
    th2, _ = _parts(temps=(300.0,))
    _, _, s2, f2, alone = _box(prec, thermostat=th2)
    ek2, pot2, T2 = alone.step(40)
    assert ex.nattempts == 2 and ex.rungs.tolist() == [0] and len(ex.attempts) == 0 and (ex.work() == 0).all()
    assert torch.equal(s.pos, s2.pos) and torch.equal(s.vel, s2.vel) and pot == pot2
    # the kinetic energy returned is the exchange record's, the run without it returns the thermostat's alpha^2 K: the same
    # sum in another order (64 eps64 K covers both) over velocities as stored (every m v'^2 within one step of the precision:
    # eps32 K in fp32, nothing in fp64), and both are returned rounded to the run's precision (half a step each in fp32)
    assert np.abs(ek.astype(np.float64) - ek2) <= (2 * EPS32 if prec == "f32" else 64 * EPS64) * ek2


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_composes_with_constraints(prec):
    import _constraints as H
    from torchmd_amd.constraints import find_constraints

    temps = (300.0, 302.0, 304.0)
    worst = {}
    for name in ("exchange", "plain"):
        th, ex = _parts(temps=temps)
        ex.rng = M.Counting(0.0)
        kw = {"exchange": ex} if name == "exchange" else {}
        mol, par, s, f, integ = _box(prec, R=3, temps=temps, constraints="water", timestep=2.0, thermostat=th, **kw)
        ek, pot, T = integ.step(40)
        assert np.isfinite(ek).all() and np.isfinite(pot).all()
        cs = find_constraints(par.masses, par.bond_params, par.angle_params, "water")
        pairs, d = cs.pairs()
        res = [H.residuals(s.pos[r].cpu().double().numpy(), s.vel[r].cpu().double().numpy(), pairs, d) for r in range(3)]
        worst[name] = (max(r[0] for r in res), max(r[1] for r in res))
        if name == "exchange":
            assert ex.nattempts == 2 and ex.rungs.tolist() == [2, 0, 1] and np.array_equal(ex.accepted, ex.attempts)
    print(f"rigid tip3p_box(12) {prec}, 3 replicas, 40 steps at 2 fs: worst bond error / velocity along a bond: with exchange "
          f"{worst['exchange'][0]:.3e} / {worst['exchange'][1]:.3e}, without {worst['plain'][0]:.3e} / {worst['plain'][1]:.3e}")
    assert worst["exchange"][0] <= CONS_TOL[prec]
    assert worst["exchange"][0] <= worst["plain"][0], worst


# ----------------------------------------------------------------------------- 5. run.py
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
        "replicas": 3, "precision": "single", "device": "cuda", "timestep": 1, "temperature": 300, "langevin_temperature": 0,
        "thermostat": "csvr", "thermostat_tau": 0.05, "thermostat_frequency": 10, "thermostat_temperature": [290, 300, 310],
        "seed": 1, "steps": 100, "output_period": 50, "save_period": 0, "log_dir": os.path.join(TMP, "log"), "output": "output"}
out = {}
def go(name, **kw):
    c = dict(conf, log_dir=os.path.join(TMP, name), **kw)
    open(os.path.join(TMP, name + ".yaml"), "w").write(yaml.safe_dump(c))
    driver.main(["--conf", os.path.join(TMP, name + ".yaml")])
    log = os.path.join(TMP, name)
    out[name] = {"files": sorted(os.listdir(log)), "rows": [open(os.path.join(log, f"monitor_{k}.csv")).read().splitlines() for k in range(3)]}
go("log")
out["module_after_off"] = "torchmd_amd.exchange" in sys.modules
go("log_remd", exchange_frequency=25, exchange_seed=5)
out["json"] = json.load(open(os.path.join(TMP, "log_remd", "exchange.json")))
print("RESULT " + json.dumps(out))
"""


def test_run_py_with_and_without_the_key(tmp_path):
    code = f"ROOT = {ROOT!r}\nTMP = {str(tmp_path)!r}\n" + _CHILD
    res = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-4000:]
    out = json.loads(next(ln for ln in res.stdout.splitlines() if ln.startswith("RESULT "))[7:])
    files = ["input.yaml"] + [f"monitor_{k}.csv" for k in range(3)] + [f"output_{k}.npy" for k in range(3)]
    # without the key: the exchange module is never imported and the files are what they were
    assert out["module_after_off"] is False
    assert out["log"]["files"] == files
    assert all(rows[0] == "iter,ns,epot,ekin,etot,T,t" and len(rows) == 3 for rows in out["log"]["rows"])
    # with it: a rung column in every monitor file, and the counts at the end
    assert out["log_remd"]["files"] == sorted(files + ["exchange.json"])
    last = []
    for rows in out["log_remd"]["rows"]:
        assert rows[0] == "iter,ns,epot,ekin,etot,T,rung,t" and len(rows) == 3
        vals = [[float(x) for x in r.split(",")] for r in rows[1:]]
        assert np.isfinite(vals).all() and all(v[6] in (0.0, 1.0, 2.0) for v in vals)
        last.append(int(vals[-1][6]))
    j = out["json"]
    assert sorted(last) == [0, 1, 2] and j["rungs"] == last
    assert j["frequency"] == 25 and j["seed"] == 5 and j["temperatures"] == [290.0, 300.0, 310.0]
    assert j["attempts"] == [2, 2] and len(j["accepted"]) == 2 and all(0 <= a <= 2 for a in j["accepted"])
