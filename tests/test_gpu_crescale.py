"""The stochastic cell-rescaling barostat on the GPU: `tmdhip_rescale_molecules` against the numpy model of
tests/_crescale.py, `Integrator(barostat=CRescaleBarostat(...))` against a composition made by hand of `step`, the pressure, the
model's mu and the kernel, the Berendsen limit, constraints, per-replica targets, the NPT volume distribution of an ideal gas,
and run.py.

Bars of the kernel test.  The shift of a molecule is formed in double from at most 200 addends, so each coordinate lies within
1 ulp_R(|x|) + 256 eps64 max|x| of the model's float64 result rounded to R; the same for velocities.  Distance vectors and
relative velocities inside a molecule see two roundings of a common shift: 2 ulp_R.  K: any order of N additions of products of
three roundings: (N + 8) eps64 sum |m v^2|.

Twin runs that cannot be bit for bit are held to the bars of `_twin_bars`: the suite's own where it has one (fp64 positions 1e-9 A,
forces FTOL, energies ERTOL * EFAC), derived from the formats as tests/test_gpu_barostat.py derives its fp32 position bar where it
has none; the observed differences are printed and recorded in DESIGN §20.

Observed (MI355X).  Constraints, 864-atom TIP4P-Ew, rigid water, PME, 200 steps at 2 fs, worst relative O-H / H-H length error
with / without the barostat: see DESIGN §20.  Ideal gas, 8 000 applications: see DESIGN §20."""

import csv
import ctypes as C

import numpy as np
import pytest
import torch

import _crescale as M
import _reduce as RM
from _golden import PREC, GoldenParameters, load

pytestmark = pytest.mark.gpu

EPS64 = float(np.finfo(np.float64).eps)
NP = {"f32": np.float32, "f64": np.float64}
WATER_TERMS = ["lj", "electrostatics", "bonds", "angles"]
# the suite's bars where force atomics make a run non-reproducible (tests/test_gpu_barostat.py): forces, energies (ERTOL * EFAC of
# max(1, |E|)), fp64 positions of two runs of the same steps
FTOL = {"f64": 1e-8, "f32": 3e-4}
ERTOL = {"f64": 1e-10, "f32": 2e-5}
EFAC = 3
XTOL64 = 1e-9
M_H, K_OH = 1.008, 450.0  # the lightest mass; the stiffest term of the flexible waters, E = k (r - r0)^2


def _dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _ulp(x, prec):
    return np.spacing(np.abs(np.asarray(x, dtype=np.float64)).astype(NP[prec])).astype(np.float64)


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int64)


# ----------------------------------------------------------------------------- 1. the kernel against the model
SIZES = [1] * 5 + [3] * 3 + [4] * 3 + [64, 65, 200]
NREP, UNIT = 17, 5  # more than one launch of 16; replica UNIT has factors exactly 1
_TABLE = {}


def _table():
    """A molecule table over a shuffled set of atoms: the CSR, the masses (the fourth atom of a four-atom molecule has none) and,
    per replica, positions, velocities and factors."""
    if not _TABLE:
        rng = np.random.default_rng(20)
        N = sum(SIZES)
        off = np.concatenate([[0], np.cumsum(SIZES)]).astype(np.int32)
        mem = rng.permutation(N).astype(np.int32)
        mass = rng.uniform(1.0, 16.0, N)
        massless = np.array([mem[off[g] + 3] for g, n in enumerate(SIZES) if n == 4])
        mass[massless] = 0.0
        pos = rng.uniform(-5.0, 45.0, (NREP, N, 3))
        vel = rng.normal(size=(NREP, N, 3)) * 0.01
        scale = 1.0 + rng.uniform(-3e-3, 3e-3, (NREP, 3))
        scale[UNIT] = 1.0
        scale[2, 1] = 1.0  # one axis alone at exactly 1
        _TABLE.update(N=N, off=off, mem=mem, mass=mass, massless=massless, pos=pos, vel=vel, scale=scale)
    return _TABLE


def _launch(prec, t):
    from torchmd_amd import crescale as X

    dev, dt = _dev(), PREC[prec]
    p = torch.as_tensor(t["pos"]).to(dt).to(dev).contiguous()
    v = torch.as_tensor(t["vel"]).to(dt)
    v[:, torch.as_tensor(t["massless"].astype(np.int64))] = float("inf")  # (a Maxwell-Boltzmann draw of a massless row: never read)
    v = v.to(dev).contiguous()
    m = torch.as_tensor(t["mass"]).to(dt).to(dev)
    off, mem = torch.as_tensor(t["off"], device=dev), torch.as_tensor(t["mem"], device=dev)
    nrec, npart = C.c_int64(), C.c_int64()
    from torchmd_amd import _lib as L

    L.check(L.load().tmdhip_rescale_molecules_workspace(NREP, len(t["off"]) - 1, C.byref(nrec), C.byref(npart)), "workspace")
    assert nrec.value == 2 * NREP and npart.value == 2 * NREP * (1 + 64) + (len(SIZES) + 2) // 2  # (rows of partials, the list of big molecules)
    rec = torch.full((NREP, 2), float("nan"), dtype=torch.float64, device=dev)
    part = torch.full((npart.value,), float("nan"), dtype=torch.float64, device=dev)
    p0, v0 = p.clone(), v.clone()
    X.rescale_molecules(p, v, m, t["scale"], off, mem, True, rec, part)
    torch.cuda.synchronize()
    return p0, v0, p, v, m, rec


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_kernel_against_model(prec):
    t = _table()
    p0, v0, p, v, m, rec = _launch(prec, t)
    x0, u0, mass = p0.cpu().double().numpy(), v0.cpu().double().numpy(), m.cpu().double().numpy()
    x1, u1, K = p.cpu().double().numpy(), v.cpu().double().numpy(), rec.cpu().numpy()
    off, mem, N = t["off"], t["mem"], t["N"]
    massless, massive = t["massless"], mass > 0
    assert np.isinf(u0[:, massless]).all() and torch.equal(_bits(v[:, massless]), _bits(v0[:, massless]))
    u0[:, massless] = u1[:, massless] = 0.0
    worst = [0.0, 0.0, 0.0, 0.0]
    for r in range(NREP):
        s = t["scale"][r]
        wx, wu = M.rescale_molecules(x0[r], u0[r], mass, s, off, mem)
        for got, want, old, k in ((x1[r], wx, x0[r], 0), (u1[r], wu, u0[r], 1)):
            rounded = want.astype(NP[prec]).astype(np.float64)
            bar = _ulp(want, prec) + 256 * EPS64 * np.abs(old).max()
            err = np.abs(got - rounded)
            worst[k] = max(worst[k], (err / bar).max())
            assert (err <= bar).all(), (r, k, (err / bar).max())
        for g in range(len(off) - 1):
            a = mem[off[g]:off[g + 1]]
            w = a[massive[a]]
            # rigid: distance vectors and relative velocities inside the molecule
            for new, old, idx in ((x1[r], x0[r], a), (u1[r], u0[r], w)):
                d = np.abs((new[idx] - new[idx[0]]) - (old[idx] - old[idx[0]]))
                bar = 2 * _ulp(np.maximum(np.abs(new[idx]), np.abs(old[idx])).max(axis=0), prec)
                worst[2] = max(worst[2], (d / bar).max())
                assert (d <= bar).all(), (r, g)
            # the molecule's momentum is divided by s
            mom0, mom1 = (mass[w, None] * u0[r][w]).sum(axis=0), (mass[w, None] * u1[r][w]).sum(axis=0)
            bar = (mass[w, None] * (_ulp(u1[r][w], prec) + 256 * EPS64 * np.abs(u0[r]).max())).sum(axis=0) + 4 * EPS64 * np.abs(mom0)
            assert (np.abs(mom1 - mom0 / s) <= bar).all(), (r, g)
        for k, u in ((0, u0[r]), (1, u1[r])):
            want, scale = M.kinetic(mass, u)
            worst[3] = max(worst[3], abs(K[r, k] - want) / (EPS64 * scale))
            assert abs(K[r, k] - want) <= (N + 8) * EPS64 * scale, (r, k)
        assert (s != 1.0).any() == (K[r, 0] != K[r, 1]) or r == UNIT
    print(f"{prec}: worst position {worst[0]:.3f} and velocity {worst[1]:.3f} of their bars, rigidity {worst[2]:.3f} of 2 ulp, "
          f"K {worst[3]:.1f} eps64 sum|m v^2| (bar {N + 8})")
    # factors exactly 1: the replica keeps its bits, and an axis at 1 keeps that column
    assert torch.equal(_bits(p[UNIT]), _bits(p0[UNIT])) and torch.equal(_bits(v[UNIT]), _bits(v0[UNIT])) and K[UNIT, 0] == K[UNIT, 1]
    assert torch.equal(_bits(p[2, :, 1]), _bits(p0[2, :, 1])) and not torch.equal(_bits(p[2, :, 0]), _bits(p0[2, :, 0]))
    fin = torch.isfinite(v0[2, :, 1])
    assert torch.equal(_bits(v[2, :, 1][fin]), _bits(v0[2, :, 1][fin]))
    # two calls give the same bits
    again = _launch(prec, t)
    assert torch.equal(_bits(again[2]), _bits(p)) and torch.equal(_bits(again[3]), _bits(v)) and torch.equal(_bits(again[5]), _bits(rec))


@pytest.mark.parametrize("prec", ["f32", "f64"])
@pytest.mark.parametrize("N", RM.SHAPES)
def test_partial_rows_and_record_bit_for_bit(N, prec):
    """The order of the fixed-order sum (tests/_reduce.py): N molecules, three of more than 64 atoms (one wave each: the rows
    behind those of the 256-thread blocks) and N - 3 of one atom, factors exactly 1 so that nothing is stored and K_after
    follows the rule of K_before.  Every partial row and the record against the model, addition by addition.  The four wave
    sums meet pairwise here."""
    from torchmd_amd import _lib as L
    from torchmd_amd import crescale as X

    dev, dt = _dev(), PREC[prec]
    off, natoms = RM.molecule_table(N)
    mass, vel = RM.velocities(2, natoms, prec, 7)
    p = torch.as_tensor(np.random.default_rng(8).uniform(-5.0, 45.0, (2, natoms, 3)), dtype=dt).to(dev).contiguous()
    v = torch.as_tensor(vel, dtype=dt).to(dev).contiguous()
    m = torch.as_tensor(mass, dtype=dt).to(dev)
    nrec, npart = C.c_int64(), C.c_int64()
    L.check(L.load().tmdhip_rescale_molecules_workspace(2, N, C.byref(nrec), C.byref(npart)), "workspace")
    rec = torch.full((2, 2), float("nan"), dtype=torch.float64, device=dev)
    part = torch.full((npart.value,), float("nan"), dtype=torch.float64, device=dev)
    p0, v0 = p.clone(), v.clone()
    X.rescale_molecules(p, v, m, np.ones((2, 3)), torch.as_tensor(off, device=dev), torch.arange(natoms, dtype=torch.int32, device=dev),
                        True, rec, part)
    torch.cuda.synchronize()
    assert torch.equal(_bits(p), _bits(p0)) and torch.equal(_bits(v), _bits(v0))  # factors of 1: nothing is stored
    nrows = (N + 255) // 256 + RM.BIG_BLOCKS
    rows, K = part[: 2 * nrows * 2].cpu().numpy().reshape(2, nrows, 2), rec.cpu().numpy()
    for r in range(2):
        want = RM.crescale_rows(mass, vel[r], off, RM.PAIRWISE)
        differ = int(((rows[r].view(np.int64) != want.view(np.int64)[:, None]).any(axis=1)).sum())
        fold = 0.5 * RM.fold(want)
        print(f"N = {N} {prec} replica {r}: {differ} of {nrows} partial rows differ from the model; K {K[r]!r}, model {fold!r}")
        assert differ == 0 and K[r, 0] == fold and K[r, 1] == fold


def test_c_refusals():
    """Every refusal returns an error before any launch: the tensors keep their bits."""
    from torchmd_amd import _lib as L

    lib, dev = L.load(), _dev()
    N, nmol = 12, 4
    p = torch.rand(2, N, 3, device=dev, dtype=torch.float64)
    v = torch.rand(2, N, 3, device=dev, dtype=torch.float64)
    m = torch.ones(N, device=dev, dtype=torch.float64)
    off = torch.arange(0, N + 1, 3, dtype=torch.int32, device=dev)
    mem = torch.arange(N, dtype=torch.int32, device=dev)
    rec, part = torch.zeros(4, device=dev, dtype=torch.float64), torch.zeros(64, device=dev, dtype=torch.float64)
    before = (p.clone(), v.clone(), rec.clone())
    ok = dict(dtype=L.F64, R=2, N=N, pos=p.data_ptr(), vel=v.data_ptr(), mass=m.data_ptr(), scale=np.full((2, 3), 1.01), nmol=nmol,
              off=off.data_ptr(), mem=mem.data_ptr(), big=0, rec=rec.data_ptr(), part=part.data_ptr())

    def call(**kw):
        a = {**ok, **kw}
        sc = None if a["scale"] is None else np.ascontiguousarray(a["scale"], dtype=np.float64)
        return lib.tmdhip_rescale_molecules(a["dtype"], a["R"], a["N"], a["pos"], a["vel"], a["mass"],
                                            None if sc is None else sc.ctypes.data_as(C.POINTER(C.c_double)), a["nmol"], a["off"], a["mem"],
                                            a["big"], a["rec"], a["part"], None)

    bad = [dict(dtype=7), dict(R=0), dict(R=70000), dict(N=0), dict(N=2**31), dict(nmol=0), dict(nmol=N + 1), dict(pos=None),
           dict(vel=None), dict(mass=None), dict(scale=None), dict(off=None), dict(mem=None), dict(rec=None), dict(part=None),
           dict(vel=p.data_ptr()), dict(scale=np.array([[1.0, 0.0, 1.0], [1.0] * 3])), dict(scale=np.array([[1.0, -1.0, 1.0], [1.0] * 3])),
           dict(scale=np.array([[1.0] * 3, [1.0, np.nan, 1.0]])), dict(scale=np.array([[1.0] * 3, [np.inf, 1.0, 1.0]]))]
    for kw in bad:
        assert call(**kw) < 0 and L.last_error().startswith("tmdhip_rescale_molecules"), kw
    n64 = C.c_int64()
    assert lib.tmdhip_rescale_molecules_workspace(0, 4, C.byref(n64), C.byref(n64)) < 0
    assert lib.tmdhip_rescale_molecules_workspace(2, 0, C.byref(n64), C.byref(n64)) < 0
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(before, (p, v, rec)))
    assert call() == 0
    torch.cuda.synchronize()
    assert not torch.equal(p, before[0]) and not torch.equal(v, before[1]) and (rec > 0).all()


# ----------------------------------------------------------------------------- 2. the integrator against a composition by hand
_SYSTEMS = {}


def _system_data(name, prec):
    from torchmd_amd.builders import tip3p_box, tip4p_box, tip4pew_forcefield, water_forcefield
    from torchmd_amd.parameters import Parameters

    key = (name, prec)
    if key not in _SYSTEMS:
        if name == "water291":
            g = load("water291")
            _SYSTEMS[key] = (GoldenParameters(g, PREC[prec]), np.asarray(g["pos"], dtype=np.float64).reshape(-1, 3),
                             np.asarray(g["box"], dtype=np.float64).reshape(-1)[:3], None, dict(cutoff=7.3, rfa=True), dict(), 1.0)
        elif name == "tip3p_list":  # 2 187 atoms: AUTO takes the cell list from 2 048 atoms on
            mol, pos, box = tip3p_box(9, seed=4)
            par = Parameters(water_forcefield(mol), mol, WATER_TERMS, precision=PREC[prec])
            _SYSTEMS[key] = (par, np.asarray(pos, dtype=np.float64), np.asarray(box, dtype=np.float64), None, dict(cutoff=7.0, rfa=True),
                             dict(), 1.0)
        else:  # 864 atoms, four-site rigid water, PME
            mol, pos, box, vs = tip4p_box(6, seed=3)
            par = Parameters(tip4pew_forcefield(mol), mol, WATER_TERMS, precision=PREC[prec])
            _SYSTEMS[key] = (par, np.asarray(pos, dtype=np.float64), np.asarray(box, dtype=np.float64), vs, dict(cutoff=9.0, pme=True),
                             dict(constraints="water"), 2.0)
    return _SYSTEMS[key]


def _make(name, prec, R=1, barostat=None, seed=3, thermostat=None):
    """(system, forces, integrator, U) of a fresh copy of the named system under Langevin at 300 K (or under `thermostat`)."""
    from torchmd_amd.forces import Forces
    from torchmd_amd.integrator import Integrator, maxwell_boltzmann
    from torchmd_amd.systems import System

    par, pos, box, vs, fkw, ikw, dt_fs = _system_data(name, prec)
    s = System(len(pos), R, PREC[prec], _dev())
    s.set_positions(pos[:, :, None])
    s.set_box(box)
    torch.manual_seed(seed)
    vel = maxwell_boltzmann(par.masses.double(), 300.0, 1)
    if vs is not None:
        vel[:, torch.as_tensor(vs.sites.astype(np.int64))] = 0.0
    s.set_velocities(vel.to(PREC[prec]).repeat(R, 1, 1))
    f = Forces(par, terms=WATER_TERMS, **fkw, **({} if vs is None else {"virtual_sites": vs}))
    U = f.compute(s.pos, s.box, s.forces)
    torch.manual_seed(seed + 8)
    bath = dict(gamma=1.0, T=300.0) if thermostat is None else dict(thermostat=thermostat)
    integ = Integrator(s, f, dt_fs, _dev(), **bath, **ikw, **({} if barostat is None else {"barostat": barostat}))
    return s, f, integ, U


def _philox(seed, r):
    return np.random.Generator(np.random.Philox(key=np.array([seed, r], dtype=np.uint64)))


def _by_hand(s, f, integ, prec, frequency, napplications, pressure_bar, temperature, tau, compressibility, rng, stochastic=True):
    """The barostat composed from public pieces and the numpy model: step, pressure terms, the model's mu from `rng` (one generator
    per replica), the kernel, compute.  Returns what `step` would return, the list of records, and the by-hand work."""
    from torchmd_amd import crescale as X

    R, dev = s.pos.shape[0], s.pos.device
    off, mem, _ = f._molecules()
    nrec, npart = C.c_int64(), C.c_int64()
    from torchmd_amd import _lib as L

    L.check(L.load().tmdhip_rescale_molecules_workspace(R, len(off) - 1, C.byref(nrec), C.byref(npart)), "workspace")
    rec = torch.zeros(R, 2, dtype=torch.float64, device=dev)
    part = torch.empty(npart.value, dtype=torch.float64, device=dev)
    offd, memd = torch.as_tensor(off, device=dev), torch.as_tensor(mem, device=dev)
    p0 = np.broadcast_to(np.asarray(pressure_bar, dtype=np.float64), (R,)) * M.BAR_TO_KCAL_MOL_A3
    records, work, out = [], np.zeros(R), None
    for _ in range(napplications):
        ek, pot, _ = integ.step(frequency)
        terms = integ._pressure_terms()
        V, p_int = terms[:, 6].copy(), terms[:, 7].copy()
        xi = np.array([g.standard_normal() for g in rng])
        mu = M.mu(pressure_bar, p_int, V, temperature, compressibility, tau, frequency, integ.dt, xi, stochastic)
        edges = torch.diagonal(s.box, dim1=-2, dim2=-1).to("cpu", torch.float64).numpy().reshape(R, 3)
        new = M.new_edges(edges, mu, NP[prec])
        X.rescale_molecules(s.pos, s.vel, integ.masses.reshape(-1), new / edges, offd, memd, bool(np.any(np.diff(off) > 64)), rec, part)
        nb = s.box.detach().clone()
        torch.diagonal(nb, dim1=-2, dim2=-1).copy_(torch.as_tensor(new).to(nb))
        s.box.copy_(nb)
        U_new = np.asarray(f.compute(s.pos, s.box, s.forces), dtype=np.float64)
        f._engine(s.pos)._md_key = None  # (positions were written behind torch's back: DESIGN §11)
        K = rec.cpu().numpy()
        V_new = new[:, 0] * new[:, 1] * new[:, 2]
        U = np.asarray(pot, dtype=np.float64)
        work += (K[:, 1] - K[:, 0]) + (U_new - U) + p0 * (V_new - V)
        records.append(dict(V=V, V_new=V_new, P_int=p_int, xi=xi, mu=mu, U=U, U_new=U_new, K_before=K[:, 0].copy(), K_after=K[:, 1].copy()))
        kin = K[:, 1].astype(NP[prec])
        out = (kin, [float(u) for u in U_new], integ._temperature(kin))
    return out, records, work


BARO = dict(pressure_bar=1.0, temperature=300.0, tau=0.5, compressibility=4.5e-5)


def _twin_bars(prec, n, napp, integ, s, frequency, baro=BARO):
    """Bars for two runs of the same `n` steps with `napp` applications where force atomics make a run non-reproducible, built as
    tests/test_gpu_barostat.py builds its own.  fp64: the suite's 1e-9 A for positions (and for the box, a length) and its force
    bar as it stands; velocities, for which the suite has no number, as below.  Otherwise from
    the formats: the forces of two runs agree within the suite's force bar dF (FTOL); a force error held for n steps moves the
    lightest atom (m_H = 1.008) by at most n^2/2 dF dt^2 / m_H and changes its velocity by n dF dt / m_H; every step, and every
    application, rounds the stored value once (eps |x|max, eps |v|max).  Two states that far apart differ in their forces by
    dF plus the stiffest curvature of the force field, the O-H bond's 2 k, times the displacement of both of its atoms.  The box:
    every application rounds the edge L once and multiplies it by mu, which differs through the pressure; the virial of two runs
    differs by at most sum |r| dF <= N L dF, so d mu <= (beta dt_p / tau_p / 3) N L dF / (3 V).  V follows as 3 dL / L, mu as dL / L.
    Energies: the suite's ERTOL * EFAC of max(1, |E|); the work is a sum over the applications of differences of two K and two
    U, and of P0 dV."""
    eps = float(np.finfo(NP[prec]).eps)
    dF, dt = FTOL[prec], integ.dt
    xmax, vmax = float(s.pos.abs().max()), float(s.vel[torch.isfinite(s.vel)].abs().max())
    N = s.pos.shape[1]
    L = float(torch.diagonal(s.box[0]).max())
    V = float(torch.diagonal(s.box[0]).prod())
    x = n * n / 2 * dF * dt * dt / M_H + (n + napp) * eps * xmax
    v = n * dF * dt / M_H + (n + napp) * eps * vmax
    beta = baro["compressibility"] / M.BAR_TO_KCAL_MOL_A3
    dtt = frequency * dt / (baro["tau"] * M.PICOSEC2TIMEU)
    box = napp * (eps * L + L * (beta * dtt / 3.0) * N * L * dF / (3.0 * V))
    if prec == "f64":  # the suite's bars as they stand
        return dict(x=XTOL64, v=v, box=XTOL64, f=dF, e=ERTOL[prec] * EFAC)
    return dict(x=x, v=v, box=box, f=dF + 2 * (2 * K_OH) * x, e=ERTOL[prec] * EFAC)


@pytest.mark.parametrize("prec", ["f32", "f64"])
@pytest.mark.parametrize("name", ["water291", "tip3p_list", "tip3p_list_wide", "tip4p_pme"])
def test_integrator_equals_the_composition_by_hand(name, prec, monkeypatch):
    """Bit for bit on the fp64 cell-list path, whose forces are stored without atomics.  The engine's energies meet in 256 slots
    per replica by atomic additions; at 4 lanes per atom (`tip3p_list`) the pair launch of 2 187 atoms has 137 waves, so no slot
    receives more than one addend of a kind and the sums do not depend on the order of arrival.  At the default width of 64
    lanes (`tip3p_list_wide`, 2 187 waves) a slot receives several and the energies carry the order in their last bit: there the
    fp64 state is still compared bit for bit and the energies at the suite's bar.  Everywhere else: `_twin_bars`, and the forces
    the integrator leaves against a fresh evaluation of its own state at the suite's force bar."""
    from torchmd_amd.crescale import CRescaleBarostat

    if name == "tip3p_list":
        monkeypatch.setenv("TMDHIP_LPA", "4")
    system = "tip3p_list" if name == "tip3p_list_wide" else name
    freq, seed = 5, 7
    bar = CRescaleBarostat(frequency=freq, seed=seed, **BARO)
    s, f, integ, _ = _make(system, prec, barostat=bar)
    out = integ.step(3 * freq)
    assert bar.applications == 3 and integ._nstep == 3 * freq
    s2, f2, integ2, _ = _make(system, prec)
    out2, records, work = _by_hand(s2, f2, integ2, prec, freq, 3, rng=[_philox(seed, 0)], **BARO)
    algo = f.stats(s.pos)["algorithm"]
    assert algo == ("celllist" if system == "tip3p_list" else "allpairs")
    last, mine = bar.last, records[-1]
    assert set(last) == {"V", "V_new", "P_int", "xi", "mu", "U", "U_new", "K_before", "K_after"}
    assert np.array_equal(last["xi"], mine["xi"])
    sites = None if _system_data(system, prec)[3] is None else torch.as_tensor(_system_data(system, prec)[3].sites.astype(np.int64))
    b = _twin_bars(prec, 3 * freq, 3, integ, s, freq)
    U, K = max(1.0, abs(out2[1][0])), max(1.0, abs(float(out2[0][0])))
    exact_state = algo == "celllist" and prec == "f64"  # no force atomics on this path
    if exact_state:
        for t, u in ((s.pos, s2.pos), (s.vel, s2.vel), (s.box, s2.box), (s.forces, s2.forces)):
            assert torch.equal(_bits(t), _bits(u))
        for k in ("V", "V_new", "P_int", "mu", "K_before", "K_after"):
            assert np.array_equal(last[k], mine[k]), k
        assert np.array_equal(out[0], out2[0]) and np.array_equal(out[2], out2[2])
    if exact_state and name == "tip3p_list":  # ... and the energies do not depend on the order of their atomics
        assert out[1] == out2[1] and np.array_equal(last["U"], mine["U"]) and np.array_equal(last["U_new"], mine["U_new"])
        assert np.array_equal(bar.work(), work)
    seen = dict(x=(s.pos - s2.pos).abs().max().item(), v=(s.vel - s2.vel).abs().max().item(), box=(s.box - s2.box).abs().max().item(),
                f=(s.forces - s2.forces).abs().max().item(), U=abs(out[1][0] - out2[1][0]) / U, K=abs(float(out[0][0]) - float(out2[0][0])) / K)
    Lmax = float(torch.diagonal(s.box[0]).max())
    for k, rel in (("V", 3 * b["box"] / Lmax), ("V_new", 3 * b["box"] / Lmax), ("mu", b["box"] / Lmax)):
        seen[k] = float(np.abs(last[k] / mine[k] - 1.0).max())
        assert seen[k] <= rel, (k, seen[k], rel)
    for k in ("U", "U_new"):
        assert np.abs(last[k] - mine[k]).max() <= b["e"] * U, k
    for k in ("K_before", "K_after"):
        assert np.abs(last[k] - mine[k]).max() <= b["e"] * K, k
    p0v = M.BAR_TO_KCAL_MOL_A3 * BARO["pressure_bar"] * float(last["V"][0])
    bar_w = 3 * (2 * b["e"] * (U + K) + p0v * 3 * b["box"] / Lmax)
    seen["work"] = float(np.abs(bar.work() - work).max())
    print(f"{name} {prec} ({algo}): twin differences max|dx| {seen['x']:.2e} (bar {b['x']:.2e}), |dv| {seen['v']:.2e} ({b['v']:.2e}), box "
          f"{seen['box']:.2e} ({b['box']:.2e}), |dF| {seen['f']:.2e} ({b['f']:.2e}), dU/|U| {seen['U']:.2e}, dK/K {seen['K']:.2e} ({b['e']:.1e}), "
          f"mu {seen['mu']:.2e}, work {seen['work']:.2e} ({bar_w:.2e}); mu = {last['mu'][0]!r}, P_int = "
          f"{last['P_int'][0] / M.BAR_TO_KCAL_MOL_A3:.1f} bar, work {bar.work()[0]:.6f}")
    assert seen["x"] <= b["x"] and seen["v"] <= b["v"] and seen["box"] <= b["box"] and seen["f"] <= b["f"], (seen, b)
    assert seen["U"] <= b["e"] and seen["K"] <= b["e"] and seen["work"] <= bar_w, (seen, b, bar_w)
    # the forces the integrator leaves are those of the rescaled state: a fresh evaluation, at the suite's force bar as it stands
    for sy, fo in ((s, f), (s2, f2)):
        fresh = torch.zeros_like(sy.forces)
        tot = fo.compute(sy.pos, sy.box, fresh)[0]
        assert (fresh - sy.forces).abs().max().item() <= FTOL[prec]
    assert abs(tot - out2[1][0]) <= b["e"] * U
    # what step() returns is the rescaled state's: K_after, U' and its temperature
    assert float(out[0][0]) == float(NP[prec](last["K_after"][0])) and out[1][0] == float(last["U_new"][0])
    assert last["V_new"][0] == float(np.prod(torch.diagonal(s.box[0]).cpu().double().numpy()))
    assert last["mu"][0] != 1.0 and bool(torch.isfinite(s.pos).all())
    if sites is not None:
        assert torch.all(s.vel[0, sites] == 0)


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_berendsen_limit_moves_the_box_by_the_models_factor(prec):
    """stochastic=False, two replicas of water291 with P0 500 bar below and 500 bar above the measured pressure: the first box
    grows, the second shrinks, each by exactly the model's mu (rounded to the box tensor's precision)."""
    from torchmd_amd.crescale import CRescaleBarostat

    s, f, integ, U = _make("water291", prec, R=2)
    p_int = integ._pressure_terms()[:, 7] / M.BAR_TO_KCAL_MOL_A3
    target = p_int + np.array([-500.0, 500.0])
    bar = CRescaleBarostat(target, 300.0, tau=0.5, frequency=10, stochastic=False, seed=2)
    edges = torch.diagonal(s.box, dim1=-2, dim2=-1).cpu().double().numpy().copy()
    rec = bar.apply(s, f, integ.masses, integ.dt, U, None)
    mu = M.mu(target, rec["P_int"], rec["V"], 300.0, 4.5e-5, 0.5, 10, integ.dt, rec["xi"], stochastic=False)
    new = torch.diagonal(s.box, dim1=-2, dim2=-1).cpu().double().numpy()
    print(f"{prec}: P_int = {p_int} bar, mu - 1 = {mu - 1}")
    assert np.array_equal(rec["mu"], mu) and np.array_equal(new, M.new_edges(edges, mu, NP[prec]))
    assert mu[0] > 1.0 > mu[1] and (new[0] > edges[0]).all() and (new[1] < edges[1]).all()
    # beta dP dt_p / tau_p / 3 with dP = 500 bar: 4.5e-5 * 500 * 0.02 / 3 = 1.5e-4
    assert np.allclose(np.abs(mu - 1.0), 1.5e-4, rtol=2e-3)
    assert np.array_equal(rec["xi"], [_philox(2, 0).standard_normal(), _philox(2, 1).standard_normal()])  # drawn all the same


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_rigid_water_survives_the_barostat(prec):
    """864-atom TIP4P-Ew, rigid water, PME, 200 steps at 2 fs: the worst relative O-H / H-H length error under the barostat is at
    most twice that of the same run without one."""
    import _constraints as H
    from torchmd_amd.constraints import find_constraints
    from torchmd_amd.crescale import CRescaleBarostat

    par, _, _, vs, _, _, _ = _system_data("tip4p_pme", prec)
    cs = find_constraints(par.masses, par.bond_params, par.angle_params, "water", virtual_sites=vs)
    pairs, d = cs.pairs()
    worst = {}
    for tag, bar in (("without", None), ("with", CRescaleBarostat(frequency=10, seed=4, **BARO))):
        s, f, integ, _ = _make("tip4p_pme", prec, barostat=bar)
        ek, pot, T = integ.step(200)
        assert np.isfinite(ek).all() and np.isfinite(pot).all()
        worst[tag] = H.residuals(s.pos[0].cpu().double().numpy(), s.vel[0].cpu().double().numpy(), pairs, d)
        if bar is not None:
            assert bar.applications == 20
            e = torch.diagonal(s.box[0]).cpu().double().numpy()
            assert e[0] == e[1] == e[2] and e[0] != _system_data("tip4p_pme", prec)[2][0]
    print(f"{prec}: worst relative bond-length error without the barostat {worst['without'][0]:.3e}, with {worst['with'][0]:.3e}; "
          f"velocity along the bonds / rms {worst['without'][1]:.3e}, {worst['with'][1]:.3e}")
    assert worst["with"][0] <= 2 * worst["without"][0]


def test_two_replicas_follow_the_chains_they_follow_alone():
    """fp64 water291, two replicas with different targets under a rescaling thermostat (whose noise, like the barostat's, is keyed
    (seed, replica); Langevin's is keyed by the row of the whole batch); the thermostat is applied first where both fall on one step."""
    from torchmd_amd.crescale import CRescaleBarostat
    from torchmd_amd.thermostat import VelocityRescale

    freq, seed, targets = 5, 9, [1.0, 2000.0]
    bar = CRescaleBarostat(targets, 300.0, tau=0.5, frequency=freq, seed=seed)
    th = VelocityRescale(300.0, tau=0.1, frequency=freq, seed=21)
    s, f, integ, _ = _make("water291", "f64", R=2, barostat=bar, thermostat=th)
    out = integ.step(3 * freq)
    assert bar.last["mu"][0] != bar.last["mu"][1] and th.applications == 3 and bar.applications == 3
    for r in range(2):
        alone = CRescaleBarostat(targets[r], 300.0, tau=0.5, frequency=freq, seed=seed)
        alone.rng = [_philox(seed, r)]
        th1 = VelocityRescale(300.0, tau=0.1, frequency=freq, seed=21)
        th1.rng = [_philox(21, r)]
        s1, f1, integ1, _ = _make("water291", "f64", R=1, barostat=alone, thermostat=th1)
        out1 = integ1.step(3 * freq)
        assert alone.last["xi"][0] == bar.last["xi"][r]
        assert float(out1[0][0]) == float(alone.last["K_after"][0])  # (the barostat rescaled last: its kinetic energy is returned)
        b = _twin_bars("f64", 3 * freq, 3, integ1, s1, freq, dict(tau=0.5, compressibility=4.5e-5))
        U = max(1.0, abs(out1[1][0]))
        dx, dv = (s1.pos[0] - s.pos[r]).abs().max().item(), (s1.vel[0] - s.vel[r]).abs().max().item()
        dbox, dU = (s1.box[0] - s.box[r]).abs().max().item(), abs(out1[1][0] - out[1][r]) / U
        dwork = abs(alone.work()[0] - bar.work()[r])
        print(f"replica {r}: alone against beside the other: max|dx| {dx:.2e}, |dv| {dv:.2e}, box {dbox:.2e}, dU/|U| {dU:.2e}, work {dwork:.2e}")
        assert dx <= b["x"] and dv <= b["v"] and dbox <= b["box"] and dU <= b["e"]
        assert dwork <= 3 * 2 * b["e"] * (U + max(1.0, float(out1[0][0]))) + 1e-9


# ----------------------------------------------------------------------------- 3. the ensemble
def test_ideal_gas_samples_the_npt_volume_distribution():
    """N = 64 non-interacting atoms (the gas of test_gpu_barostat.py), 300 K, P0 such that (N + 1) kT / P0 = 27 000 A^3, beta = 1 / P0,
    an application every 50 steps of 1 fs under Langevin with gamma dt_p = 1, dt_p / tau_p = 0.1: 8 000 applications, the first fifth
    discarded.  <V> within 4 block standard errors (10 blocks) plus 0.5 % of 27 000; sigma_V / <V> within 15 % of 1 / sqrt(65)."""
    from torchmd_amd.builders import Topology
    from torchmd_amd.crescale import CRescaleBarostat
    from torchmd_amd.forcefields.ff_yaml import YamlForceField
    from torchmd_amd.forces import Forces
    from torchmd_amd.integrator import Integrator, maxwell_boltzmann
    from torchmd_amd.parameters import Parameters
    from torchmd_amd.systems import System

    N, T, target, napp, freq = 64, 300.0, 27000.0, 8000, 50
    P = (N + 1) * M.BOLTZMAN * T / target / M.BAR_TO_KCAL_MOL_A3  # bar
    dtp_ps = freq * 1.0e-3
    edge = target ** (1.0 / 3.0)
    ff = {"atomtypes": ["X"], "lj": {"X": {"sigma": 3.0, "epsilon": 0.0}}, "electrostatics": {"X": {"charge": 0.0}}, "masses": {"X": 10.0}}
    mol = Topology(atomtype=np.full(N, "X", dtype=object), charge=np.zeros(N, dtype=np.float32), masses=np.full(N, 10.0, dtype=np.float32))
    par = Parameters(YamlForceField(mol, ff), mol, ["lj"], precision=torch.float64)
    s = System(N, 1, torch.float64, _dev())
    g = (np.arange(4) + 0.5) * edge / 4
    s.set_positions(np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3)[:, :, None])
    s.set_box(np.array([edge] * 3))
    torch.manual_seed(5)
    s.set_velocities(maxwell_boltzmann(par.masses, T, 1))
    f = Forces(par, terms=["lj"], cutoff=9.0)
    assert f.compute(s.pos, s.box, s.forces)[0] == 0.0
    bar = CRescaleBarostat(P, T, tau=10.0 * dtp_ps, compressibility=1.0 / P, frequency=freq, seed=17)
    integ = Integrator(s, f, 1.0, _dev(), gamma=1.0 / dtp_ps, T=T, barostat=bar)
    assert abs(bar.dt_over_tau(integ.dt) - 0.1) < 1e-12
    vols = np.empty(napp)
    for i in range(napp):
        _, pot, _ = integ.step(freq)
        assert pot[0] == 0.0
        vols[i] = bar.last["V_new"][0]
    assert bar.applications == napp
    mean, se, rel, _ = M.block_stats(vols[napp // 5:], 10)
    print(f"ideal gas, {napp} applications: <V> / {target:.0f} - 1 = {mean / target - 1:+.4f} (block error {se / target:.4f}), "
          f"sigma / <V> = {rel:.4f} (1 / sqrt(65) = {1 / np.sqrt(N + 1):.4f})")
    assert abs(mean - target) <= 4 * se + 0.005 * target
    assert abs(rel * np.sqrt(N + 1) - 1.0) <= 0.15


# ----------------------------------------------------------------------------- 4. run.py
def _run_py(tmp_path, tag, **keys):
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
            "cutoff": 7.3, "rfa": True, "replicas": 1, "precision": "double", "device": "cuda", "timestep": 1, "temperature": 300,
            "langevin_gamma": 1.0, "langevin_temperature": 300, "seed": 1, "steps": 40, "output_period": 10, "save_period": 40,
            "log_dir": str(tmp_path / tag), "output": "output", "barostat_pressure": 1.0, "barostat_frequency": 5, **keys}
    cpath = tmp_path / f"{tag}.yaml"
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
    with open(tmp_path / tag / "monitor_0.csv") as fh:
        rows = list(csv.DictReader(line for line in fh if not line.startswith("#")))
    return args, run, captured["integ"], rows, np.load(tmp_path / tag / "output_box_0.npy")


def test_run_py_crescale_and_monte_carlo(tmp_path):
    from torchmd_amd.barostat import MonteCarloBarostat
    from torchmd_amd.crescale import CRescaleBarostat

    args, run, integ, rows, boxes = _run_py(tmp_path, "crescale", barostat="crescale", barostat_tau=0.5, barostat_compressibility=5e-5)
    bar = integ.barostat
    assert isinstance(bar, CRescaleBarostat) and bar.applications == 8 and bar.tau == 0.5 and bar.compressibilities.tolist() == [5e-5]
    assert bar.temperatures.tolist() == [300.0] and bar.pressures_bar.tolist() == [1.0] and bar.frequency == 5
    assert list(rows[0]) == ["iter", "ns", "epot", "ekin", "etot", "T", "volume", "t"] and len(rows) == 4 and boxes.shape == (4, 3)
    edges = torch.diagonal(integ.systems.box[0]).cpu().double().numpy()
    assert np.array_equal(boxes[-1], edges) and float(rows[-1]["volume"]) == float(np.prod(edges))
    assert float(rows[-1]["volume"]) == bar.last["V_new"][0] and float(rows[-1]["epot"]) == float(bar.last["U_new"][0])
    assert float(rows[-1]["ekin"]) == float(bar.last["K_after"][0])
    assert len({r["volume"] for r in rows}) == 4  # every application moves the box
    # the Monte Carlo configuration: the barostat it made before, driven as before: equal to the run made by hand
    args, run, integ, rows, boxes = _run_py(tmp_path, "montecarlo")
    assert type(integ.barostat) is MonteCarloBarostat and integ.barostat.frequency == 5 and integ.barostat.attempts[0] == 8
    assert list(rows[0]) == ["iter", "ns", "epot", "ekin", "etot", "T", "volume", "t"] and boxes.shape == (4, 3)
    from torchmd_amd.integrator import Integrator
    from torchmd_amd.wrapper import Wrapper

    mol, system, forces = run.setup(args)
    torch.manual_seed(args.seed)
    twin = MonteCarloBarostat(1.0, 300.0, 5)
    hand = Integrator(system, forces, args.timestep, torch.device(args.device), gamma=args.langevin_gamma, T=args.langevin_temperature,
                      constraints=None, barostat=twin)
    wrapper = Wrapper(mol.numAtoms, mol.bonds, torch.device(args.device))
    forces.compute(system.pos, system.box, system.forces)
    for i in range(4):
        ek, pot, _ = hand.step(10)
        wrapper.wrap(system.pos, system.box)
        e = torch.diagonal(system.box[0]).cpu().double().numpy()
        assert np.allclose(boxes[i], e, rtol=1e-9, atol=0) and abs(float(rows[i]["epot"]) - pot[0]) <= 3e-10 * abs(pot[0]), i
    assert np.array_equal(twin.accepted, integ.barostat.accepted)
