"""The generalized-Born implicit solvent on the device: the three pair passes of gb.hip against the float64 numpy
model (`_gb.py`) on the same positions, `Forces(implicit_solvent=)`, `Integrator.step` under it — where the GB force never
enters the pair or step kernels but is applied as an impulse between their launches — against a loop made by hand that
integrates compute()'s total force step by step, and what composes with it.

Bars.  Kernel against model: (c eps_R + M eps64) S per quantity, S the model's sum of the absolute addends of the quantity
with the sums of what it depends on carried through to first order (`_gb.evaluate(bounds=True)`), M the number of addends
(7 (N - 1) + 8), c = 32: the roundings on the path to the worst addend of t in the context's precision (r from d: 3.5
half-ulps; r + sigma: 4.5; |r - sigma| >= rho: up to 10 relative to its value for the default tables; l^2: twice that; times
r / 4 and the subtraction: 28 half-ulps = 14 eps; ln(u/l): 17 half-ulps of the l and u addends; G, g, h: below 12 eps each),
doubled for the two sides of a pair that meet in F.  In fp32 the model forms d with float32 operations, as the kernels do, and
computes the rest in float64.  Trajectories: fp64 within 64 eps64 x steps x max|pos| (max|vel|) of the by-hand loop; fp32
within twice the deviation of the by-hand fp32 loop from the by-hand fp64 loop, measured here, with a control (the by-hand loop
under another solvent dielectric) that must miss that bar by more than 10x: the construction of tests/test_gpu_restraints.py."""

import ctypes as C
import os

import numpy as np
import pytest
import torch

import _gb as M
from _golden import PREC, GoldenParameters, load

pytestmark = pytest.mark.gpu

NP = {"f32": np.float32, "f64": np.float64}
EPS = {"f32": float(np.finfo(np.float32).eps), "f64": float(np.finfo(np.float64).eps)}
EPS64 = EPS["f64"]
C_REAL = 32
ERTOL = {"f64": 1e-10, "f32": 2e-5}  # tests/test_gpu_parity.py: energies (relative, x EFAC)
EFAC = 3
SEEDS = {1: 3, 2: 4, 40: 5, 63: 7, 64: 8, 65: 2, 130: 0}


def _dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _bits(t):
    return t.cpu().contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int64)


class _ClusterPar:
    """What `Forces` asks of its parameters, for a cluster of charged atoms with (optionally) harmonic bonds."""

    def __init__(self, charges, dtype, bonds=None, r0=None, k=100.0, mass=12.0):
        n = len(charges)
        self.masses = torch.full((n,), mass, dtype=dtype)
        self.charges = torch.tensor(np.asarray(charges), dtype=dtype)
        self.nonbonded_params = None
        self.bond_params = self.angle_params = self.dihedral_params = self.improper_params = self.nonbonded_14_params = None
        if bonds is not None:
            nb = len(bonds)
            self.bond_params = {"idx": torch.tensor(np.asarray(bonds, dtype=np.int64)),
                                "map": torch.tensor(np.stack([np.arange(nb), np.arange(nb)], axis=1)),
                                "params": torch.tensor(np.stack([np.full(nb, k), np.asarray(r0)], axis=1), dtype=dtype)}
        self.mapped_atom_types = torch.zeros(n, dtype=torch.int64)
        self.natoms = n
        self.device = "cpu"

    def get_exclusions(self, types=("bonds", "angles", "1-4"), fullarray=False):
        return [] if self.bond_params is None or "bonds" not in types else self.bond_params["idx"].numpy().tolist()


def _gb(rad, sc, **kw):
    from torchmd_amd.implicit import GeneralizedBorn

    return GeneralizedBorn(rad, sc, **kw)


def _replica_clusters(n, R, prec):
    """R clusters with the topology (charges, radii, scales) of the first and positions of their own, rounded to `prec`."""
    pos0, q, rad, sc = M.cluster(n, SEEDS.get(n, n))
    pos = np.stack([pos0] + [M.cluster(n, 100 + 7 * r + n)[0] for r in range(1, R)])
    return pos.astype(NP[prec]).astype(np.float64), q, rad, sc


_MODEL = {}


def _model(n, R, prec, **kw):
    """The model's answer for `_replica_clusters(n, R, prec)`, computed once per session and shared."""
    key = (n, R, prec, tuple(sorted(kw.items())))
    if key not in _MODEL:
        pos, q, rad, sc = _replica_clusters(n, R, prec)
        # (the engine's charges carry sqrt(k_e) and are rounded to the context's precision: one more half-ulp per charge, inside c)
        _MODEL[key] = [M.evaluate(pos[r], q, rad, sc, dtype=NP[prec], bounds=True, **kw) for r in range(R)]
    return _MODEL[key]


def _evaluate(n, R, prec, **kw):
    """(Forces, pos tensor, forces tensor, details) of a context that holds nothing but the model."""
    from torchmd_amd.forces import Forces

    pos, q, rad, sc = _replica_clusters(n, R, prec)
    f = Forces(_ClusterPar(q, PREC[prec]), terms=[], implicit_solvent=_gb(rad, sc, **kw))
    p = torch.as_tensor(pos, dtype=PREC[prec]).to(_dev()).contiguous()
    box = torch.zeros(R, 3, 3, dtype=PREC[prec], device=_dev())
    frc = torch.zeros_like(p)
    details = f.compute(p, box, frc, returnDetails=True)
    return f, p, box, frc, details


def _check_against_model(what, f, p, frc, details, model, prec):
    """B, E_GB, E_SA and F of every replica against the model at the rounding bars; returns the worst observed multiples of
    eps_R S."""
    B = f.born_radii(p)
    gb = f.implicit_solvent
    F = frc.cpu().double().numpy()
    worst = {"B": 0.0, "E_gb": 0.0, "E_sa": 0.0, "F": 0.0}
    for r, o in enumerate(model):
        u = C_REAL * EPS[prec] + o["M"] * EPS64
        errs = {"B": (np.abs(B[r] - o["B"]), o["S_B"]), "E_gb": (abs(gb.energy[r, 0] - o["E_gb"]), o["S_Egb"]),
                "E_sa": (abs(gb.energy[r, 1] - o["E_sa"]), o["S_Esa"]),
                # (the store of F rounds once more in the context's precision: half an ulp of |F|, inside c S_F)
                "F": (np.abs(F[r] - o["F"]).max(axis=1), o["S_F"])}
        for k, (err, S) in errs.items():
            mult = float(np.max(err / np.maximum(S, 1e-300))) / EPS[prec]
            worst[k] = max(worst[k], mult)
            assert np.all(err <= u * S), (what, prec, r, k, float(np.max(err / np.maximum(S, 1e-300))), u)
        assert abs(details[r]["implicit_solvent"] - (gb.energy[r, 0] + gb.energy[r, 1])) <= 4 * EPS64 * abs(details[r]["implicit_solvent"])
    print(f"{what} {prec}: worst error in units of eps_R S (bar {C_REAL} + M eps64 / eps_R): " + ", ".join(f"{k} {v:.3g}" for k, v in worst.items()))
    return worst


# ----------------------------------------------------------------------------- the kernels against the model
@pytest.mark.parametrize("prec", ["f32", "f64"])
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 130])
def test_kernel_against_model(n, prec):
    f, p, box, frc, details = _evaluate(n, 1, prec)
    model = _model(n, 1, prec)
    if n >= 63:
        assert (model[0]["regimes"][1:3] > 0).all()
    _check_against_model(f"N = {n}", f, p, frc, details, model, prec)
    if n == 1:  # the self term only: B = rho, no force
        rad = _replica_clusters(1, 1, prec)[2]
        assert abs(f.born_radii(p)[0, 0] - (rad[0] - M.OFFSET)) <= 4 * EPS64 * rad[0] and (frc == 0).all()


@pytest.mark.parametrize("prec", ["f32", "f64"])
@pytest.mark.parametrize("nsplit", [1, 2, 3])
def test_kernel_forced_split(nsplit, prec, monkeypatch):
    monkeypatch.setenv("TMDHIP_GB_NSPLIT", str(nsplit))
    f, p, box, frc, details = _evaluate(130, 1, prec)
    assert (_model(130, 1, prec)[0]["regimes"][1:] > 0).all()  # separate, overlapping and engulfed pairs
    _check_against_model(f"N = 130, nsplit = {nsplit}", f, p, frc, details, _model(130, 1, prec), prec)


@pytest.mark.parametrize("prec", ["f32", "f64"])
@pytest.mark.parametrize("R", [3, 17])
def test_kernel_replicas_with_positions_of_their_own(R, prec):
    f, p, box, frc, details = _evaluate(65, R, prec)
    _check_against_model(f"N = 65, R = {R}", f, p, frc, details, _model(65, R, prec), prec)
    B = f.born_radii(p)
    assert not np.array_equal(B[0], B[R - 1])


def test_two_calls_give_the_same_bits():
    for prec in ("f32", "f64"):
        f, p, box, frc, details = _evaluate(65, 17, prec)
        B, E = f.born_radii(p), f.implicit_solvent.energy.copy()
        frc2 = torch.zeros_like(p)
        f.compute(p, box, frc2)
        assert torch.equal(_bits(frc), _bits(frc2)) and np.array_equal(B.view(np.int64), f.born_radii(p).view(np.int64))
        assert np.array_equal(E.view(np.int64), f.implicit_solvent.energy.view(np.int64))
        # ... and a context of its own
        f3, p3, _, frc3, _ = _evaluate(65, 17, prec)
        assert torch.equal(_bits(frc), _bits(frc3)) and np.array_equal(E.view(np.int64), f3.implicit_solvent.energy.view(np.int64))


def test_gamma_zero_removes_the_surface_term():
    f, p, box, frc, details = _evaluate(65, 1, "f64", surface_tension=0.0)
    assert f.implicit_solvent.energy[0, 1] == 0.0
    g, _, _, _, _ = _evaluate(65, 1, "f64")
    assert g.implicit_solvent.energy[0, 1] > 0.0 and g.implicit_solvent.energy[0, 0] == f.implicit_solvent.energy[0, 0]


def test_forces_against_central_differences_of_compute():
    """Independent of the model, fp64: F from compute() against central differences of compute()'s own total energy, N = 65,
    12 coordinates.  Bar: 10 |FD(h) - FD(h/2)| + 64 eps64 S, S = the sum of the absolute addends of the energy (the model's
    S_Egb + S_Esa, the one place the model is used) over h: the rounding of the two energies of a difference."""
    f, p, box, frc, details = _evaluate(65, 1, "f64")
    o = _model(65, 1, "f64")[0]
    h = 1e-4
    S = (o["S_Egb"] + o["S_Esa"]) / h
    F = frc.cpu().numpy()[0]
    rng = np.random.default_rng(5)
    coords = [(int(a), int(c)) for a, c in zip(rng.choice(65, 12, replace=False), rng.integers(0, 3, 12))]

    def fd(step, a, c):
        e = []
        for sgn in (1.0, -1.0):
            q = p.clone()
            q[0, a, c] += sgn * step
            e.append(f.compute(q, box, None, calculateForces=False)[0])
        return -(e[0] - e[1]) / (2 * step)

    worst = 0.0
    for a, c in coords:
        d1, d2 = fd(h, a, c), fd(h / 2, a, c)
        bar = 10 * abs(d1 - d2) + 64 * EPS64 * S
        worst = max(worst, abs(d1 - F[a, c]) / bar)
        assert abs(d1 - F[a, c]) <= bar, (a, c, d1, d2, F[a, c], bar)
    print(f"central differences of compute(): worst |FD - F| / bar = {worst:.3f}, max|F| = {np.abs(F).max():.2f}")


# ----------------------------------------------------------------------------- thrombin
def _thrombin(prec):
    g = load("thrombin")
    par = GoldenParameters(g, PREC[prec])
    # (float32-rounded positions for both precisions: the ones the recorded model of tests/golden/thrombin_gb.npz was given)
    pos = np.asarray(g["pos"], dtype=np.float64).reshape(-1, 3).astype(np.float32).astype(np.float64)
    return g, par, pos


THROMBIN_TERMS = ["bonds", "angles", "dihedrals", "impropers", "1-4", "electrostatics", "lj"]


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_thrombin_against_the_chunked_model(prec):
    from torchmd_amd.forces import Forces
    from torchmd_amd.implicit import GeneralizedBorn

    g, par, pos = _thrombin(prec)
    gb = GeneralizedBorn.from_parameters(par)
    key = ("thrombin", prec)
    if key not in _MODEL:
        # the chunked model takes 12 s of numpy per evaluation: its answer is recorded (`python tests/_gb.py` writes the file,
        # tests/test_gb_host.py holds the file to the model)
        ref = load(M.THROMBIN_GOLDEN)
        _MODEL[key] = [dict(B=ref[prec + "_B"], F=ref[prec + "_F"], E_gb=float(ref[prec + "_E"][0]), E_sa=float(ref[prec + "_E"][1]),
                            S_B=ref["S_B"], S_F=ref["S_F"], S_Egb=float(ref["S_E"][0]), S_Esa=float(ref["S_E"][1]), M=int(ref["M"]))]
    f = Forces(_ClusterPar(par.charges.double().numpy(), PREC[prec]), terms=[], implicit_solvent=gb)
    p = torch.as_tensor(pos[None], dtype=PREC[prec]).to(_dev()).contiguous()
    box = torch.zeros(1, 3, 3, dtype=PREC[prec], device=_dev())
    frc = torch.zeros_like(p)
    details = f.compute(p, box, frc, returnDetails=True)
    _check_against_model("thrombin", f, p, frc, details, _MODEL[key], prec)
    # compute() with the force field: the entry is GB + SA, the total is the vacuum total plus the entry, the forces add
    vac = Forces(par, terms=THROMBIN_TERMS)
    full = Forces(par, terms=THROMBIN_TERMS, implicit_solvent=gb)
    Fv, Ff = torch.zeros_like(p), torch.zeros_like(p)
    ev = vac.compute(p, box, Fv, returnDetails=True)[0]
    ef = full.compute(p, box, Ff, returnDetails=True)[0]
    o = _MODEL[key][0]
    assert "implicit_solvent" not in ev and abs(ef["implicit_solvent"] - details[0]["implicit_solvent"]) == 0.0
    tv, tf = sum(ev.values()), full.compute(p, box, None, calculateForces=False)[0]
    assert abs(tf - (tv + ef["implicit_solvent"])) <= ERTOL[prec] * EFAC * max(1.0, abs(tf))
    u = C_REAL * EPS[prec] + o["M"] * EPS64
    diff = np.abs((Ff - Fv).cpu().double().numpy()[0] - o["F"]).max(axis=1)
    # (Ff - Fv carries the rounding of the vacuum force's store as well: an ulp of the larger of the two forces)
    room = 2 * EPS[prec] * np.abs(Fv.cpu().double().numpy()[0]).max(axis=1) if prec == "f32" else 0.0
    assert (diff <= u * o["S_F"] + room).all()
    print(f"thrombin {prec}: E_GB {o['E_gb']:.3f}, E_SA {o['E_sa']:.3f}, B in [{o['B'].min():.2f}, {o['B'].max():.2f}]")


def test_thrombin_nve_drift_is_that_of_the_vacuum_run():
    """NVE, fp64, 0.5 fs, 200 steps: max |E(t) - E(0)| is at most twice that of the same run without implicit_solvent=, made
    here on the same start.  A missing chain-rule term shows up as drift.  The factor 2 is a condition, as §20's rigid-water bar."""
    from torchmd_amd.forces import Forces
    from torchmd_amd.implicit import GeneralizedBorn
    from torchmd_amd.integrator import Integrator, maxwell_boltzmann
    from torchmd_amd.systems import System

    g, par, pos = _thrombin("f64")
    drift = {}
    for name in ("vacuum", "solvated"):
        extra = {"implicit_solvent": GeneralizedBorn.from_parameters(par)} if name == "solvated" else {}
        s = System(len(pos), 1, torch.float64, _dev())
        s.set_positions(pos[:, :, None])
        s.set_box(np.zeros(3))
        torch.manual_seed(4)
        s.set_velocities(maxwell_boltzmann(par.masses, 300.0, 1))
        f = Forces(par, terms=THROMBIN_TERMS, **extra)
        f.compute(s.pos, s.box, s.forces)
        integ = Integrator(s, f, 0.5, _dev())
        e = []
        for _ in range(10):
            ek, ep, _ = integ.step(20)
            e.append(float(ek[0]) + ep[0])
        drift[name] = np.abs(np.asarray(e) - e[0]).max()
    print(f"thrombin NVE, 200 steps of 0.5 fs: max|E - E0| vacuum {drift['vacuum']:.3e}, with GB {drift['solvated']:.3e} kcal/mol")
    assert drift["solvated"] <= 2 * drift["vacuum"]


# ----------------------------------------------------------------------------- dynamics
def _bonded_cluster(prec, R=1):
    """130 charged atoms at a density without overlaps of the vacuum terms (no two closer than 1.6 A), every atom bonded to its
    nearest neighbour at their present distance; vacuum terms: bonds and Coulomb."""
    rng = np.random.default_rng(17)
    n, edge = 130, 7.0 * (130 / 40.0) ** (1.0 / 3.0) * 1.25
    pos = np.zeros((0, 3))
    while len(pos) < n:
        x = rng.uniform(0.0, edge, size=3)
        if len(pos) == 0 or np.sqrt(((pos - x) ** 2).sum(axis=1)).min() > 1.6:
            pos = np.vstack([pos, x])
    _, q, rad, sc = M.cluster(n, 0)
    q = 0.5 * q
    d = np.sqrt(((pos[:, None] - pos[None]) ** 2).sum(axis=2)) + 1e9 * np.eye(n)
    bonds = sorted({(min(i, int(j)), max(i, int(j))) for i, j in enumerate(d.argmin(axis=1))})
    r0 = [d[i, j] for i, j in bonds]
    par = _ClusterPar(q, PREC[prec], bonds=bonds, r0=r0)
    vel0 = torch.as_tensor(0.01 * np.random.default_rng(8).standard_normal((R, n, 3)))
    return pos, par, rad, sc, vel0


def _cluster_system(pos, vel0, prec, R):
    from torchmd_amd.systems import System

    s = System(len(pos), R, PREC[prec], _dev())
    s.set_positions(np.repeat(pos[:, :, None], R, axis=2))
    s.set_box(np.zeros(3))
    s.set_velocities(vel0.to(PREC[prec]))
    return s


CUTS = (1, 2, 7)
TERMS = ["bonds", "electrostatics"]


def _by_hand(prec, langevin, fkw, R=1, **gbkw):
    """The truth: tmdhip_first_vv, compute()'s total force (the asynchronous evaluation the minimiser uses), tmdhip_(langevin_)second_vv."""
    from torchmd_amd import _lib as L
    from torchmd_amd.forces import Forces
    from torchmd_amd.integrator import Integrator

    pos, par, rad, sc, vel0 = _bonded_cluster(prec, R)
    s = _cluster_system(pos, vel0, prec, R)
    f = Forces(par, terms=TERMS, implicit_solvent=_gb(rad, sc, **gbkw), **fkw)
    torch.manual_seed(77)
    integ = Integrator(s, f, 1.0, _dev(), **(dict(gamma=50.0, T=300.0) if langevin else {}))
    integ._check_layout()
    lib, code, N = L.load(), L.dtype_code(s.pos.dtype), s.pos.shape[1]
    f._compute_async(s.pos, s.box, s.forces, want_energy=False)
    st = C.c_void_p(torch.cuda.current_stream(_dev()).cuda_stream)
    for step in range(sum(CUTS)):
        L.check(lib.tmdhip_first_vv(code, R, N, s.pos.data_ptr(), s.vel.data_ptr(), s.forces.data_ptr(), integ.masses.data_ptr(), integ.dt, st))
        f._compute_async(s.pos, s.box, s.forces, want_energy=False)
        if langevin:
            L.check(lib.tmdhip_langevin_second_vv(code, R, N, s.vel.data_ptr(), s.forces.data_ptr(), integ.masses.data_ptr(),
                                                  integ.vcoeff.data_ptr(), integ.dt, float(integ.gamma), integ._seed, step, st))
        else:
            L.check(lib.tmdhip_second_vv(code, R, N, s.vel.data_ptr(), s.forces.data_ptr(), integ.masses.data_ptr(), integ.dt, st))
    return s.pos.cpu().double().numpy(), s.vel.cpu().double().numpy()


def _under_test(prec, langevin, fkw, R=1):
    from torchmd_amd.forces import Forces
    from torchmd_amd.integrator import Integrator

    pos, par, rad, sc, vel0 = _bonded_cluster(prec, R)
    s = _cluster_system(pos, vel0, prec, R)
    f = Forces(par, terms=TERMS, implicit_solvent=_gb(rad, sc), **fkw)
    f.compute(s.pos, s.box, s.forces)
    torch.manual_seed(77)
    integ = Integrator(s, f, 1.0, _dev(), **(dict(gamma=50.0, T=300.0) if langevin else {}))
    out = None
    for n in CUTS:
        out = integ.step(n)
    return s.pos.cpu().double().numpy(), s.vel.cpu().double().numpy(), out, f, s


PATHS = {"allpairs": dict(algorithm="allpairs"), "celllist": dict(algorithm="celllist", cutoff=6.0)}


@pytest.mark.parametrize("langevin", [False, True], ids=["nve", "langevin"])
@pytest.mark.parametrize("path", ["allpairs", "celllist"])
@pytest.mark.parametrize("prec", ["f64", "f32"])
def test_trajectory_against_the_loop_made_by_hand(prec, path, langevin, monkeypatch):
    monkeypatch.setenv("TMDHIP_VSKIN", "0")
    fkw = PATHS[path]
    R = 2 if path == "allpairs" else 1  # (all-pairs contexts step their replicas together: that branch of the loop)
    tp, tv = _by_hand("f64", langevin, fkw, R)
    p, v, out, f, s = _under_test(prec, langevin, fkw, R)
    assert f.stats(s.pos)["algorithm"] == path
    dp, dv = np.abs(p - tp).max(), np.abs(v - tv).max()
    if prec == "f64":
        bar_p, bar_v = 64 * EPS64 * 10 * np.abs(tp).max(), 64 * EPS64 * 10 * np.abs(tv).max()
    else:
        hp, hv = _by_hand("f32", langevin, fkw, R)
        bar_p, bar_v = 2 * np.abs(hp - tp).max(), 2 * np.abs(hv - tv).max()
        cp, cv = _by_hand("f32", langevin, fkw, R, solvent_dielectric=2.0)  # the control misses the bar by more than 10x
        assert np.abs(cp - tp).max() > 10 * bar_p and np.abs(cv - tv).max() > 10 * bar_v
    print(f"{prec} {path} {'Langevin' if langevin else 'NVE'}: |dpos| = {dp:.2e} (bar {bar_p:.2e}), |dvel| = {dv:.2e} (bar {bar_v:.2e})")
    assert dp <= bar_p and dv <= bar_v
    # the energies step() returns include GB + SA: compute()'s total at the final positions, and the forces left are total
    F2 = torch.zeros_like(s.pos)
    tot = f.compute(s.pos, s.box, F2)
    gbe = f.implicit_solvent.energy.sum(axis=1)
    for r in range(R):
        assert abs(out[1][r] - tot[r]) <= ERTOL[prec] * EFAC * max(1.0, abs(tot[r])), (r, out[1][r], tot[r])
        assert abs(gbe[r]) > 10.0 and abs(out[1][r] - (tot[r] - gbe[r])) > 100 * ERTOL[prec] * EFAC * abs(tot[r])
    assert np.abs((s.forces - F2).cpu().double().numpy()).max() <= (3e-3 if prec == "f32" else 1e-7)


# ----------------------------------------------------------------------------- composition
def test_minimize_fire_lowers_the_total_and_converges():
    """The N = 65 cluster as one chain 0-1-...-64 with every atom also bonded to its nearest neighbour, r0 = 1.5 A (a cluster
    without a repulsive term cannot carry bare Coulomb forces: the vacuum part is the bonds alone; a connected topology,
    because fragments that only the GB term couples drift apart for tens of thousands of iterations: the first version of
    this test, nearest-neighbour bonds alone, was at max|F| = 2.5 after 5000): FIRE sees the total force, GB included."""
    from torchmd_amd.forces import Forces
    from torchmd_amd.minimizers import minimize_fire

    pos, q, rad, sc = _replica_clusters(65, 1, "f64")
    d = np.sqrt(((pos[0][:, None] - pos[0][None]) ** 2).sum(axis=2)) + 1e9 * np.eye(65)
    bonds = sorted({(min(i, int(j)), max(i, int(j))) for i, j in enumerate(d.argmin(axis=1))} | {(i, i + 1) for i in range(64)})
    par = _ClusterPar(q, torch.float64, bonds=bonds, r0=[1.5] * len(bonds))
    s = _cluster_system(pos[0], torch.zeros(1, 65, 3), "f64", 1)
    f = Forces(par, terms=["bonds"], implicit_solvent=_gb(rad, sc))
    e0 = f.compute(s.pos, s.box, s.forces, returnDetails=True)[0]
    f0 = s.forces.norm(dim=2).max().item()
    minimize_fire(s, f, fmax=0.5, steps=20000)
    F = torch.zeros_like(s.pos)
    e1 = f.compute(s.pos, s.box, F, returnDetails=True)[0]
    fmax = F.norm(dim=2).max().item()
    print(f"FIRE with implicit solvent: E {sum(e0.values()):.3f} -> {sum(e1.values()):.3f} (GB + SA {e0['implicit_solvent']:.3f} -> "
          f"{e1['implicit_solvent']:.3f}), max|F_total| {f0:.2f} -> {fmax:.3f}")
    assert sum(e1.values()) < sum(e0.values()) and fmax <= 0.5 < f0
    # the bonds alone are not at rest there: the minimum is that of the total
    Fb = torch.zeros_like(s.pos)
    Forces(par, terms=["bonds"]).compute(s.pos, s.box, Fb)
    assert Fb.norm(dim=2).max().item() > 0.5


def test_exchange_ladder_conserves_its_quantity():
    """A 4-rung ladder under `exchange=`: E_kin + E_pot - heat - work of every slot over 60 steps (six thermostat
    applications, three attempts) drifts at most twice as far as in the same run without implicit_solvent= (§16's conserved
    quantity; the condition of the thrombin NVE test), and the energies the attempts decide on are compute()'s totals."""
    from torchmd_amd.exchange import ReplicaExchange
    from torchmd_amd.forces import Forces
    from torchmd_amd.integrator import Integrator
    from torchmd_amd.thermostat import VelocityRescale

    drift = {}
    for name in ("vacuum", "solvated"):
        pos, par, rad, sc, vel0 = _bonded_cluster("f64", 4)
        s = _cluster_system(pos, vel0, "f64", 4)
        f = Forces(par, terms=TERMS, **({"implicit_solvent": _gb(rad, sc)} if name == "solvated" else {}))
        f.compute(s.pos, s.box, s.forces)
        th, ex = VelocityRescale([300.0, 320.0, 340.0, 360.0], tau=0.1, frequency=10, seed=31), ReplicaExchange(frequency=20, seed=31)
        integ = Integrator(s, f, 0.5, _dev(), thermostat=th, exchange=ex)
        q = []
        for _ in range(6):
            ek, ep, _ = integ.step(10)
            work = ex.work()  # (None before the first attempt)
            q.append(np.asarray(ek, dtype=np.float64) + np.asarray(ep) - th.heat() - (0.0 if work is None else work))
        drift[name] = np.abs(np.asarray(q) - q[0]).max()
        assert ex.nattempts == 3
        if name == "solvated":
            tot = f.compute(s.pos, s.box, torch.zeros_like(s.pos))
            assert np.allclose(ex.record["U"], tot, rtol=1e-9) and np.abs(f.implicit_solvent.energy.sum(axis=1)).min() > 10.0
    print(f"ladder: drift of E_kin + E_pot - heat - work: vacuum {drift['vacuum']:.3e}, with GB {drift['solvated']:.3e} kcal/mol")
    assert drift["solvated"] <= 2 * drift["vacuum"]


def test_composes_with_hbond_constraints_restraints_and_metadynamics():
    """Thrombin, fp32, Langevin at 2 fs with constraints="hbonds", a distance restraint and a metadynamics bias on another
    distance, all three impulses behind one another: the X-H bonds keep their lengths as well as in the same run without the
    model (bar: twice that run's worst relative error plus 8 eps32, the condition of §17's constrained-water test), and the
    energy `step` returns is compute()'s total with all three entries in it."""
    from torchmd_amd.forces import Forces
    from torchmd_amd.implicit import GeneralizedBorn
    from torchmd_amd.integrator import Integrator, maxwell_boltzmann
    from torchmd_amd.metadynamics import Metadynamics
    from torchmd_amd.restraints import Restraints
    from torchmd_amd.systems import System

    g, par, pos = _thrombin("f32")
    heavy = np.flatnonzero(par.masses.numpy() > 2.0)
    a, b, c, d = (int(heavy[k]) for k in (10, 400, 800, 1500))
    dist = lambda i, j: float(np.linalg.norm(pos[i] - pos[j]))  # noqa: E731
    worst = {}
    for name in ("vacuum", "solvated"):
        rs = Restraints(1)
        rs.add_distance([[a, b]], dist(a, b) + 0.5, 20.0)
        md = Metadynamics(("distance", (c, d)), sigma=0.3, height=0.5, frequency=10, temperature=300.0, bias_factor=8.0,
                          grid_min=max(dist(c, d) - 6.0, 0.5), grid_max=dist(c, d) + 6.0, grid_bins=120)
        extra = {"implicit_solvent": GeneralizedBorn.from_parameters(par)} if name == "solvated" else {}
        s = System(len(pos), 1, torch.float32, _dev())
        s.set_positions(pos[:, :, None])
        s.set_box(np.zeros(3))
        torch.manual_seed(4)
        s.set_velocities(maxwell_boltzmann(par.masses, 300.0, 1))
        f = Forces(par, terms=THROMBIN_TERMS, restraints=rs, metadynamics=md, **extra)
        f.compute(s.pos, s.box, s.forces)
        integ = Integrator(s, f, 2.0, _dev(), gamma=1.0, T=300.0, constraints="hbonds")
        out = integ.step(45)  # (not a multiple of the bias frequency: a call that ends on a deposition returns V from before it)
        p = s.pos[0].cpu().double().numpy()
        cs = integ.constraints
        off, atoms, d0 = np.asarray(cs.offsets), np.asarray(cs.atoms), np.asarray(cs.dist)
        err = 0.0
        for cl in range(len(off) - 1):  # (a cluster is its central atom followed by its hydrogens, a length per entry)
            for k in range(off[cl] + 1, off[cl + 1]):
                err = max(err, abs(np.linalg.norm(p[atoms[off[cl]]] - p[atoms[k]]) / d0[k] - 1.0))
        assert len(off) > 1000
        worst[name] = err
        det = f.compute(s.pos, s.box, torch.zeros_like(s.pos), returnDetails=True)[0]
        tot = sum(det.values())
        assert np.isfinite(tot) and abs(out[1][0] - tot) <= ERTOL["f32"] * EFAC * max(1.0, abs(tot)), (out[1][0], tot)
        assert det["restraints"] > 0.0 and "metadynamics" in det and len(md.hills()) == 4
        if name == "solvated":
            assert det["implicit_solvent"] < -1000.0
    print(f"hbonds + restraints + metadynamics on thrombin, 45 steps of 2 fs: worst X-H length error vacuum {worst['vacuum']:.2e}, "
          f"with GB {worst['solvated']:.2e}")
    assert worst["solvated"] <= 2 * worst["vacuum"] + 8 * EPS["f32"]


# ----------------------------------------------------------------------------- the C interface
def test_library_refusals_launch_nothing():
    from torchmd_amd import _lib as L
    from torchmd_amd.forces import Forces

    pos, q, rad, sc = _replica_clusters(65, 1, "f64")
    gb = _gb(rad, sc)
    f = Forces(_ClusterPar(q, torch.float64), terms=[], implicit_solvent=gb)
    p = torch.as_tensor(pos, dtype=torch.float64).to(_dev()).contiguous()
    eng = f._engine(p)
    lib = eng.lib
    frc = torch.zeros_like(p)
    before = _bits(frc).clone()

    def desc(**kw):
        d = L.GbDesc()
        d.struct_size = C.sizeof(L.GbDesc)
        d.enable = 1
        r, s = np.array(kw.pop("radii", rad), dtype=np.float64), np.array(kw.pop("scale", sc), dtype=np.float64)
        d.radii_host, d.scale_host = r.ctypes.data_as(C.c_void_p), s.ctypes.data_as(C.c_void_p)
        d.solute_dielectric, d.solvent_dielectric, d.surface_tension, d.probe_radius = 1.0, 78.5, 0.0054, 1.4
        for k, v in kw.items():
            setattr(d, k, v)
        return d, (r, s)

    def refused(expect, ctx=None, **kw):
        d, keep = desc(**kw)
        assert lib.tmdhip_set_gb(ctx or eng.ctx, C.byref(d)) < 0
        assert expect in L.last_error(), (expect, L.last_error())

    def poked(a, i, v):
        b = np.array(a, dtype=np.float64)
        b[i] = v
        return b

    assert lib.tmdhip_set_gb(eng.ctx, None) < 0 and lib.tmdhip_set_gb(None, None) < 0
    refused("size mismatch", struct_size=8)
    refused("null", radii_host=None)
    refused("radius", radii=poked(rad, 3, 0.09))
    refused("radius", radii=poked(rad, 3, np.nan))
    refused("scale", scale=poked(sc, 5, -0.1))
    refused("dielectric", solute_dielectric=0.0)
    refused("dielectric", solvent_dielectric=-2.0)
    # a box with a non-zero edge: refused by the evaluation and by tmdhip_md_run, nothing launched
    boxes = np.array([[30.0, 0.0, 0.0]])
    ptr = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    st = C.c_void_p(torch.cuda.current_stream(_dev()).cuda_stream)
    gb.sync(eng)
    assert lib.tmdhip_gb_apply(eng.ctx, ptr(p), boxes.ctypes.data_as(C.POINTER(C.c_double)), ptr(frc), None, None, 0.0, None, st) < 0
    assert "open boundaries" in L.last_error()
    v, mt = torch.zeros_like(p), torch.full((65,), 12.0, dtype=torch.float64, device=_dev())
    assert lib.tmdhip_gb_apply(eng.ctx, ptr(p), np.zeros((1, 3)).ctypes.data_as(C.POINTER(C.c_double)), None, ptr(v), None, 1.0, None, st) < 0
    assert "masses" in L.last_error()
    d = L.MdDesc()
    d.struct_size = C.sizeof(L.MdDesc)
    d.niter, d.pos_dev, d.vel_dev, d.forces_dev = 2, p.data_ptr(), v.data_ptr(), frc.data_ptr()
    d.mass_dev, d.box_host, d.dt = mt.data_ptr(), boxes.ctypes.data_as(C.c_void_p), 0.5
    assert lib.tmdhip_md_run(eng.ctx, C.byref(d), st) < 0 and "open boundaries" in L.last_error()
    torch.cuda.synchronize()
    assert torch.equal(_bits(frc), before) and (v == 0).all() and torch.equal(_bits(p), _bits(torch.as_tensor(pos).to(_dev())))
    # contexts that cannot hold the model: the reaction field, PME, virtual sites, passive atoms
    g = Forces(_ClusterPar(q, torch.float64), terms=["electrostatics"], cutoff=6.0, rfa=True)
    refused("reaction field", ctx=g._engine(p).ctx)
    h = Forces(_ClusterPar(q, torch.float64), terms=["electrostatics"], cutoff=6.0, pme=True, pme_grid=(16, 16, 16))
    refused("PME", ctx=h._engine(p).ctx)
    k = Forces(_ClusterPar(q, torch.float64), terms=[])
    engk = k._engine(p)
    types, charges = np.zeros(65, np.int32), np.zeros(65, np.float64)
    L.check(lib.tmdhip_update_atoms(engk.ctx, 65, types.ctypes.data_as(C.c_void_p), charges.ctypes.data_as(C.c_void_p), 40), "tmdhip_update_atoms")
    refused("passive atoms", ctx=engk.ctx)
    w = Forces(_ClusterPar(q, torch.float64), terms=[])
    engw = w._engine(p)
    vd = L.VsiteDesc()
    vd.struct_size = C.sizeof(L.VsiteDesc)
    vd.enable, vd.nsites = 1, 1
    site, parent, weight = np.array([7], np.int32), np.array([[1, 2, -1]], np.int32), np.array([[0.5, 0.5, 0.0]])
    vd.site_host, vd.parent_host, vd.weight_host = (a.ctypes.data_as(C.c_void_p) for a in (site, parent, weight))
    L.check(lib.tmdhip_set_vsites(engw.ctx, C.byref(vd)), "tmdhip_set_vsites")
    refused("virtual sites", ctx=engw.ctx)
    # a context without the model: nothing added, energies zero, no Born radii; enable = 0 releases
    e = torch.full((1, 2), -1.0, dtype=torch.float64, device=_dev())
    zero = np.zeros((1, 3))
    assert lib.tmdhip_gb_apply(engk.ctx, ptr(p), zero.ctypes.data_as(C.POINTER(C.c_double)), ptr(frc), None, None, 0.0, ptr(e), st) == 0
    assert torch.equal(_bits(frc), before) and (e == 0).all()
    out = np.zeros((1, 65))
    assert lib.tmdhip_gb_born_radii(engk.ctx, out.ctypes.data_as(C.POINTER(C.c_double))) < 0
    d0, keep = desc(enable=0)
    assert lib.tmdhip_set_gb(eng.ctx, C.byref(d0)) == 0
    assert lib.tmdhip_gb_apply(eng.ctx, ptr(p), zero.ctypes.data_as(C.POINTER(C.c_double)), ptr(frc), None, None, 0.0, ptr(e), st) == 0
    assert torch.equal(_bits(frc), before) and (e == 0).all()


def test_python_refusals_on_the_device():
    from torchmd_amd.forces import Forces

    pos, q, rad, sc = _replica_clusters(65, 1, "f64")
    f = Forces(_ClusterPar(q, torch.float64), terms=[], implicit_solvent=_gb(rad, sc))
    p = torch.as_tensor(pos, dtype=torch.float64).to(_dev()).contiguous()
    box = torch.zeros(1, 3, 3, dtype=torch.float64, device=_dev())
    box[0].diagonal().fill_(30.0)
    with pytest.raises(ValueError, match="open boundaries"):
        f.compute(p, box, torch.zeros_like(p))
    with pytest.raises(ValueError, match="implicit_solvent"):
        f.virial(p, box)


# ----------------------------------------------------------------------------- run.py
_CHILD = r"""
import json, os, sys
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
import numpy as np, torch, yaml
import test_gpu_driver as D
from _golden import load
from torchmd_amd import run as driver
from torchmd_amd.builders import TIP3P_FF
g = dict(load("water291"))
g["box"] = np.zeros_like(g["box"])
psf, pdb, ff = (os.path.join(TMP, n) for n in ("structure.psf", "structure.pdb", "water_forcefield.yaml"))
D._write_psf(psf, g); D._write_pdb(pdb, g)
open(ff, "w").write(yaml.safe_dump(TIP3P_FF))
conf = {"structure": [psf, pdb], "forcefield": ff, "forceterms": ["LJ", "Bonds", "Angles", "Electrostatics"], "cutoff": None,
        "replicas": 2, "precision": "double", "device": "cuda", "timestep": 1, "temperature": 300, "langevin_temperature": 300,
        "langevin_gamma": 1.0, "seed": 1, "steps": 40, "output_period": 20, "save_period": 0, "output": "output"}
out = {}
def go(name, **kw):
    c = dict(conf, log_dir=os.path.join(TMP, name), **kw)
    open(os.path.join(TMP, name + ".yaml"), "w").write(yaml.safe_dump(c))
    args = driver.get_args(["--conf", os.path.join(TMP, name + ".yaml")])
    mol, system, forces = driver.setup(args)
    driver.dynamics(args, mol, system, forces)
    log = os.path.join(TMP, name)
    tot = forces.compute(system.pos, system.box, torch.zeros_like(system.pos), returnDetails=True)
    out[name] = {"files": sorted(os.listdir(log)), "rows": [open(os.path.join(log, f"monitor_{k}.csv")).read().splitlines() for k in range(2)],
                 "state": [{k: float(v) for k, v in t.items()} for t in tot]}
go("log")
out["module_after_off"] = "torchmd_amd.implicit" in sys.modules
go("log_gb", implicit_solvent="obc2", surface_tension=0.005)
print("RESULT " + json.dumps(out))
"""


def test_run_py_with_and_without_the_key(tmp_path):
    import json
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = f"ROOT = {root!r}\nTMP = {str(tmp_path)!r}\n" + _CHILD
    res = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, cwd=root)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-4000:]
    out = json.loads(next(ln for ln in res.stdout.splitlines() if ln.startswith("RESULT "))[7:])
    assert out["module_after_off"] is False  # without the key the module is never imported
    assert all(rows[0] == "iter,ns,epot,ekin,etot,T,t" and len(rows) == 3 for rows in out["log"]["rows"])
    for k, rows in enumerate(out["log_gb"]["rows"]):
        assert rows[0] == "iter,ns,epot,ekin,etot,T,implicit_solvent,t" and len(rows) == 3
        last = [float(x) for x in rows[-1].split(",")]
        state = out["log_gb"]["state"][k]
        # the last monitor row is the integrator's state: compute() at the final positions gives the same energies
        assert abs(last[6] - state["implicit_solvent"]) <= 1e-9 * abs(state["implicit_solvent"]) and last[6] < -1.0
        assert abs(last[2] - sum(state.values())) <= 1e-9 * abs(sum(state.values()))
