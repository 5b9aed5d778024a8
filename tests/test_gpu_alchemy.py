"""Alchemical decoupling on the GPU, fp32 and fp64: full coupling against the plain engine, full decoupling
against the oracle's two separate systems, intermediate couplings against the numpy model (`_alchemy.py`) at rounding bounds,
forces and dU/dlambda against central differences of compute()'s own energy, foreign energies, bitwise reproducibility, rows
out of reach left alone, the MD loop against a by-hand loop, and the invariants (NVE drift, FIRE, constraints, refusals, run.py).

Bars.  End points: tests/test_gpu_parity.py's (forces 1e-8 / 3e-4; energies 1e-10 / 2e-5 x EFAC relative to max(1, |entry|) per
entry, summed over the entries of a total: `_total_bar`).  Kernel against
model: (C_GPU eps_R + M eps64) S per force component and per energy, S the sum of the absolute addends (the model returns it),
M the number of addends of the longest double sum (pairs of one atom, or blocks of a fold).  C_GPU = 64: the header's 40 eps on
its worst addend (tests/test_alchemy_host.py), the charge product of two rounded scaled charges (1.5), the product d fs (0.5),
the rounding of the pair vector's components into r^2 carried through r^-18 (9), rounded up."""

import ctypes as C
import os
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import _alchemy as M

pytestmark = pytest.mark.gpu

PREC = {"f32": torch.float32, "f64": torch.float64}
NP = {"f32": np.float32, "f64": np.float64}
EPS = {"f32": float(np.finfo(np.float32).eps), "f64": float(np.finfo(np.float64).eps)}
EPS64 = EPS["f64"]
FTOL = {"f64": 1e-8, "f32": 3e-4}  # tests/test_gpu_parity.py: forces, energies (relative, x EFAC)
ERTOL = {"f64": 1e-10, "f32": 2e-5}
EFAC = 3
C_GPU = 64
CUT, SWD = 9.0, 7.5
TERMS = ["lj", "electrostatics", "bonds", "angles", "dihedrals", "1-4"]
# (solute atoms, environment atoms, box edge): every size at which a kernel takes another path (tiles of 64, more than one block)
SHAPES = [(1, 130, 20.0), (3, 1, 20.0), (63, 63, 24.0), (64, 64, 24.0), (65, 65, 24.0), (130, 200, 30.0)]


def _dev():
    return torch.device("cuda:0")


def _stream(dev):
    return C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


class ChainPar:
    """Duck type of `Parameters` for a `_alchemy.chain_system`: bonds, angles, one-term torsions and 1-4 pairs on the chain."""

    def __init__(self, sysd, prec, keep=None):
        dt = PREC[prec]
        idx = np.arange(sysd["N"]) if keep is None else np.asarray(keep)
        remap = -np.ones(sysd["N"], dtype=np.int64)
        remap[idx] = np.arange(len(idx))
        self.charges = torch.tensor(sysd["q"][idx], dtype=dt)
        self.masses = torch.full((len(idx), 1), 12.0, dtype=dt)
        self.mapped_atom_types = torch.tensor(sysd["cls"][idx])
        self.natoms = len(idx)
        self.device = "cpu"
        self.A, self.B = torch.tensor(sysd["A"], dtype=dt), torch.tensor(sysd["B"], dtype=dt)
        self.nonbonded_params = None

        def table(tuples, prm):
            tuples = np.asarray(tuples, dtype=np.int64)
            if len(tuples) == 0 or (remap[tuples] < 0).any():
                return None
            m = np.arange(len(tuples))
            return {"idx": torch.tensor(remap[tuples]), "map": torch.tensor(np.stack([m, m], axis=1)),
                    "params": torch.tensor(np.tile(np.asarray(prm, dtype=np.float64), (len(tuples), 1)), dtype=dt)}

        n = len(sysd["atoms"])
        tors = np.array([(k, k + 1, k + 2, k + 3) for k in range(n - 3)], dtype=np.int64).reshape(-1, 4)
        self.bond_params = table(sysd["bonds"], (150.0, 1.5))
        self.angle_params = table(sysd["angles"], (20.0, 1.9))
        self.dihedral_params = table(tors, (0.4, 0.3, 2.0))
        self.improper_params = None
        self.nonbonded_14_params = table(sysd["pairs14"], (3.0e3, 40.0, 2.0, 1.2))

    def get_AB(self):
        return self.A, self.B

    def get_exclusions(self, types=("bonds", "angles", "1-4"), fullarray=False):
        ex = []
        if self.bond_params is not None and "bonds" in types:
            ex += self.bond_params["idx"].numpy().tolist()
        if self.angle_params is not None and "angles" in types:
            ex += self.angle_params["idx"].numpy()[:, [0, 2]].tolist()
        if self.dihedral_params is not None and "1-4" in types:
            ex += self.dihedral_params["idx"].numpy()[:, [0, 3]].tolist()
        return ex


_CASES = {}


def _case(n, nenv, edge, periodic=True):
    key = (n, nenv, edge, periodic)
    if key not in _CASES:
        _CASES[key] = M.chain_system(n, nenv, seed=n + nenv, edge=edge, periodic=periodic)
    return _CASES[key]


def _rounded(sysd, prec):
    """The model's inputs as a context of this precision holds them."""
    t = NP[prec]
    out = dict(sysd)
    for k in ("q", "A", "B"):
        out[k] = sysd[k].astype(t).astype(np.float64)
    out["scee"] = sysd["scee"].astype(t).astype(np.float64)
    out["pos"] = sysd["pos"].astype(t).astype(np.float64)
    return out


def _tensors(pos, box, R, prec, jitter=0.0, seed=0):
    rng = np.random.default_rng(seed)
    p = np.stack([pos + (rng.normal(scale=jitter, size=pos.shape) if (jitter and r) else 0.0) for r in range(R)])
    tp = torch.tensor(p, dtype=PREC[prec], device=_dev()).contiguous()
    tb = torch.zeros(R, 3, 3, dtype=PREC[prec], device=_dev())
    for r in range(R):
        tb[r].diagonal().copy_(torch.as_tensor(box, dtype=PREC[prec]))
    return tp, tb


def _forces(sysd, prec, al=None, keep=None, **kw):
    from torchmd_amd.forces import Forces

    par = ChainPar(sysd, prec, keep)
    terms = [t for t in TERMS if not (t in ("dihedrals", "1-4") and par.dihedral_params is None)]
    terms = [t for t in terms if not (t == "bonds" and par.bond_params is None) and not (t == "angles" and par.angle_params is None)]
    kw.setdefault("cutoff", CUT)
    if kw["cutoff"] is not None:
        kw.setdefault("switch_dist", SWD)
        kw.setdefault("rfa", True)
    return Forces(par, terms=terms, **({"alchemical": al} if al is not None else {}), **kw), par


def _alch_only(f, pos, box, want_forces=True):
    """The alchemical part alone through tmdhip_alchemical_apply: (five numbers [R, 5], forces [R, N, 3]) as float64 numpy."""
    eng = f._engine(pos)
    eng.sync_alchemical(f)
    F = torch.zeros_like(pos) if want_forces else None
    eng.apply_alchemical(f.alchemical, pos, f._replica_boxes(box, pos.shape[0]), F, True)
    torch.cuda.synchronize()
    return eng.abuf.cpu().numpy().copy(), (F.cpu().double().numpy() if want_forces else None)


def _model(sysd, prec, pos_r, lv, le, reference=True, **kw):
    s = _rounded(sysd, prec)
    kw.setdefault("cutoff", CUT)
    if kw["cutoff"] is not None:
        kw.setdefault("switch_dist", SWD)
        kw.setdefault("rfa", True)
    return M.evaluate(pos_r, s["box"], s["atoms"], s["q"], s["cls"], s["A"], s["B"], lv, le, alpha=0.5, excl=s["excl"], pairs14=s["pairs14"],
                      scee=s["scee"], dtype=NP[prec], reference_switch=reference, **kw)


def _total_bar(prec, *details):
    """test_gpu_parity.py's energy bar for a total: the sum over its entries of ERTOL x EFAC x max(1, |entry|), the entries of
    every `returnDetails` dict given (the larger of the two where both have the entry)."""
    keys = set().union(*[d.keys() for d in details])
    return sum(ERTOL[prec] * EFAC * max(1.0, max(abs(d.get(k, 0.0)) for d in details)) for k in keys)


def _lambda_ladder(R):
    lv = np.array([0.5, 1.0, 0.0, 0.85, 1.0, 0.15] * 3)[:R]
    le = np.array([0.0, 0.4, 0.0, 0.0, 1.0, 0.0] * 3)[:R]
    return lv, le


# ----------------------------------------------------------------------------- end points
@pytest.mark.parametrize("prec", ["f32", "f64"])
@pytest.mark.parametrize("n,nenv,edge", SHAPES)
def test_full_coupling_equals_the_plain_engine(prec, n, nenv, edge):
    from torchmd_amd import Alchemical

    sysd = _case(n, nenv, edge)
    pos, box = _tensors(sysd["pos"], sysd["box"], 1, prec)
    plain, _ = _forces(sysd, prec)
    alch, _ = _forces(sysd, prec, Alchemical(sysd["atoms"], 1.0, 1.0))
    F0, F1 = torch.zeros_like(pos), torch.zeros_like(pos)
    d0 = plain.compute(pos, box, F0, returnDetails=True)
    d1 = alch.compute(pos, box, F1, returnDetails=True)
    e0, e1 = [sum(d0[0].values())], sum(d1[0].values())
    err = (F1 - F0).abs().max().item()
    print(f"{prec} n={n} |E|={nenv}: total {e1:.6f} vs {e0[0]:.6f}, max |dF| = {err:.2e}, alchemical entry {d1[0]['alchemical']:.4f}")
    assert abs(e1 - e0[0]) <= _total_bar(prec, d0[0], d1[0])
    assert err <= FTOL[prec]
    if nenv > 1:
        assert abs(d1[0]["alchemical"]) > 0


@pytest.mark.parametrize("prec", ["f32", "f64"])
@pytest.mark.parametrize("n,nenv,edge", [(3, 1, 20.0), (65, 65, 24.0), (130, 200, 30.0)])
def test_full_decoupling_equals_two_separate_systems(prec, n, nenv, edge):
    from oracle import torchmd_oracle as orc
    from torchmd_amd import Alchemical

    sysd = _case(n, nenv, edge)
    pos, box = _tensors(sysd["pos"], sysd["box"], 1, prec)
    alch, _ = _forces(sysd, prec, Alchemical(sysd["atoms"], 0.0, 0.0))
    F1 = torch.zeros_like(pos)
    e1 = alch.compute(pos, box, F1)[0]
    want_e, want_F = 0.0, np.zeros((sysd["N"], 3))
    for keep in (np.arange(n), np.arange(n, sysd["N"])):
        par = ChainPar(sysd, prec, keep)
        terms = [t for t in TERMS if getattr(par, {"bonds": "bond_params", "angles": "angle_params", "dihedrals": "dihedral_params",
                                                     "1-4": "nonbonded_14_params"}.get(t, "charges")) is not None]
        if "dihedrals" not in terms:
            terms = [t for t in terms if t != "1-4"]
        pots, oF, _ = orc.compute(par, pos[:, keep].cpu(), box.cpu(), terms, cutoff=CUT, rfa=True, switch_dist=SWD)
        want_e += sum(pots[0].values())
        want_F[keep] += oF[0].double().numpy()
    err = np.abs(F1[0].cpu().double().numpy() - want_F).max()
    print(f"{prec} n={n} |E|={nenv}: total {e1:.6f} vs oracle {want_e:.6f}, max |dF| = {err:.2e}")
    assert abs(e1 - want_e) <= ERTOL[prec] * EFAC * max(1.0, abs(want_e))
    assert err <= FTOL[prec]


# ----------------------------------------------------------------------------- the kernels against the model
def _kernel_against_model(prec, sysd, R, pos=None, lam=None, **kw):
    from torchmd_amd import Alchemical

    lv, le = _lambda_ladder(R) if lam is None else (np.full(R, lam[0]), np.full(R, lam[1]))
    p, box = _tensors(sysd["pos"] if pos is None else pos, sysd["box"], R, prec, jitter=0.05, seed=3)
    f, _ = _forces(sysd, prec, Alchemical(sysd["atoms"], lv, le), **kw)
    E, F = _alch_only(f, p, box)
    worst_f = worst_e = 0.0
    for r in range(R):
        pr = p[r].cpu().double().numpy()
        o = _model(sysd, prec, pr, lv[r], le[r], **kw)
        Mf = sysd["N"] + 8  # addends of an atom's double sum: at most one per partner, plus the splits
        bar = (C_GPU * EPS[prec] + Mf * EPS64) * o["S_F"][:, None] + 1e-300
        err = np.abs(F[r] - o["F"])
        assert (err <= bar).all(), (prec, r, np.unravel_index(np.argmax(err / bar), err.shape), (err / bar).max())
        worst_f = max(worst_f, float((err / bar).max()))
        want = np.array([o["E_lj"], o["E_el"], o["E_intra"], o["dv"], o["de"]])
        npairs = len(sysd["atoms"]) * sysd["N"]
        ebar = (C_GPU * EPS[prec] + (64 + npairs) * EPS64) * o["S_E"] + 1e-300
        assert (np.abs(E[r] - want) <= ebar).all(), (prec, r, E[r], want, ebar)
        worst_e = max(worst_e, float((np.abs(E[r] - want) / ebar).max()))
        if lv[r] == 0.0:
            assert E[r, 0] == 0.0 and E[r, 1] == 0.0
    return worst_f, worst_e, f, p, box


@pytest.mark.parametrize("prec", ["f32", "f64"])
@pytest.mark.parametrize("n,nenv,edge", SHAPES)
def test_kernel_against_model(prec, n, nenv, edge):
    wf, we, *_ = _kernel_against_model(prec, _case(n, nenv, edge), 3)
    print(f"{prec} n={n} |E|={nenv} R=3: worst force err / bar = {wf:.3f}, worst energy err / bar = {we:.3f}")


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_kernel_past_a_chunk_of_sixteen_replicas_and_bitwise(prec, monkeypatch):
    """17 replicas with one coupling each; two calls and a second context agree bit for bit; a forced split of the solute
    pass changes nothing but the order of a few additions."""
    sysd = _case(65, 65, 24.0)
    wf, we, f, p, box = _kernel_against_model(prec, sysd, 17)
    E1, F1 = _alch_only(f, p, box)
    E2, F2 = _alch_only(f, p, box)
    assert np.array_equal(E1, E2) and np.array_equal(F1, F2)
    from torchmd_amd import Alchemical

    lv, le = _lambda_ladder(17)
    g, _ = _forces(sysd, prec, Alchemical(sysd["atoms"], lv, le))
    E3, F3 = _alch_only(g, p, box)
    assert np.array_equal(E1, E3) and np.array_equal(F1, F3)
    monkeypatch.setenv("TMDHIP_ALCHEMY_SPHERE", "1")  # the early-outs skip work that adds nothing: the same bits
    k, _ = _forces(sysd, prec, Alchemical(sysd["atoms"], lv, le))
    E5, F5 = _alch_only(k, p, box)
    assert np.array_equal(E1, E5) and np.array_equal(F1, F5)
    monkeypatch.setenv("TMDHIP_ALCHEMY_NSPLIT", "3")
    monkeypatch.setenv("TMDHIP_ALCHEMY_SPHERE", "0")
    h, _ = _forces(sysd, prec, Alchemical(sysd["atoms"], lv, le))
    E4, F4 = _alch_only(h, p, box)
    assert np.array_equal(E1, E4)  # the energies come from the environment pass alone
    assert np.abs(F4 - F1).max() <= 8 * EPS[prec] * np.abs(F1).max()
    print(f"{prec} R=17: worst force err / bar = {wf:.3f}, energy {we:.3f}")


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_open_boundaries_and_one_open_axis(prec):
    sysd = dict(_case(5, 70, 16.0, periodic=False))
    wf, we, *_ = _kernel_against_model(prec, sysd, 1, cutoff=None)
    sysd["box"] = np.array([20.0, 0.0, 21.0])
    wf2, we2, *_ = _kernel_against_model(prec, sysd, 2)
    print(f"{prec} open: {wf:.3f} {we:.3f}; one open axis: {wf2:.3f} {we2:.3f}")


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_edge_positions(prec):
    """Solute atoms across a box face (unwrapped coordinates) and one coincident cross pair at lambda_vdw = 0.5."""
    sysd = dict(_case(3, 65, 20.0))
    base = sysd["pos"].copy()
    base[:3] += np.array([20.0 - base[0, 0] - 0.4, 0.0, 0.0])  # the chain straddles the x face
    wf0, we0, *_ = _kernel_against_model(prec, sysd, 1, pos=base)
    pos = base.copy()
    pos[3] = pos[2]  # coincident cross pair; lambda_vdw = 0.5 on replica 0
    wf, we, *_ = _kernel_against_model(prec, sysd, 1, pos=pos)
    print(f"{prec} edges: across a face {wf0:.3f} {we0:.3f}, coincident pair {wf:.3f} {we:.3f}")


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_cutoff_decision_at_r_equal_cutoff(prec):
    """One cross pair at r = cutoff exactly and one ulp to either side, where the pair has a jump at the cutoff: no switch, plain
    1 / r, full coupling, a charged solute atom and a charged environment atom of the Lennard-Jones class (q q k_e / r_c = -8.9
    kcal/mol).  The solute is one atom, so the pair is the environment atom's only one: in impulse mode its velocity row is
    written at -1 and 0 ulp and bitwise untouched at +1 ulp.  The kernel must agree with the model, whose decision is
    sqrt(|d|^2) <= cutoff in the context's precision, at all three positions; a kernel that decided otherwise at any of them
    would miss the energy by the whole jump, more than a hundred times the bar."""
    from torchmd_amd import _lib as L
    from torchmd_amd import Alchemical

    t = NP[prec]
    sysd = dict(_case(1, 130, 20.0))
    q = sysd["q"].copy()
    q[0] = 0.3
    sysd["q"] = q
    base = sysd["pos"].copy()
    base[:, 2] += 10.0 - base[0, 2]
    base[0, 2] = 10.0  # 10 - x and 10 - (10 - x) are exact in either precision for x within an ulp of 9
    far = base[1:] - base[0]
    far -= 20.0 * np.rint(far / 20.0)
    dist = np.linalg.norm(far, axis=1)
    dist[sysd["cls"][1:] != 2] = -1.0
    lonely = 1 + int(np.argmax(dist))
    assert sysd["cls"][lonely] == 2 and sysd["q"][lonely] == -0.8
    kw = dict(switch_dist=None, rfa=False)
    seen, energies = [], []
    for off in (-1, 0, 1):
        pos = base.astype(t)
        x = t(CUT)
        for _ in range(abs(off)):
            x = np.nextafter(x, t(np.inf) if off > 0 else t(0))
        pos[lonely] = pos[0]
        pos[lonely, 2] = t(pos[0, 2] - x)
        d, r2 = M.pair_vectors(pos[0].astype(np.float64), pos[lonely].astype(np.float64), sysd["box"], t)
        assert d[2] == float(x) and d[0] == 0.0 and d[1] == 0.0  # exactly that separation in the context's precision
        seen.append(bool(r2 <= M.r2max(CUT, t)))
        wf, we, f, p, box = _kernel_against_model(prec, sysd, 1, pos=pos.astype(np.float64), lam=(1.0, 1.0), **kw)
        E, _ = _alch_only(f, p, box)
        energies.append(E[0, 1])
        o = _model(sysd, prec, p[0].cpu().double().numpy(), 1.0, 1.0, **kw)
        assert bool(o["near"][lonely]) == seen[-1]
        # impulse mode: the row of the environment atom is written if and only if the pair is inside
        eng = f._engine(p)
        rng = np.random.default_rng(2)
        v0 = torch.tensor(rng.normal(size=tuple(p.shape)), dtype=PREC[prec], device=_dev())
        vel = v0.clone()
        mass = torch.full((sysd["N"],), 12.0, dtype=PREC[prec], device=_dev())
        L.check(eng.lib.tmdhip_alchemical_apply(eng.ctx, C.c_void_p(p.data_ptr()), f._replica_boxes(box, 1).ctypes.data_as(C.POINTER(C.c_double)),
                                                C.c_void_p(), C.c_void_p(vel.data_ptr()), C.c_void_p(mass.data_ptr()), 0.37, C.c_void_p(),
                                                _stream(_dev())), "tmdhip_alchemical_apply")
        torch.cuda.synchronize()
        same = bool((vel[0, lonely] == v0[0, lonely]).all())
        assert same == (not seen[-1]), (off, same, seen[-1])
    assert seen == [True, True, False], seen
    jump = M.KE * 0.3 * -0.8 / CUT
    ebar = (C_GPU * EPS[prec] + (64 + sysd["N"]) * EPS64) * o["S_E"][1]
    print(f"{prec} cutoff decision: cross el at -1, 0, +1 ulp = {energies}, jump {jump:.4f}, bar {ebar:.2e}")
    assert abs((energies[1] - energies[2]) - jump) <= 2 * ebar + 1e-5 * abs(jump) and abs(jump) > 100 * ebar
    assert abs(energies[0] - energies[1]) <= 2 * ebar + 1e-5 * abs(jump)


def _sum_of_absolute_addends(sysd, pos_np, lv, le, details):
    """The sum of the absolute addends of compute()'s total: the model's for the alchemical part, the model's pair formula for
    the environment's own pairs, the 1-4 Lennard-Jones terms written out, and the bonded entries, which are sums of
    non-negative addends each (k x^2, k (1 + cos))."""
    n, N = len(sysd["atoms"]), sysd["N"]
    S = _model(sysd, "f64", pos_np, lv, le, reference=False)["S_E"][:3].sum()
    env = np.arange(n, N)
    if len(env) > 1:
        S += M.evaluate(pos_np, sysd["box"], env, sysd["q"], sysd["cls"], sysd["A"], sysd["B"], 1.0, 1.0, cutoff=CUT, switch_dist=SWD,
                        rfa=True)["S_E"][2]
    for i, j in sysd["pairs14"]:
        d, r2 = M.pair_vectors(pos_np[i], pos_np[j], sysd["box"])
        S += (3.0e3 / r2**6 + 40.0 / r2**3) / 2.0
    return S + sum(abs(details.get(k, 0.0)) for k in ("bonds", "angles", "dihedrals"))


@pytest.mark.parametrize("n,nenv,edge", SHAPES)
def test_forces_and_derivatives_against_central_differences(n, nenv, edge):
    """fp64: F = -dE/dx of compute()'s own total (exact switch derivative), and alchemical_terms()' dU/dlambda against central
    differences in lambda of compute()'s "alchemical" entry.  Bar 10 |FD(h) - FD(h/2)| + 64 eps64 S_E / h, §21's: S_E is the sum
    of the absolute addends of the energy that is differenced (`_sum_of_absolute_addends`)."""
    from torchmd_amd import Alchemical

    sysd = _case(n, nenv, edge)
    N = sysd["N"]
    atoms = sorted({0, n // 2, n - 1, n, N - 1})
    worst = 0.0
    for lv, le in ((0.5, 0.0), (1.0, 0.4)):
        al = Alchemical(sysd["atoms"], lv, le)
        f, _ = _forces(sysd, "f64", al, switch_mode="exact")
        pos, box = _tensors(sysd["pos"], sysd["box"], 1, "f64")
        F = torch.zeros_like(pos)
        d = f.compute(pos, box, F, returnDetails=True)[0]
        floor = 64 * EPS64 * _sum_of_absolute_addends(sysd, sysd["pos"], lv, le, d) / 1e-5
        Fh = F[0].cpu().numpy()
        terms = f.alchemical_terms()[0]  # (of this evaluation: the displaced ones below replace it)

        def fd(h, i, c):
            out = []
            for sgn in (1, -1):
                p = pos.clone()
                p[0, i, c] += sgn * h
                out.append(f.compute(p, box, None, calculateForces=False)[0])
            return -(out[0] - out[1]) / (2 * h)

        for i in atoms:
            for c in range(3):
                a, b = fd(1e-5, i, c), fd(5e-6, i, c)
                bar = 10 * abs(a - b) + floor
                assert abs(Fh[i, c] - a) <= bar, (lv, le, i, c, Fh[i, c], a, b, floor)
                worst = max(worst, abs(Fh[i, c] - a) / bar)
        S_al = _model(sysd, "f64", sysd["pos"], lv, le, reference=False)["S_E"][:3].sum()
        for which in (0, 1):
            x0 = (lv, le)[which]
            vals = []
            for h in (1e-5, 5e-6):
                es = []
                for x in (x0 + h, x0 - h):
                    l = [lv, le]
                    l[which] = x
                    if not (0 <= x <= 1) or (l[1] != 0 and l[0] != 1):
                        es = None
                        break
                    al.set_lambdas(l[0], l[1])
                    es.append(f.compute(pos, box, None, returnDetails=True, calculateForces=False)[0]["alchemical"])
                if es is None:
                    vals = None
                    break
                vals.append((es[0] - es[1]) / (2 * h))
            al.set_lambdas(lv, le)
            if vals is not None:
                bar = 10 * abs(vals[0] - vals[1]) + 64 * EPS64 * S_al / 1e-5
                assert abs(terms[3 + which] - vals[0]) <= bar, (which, terms, vals)
                worst = max(worst, abs(terms[3 + which] - vals[0]) / bar)
    print(f"f64 n={n} |E|={nenv}: worst |analytic - FD| / bar = {worst:.3f}")


@pytest.mark.parametrize("prec", ["f32", "f64"])
@pytest.mark.parametrize("n,nenv,edge", SHAPES)
def test_foreign_energies_equal_the_entry_at_that_state(prec, n, nenv, edge):
    from torchmd_amd import Alchemical

    sysd = _case(n, nenv, edge)
    R = 3
    lv, le = _lambda_ladder(R)
    al = Alchemical(sysd["atoms"], lv, le)
    f, _ = _forces(sysd, prec, al)
    pos, box = _tensors(sysd["pos"], sysd["box"], R, prec, jitter=0.05, seed=4)
    states = np.array([[1.0, 1.0], [1.0, 0.5], [1.0, 0.0], [0.75, 0.0], [0.5, 0.0], [0.25, 0.0], [0.0, 0.0]] + [[k / 40.0, 0.0] for k in range(1, 27)])
    assert len(states) == 33  # more than one call of 32
    got = f.alchemical_energies(pos, box, states)
    assert got.shape == (R, 33) and (got[:, 6] == 0.0).all()
    for k in (0, 1, 3, 4, 20, 32):
        al.set_lambdas(states[k, 0], states[k, 1])
        E, _ = _alch_only(f, pos, box, want_forces=False)
        for r in range(R):
            o = _model(sysd, prec, pos[r].cpu().double().numpy(), states[k, 0], states[k, 1])
            # (either side carries the kernel-against-model bar)
            bar = 2 * (C_GPU * EPS[prec] + (64 + n * sysd["N"]) * EPS64) * (o["S_E"][0] + o["S_E"][1]) + 1e-300
            assert abs(got[r, k] - (E[r, 0] + E[r, 1])) <= bar, (k, r, got[r, k], E[r], bar)
            assert abs(got[r, k] - (o["E_lj"] + o["E_el"])) <= bar
    with pytest.raises(ValueError):
        f.alchemical_energies(pos, box, [[0.5, 0.5]])


@pytest.mark.parametrize("prec", ["f32", "f64"])
@pytest.mark.parametrize("n,nenv,edge", SHAPES + [(5, 400, 40.0)])
def test_rows_out_of_reach_are_untouched_in_impulse_mode(prec, n, nenv, edge):
    from torchmd_amd import _lib as L
    from torchmd_amd import Alchemical

    s = _case(n, nenv, edge)
    al = Alchemical(s["atoms"], 0.5, 0.0)
    f, par = _forces(s, prec, al)
    pos, box = _tensors(s["pos"], s["box"], 2, prec)
    eng = f._engine(pos)
    eng.sync_alchemical(f)
    rng = np.random.default_rng(1)
    v0 = torch.tensor(rng.normal(size=tuple(pos.shape)), dtype=PREC[prec], device=_dev())
    vel = v0.clone()
    mass = torch.full((s["N"],), 12.0, dtype=PREC[prec], device=_dev())
    mass[-1] = 0.0  # a row without mass is left alone
    L.check(eng.lib.tmdhip_alchemical_apply(eng.ctx, C.c_void_p(pos.data_ptr()), f._replica_boxes(box, 2).ctypes.data_as(C.POINTER(C.c_double)),
                                            C.c_void_p(), C.c_void_p(vel.data_ptr()), C.c_void_p(mass.data_ptr()), 0.37, C.c_void_p(),
                                            _stream(_dev())), "tmdhip_alchemical_apply")
    torch.cuda.synchronize()
    o = _model(s, prec, pos[0].cpu().double().numpy(), 0.5, 0.0)
    near = o["near"]
    same = (vel == v0).all(dim=2).cpu().numpy()
    assert same[:, ~near].all() and same[:, -1].all()
    moved = ~same[0]
    # a row inside the reach is written; what it holds changes where the model's impulse is more than a few roundings of the
    # velocity (an atom of the all-zero class at lambda_elec = 0, or a pair at the end of the switch, feels nothing)
    dv = 0.37 * np.abs(o["F"]) / 12.0
    felt = (dv > 8 * EPS[prec] * np.abs(v0[0].cpu().double().numpy())).any(axis=1)
    felt[-1] = False  # (the row without mass)
    assert not felt[~near].any() and moved[felt].all() and felt.sum() >= min(2, s["N"] - 1)
    if (n, nenv) == (5, 400):
        assert (~near).sum() > 100


# ----------------------------------------------------------------------------- TIP3P: the engine's own paths
WATER_TERMS = ["lj", "electrostatics", "bonds", "angles"]


def _water(prec, nside=6):
    from torchmd_amd.builders import tip3p_box, water_forcefield
    from torchmd_amd.parameters import Parameters

    mol, pos, box = tip3p_box(nside, seed=21)
    par = Parameters(water_forcefield(mol), mol, WATER_TERMS, precision=PREC[prec])
    return mol, np.asarray(pos, dtype=np.float64), np.asarray(box, dtype=np.float64), par


def _water_system(mol, pos, box, prec, R, vel0=None):
    from torchmd_amd.systems import System

    s = System(mol.numAtoms, R, PREC[prec], _dev())
    s.set_positions(np.repeat(pos[:, :, None], R, axis=2))
    s.set_box(box)
    if vel0 is not None:
        s.set_velocities(vel0.to(PREC[prec]))
    return s


def _vel0(mol, R, T=300.0):
    from torchmd_amd.builders import water_forcefield
    from torchmd_amd.integrator import maxwell_boltzmann
    from torchmd_amd.parameters import Parameters

    torch.manual_seed(5)
    return maxwell_boltzmann(Parameters(water_forcefield(mol), mol, WATER_TERMS, precision=torch.float64).masses, T, R)


SOLUTE_WATER = [300, 301, 302]


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_water_solute_end_points_and_the_charge_table(prec):
    """One water of the 648-atom box as the solute: lambda = (1, 1) is the plain box; the fp32 context keeps its
    charge-by-class path (the null class did not merge with a charged class)."""
    from torchmd_amd import Alchemical
    from torchmd_amd.forces import Forces

    mol, pos, box, par = _water(prec)
    kw = dict(cutoff=CUT, rfa=True, switch_dist=SWD)
    s0, s1 = _water_system(mol, pos, box, prec, 1), _water_system(mol, pos, box, prec, 1)
    plain = Forces(par, terms=WATER_TERMS, **kw)
    alch = Forces(par, terms=WATER_TERMS, alchemical=Alchemical(SOLUTE_WATER), **kw)
    d0 = plain.compute(s0.pos, s0.box, s0.forces, returnDetails=True)[0]
    d1 = alch.compute(s1.pos, s1.box, s1.forces, returnDetails=True)[0]
    e0, e1 = sum(d0.values()), sum(d1.values())
    err = (s0.forces - s1.forces).abs().max().item()
    print(f"{prec} water solute: {e1:.6f} vs {e0:.6f}, max |dF| = {err:.2e}")
    assert abs(e1 - e0) <= _total_bar(prec, d0, d1) and err <= FTOL[prec]
    if prec == "f32":
        assert alch.stats(s1.pos)["charge_by_class"] == plain.stats(s0.pos)["charge_by_class"] == 1


def _by_hand(case, prec, al, cuts, langevin, algorithm="auto", restraints=None):
    """The truth: tmdhip_first_vv, the total force of an evaluation (the alchemical part added in force mode),
    tmdhip_(langevin_)second_vv."""
    from torchmd_amd import _lib as L
    from torchmd_amd.forces import Forces
    from torchmd_amd.integrator import Integrator

    mol, pos, box, par, vel0, R, kw = case
    s = _water_system(mol, pos, box, prec, R, vel0)
    f = Forces(par, terms=WATER_TERMS, alchemical=al, algorithm=algorithm, restraints=restraints, **kw)
    torch.manual_seed(77)
    integ = Integrator(s, f, 1.0, _dev(), **(dict(gamma=50.0, T=300.0) if langevin else {}))
    integ._check_layout()
    lib, code, N = L.load(), L.dtype_code(s.pos.dtype), s.pos.shape[1]
    f._compute_async(s.pos, s.box, s.forces, want_energy=False)
    st = _stream(_dev())
    for step in range(sum(cuts)):
        L.check(lib.tmdhip_first_vv(code, R, N, s.pos.data_ptr(), s.vel.data_ptr(), s.forces.data_ptr(), integ.masses.data_ptr(), integ.dt, st))
        f._compute_async(s.pos, s.box, s.forces, want_energy=False)
        if langevin:
            L.check(lib.tmdhip_langevin_second_vv(code, R, N, s.vel.data_ptr(), s.forces.data_ptr(), integ.masses.data_ptr(),
                                                  integ.vcoeff.data_ptr(), integ.dt, float(integ.gamma), integ._seed, step, st))
        else:
            L.check(lib.tmdhip_second_vv(code, R, N, s.vel.data_ptr(), s.forces.data_ptr(), integ.masses.data_ptr(), integ.dt, st))
    return s.pos.cpu().double().numpy(), s.vel.cpu().double().numpy()


def _under_test(case, prec, al, cuts, langevin, algorithm="auto", restraints=None):
    from torchmd_amd.forces import Forces
    from torchmd_amd.integrator import Integrator

    mol, pos, box, par, vel0, R, kw = case
    s = _water_system(mol, pos, box, prec, R, vel0)
    f = Forces(par, terms=WATER_TERMS, alchemical=al, algorithm=algorithm, restraints=restraints, **kw)
    f.compute(s.pos, s.box, s.forces)
    torch.manual_seed(77)
    integ = Integrator(s, f, 1.0, _dev(), **(dict(gamma=50.0, T=300.0) if langevin else {}))
    out = None
    for n in cuts:
        out = integ.step(n)
    return s.pos.cpu().double().numpy(), s.vel.cpu().double().numpy(), out, f, s


CUTS = (1, 2, 7)


def _check_return(prec, out, f, s):
    F2 = torch.zeros_like(s.pos)
    tot = f.compute(s.pos, s.box, F2)
    for r in range(s.pos.shape[0]):
        assert abs(out[1][r] - tot[r]) <= ERTOL[prec] * EFAC * max(1.0, abs(tot[r])), (r, out[1][r], tot[r])
    assert (s.forces - F2).abs().max().item() <= FTOL[prec] * 10


@pytest.mark.parametrize("langevin", [False, True], ids=["nve", "langevin"])
@pytest.mark.parametrize("algorithm", ["celllist", "allpairs"])
def test_trajectory_fp64(algorithm, langevin, monkeypatch):
    from torchmd_amd import Alchemical

    monkeypatch.setenv("TMDHIP_VSKIN", "0")
    nside = 12 if algorithm == "celllist" else 6
    mol, pos, box, par = _water("f64", nside)
    R = 3
    case = (mol, pos, box, par, _vel0(mol, R), R, dict(cutoff=CUT, rfa=True, switch_dist=SWD))
    lam = ([0.5, 1.0, 0.0], [0.0, 0.5, 0.0])
    tp, tv = _by_hand(case, "f64", Alchemical(SOLUTE_WATER, *lam), CUTS, langevin, algorithm)
    p, v, out, f, s = _under_test(case, "f64", Alchemical(SOLUTE_WATER, *lam), CUTS, langevin, algorithm)
    assert f.stats(s.pos)["algorithm"] == algorithm
    bar_p, bar_v = 64 * EPS64 * 10 * np.abs(tp).max(), 64 * EPS64 * 10 * np.abs(tv).max()
    print(f"fp64 {algorithm} {'Langevin' if langevin else 'NVE'}: |dpos| = {np.abs(p - tp).max():.2e} (bar {bar_p:.2e}), "
          f"|dvel| = {np.abs(v - tv).max():.2e} (bar {bar_v:.2e})")
    assert np.abs(p - tp).max() <= bar_p and np.abs(v - tv).max() <= bar_v
    cp, cv = _by_hand(case, "f64", Alchemical(SOLUTE_WATER, [0.6, 1.0, 0.1], [0.0, 0.4, 0.0]), CUTS, langevin, algorithm)
    assert np.abs(cp - tp).max() > 10 * bar_p and np.abs(cv - tv).max() > 10 * bar_v
    _check_return("f64", out, f, s)


@pytest.mark.parametrize("langevin", [False, True], ids=["nve", "langevin"])
def test_trajectory_fp32_fused_batched(langevin, monkeypatch):
    from torchmd_amd import Alchemical

    monkeypatch.setenv("TMDHIP_VSKIN", "0")
    R = 3
    mol, pos, box, par32 = _water("f32", 12)
    _, _, _, par64 = _water("f64", 12)
    vel0 = _vel0(mol, R)
    kw = dict(cutoff=CUT, rfa=True, switch_dist=SWD)
    lam = ([0.5, 1.0, 0.0], [0.0, 0.5, 0.0])
    tp, tv = _by_hand((mol, pos, box, par64, vel0, R, kw), "f64", Alchemical(SOLUTE_WATER, *lam), CUTS, langevin)
    hp, hv = _by_hand((mol, pos, box, par32, vel0, R, kw), "f32", Alchemical(SOLUTE_WATER, *lam), CUTS, langevin)
    p, v, out, f, s = _under_test((mol, pos, box, par32, vel0, R, kw), "f32", Alchemical(SOLUTE_WATER, *lam), CUTS, langevin)
    noise_p, noise_v = np.abs(hp - tp).max(), np.abs(hv - tv).max()
    dp, dv = np.abs(p - tp).max(), np.abs(v - tv).max()
    print(f"fp32 fused R=3 {'Langevin' if langevin else 'NVE'}: |dpos| = {dp:.2e} (by hand {noise_p:.2e}), |dvel| = {dv:.2e} (by hand {noise_v:.2e})")
    st = [f.stats(s.pos, r) for r in range(R)]
    assert all(x["steps_in_pair_launch"] >= 5 for x in st) and st[0]["batched_launches"] >= 5, st
    assert dp <= 2 * noise_p and dv <= 2 * noise_v
    cp, cv = _by_hand((mol, pos, box, par32, vel0, R, kw), "f32", Alchemical(SOLUTE_WATER, [0.6, 1.0, 0.1], [0.0, 0.4, 0.0]), CUTS, langevin)
    assert np.abs(cp - tp).max() > 10 * 2 * noise_p and np.abs(cv - tv).max() > 10 * 2 * noise_v
    _check_return("f32", out, f, s)


# ----------------------------------------------------------------------------- two side terms at once
RESTRAINED = [SOLUTE_WATER[0], 0]  # an oxygen of the solute and one of the environment
RESTRAINT_K = (20.0, 40.0, 0.0)  # kcal/mol/A^2, one strength per replica


def _held(pos, k=RESTRAINT_K):
    """Position restraints that hold the two oxygens 0.5 A off their start, with one strength per replica."""
    from torchmd_amd import Restraints

    return Restraints(3).add_position(RESTRAINED, pos[RESTRAINED] + np.array([0.5, 0.0, 0.0]), np.repeat(np.array(k)[:, None], 2, axis=1))


def _check_both_reported(f, s):
    d = f.compute(s.pos, s.box, torch.zeros_like(s.pos), returnDetails=True)[0]
    assert d["alchemical"] != 0.0 and d["restraints"] != 0.0, d


@pytest.mark.parametrize("langevin", [False, True], ids=["nve", "langevin"])
@pytest.mark.parametrize("algorithm", ["celllist", "allpairs"])
def test_two_side_terms_trajectory_fp64(algorithm, langevin, monkeypatch):
    """An alchemical solute and restraints together: every active side term is launched at the per-replica dispatch site of
    tmdhip_md_run (cell list) and at the replicas-together one (all pairs).  The control leaves the restraints out."""
    from torchmd_amd import Alchemical

    monkeypatch.setenv("TMDHIP_VSKIN", "0")
    mol, pos, box, par = _water("f64", 12 if algorithm == "celllist" else 6)
    R = 3
    case = (mol, pos, box, par, _vel0(mol, R), R, dict(cutoff=CUT, rfa=True, switch_dist=SWD))
    lam = ([0.5, 1.0, 0.0], [0.0, 0.5, 0.0])
    tp, tv = _by_hand(case, "f64", Alchemical(SOLUTE_WATER, *lam), CUTS, langevin, algorithm, _held(pos))
    p, v, out, f, s = _under_test(case, "f64", Alchemical(SOLUTE_WATER, *lam), CUTS, langevin, algorithm, _held(pos))
    assert f.stats(s.pos)["algorithm"] == algorithm
    bar_p, bar_v = 64 * EPS64 * 10 * np.abs(tp).max(), 64 * EPS64 * 10 * np.abs(tv).max()
    print(f"fp64 {algorithm} {'Langevin' if langevin else 'NVE'}, two terms: |dpos| = {np.abs(p - tp).max():.2e} (bar {bar_p:.2e}), "
          f"|dvel| = {np.abs(v - tv).max():.2e} (bar {bar_v:.2e})")
    assert np.abs(p - tp).max() <= bar_p and np.abs(v - tv).max() <= bar_v
    cp, cv = _by_hand(case, "f64", Alchemical(SOLUTE_WATER, *lam), CUTS, langevin, algorithm, _held(pos, (0.0, 0.0, 0.0)))
    assert np.abs(cp - tp).max() > 10 * bar_p and np.abs(cv - tv).max() > 10 * bar_v
    _check_return("f64", out, f, s)
    _check_both_reported(f, s)


@pytest.mark.parametrize("langevin", [False, True], ids=["nve", "langevin"])
def test_two_side_terms_trajectory_fp32_fused_batched(langevin, monkeypatch):
    """The same through the batched pair + step launch: one impulse launch per active side term serves all replicas."""
    from torchmd_amd import Alchemical

    monkeypatch.setenv("TMDHIP_VSKIN", "0")
    R = 3
    mol, pos, box, par32 = _water("f32", 12)
    _, _, _, par64 = _water("f64", 12)
    vel0 = _vel0(mol, R)
    kw = dict(cutoff=CUT, rfa=True, switch_dist=SWD)
    lam = ([0.5, 1.0, 0.0], [0.0, 0.5, 0.0])
    tp, tv = _by_hand((mol, pos, box, par64, vel0, R, kw), "f64", Alchemical(SOLUTE_WATER, *lam), CUTS, langevin, restraints=_held(pos))
    hp, hv = _by_hand((mol, pos, box, par32, vel0, R, kw), "f32", Alchemical(SOLUTE_WATER, *lam), CUTS, langevin, restraints=_held(pos))
    p, v, out, f, s = _under_test((mol, pos, box, par32, vel0, R, kw), "f32", Alchemical(SOLUTE_WATER, *lam), CUTS, langevin,
                                  restraints=_held(pos))
    noise_p, noise_v = np.abs(hp - tp).max(), np.abs(hv - tv).max()
    dp, dv = np.abs(p - tp).max(), np.abs(v - tv).max()
    print(f"fp32 fused R=3 {'Langevin' if langevin else 'NVE'}, two terms: |dpos| = {dp:.2e} (by hand {noise_p:.2e}), "
          f"|dvel| = {dv:.2e} (by hand {noise_v:.2e})")
    st = [f.stats(s.pos, r) for r in range(R)]
    assert all(x["steps_in_pair_launch"] >= 5 for x in st) and st[0]["batched_launches"] >= 5, st
    assert dp <= 2 * noise_p and dv <= 2 * noise_v
    cp, cv = _by_hand((mol, pos, box, par32, vel0, R, kw), "f32", Alchemical(SOLUTE_WATER, *lam), CUTS, langevin,
                      restraints=_held(pos, (0.0, 0.0, 0.0)))
    assert np.abs(cp - tp).max() > 10 * 2 * noise_p and np.abs(cv - tv).max() > 10 * 2 * noise_v
    _check_return("f32", out, f, s)
    _check_both_reported(f, s)


# ----------------------------------------------------------------------------- invariants
def test_nve_drift_is_at_most_twice_the_plain_run():
    from torchmd_amd import Alchemical
    from torchmd_amd.forces import Forces
    from torchmd_amd.integrator import Integrator

    mol, pos, box, par = _water("f64")
    drift = {}
    for name in ("plain", "alchemical"):
        s = _water_system(mol, pos, box, "f64", 1, _vel0(mol, 1, 150.0))
        al = Alchemical(SOLUTE_WATER, 0.5, 0.0) if name == "alchemical" else None
        f = Forces(par, terms=WATER_TERMS, cutoff=CUT, rfa=True, switch_dist=SWD, switch_mode="exact", **({"alchemical": al} if al else {}))
        f.compute(s.pos, s.box, s.forces)
        integ = Integrator(s, f, 0.25, _dev())
        e = []
        for _ in range(8):
            ek, ep, _ = integ.step(25)
            e.append(ek[0] + ep[0])
        drift[name] = max(e) - min(e)
    print(f"NVE, 200 steps of 0.25 fs: total-energy spread plain {drift['plain']:.3e}, lambda_vdw 0.5 {drift['alchemical']:.3e}")
    assert drift["alchemical"] <= 2 * drift["plain"]


def test_minimize_fire_reaches_fmax():
    from torchmd_amd import Alchemical
    from torchmd_amd.forces import Forces
    from torchmd_amd.minimizers import minimize_fire

    mol, pos, box, par = _water("f64")
    s = _water_system(mol, pos, box, "f64", 2)
    f = Forces(par, terms=WATER_TERMS, cutoff=CUT, rfa=True, switch_dist=SWD, alchemical=Alchemical(SOLUTE_WATER, [0.5, 1.0], [0.0, 1.0]))
    minimize_fire(s, f, fmax=5.0, steps=2000)
    F = torch.zeros_like(s.pos)
    f.compute(s.pos, s.box, F)
    fm = F.norm(dim=2).max().item()
    print(f"FIRE: largest atom force {fm:.3f}")
    assert fm <= 5.0


def test_constraints_on_the_solute_hold():
    """constraints="water" at 2 fs with a water as the solute: every bond length, the solute's included, is kept at the
    constraint solver's own tolerance (tests/test_gpu_constraints.py: 1e-10 relative in fp64)."""
    from torchmd_amd import Alchemical
    from torchmd_amd.forces import Forces
    from torchmd_amd.integrator import Integrator

    mol, pos, box, par = _water("f64")
    s = _water_system(mol, pos, box, "f64", 1, _vel0(mol, 1))
    f = Forces(par, terms=WATER_TERMS, cutoff=CUT, rfa=True, switch_dist=SWD, alchemical=Alchemical(SOLUTE_WATER, 0.5, 0.0))
    f.compute(s.pos, s.box, s.forces)
    integ = Integrator(s, f, 2.0, _dev(), gamma=1.0, T=300.0, constraints="water")
    for _ in range(5):
        integ.step(20)
    p = s.pos[0].cpu().double().numpy()
    cs = integ.constraints
    w = np.asarray(cs.waters)
    assert (w == np.array(SOLUTE_WATER)).all(axis=1).any()
    d = np.stack([np.linalg.norm(p[w[:, 0]] - p[w[:, 1]], axis=1), np.linalg.norm(p[w[:, 0]] - p[w[:, 2]], axis=1),
                  np.linalg.norm(p[w[:, 1]] - p[w[:, 2]], axis=1)], axis=1)
    d0 = np.asarray(cs.water_dist)
    want = np.stack([d0[:, 0], d0[:, 0], d0[:, 1]], axis=1)
    dev = np.abs(d / want - 1.0).max()
    print(f"bond lengths with a decoupling water: worst relative error {dev:.2e}")
    assert dev <= 1e-10 and np.isfinite(p).all()


def test_library_refusals_launch_nothing():
    from torchmd_amd import _lib as L
    from torchmd_amd import Alchemical

    sysd = _case(3, 65, 20.0)
    f, par = _forces(sysd, "f64", Alchemical(sysd["atoms"], 1.0, 1.0))
    pos, box = _tensors(sysd["pos"], sysd["box"], 1, "f64")
    eng = f._engine(pos)
    eng.sync_alchemical(f)
    lib = eng.lib

    def desc(**kw):
        d = L.AlchemicalDesc()
        d.struct_size = C.sizeof(L.AlchemicalDesc)
        d.enable, d.natoms, d.nreplicas, d.alpha = 1, 3, 1, 0.5
        keep = dict(atoms=np.array([0, 1, 2], dtype=np.int32), q=np.zeros(3), cls=np.zeros(3, dtype=np.int32), lv=np.array([1.0]), le=np.array([1.0]))
        keep.update({k: v for k, v in kw.items() if k in keep})
        d.atoms_host, d.charges_host, d.classes_host = (keep[k].ctypes.data_as(C.c_void_p) for k in ("atoms", "q", "cls"))
        d.lambda_vdw_host, d.lambda_elec_host = keep["lv"].ctypes.data_as(C.c_void_p), keep["le"].ctypes.data_as(C.c_void_p)
        for k, v in kw.items():
            if k not in keep:
                setattr(d, k, v)
        return d, keep

    vel = torch.zeros_like(pos)
    bad = [desc(struct_size=8), desc(atoms=np.array([0, 1, 99], dtype=np.int32)), desc(atoms=np.array([0, 1, 1], dtype=np.int32)),
           desc(lv=np.array([1.2])), desc(lv=np.array([0.5]), le=np.array([0.5])), desc(alpha=-1.0), desc(nreplicas=2),
           desc(atoms=np.array([0, 1, 3], dtype=np.int32)), desc(cls=np.array([0, 1, 77], dtype=np.int32))]
    for d, keep in bad:
        assert lib.tmdhip_set_alchemical(eng.ctx, C.byref(d)) != 0, L.last_error() if hasattr(L, "last_error") else ""
    assert lib.tmdhip_set_alchemical(eng.ctx, None) != 0
    # the state that was there still serves; apply without positions is refused; a context without the state launches nothing
    E, _ = _alch_only(f, pos, box)
    assert np.isfinite(E).all()
    assert lib.tmdhip_alchemical_apply(eng.ctx, C.c_void_p(), None, C.c_void_p(), C.c_void_p(vel.data_ptr()), C.c_void_p(), 1.0, C.c_void_p(),
                                       _stream(_dev())) != 0
    plain, _ = _forces(sysd, "f64")
    e2 = plain._engine(pos)
    out = torch.ones(1, 5, dtype=torch.float64, device=_dev())
    assert lib.tmdhip_alchemical_apply(e2.ctx, C.c_void_p(pos.data_ptr()), f._replica_boxes(box, 1).ctypes.data_as(C.POINTER(C.c_double)),
                                       C.c_void_p(), C.c_void_p(vel.data_ptr()), C.c_void_p(), 1.0, C.c_void_p(out.data_ptr()), _stream(_dev())) == 0
    torch.cuda.synchronize()
    assert not vel.any() and not out.any()
    # a context that still counts the solute itself is refused
    d, keep = desc()
    assert lib.tmdhip_set_alchemical(e2.ctx, C.byref(d)) != 0


def test_python_refusals():
    from torchmd_amd import Alchemical
    from torchmd_amd.forces import Forces

    mol, pos, box, par = _water("f64")
    kw = dict(cutoff=CUT, rfa=True)
    with pytest.raises(ValueError, match="closed under the topology"):
        Forces(par, terms=WATER_TERMS, alchemical=Alchemical([300, 301]), **kw)
    with pytest.raises(ValueError):
        Forces(par, terms=WATER_TERMS, alchemical=Alchemical([10 ** 6]), **kw)
    with pytest.raises(ValueError, match="pme"):
        Forces(par, terms=WATER_TERMS, alchemical=Alchemical(SOLUTE_WATER), cutoff=CUT, pme=True)
    with pytest.raises(ValueError, match="repulsion"):
        Forces(par, terms=WATER_TERMS + ["repulsion"], alchemical=Alchemical(SOLUTE_WATER), **kw)
    f = Forces(par, terms=WATER_TERMS, alchemical=Alchemical(SOLUTE_WATER), **kw)
    s = _water_system(mol, pos, box, "f64", 1)
    with pytest.raises(ValueError, match="alchemical"):
        f.virial(s.pos, s.box)
    with pytest.raises(ValueError, match="no evaluation yet"):
        f.alchemical_terms()
    with pytest.raises(ValueError):
        Forces(par, terms=WATER_TERMS, **kw).alchemical_terms()


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
        "replicas": 2, "precision": "single", "device": "cuda", "timestep": 1, "temperature": 300, "langevin_temperature": 300,
        "langevin_gamma": 1.0, "seed": 1, "steps": 40, "output_period": 20, "save_period": 0, "output": "output"}
out = {}
def go(name, **kw):
    c = dict(conf, log_dir=os.path.join(TMP, name), **kw)
    open(os.path.join(TMP, name + ".yaml"), "w").write(yaml.safe_dump(c))
    driver.main(["--conf", os.path.join(TMP, name + ".yaml")])
    log = os.path.join(TMP, name)
    out[name] = {"files": sorted(os.listdir(log)), "rows": [open(os.path.join(log, f"monitor_{k}.csv")).read().splitlines() for k in range(2)]}
go("log")
out["module_after_off"] = "torchmd_amd.alchemy" in sys.modules
go("log_al", alchemical={"atoms": [30, 31, 32], "lambda_vdw": [0.5, 1.0], "lambda_elec": [0.0, 1.0], "alpha": 0.5,
                          "states": [[1.0, 1.0], [0.5, 0.0], [0.0, 0.0]]})
out["states"] = [np.load(os.path.join(TMP, "log_al", f"output_states_{k}.npy")).tolist() for k in range(2)]
print("RESULT " + json.dumps(out))
"""


def test_run_py_with_the_mapping(tmp_path):
    import json

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = f"ROOT = {root!r}\nTMP = {str(tmp_path)!r}\n" + _CHILD
    res = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, cwd=root)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-4000:]
    out = json.loads(next(ln for ln in res.stdout.splitlines() if ln.startswith("RESULT "))[7:])
    files = ["input.yaml"] + [f"monitor_{k}.csv" for k in range(2)] + [f"output_{k}.npy" for k in range(2)]
    assert out["module_after_off"] is False  # without the key the module is never imported
    assert out["log"]["files"] == files
    assert out["log_al"]["files"] == sorted(files + [f"output_states_{k}.npy" for k in range(2)])
    for k, rows in enumerate(out["log_al"]["rows"]):
        assert rows[0] == "iter,ns,epot,ekin,etot,T,alchemical,dudl_vdw,dudl_elec,t" and len(rows) == 3
        vals = np.array([[float(x) for x in r.split(",")] for r in rows[1:]])
        assert np.isfinite(vals).all() and (vals[:, 6] != 0).all() and (vals[:, 7] != 0).all() and (vals[:, 8] != 0).all()
        st = np.array(out["states"][k])
        assert st.shape == (2, 3) and np.isfinite(st).all() and (st[:, 2] == 0.0).all() and (st[:, 0] != 0).all()


def test_python_refusals_of_combinations():
    """torch.vmap, batch=, barostat=, implicit_solvent=, virtual_sites= and a cross pair with A > 0 >= B: ValueError, the last one
    when the Forces object is built."""
    from torchmd_amd import Alchemical
    from torchmd_amd.barostat import MonteCarloBarostat
    from torchmd_amd.builders import tip4p_box, tip4pew_forcefield
    from torchmd_amd.forces import Forces
    from torchmd_amd.implicit import GeneralizedBorn
    from torchmd_amd.integrator import Integrator
    from torchmd_amd.parameters import Parameters

    mol, pos, box, par = _water("f64")
    kw = dict(cutoff=CUT, rfa=True)
    f = Forces(par, terms=WATER_TERMS, alchemical=Alchemical(SOLUTE_WATER), **kw)
    s = _water_system(mol, pos, box, "f64", 1, _vel0(mol, 1))
    with pytest.raises(ValueError, match="vmap"):
        torch.vmap(lambda p: f.compute(p, s.box, None, toNumpy=False))(torch.stack([s.pos, s.pos]))
    with pytest.raises(ValueError, match="vmap"):
        torch.vmap(lambda p: torch.as_tensor(f.alchemical_energies(p, s.box, [[1.0, 1.0]])))(torch.stack([s.pos, s.pos]))
    with pytest.raises(ValueError, match="batch"):
        Integrator(s, f, 1.0, _dev(), gamma=0.1, T=300.0, batch=torch.zeros(mol.numAtoms, dtype=torch.long))
    with pytest.raises(ValueError, match="barostat"):
        Integrator(s, f, 1.0, _dev(), gamma=0.1, T=300.0, barostat=MonteCarloBarostat(1.0, 300.0, 25))
    with pytest.raises(ValueError, match="implicit_solvent"):
        Forces(par, terms=WATER_TERMS, alchemical=Alchemical(SOLUTE_WATER), implicit_solvent=GeneralizedBorn.from_parameters(par))
    mol4, pos4, box4, vs = tip4p_box(2, seed=1)
    par4 = Parameters(tip4pew_forcefield(mol4), mol4, WATER_TERMS, precision=torch.float64)
    with pytest.raises(ValueError, match="virtual_sites"):
        Forces(par4, terms=WATER_TERMS, virtual_sites=vs, alchemical=Alchemical([0, 1, 2, 3]), cutoff=4.0, rfa=True)
    bad = dict(_case(3, 65, 20.0))
    bad["B"] = bad["B"].copy()
    bad["B"][0, 2] = bad["B"][2, 0] = 0.0
    with pytest.raises(ValueError, match="A > 0 >= B"):
        _forces(bad, "f64", Alchemical(bad["atoms"]))


def test_library_refusals_by_context():
    """tmdhip_set_alchemical refuses a context with PME, with the generalized-Born model, with the repulsion term, and a cross
    pair with A > 0 >= B (reached here past the Python check); refused calls change nothing: the state that was there gives the
    same bits afterwards."""
    from torchmd_amd import _lib as L
    from torchmd_amd import Alchemical
    from torchmd_amd.forces import Forces
    from torchmd_amd.implicit import GeneralizedBorn

    lib = L.load()

    def desc(n_atoms=3):
        d = L.AlchemicalDesc()
        d.struct_size = C.sizeof(L.AlchemicalDesc)
        d.enable, d.natoms, d.nreplicas, d.alpha = 1, n_atoms, 1, 0.5
        keep = [np.arange(n_atoms, dtype=np.int32), np.zeros(n_atoms), np.zeros(n_atoms, dtype=np.int32), np.array([1.0]), np.array([1.0])]
        d.atoms_host, d.charges_host, d.classes_host, d.lambda_vdw_host, d.lambda_elec_host = (a.ctypes.data_as(C.c_void_p) for a in keep)
        return d, keep

    mol, pos, box, par = _water("f64")
    s = _water_system(mol, pos, box, "f64", 1)
    for kw, word in ((dict(cutoff=CUT, pme=True), "PME"), (dict(terms=["repulsion"], cutoff=CUT), "repulsion")):
        terms = kw.pop("terms", WATER_TERMS)
        f = Forces(par, terms=terms, **kw)
        f.compute(s.pos, s.box, s.forces)
        d, keep = desc()
        assert lib.tmdhip_set_alchemical(f._engine(s.pos).ctx, C.byref(d)) != 0 and word in L.last_error()
    s0 = _water_system(mol, pos, np.zeros(3), "f64", 1)
    f = Forces(par, terms=WATER_TERMS, implicit_solvent=GeneralizedBorn.from_parameters(par))
    f.compute(s0.pos, s0.box, s0.forces)
    d, keep = desc()
    assert lib.tmdhip_set_alchemical(f._engine(s0.pos).ctx, C.byref(d)) != 0 and "generalized-Born" in L.last_error()
    # A > 0 >= B: only the context's own table can say so at this level
    bad = dict(_case(3, 65, 20.0))
    bad["B"] = bad["B"].copy()
    bad["B"][0, 2] = bad["B"][2, 0] = 0.0
    al = Alchemical(bad["atoms"])
    al.check = lambda *a, **k: None  # (past the Python check)
    f, _ = _forces(bad, "f64", al)
    p, b = _tensors(bad["pos"], bad["box"], 1, "f64")
    with pytest.raises(Exception, match="A > 0 >= B"):
        f._engine(p).sync_alchemical(f)
    # refused calls on a context that has a state leave it as it was
    good = _case(3, 65, 20.0)
    g, _ = _forces(good, "f64", Alchemical(good["atoms"], 0.5, 0.0))
    p, b = _tensors(good["pos"], good["box"], 1, "f64")
    E0, F0 = _alch_only(g, p, b)
    for change in (dict(alpha=-1.0), dict(natoms=4), dict(nreplicas=2), dict(struct_size=8)):
        d, keep = desc()
        for k, v in change.items():
            setattr(d, k, v)
        assert lib.tmdhip_set_alchemical(g._engine(p).ctx, C.byref(d)) != 0
    E1, F1 = _alch_only(g, p, b)
    assert np.array_equal(E0, E1) and np.array_equal(F0, F1)
