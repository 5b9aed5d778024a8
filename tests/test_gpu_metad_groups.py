"""Metadynamics on CVs of groups of atoms on the device: the kernels of metad_group.hip against the numpy model
(`Metadynamics.energy_forces`, `deposit_model` of a grouped bias), and `Integrator.step` under such a bias against the by-hand
loop of tests/test_gpu_restraints.py, whose parts know nothing of a bias.

Bars.  CVs (reported and logged) against the model: c eps64 sum|addends|, c counted from the operation sequence
(`_metad_groups.cv_bars`: the addends of a coordination CV are the model's to the bit, the device passes each through
chunk + 6 + 2 + rows / 64 + 6 additions and the model's sum is exact; 4 eps64 |s| for a CV of centres, where acos alone is not
shared).  Forces and velocities: fp64 within 1e-9 of the largest bias force or kick, fp32 rows within 1 ulp of
dtype(float64(in) + model) (the bars of tests/test_gpu_metad.py).  Grid nodes: within 8 eps64 x sum|terms| of the model fed with
the LOGGED centres (§18 (i): a centre that differs by the rounding of a sum moves a far node's term by |Delta| / sigma^2 ulps,
so the CVs are compared separately).  Finite differences: 10 |FD(h) - FD(h/2)| + 4 eps64 S_E / h, S_E the sum of the absolute
addends of the energy: those of the interpolant plus |dV/ds_c| times those of s_c.  Trajectories: as tests/test_gpu_restraints.py."""

import ctypes as C
import os

import numpy as np
import pytest
import torch

import _metad as M
import _metad_groups as G
import test_gpu_metad as TM
import test_gpu_restraints as TR
from _golden import PREC, GoldenParameters, load
from torchmd_amd.integrator import BOLTZMAN
from torchmd_amd.metadynamics import Metadynamics, coordination_pairs

pytestmark = pytest.mark.gpu

EPS64 = np.finfo(np.float64).eps
_dev, _bits, _tensor, _stream, _ulp = TR._dev, TR._bits, TR._tensor, TR._stream, TR._ulp
_context, _apply, _state, _rounded, _boxes = TM._context, TM._apply, TM._state, TM._rounded, TM._boxes
WATER_TERMS = TR.WATER_TERMS


def _kernel_against_model(prec, name, repeats, R=3, walkers="independent", second_context=False):
    pos, box, mass, md = G.kernel_case(name, R=R, walkers=walkers)
    N = pos.shape[1]
    pos, mass = _rounded(pos, prec), _rounded(mass, prec)
    f0, eng = _context(mass, md, prec, R)  # (hands the masses over: the default weights)
    assert md.check_extent(pos, box)
    grid = G.prefill(md, pos, box)
    md.set_grid(grid)
    md.sync(eng)
    rng = np.random.default_rng(99)
    p7 = _rounded(G.moved(pos, 7, box), prec)
    f_in = _rounded(rng.normal(0.0, 20.0, (R, N, 3)), prec)
    v_in = _rounded(rng.normal(0.0, 0.05, (R, N, 3)), prec)
    kick = 0.0123
    E, F, S = md.energy_forces(p7, box, grid)
    touched = np.zeros(N, dtype=bool)
    touched[md.row_atom] = True
    assert 0 < touched.sum() < N
    p, m = _tensor(p7, prec), _tensor(mass, prec)

    def once(mode, e=eng):
        f, v = _tensor(f_in, prec), _tensor(v_in, prec)
        o = torch.full((R, 3), -1.0, dtype=torch.float64, device=_dev())
        if mode == "finish":
            _apply(e, p, box, forces=f, vel=v, mass=m, kick=kick, out=o)
        elif mode == "impulse":
            _apply(e, p, box, vel=v, mass=m, kick=kick)
        else:
            _apply(e, p, box, forces=f, out=o)
        return f, v, o

    f, v, o = once("finish")
    got_f, got_v, got_o = f.cpu().double().numpy(), v.cpu().double().numpy(), o.cpu().numpy()
    fb = np.abs(F).max()
    assert fb > 0.5, fb  # (something was added)
    # ---- the reported CVs and V
    worst = 0.0
    for r in range(R):
        bars = G.cv_bars(md, p7[r], box)
        ds = np.abs(got_o[r, 1:1 + md.ncv] - S[r])
        worst = max(worst, (ds / bars).max())
        assert (ds <= bars).all(), (name, r, ds, bars)
        g = md._grid_of(grid, r)
        dV = md.interp(g, S[r])[1]
        v_bar = 16 * EPS64 * M.interp_magnitude(md, g, S[r])[0] + float(np.sum(np.abs(dV) * bars))
        assert abs(got_o[r, 0] - E[r]) <= v_bar, (name, r, got_o[r, 0], E[r], v_bar)
    if prec == "f32":
        want_f = _rounded(f_in + F, prec)
        want_v = _rounded(v_in + kick * F / mass[None, :, None], prec)
        df = (np.abs(got_f - want_f) / _ulp(want_f, prec)).max()
        dv = (np.abs(got_v - want_v) / _ulp(want_v, prec)).max()
        print(f"{prec} {name} R={R}: CVs {worst:.3f} of their bars, forces {df:.2f} ulp, velocities {dv:.2f} ulp, max|F_b| = {fb:.3f}")
        assert df <= 1.0 and dv <= 1.0
    else:
        df = np.abs(got_f - (f_in + F)).max() / fb
        dv = np.abs(got_v - (v_in + kick * F / mass[None, :, None])).max() / (kick * fb / mass.min())
        print(f"{prec} {name} R={R}: CVs {worst:.3f} of their bars, forces {df:.2e} max|F_b|, velocities {dv:.2e} of the largest kick, "
              f"max|F_b| = {fb:.3f}")
        assert df <= 1e-9 and dv <= 1e-9
    # rows of atoms in no CV: never written
    assert torch.equal(_bits(f)[:, ~touched], _bits(_tensor(f_in, prec))[:, ~touched])
    assert torch.equal(_bits(v)[:, ~touched], _bits(_tensor(v_in, prec))[:, ~touched])
    # the impulse writes the velocities only, by the same rule; the evaluation writes no velocity
    fi, vi, _ = once("impulse")
    assert torch.equal(_bits(vi), _bits(v)) and torch.equal(_bits(fi), _bits(_tensor(f_in, prec)))
    fe, ve, oe = once("evaluate")
    assert torch.equal(_bits(fe), _bits(f)) and torch.equal(_bits(ve), _bits(_tensor(v_in, prec))) and torch.equal(oe, o)
    for _ in range(repeats):  # no atomics: the same bits every time
        f2, v2, o2 = once("finish")
        assert torch.equal(_bits(f2), _bits(f)) and torch.equal(_bits(v2), _bits(v)) and torch.equal(o2, o)
    if second_context:  # ... and in another context
        _, _, _, md2 = G.kernel_case(name, R=R, walkers=walkers)
        f1, eng2 = _context(mass, md2, prec, R)
        md2.set_grid(grid)
        md2.sync(eng2)
        f3, v3, o3 = once("finish", eng2)
        assert torch.equal(_bits(f3), _bits(f)) and torch.equal(_bits(v3), _bits(v)) and torch.equal(o3, o)
    return md, eng, pos, box, mass


@pytest.mark.parametrize("name", G.KERNEL_CASES)
@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_kernel_against_model(prec, name):
    _kernel_against_model(prec, name, repeats=20, second_context=True)


def test_kernel_past_a_chunk_of_sixteen_replicas():
    _kernel_against_model("f32", "coordination 1x257, 65x64 overlapping", repeats=1, R=17)
    _kernel_against_model("f64", "shared atom", repeats=1, R=17)


# ----------------------------------------------------------------------------- depositions
def _deposit_five(prec, name, R=3, walkers="independent"):
    """Five depositions on the device; the model's chain at the same (rounded) positions; the model fed with the LOGGED
    centres; the logged centres against the model's CVs."""
    pos, box, mass, md = G.kernel_case(name, R=R, walkers=walkers)
    pos, mass = _rounded(pos, prec), _rounded(mass, prec)
    _context(mass, md, prec, R)
    grid, fed, mag = np.zeros_like(md.grid), np.zeros_like(md.grid), np.zeros_like(md.grid)
    worst = 0.0
    for k in range(5):
        pk = _rounded(G.moved(pos, k, box), prec)
        md.deposit(_state(pk, box, prec))
        grid, rows = md.deposit_model(pk, box, grid)
        log = md.hills()[k]
        for r in range(R):
            bars = G.cv_bars(md, pk[r], box)
            ds = np.abs(log[r, : md.ncv] - rows[r, : md.ncv])
            worst = max(worst, (ds / bars).max())
            assert (ds <= bars).all(), (name, k, r, ds, bars)
        # the heights: the closed form on the model's V at the LOGGED centres of the grid fed so far
        for r in range(R):
            g = 0 if walkers == "shared" else r
            V = md.interp(fed[g], log[r, : md.ncv])[0]
            w = md.hill_height(V)
            assert abs(log[r, md.ncv] - w) <= 1e-10 * w, (k, r, log[r, md.ncv], w)
        for r in range(R):
            g = 0 if walkers == "shared" else r
            t = md.gauss_terms(log[r, : md.ncv], log[r, md.ncv])
            fed[g] += t
            mag[g] += np.abs(t)
    dev = md.grid
    node = (np.abs(dev - fed) / np.maximum(mag, 1e-300)).max() / EPS64
    print(f"{prec} {name} R={R} {walkers}: logged CVs {worst:.3f} of their bars; nodes {node:.2f} eps64 x sum|terms| from the sums of the "
          f"logged hills; lowest height {md.hills()[..., md.ncv].min():.4f} of {md.height}")
    # (a far node's term below the smallest normal number carries an absolute rounding, not a relative one: the floor)
    assert (np.abs(dev - fed) <= 8 * EPS64 * mag + np.finfo(np.float64).tiny).all() and fed[..., 0].max() > 1.0
    assert md.hills()[..., md.ncv].min() < 0.9 * md.height  # (well-tempered: hills on top of a bias are lower)
    assert np.abs(dev - grid).max() <= 1e-6 * np.abs(grid).max()  # (the model's own chain: its CVs differ by the sums' rounding)
    return md, dev


@pytest.mark.parametrize("name", ["shared atom", "coordination 1x257, 65x64 overlapping", "zero box"])
@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_five_depositions(prec, name):
    _deposit_five(prec, name)


@pytest.mark.parametrize("R", [4, 17])
def test_shared_walkers_fill_one_grid_in_replica_order(R):
    md, g1 = _deposit_five("f64", "coordination 64x65, 130x1", R=R, walkers="shared")
    assert g1.shape[0] == 1 and md.hills().shape == (5, R, 3)
    md2, g2 = _deposit_five("f64", "coordination 64x65, 130x1", R=R, walkers="shared")
    assert np.array_equal(g1.view(np.int64), g2.view(np.int64)) and np.array_equal(md.hills().view(np.int64), md2.hills().view(np.int64))


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_device_heights_on_a_node_follow_the_closed_form(prec):
    """A group distance of two pairs whose centres lie 2.5 Å apart exactly, in either dtype: s0 = node 12."""
    md = Metadynamics(("group_distance", ({"atoms": [0, 1], "weights": [1.0, 1.0]}, {"atoms": [2, 3], "weights": [1.0, 3.0]})), sigma=0.25,
                      height=1.5, frequency=1, temperature=300.0, bias_factor=5.0, grid_min=1.0, grid_max=5.0, grid_bins=32)
    pos = np.array([[[-0.5, 0.0, 0.0], [0.5, 0.0, 0.0], [1.0, 0.0, 0.0], [3.0, 0.0, 0.0], [7.0, 7.0, 7.0]]])  # centres 0 and 2.5
    _context(np.ones(5), md, prec, 1)
    st = _state(pos, np.zeros(3), prec)
    for _ in range(3):
        md.deposit(st)
    log = md.hills()[:, 0]
    kdt = BOLTZMAN * 4.0 * 300.0
    want = [1.5, 1.5 * np.exp(-1.5 / kdt), 1.5 * np.exp(-(1.5 + 1.5 * np.exp(-1.5 / kdt)) / kdt)]
    print(f"{prec}: heights {log[:, 1]}, closed form {want}, relative deviation {np.abs(log[:, 1] / want - 1).max() / EPS64:.2f} eps64")
    assert (log[:, 0] == 2.5).all()
    assert (np.abs(log[:, 1] - want) <= 4 * EPS64 * np.asarray(want)).all()
    assert md.grid[0, 12, 0] == (log[0, 1] + log[1, 1]) + log[2, 1] and md.grid[0, 12, 1] == 0.0


# ----------------------------------------------------------------------------- forces against differences of compute()'s energy
def _energy_addends(md, grid, pos, box):
    """S_E of one replica: the interpolant's absolute addends plus |dV/ds_c| times those of s_c (a coordination CV: sum|f|; a
    CV of centres: |s|)."""
    s, _ = md.cv_values(pos, box)
    g = md._grid_of(grid, 0)
    dV = md.interp(g, s)[1]
    S = M.interp_magnitude(md, g, s)[0]
    for c in range(md.ncv):
        S += abs(dV[c]) * (G.coordination_magnitudes(md, c, pos, box)[0] if md.cv_kind[c] == 5 else abs(s[c]))
    return S


@pytest.mark.parametrize("which", ["centres", "coordination"])
def test_forces_are_the_derivative_of_the_energy_compute_reports(which):
    from torchmd_amd.forces import Forces

    pos, mass = G.lattice(R=1, seed=8)
    pos, box = pos[0], np.full(3, G.L)
    if which == "centres":
        a, b = G.nearest(pos, [0.5, 15.0, 15.0], 30, box), G.nearest(pos, [9.0, 17.0, 13.0], 8, box)
        md = Metadynamics(("group_distance", (a, b)), sigma=0.4, height=1.0, frequency=1000, temperature=300.0, bias_factor=8.0,
                          grid_min=2.0, grid_max=16.0, grid_bins=80)
        probe = [a[0], a[7], b[3]]
    else:
        # partners on both sides of d_max = 9: the 400 atoms nearest to the ion reach beyond 11 Å
        ion, partners = G.nearest(pos, [15.0, 15.0, 15.0], 1, box), G.nearest(pos, [15.0, 15.0, 15.0], 400, box)
        md = Metadynamics(("coordination", (ion, partners), G.SWITCH), sigma=0.5, height=1.0, frequency=1000, temperature=300.0,
                          bias_factor=8.0, grid_min=0.0, grid_max=40.0, grid_bins=200)
        probe = [ion[0], partners[5], partners[60], partners[399]]
    md.frozen = True
    f = Forces(TR._BarePar(mass, torch.float64), terms=[], metadynamics=md)
    grid = G.prefill(md, pos[None], box, offsets=((0.6, 30.0), (-1.0, 12.0), (1.8, 8.0), (0.1, 5.0), (-2.5, 9.0)))
    md.set_grid(grid)
    if which == "coordination":
        d = np.linalg.norm(G.min_image(pos[partners] - pos[ion[0]], box), axis=1)
        assert (d < 9.0).sum() > 100 and (d > 9.0).sum() > 100
    bt = torch.zeros(1, 3, 3, dtype=torch.float64)
    bt[0, range(3), range(3)] = torch.as_tensor(box)
    bt = bt.to(_dev())

    def energy(x):
        return f.compute(_tensor(x[None], "f64"), bt, torch.zeros(1, len(x), 3, dtype=torch.float64, device=_dev()))[0]

    F = torch.zeros(1, len(pos), 3, dtype=torch.float64, device=_dev())
    f.compute(_tensor(pos[None], "f64"), bt, F)
    F = F.cpu().numpy()[0]
    S_E = _energy_addends(md, grid, pos, box)
    h, worst = 1e-5, 0.0
    assert np.abs(F[probe]).max() > 0.1
    for a in probe:
        for k in range(3):
            fd = []
            for hh in (h, 0.5 * h):
                xp, xm = pos.copy(), pos.copy()
                xp[a, k] += hh
                xm[a, k] -= hh
                fd.append(-(energy(xp) - energy(xm)) / (2.0 * hh))
            bar = 10.0 * abs(fd[0] - fd[1]) + 4.0 * EPS64 * S_E / h
            worst = max(worst, abs(F[a, k] - fd[1]) / bar)
            assert abs(F[a, k] - fd[1]) <= bar, (which, a, k, F[a, k], fd, bar)
    print(f"{which}: worst |F - FD| = {worst:.3f} of the bar; max|F| on the probed atoms {np.abs(F[probe]).max():.3f}")


# ----------------------------------------------------------------------------- trajectories on the 5 184-atom box
def _tip3p(prec, R):
    """tests/test_gpu_restraints.py's `_tip3p` on `tip3p_box(nside=12)` as it comes (the lattice start of the issue)."""
    from torchmd_amd.builders import tip3p_box, water_forcefield
    from torchmd_amd.integrator import maxwell_boltzmann
    from torchmd_amd.parameters import Parameters

    mol, pos, box = tip3p_box(nside=12)
    par = Parameters(water_forcefield(mol), mol, WATER_TERMS, precision=PREC[prec])
    torch.manual_seed(5)
    vel0 = maxwell_boltzmann(Parameters(water_forcefield(mol), mol, WATER_TERMS, precision=torch.float64).masses, 300, R)
    return mol, np.asarray(pos, dtype=np.float64), np.asarray(box, dtype=np.float64), par, vel0


def _tip3p_bias(pos, box, R):
    """CV 1: the coordination of oxygen 0 with all 1 728 oxygens (itself among them: skipped); CV 2: the distance of two
    mass-weighted groups of 8 waters, one of them across a face.  Three hills per replica beside the start, frozen."""
    p = pos[:, :, 0] if pos.ndim == 3 else pos
    Lb = np.asarray(box, dtype=np.float64).reshape(-1)[:3]
    ox = np.arange(0, len(p), 3)
    f, _ = coordination_pairs(p, Lb, [0], ox, r0=3.5, n=6, d_max=9.0)
    s0 = f.sum()
    assert abs(s0 - 7.05) < 0.05, s0  # (the lattice start)

    def waters(centre):
        near = G.nearest(p[ox], centre, 8, Lb)
        return [int(3 * w + k) for w in near for k in range(3)]

    ga, gb = waters([0.3, 0.5 * Lb[1], 0.5 * Lb[2]]), waters([11.0, 0.4 * Lb[1], 0.6 * Lb[2]])
    assert np.ptp(p[ga][:, 0]) > 0.5 * Lb[0]  # across a face
    md = Metadynamics([("coordination", ([0], [int(a) for a in ox]), {"r0": 3.5, "n": 6, "d_max": 9.0}), ("group_distance", (ga, gb))],
                      sigma=[0.2, 0.3], height=1.0, frequency=1000, temperature=300.0, bias_factor=8.0, grid_min=[0.0, 4.0],
                      grid_max=[14.0, 20.0], grid_bins=[140, 128], nreplicas=R)
    return md


def _fill(md, pos, box, R):
    """Three hills per replica beside the start (the masses, the default weights, must be in place), frozen."""
    p = pos[:, :, 0] if pos.ndim == 3 else pos
    Lb = np.asarray(box, dtype=np.float64).reshape(-1)[:3]
    grid = G.prefill(md, np.repeat(p[None], R, axis=0), Lb, offsets=((1.0, 30.0), (-1.7, 12.0), (3.0, 8.0)))
    md.set_grid(grid)
    md.frozen = True
    return grid


def _biased(prec, R):
    mol, pos, box, par, vel0 = _tip3p(prec, R)
    md = _tip3p_bias(pos, box, R)
    md.masses = par.masses.detach().cpu().double().reshape(-1).numpy()
    grid = _fill(md, pos, box, R)
    return mol, pos, box, par, vel0, md, grid


@pytest.mark.parametrize("langevin", [False, True], ids=["nve", "langevin"])
def test_trajectory_fp64_list_path(langevin, monkeypatch):
    monkeypatch.setenv("TMDHIP_VSKIN", "0")
    mol, pos, box, par, vel0, md, grid = _biased("f64", 1)
    case = (mol, pos, box, par, vel0, 1, WATER_TERMS, dict(cutoff=9.0, rfa=True))
    tp, tv = TR._by_hand(case, "f64", TM._Model(md, grid), TR.CUTS, langevin)
    p, v, frc, out, f, s, integ = TR._under_test(case, "f64", None, TR.CUTS, langevin, metadynamics=md)
    bar_p, bar_v = 64 * EPS64 * 10 * np.abs(tp).max(), 64 * EPS64 * 10 * np.abs(tv).max()
    print(f"fp64 list path, {'Langevin' if langevin else 'NVE'}: |dpos| = {np.abs(p - tp).max():.2e} (bar {bar_p:.2e}), "
          f"|dvel| = {np.abs(v - tv).max():.2e} (bar {bar_v:.2e})")
    assert f.stats(s.pos)["algorithm"] == "celllist" and f.stats(s.pos)["steps_in_pair_launch"] == 0
    assert np.abs(p - tp).max() <= bar_p and np.abs(v - tv).max() <= bar_v
    assert md.nhills == 0 and np.array_equal(md.grid, grid)  # frozen: nothing was deposited
    TM._check_return("f64", out, f, s, md, grid, frc)


@pytest.mark.parametrize("R", [1, 3], ids=["lone", "batched"])
def test_trajectory_fp32_fused(R, monkeypatch):
    monkeypatch.setenv("TMDHIP_VSKIN", "0")
    mol, pos, box, par32, vel0, md, grid = _biased("f32", R)
    _, _, _, par64, _ = _tip3p("f64", R)
    if R == 3:
        assert not np.array_equal(grid[0], grid[1]) and not np.array_equal(grid[1], grid[2])
    kw = dict(cutoff=9.0, rfa=True)
    case64 = (mol, pos, box, par64, vel0, R, WATER_TERMS, kw)
    case32 = (mol, pos, box, par32, vel0, R, WATER_TERMS, kw)
    model = TM._Model(md, grid)
    tp, tv = TR._by_hand(case64, "f64", model, TR.CUTS, False)
    hp, hv = TR._by_hand(case32, "f32", model, TR.CUTS, False)
    p, v, frc, out, f, s, integ = TR._under_test(case32, "f32", None, TR.CUTS, False, metadynamics=md)
    noise_p, noise_v = np.abs(hp - tp).max(), np.abs(hv - tv).max()
    dp, dv = np.abs(p - tp).max(), np.abs(v - tv).max()
    print(f"fp32 fused R={R}: |dpos| = {dp:.2e} (by hand {noise_p:.2e}), |dvel| = {dv:.2e} (by hand {noise_v:.2e})")
    st = [f.stats(s.pos, r) for r in range(R)]
    assert all(x["steps_in_pair_launch"] >= 5 for x in st), st  # the interior steps of 2 + 7 were made by pair launches
    if R == 3:
        assert st[0]["batched_launches"] >= 5
    assert dp <= 2 * noise_p and dv <= 2 * noise_v
    # the control: the same by-hand loop with the model's grid halved misses that bar by more than 10x
    cp, cv = TR._by_hand(case32, "f32", TM._Model(md, 0.5 * grid), TR.CUTS, False)
    assert np.abs(cp - tp).max() > 10 * 2 * noise_p and np.abs(cv - tv).max() > 10 * 2 * noise_v
    TM._check_return("f32", out, f, s, md, grid, frc)


# ----------------------------------------------------------------------------- alanine dipeptide: phi beside a coordination CV
CARBONYL_O = 5


def _ala2(prec, frozen=False):
    from torchmd_amd.forces import Forces
    from torchmd_amd.integrator import Integrator
    from torchmd_amd.systems import System

    g = load("ala2")
    par = GoldenParameters(g, PREC[prec])
    mass = par.masses.detach().cpu().double().reshape(-1).numpy()
    water_o = [int(a) for a in np.arange(22, len(mass)) if mass[a] > 15.0]
    assert len(water_o) == (len(mass) - 22) // 3 and 15.0 < mass[CARBONYL_O] < 17.0
    md = Metadynamics([("dihedral", TM.PHI), ("coordination", ([CARBONYL_O], water_o), {"r0": 3.0, "n": 6, "d_max": 8.0})], sigma=[0.35, 0.15],
                      height=0.6, frequency=50, temperature=300.0, bias_factor=6.0, grid_min=[None, 0.0], grid_max=[None, 9.0],
                      grid_bins=[40, 120])
    md.frozen = frozen
    pos = np.asarray(g["pos"], dtype=np.float64).reshape(-1, 3)
    s = System(len(pos), 1, PREC[prec], _dev())
    s.set_positions(pos[:, :, None])
    s.set_box(np.asarray(g["box"], dtype=np.float64).reshape(-1)[:3])
    rng = np.random.default_rng(8)
    s.set_velocities(torch.as_tensor(0.01 * rng.standard_normal((1, len(pos), 3))).to(PREC[prec]))
    f = Forces(par, terms=TM.ALL_TERMS, metadynamics=md, **TM.ALA2_KW)
    f.compute(s.pos, s.box, s.forces)
    assert f.stats(s.pos)["algorithm"] == "celllist"
    torch.manual_seed(3)
    return g, md, s, f, Integrator(s, f, 1.0, _dev())


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_ala2_hills_follow_the_trajectory(prec, monkeypatch):
    monkeypatch.setenv("TMDHIP_VSKIN", "0")
    g, md, s, f, integ = _ala2(prec)
    box = np.diagonal(s.box.cpu().double().numpy(), axis1=1, axis2=2)
    fed = np.zeros_like(md.grid)
    for k in range(4):
        integ.step(50)
        assert md.nhills == k + 1
        pk = s.pos.cpu().double().numpy()
        _, rows = md.deposit_model(pk, box, fed)
        got = md.hills()[k]
        bars = G.cv_bars(md, pk[0], box[0])
        ds, dw = np.abs(got[0, :2] - rows[0, :2]), abs(got[0, 2] / rows[0, 2] - 1.0)
        print(f"{prec} hill {k}: s = {got[0, :2]}, w = {got[0, 2]:.6f}; |ds| = {ds} (bars {bars}), |dw/w| = {dw:.2e}")
        assert (ds <= bars).all() and dw <= 1e-10
        fed[0] += md.gauss_terms(got[0, :2], got[0, 2])
    assert np.abs(md.grid - fed).max() <= 1e-11 * np.abs(fed).max() and fed[..., 0].max() > 0.5
    assert np.allclose(md.cv[0], md.hills()[3, 0, :2], atol=1e-6)  # (the CVs of the last step are those of the last hill)


def test_ala2_save_load_continues_bit_for_bit(tmp_path, monkeypatch):
    monkeypatch.setenv("TMDHIP_VSKIN", "0")
    g, md, s, f, integ = _ala2("f32")
    integ.step(100)
    md.save(str(tmp_path / "bias.npz"))
    pos, vel, frc = s.pos.clone(), s.vel.clone(), s.forces.clone()
    f.invalidate_lists(s.pos)  # (the Verlet list is no part of a restart: the twin below builds its own at this step too)
    integ.step(100)
    want_log, want_grid, want_pos = md.hills(), md.grid.copy(), s.pos.clone()
    g2, md2, s2, f2, integ2 = _ala2("f32")
    md2.load(str(tmp_path / "bias.npz"))
    assert md2.nhills == 2
    s2.pos.copy_(pos), s2.vel.copy_(vel), s2.forces.copy_(frc)
    f2.invalidate_lists(s2.pos)
    integ2._nstep = 100
    integ2.step(100)
    assert np.array_equal(md2.hills().view(np.int64), want_log.view(np.int64))
    assert np.array_equal(md2.grid.view(np.int64), want_grid.view(np.int64)) and torch.equal(_bits(s2.pos), _bits(want_pos))


# ----------------------------------------------------------------------------- rigid water
def test_rigid_water_with_a_biased_coordination_number():
    """constraints="water" at 2 fs with a coordination CV on an oxygen: the bond lengths are kept as well as without a bias (the
    bar of tests/test_gpu_constraints.py as tests/test_gpu_metad.py applies it: four times the plain run's worst bond error plus
    8 eps64)."""
    from torchmd_amd.builders import tip3p_box, water_forcefield
    from torchmd_amd.forces import Forces
    from torchmd_amd.integrator import Integrator, maxwell_boltzmann
    from torchmd_amd.parameters import Parameters

    mol, pos, box = tip3p_box(6, seed=3)
    pos = np.asarray(pos, dtype=np.float64)
    par = Parameters(water_forcefield(mol), mol, WATER_TERMS, precision=torch.float64)
    p0 = pos[:, :, 0] if pos.ndim == 3 else pos
    Lb = np.asarray(box, dtype=np.float64).reshape(-1)[:3]
    ox = [int(a) for a in np.arange(0, len(p0), 3)]
    d_max = min(9.0, 0.49 * Lb.min())
    dev_bond = {}
    for name in ("plain", "biased"):
        md = None
        if name == "biased":
            md = Metadynamics(("coordination", ([ox[40]], ox), {"r0": 3.5, "n": 6, "d_max": d_max}), sigma=0.2, height=1.5, frequency=20,
                              temperature=300.0, bias_factor=8.0, grid_min=0.0, grid_max=14.0, grid_bins=140)
        torch.manual_seed(9)
        vel0 = maxwell_boltzmann(par.masses, 300.0, 1)
        s = TR._system(mol, pos, box, vel0, "f64", 1)
        f = Forces(par, terms=WATER_TERMS, cutoff=7.0, rfa=True, **({} if md is None else {"metadynamics": md}))
        f.compute(s.pos, s.box, s.forces)
        integ = Integrator(s, f, 2.0, _dev(), gamma=1.0, T=300.0, constraints="water")
        integ.step(200)
        p = s.pos[0].cpu().double().numpy()
        cs = integ.constraints
        w = np.asarray(cs.waters)
        dd = np.stack([np.linalg.norm(p[w[:, 0]] - p[w[:, 1]], axis=1), np.linalg.norm(p[w[:, 0]] - p[w[:, 2]], axis=1),
                       np.linalg.norm(p[w[:, 1]] - p[w[:, 2]], axis=1)], axis=1)
        d0 = np.asarray(cs.water_dist)
        dev_bond[name] = np.abs(dd / np.stack([d0[:, 0], d0[:, 0], d0[:, 1]], axis=1) - 1.0).max()
        if md is not None:
            assert md.nhills == 10 and md.grid[0, :, 0].max() > 1.0
    print(f"bond lengths: plain {dev_bond['plain']:.2e}, biased {dev_bond['biased']:.2e}")
    assert dev_bond["biased"] <= 4 * dev_bond["plain"] + 8 * EPS64


# ----------------------------------------------------------------------------- what is refused
def test_library_refusals_leave_the_bias_in_place():
    from torchmd_amd import _lib as L
    from torchmd_amd.forces import Forces

    pos, box, mass, md = G.kernel_case("coordination 1x257, 65x64 overlapping")
    f, eng = _context(mass, md, "f64", 3)
    lib = eng.lib
    grid = G.prefill(md, pos, box)
    md.set_grid(grid)
    md.sync(eng)
    p = _tensor(pos, "f64")
    ref_f = _tensor(np.zeros_like(pos), "f64")
    ref_o = torch.zeros(3, 3, dtype=torch.float64, device=_dev())
    _apply(eng, p, box, forces=ref_f, out=ref_o)
    assert ref_f.abs().max().item() > 0.5

    def same_bits():
        f2, o2 = _tensor(np.zeros_like(pos), "f64"), torch.zeros(3, 3, dtype=torch.float64, device=_dev())
        _apply(eng, p, box, forces=f2, out=o2)
        return torch.equal(_bits(f2), _bits(ref_f)) and torch.equal(o2, ref_o)

    def refused(change, expect):
        d, keep = md.group_descriptor()
        change(d, keep)
        assert lib.tmdhip_set_metadynamics_groups(eng.ctx, C.byref(d)) < 0
        assert expect in L.last_error(), (expect, L.last_error())

    def set_(name, value, index=None):
        def change(d, keep):
            if index is None:
                setattr(d, name, value)
            elif isinstance(index, tuple):
                getattr(d, name)[index[0]][index[1]] = value
            else:
                getattr(d, name)[index] = value
        return change

    def poke(which, where, value):
        def change(d, keep):
            keep[which][where] = value
        return change

    refused(set_("struct_size", 8), "size mismatch")
    refused(set_("nreplicas", 2), "nreplicas")
    refused(set_("ncv", 3), "more than 2 CVs")
    refused(set_("ncv", 0), "at least one")
    refused(set_("kind", 1, 0), "unknown kind")
    refused(set_("kind", 6, 1), "unknown kind")
    refused(poke(0, 1, 0), "is empty")
    refused(poke(1, 3, 5000), "out of range")
    refused(poke(1, 3, -1), "out of range")
    refused(lambda d, keep: keep[1].__setitem__(3, keep[1][2]), "repeated")
    refused(poke(2, 4, 0.0), "weights")
    refused(poke(2, 4, float("nan")), "weights")
    refused(set_("groups", 9, (0, 1)), "group index out of range")
    refused(set_("groups", 0, (1, 2)), "wrong number of groups")
    refused(lambda d, keep: (set_("kind", 2, 0)(d, keep), set_("groups", 0, (0, 1))(d, keep)), "named twice")
    refused(set_("coord_r0", 0.0, 0), "r0")
    refused(set_("coord_n", 1, 0), "n must")
    refused(set_("coord_n", 25, 1), "n must")
    refused(set_("coord_d0", -0.1, 0), "d0")
    refused(lambda d, keep: (set_("coord_d0", 9.5, 0)(d, keep)), "d_max")
    refused(set_("sigma", 0.0, 0), "sigma")
    refused(set_("bins", 0, 1), "bins")
    refused(set_("grid_min", 500.0, 1), "grid_min")
    refused(set_("bins", 30, 0), "sigma / 2")
    assert same_bits() and np.array_equal(md.fetch(), grid)
    # where a run or an evaluation starts: d_max beyond half the shortest edge, no d_max in a periodic box, a CV atom without mass
    small = np.array([30.0, 17.0, 30.0])
    assert _apply(eng, p, small, forces=_tensor(np.zeros_like(pos), "f64"), check=False) < 0 and "half the shortest" in L.last_error()
    row = torch.zeros(3, 3, dtype=torch.float64, device=_dev())
    bx = _boxes(small, 3)
    assert lib.tmdhip_metad_deposit(eng.ctx, C.c_void_p(p.data_ptr()), bx.ctypes.data_as(C.POINTER(C.c_double)), 1.0, 1.0, 0,
                                    C.c_void_p(row.data_ptr()), _stream(p.device)) < 0 and "half the shortest" in L.last_error()
    torch.cuda.synchronize()
    assert (row == 0).all() and np.array_equal(md.fetch(), grid)
    v = _tensor(np.zeros_like(pos), "f64")
    m0 = mass.copy()
    m0[md.row_atom[3]] = 0.0
    assert _apply(eng, p, box, vel=v, mass=_tensor(m0, "f64"), kick=1.0, check=False) < 0 and "no mass" in L.last_error()
    assert torch.equal(_bits(v), torch.zeros_like(_bits(v))) and same_bits()
    # a CV atom that is a virtual site of the context
    vd = L.VsiteDesc()
    vd.struct_size = C.sizeof(L.VsiteDesc)
    vd.enable, vd.nsites = 1, 1
    free = [a for a in range(pos.shape[1]) if a not in set(md.row_atom.tolist())][:2]
    site, parent, weight = np.array([md.row_atom[3]], np.int32), np.array([[free[0], free[1], -1]], np.int32), np.array([[0.5, 0.5, 0.0]])
    vd.site_host, vd.parent_host, vd.weight_host = (a.ctypes.data_as(C.c_void_p) for a in (site, parent, weight))
    L.check(lib.tmdhip_set_vsites(eng.ctx, C.byref(vd)), "tmdhip_set_vsites")
    refused(lambda d, keep: None, "virtual site")
    vd.enable = 0
    L.check(lib.tmdhip_set_vsites(eng.ctx, C.byref(vd)), "tmdhip_set_vsites")
    assert same_bits()
    # a context with passive atoms
    f2 = Forces(TR._BarePar(mass, PREC["f64"]), terms=[])
    eng2 = f2._engine(torch.zeros(3, len(mass), 3, dtype=torch.float64, device=_dev()))
    types_, charges = np.zeros(len(mass), np.int32), np.zeros(len(mass), np.float64)
    L.check(lib.tmdhip_update_atoms(eng2.ctx, len(mass), types_.ctypes.data_as(C.c_void_p), charges.ctypes.data_as(C.c_void_p), len(mass) - 50),
            "tmdhip_update_atoms")
    d, keep = md.group_descriptor()
    assert lib.tmdhip_set_metadynamics_groups(eng2.ctx, C.byref(d)) < 0 and "passive atoms" in L.last_error()
    # a periodic box without d_max
    _, _, _, open_md = G.kernel_case("zero box")
    f3, eng3 = _context(mass, open_md, "f64", 3)
    assert _apply(eng3, p, box, forces=_tensor(np.zeros_like(pos), "f64"), check=False) < 0 and "needs d_max" in L.last_error()
    # tmdhip_set_metadynamics(enable = 0) releases a group bias; an old-kind bias set afterwards equals a fresh context's
    off = L.MetadDesc()
    off.struct_size, off.enable = C.sizeof(L.MetadDesc), 0
    assert lib.tmdhip_set_metadynamics(eng.ctx, C.byref(off)) == 0
    f4, o4 = _tensor(np.zeros_like(pos), "f64"), torch.full((3, 3), -1.0, dtype=torch.float64, device=_dev())
    _apply(eng, p, box, forces=f4, out=o4)
    assert (f4 == 0).all() and (o4 == 0).all()
    old = Metadynamics(("distance", (3, 700)), sigma=0.4, height=1.0, frequency=1, temperature=300.0, grid_min=1.0, grid_max=26.0,
                       grid_bins=150, nreplicas=3)
    og = np.zeros_like(old.grid)
    for r in range(3):
        og[r] += old.gauss_terms(np.array([old.cv_values(pos[r], box)[0][0] + 0.3]), 20.0)
    d_old = old.descriptor()
    L.check(lib.tmdhip_set_metadynamics(eng.ctx, C.byref(d_old)), "tmdhip_set_metadynamics")
    L.check(lib.tmdhip_metad_set_grid(eng.ctx, og.ctypes.data_as(C.POINTER(C.c_double)), og.size), "tmdhip_metad_set_grid")
    fa, oa = _tensor(np.zeros_like(pos), "f64"), torch.zeros(3, 3, dtype=torch.float64, device=_dev())
    _apply(eng, p, box, forces=fa, out=oa)
    old2 = Metadynamics(("distance", (3, 700)), sigma=0.4, height=1.0, frequency=1, temperature=300.0, grid_min=1.0, grid_max=26.0,
                        grid_bins=150, nreplicas=3)
    old2.set_grid(og)
    f5, eng5 = _context(mass, old2, "f64", 3)
    fb, ob = _tensor(np.zeros_like(pos), "f64"), torch.zeros(3, 3, dtype=torch.float64, device=_dev())
    _apply(eng5, p, box, forces=fb, out=ob)
    assert fa.abs().max().item() > 0.5 and torch.equal(_bits(fa), _bits(fb)) and torch.equal(oa, ob)


def test_python_refusals():
    from torchmd_amd.forces import Forces

    pos, box, mass, md = G.kernel_case("zero box")
    f = Forces(TR._BarePar(mass, torch.float64), terms=[], metadynamics=md)
    with pytest.raises(ValueError, match="needs d_max"):
        md.deposit(_state(pos, np.full(3, 30.0), "f64"))
    with pytest.raises(ValueError, match="beyond the system"):
        Forces(TR._BarePar(mass[:100], torch.float64), terms=[], metadynamics=G.kernel_case("centres")[3])
    m0 = mass.copy()
    m0[md.row_atom[0]] = 0.0
    with pytest.raises(ValueError, match="no mass"):
        Forces(TR._BarePar(m0, torch.float64), terms=[], metadynamics=G.kernel_case("zero box")[3])
    with pytest.raises(ValueError, match="replicas"):
        f.compute(_tensor(pos[:2], "f64"), torch.zeros(2, 3, 3, dtype=torch.float64, device=_dev()), _tensor(np.zeros_like(pos[:2]), "f64"))


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
g = load("water291")
psf, pdb, ff = (os.path.join(TMP, n) for n in ("structure.psf", "structure.pdb", "water_forcefield.yaml"))
D._write_psf(psf, g); D._write_pdb(pdb, g)
open(ff, "w").write(yaml.safe_dump(TIP3P_FF))
oxy = os.path.join(TMP, "oxygens.npy")
np.save(oxy, np.arange(0, 291, 3))
conf = {"structure": [psf, pdb], "forcefield": ff, "forceterms": ["LJ", "Bonds", "Angles", "Electrostatics"], "cutoff": 7.3, "rfa": True,
        "replicas": 2, "precision": "single", "device": "cuda", "timestep": 1, "temperature": 300, "langevin_temperature": 300,
        "langevin_gamma": 1.0, "seed": 1, "steps": 40, "output_period": 20, "save_period": 0, "output": "output",
        "log_dir": os.path.join(TMP, "log_md"),
        "metadynamics": {"cvs": [["group_distance", [[0, 1, 2], [30, 31, 32, 33, 34, 35]]], ["coordination", [[60], oxy], {"r0": 3.5, "n": 6, "d_max": 7.0}]],
                         "sigma": [0.4, 0.2], "height": 1.0, "frequency": 10, "temperature": 300, "bias_factor": 6,
                         "grid_min": [0.5, 0.0], "grid_max": [12.5, 12.0], "grid_bins": [60, 120]}}
open(os.path.join(TMP, "log_md.yaml"), "w").write(yaml.safe_dump(conf))
driver.main(["--conf", os.path.join(TMP, "log_md.yaml")])
log = os.path.join(TMP, "log_md")
out = {"files": sorted(os.listdir(log)), "rows": [open(os.path.join(log, f"monitor_{k}.csv")).read().splitlines() for k in range(2)]}
h = np.load(os.path.join(log, "output_hills.npy"))
z = np.load(os.path.join(log, "output_bias_grid.npz"))
out["hills"] = list(h.shape); out["grid"] = list(z["grid"].shape); out["vmax"] = float(z["grid"][..., 0].max())
out["cv"] = h[-1].tolist()
print("RESULT " + json.dumps(out))
"""


def test_run_py_with_the_new_cv_forms(tmp_path):
    import json
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = f"ROOT = {root!r}\nTMP = {str(tmp_path)!r}\n" + _CHILD
    res = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, cwd=root)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-4000:]
    out = json.loads(next(ln for ln in res.stdout.splitlines() if ln.startswith("RESULT "))[7:])
    files = ["input.yaml"] + [f"monitor_{k}.csv" for k in range(2)] + [f"output_{k}.npy" for k in range(2)]
    assert out["files"] == sorted(files + ["output_hills.npy", "output_bias_grid.npz"])
    for rows in out["rows"]:
        assert rows[0] == "iter,ns,epot,ekin,etot,T,bias,cv0,cv1,t" and len(rows) == 3
        vals = np.array([[float(x) for x in r.split(",")] for r in rows[1:]])
        assert np.isfinite(vals).all() and (vals[:, 6] > 0.0).all() and (vals[:, 7:9] > 0.5).all()
    assert out["hills"] == [4, 2, 3] and out["grid"] == [2, 61, 121, 4] and out["vmax"] > 0.5
    cv = np.asarray(out["cv"])
    assert (cv[:, 0] > 0.5).all() and (cv[:, 1] > 1.0).all() and (cv[:, 1] < 12.0).all()
