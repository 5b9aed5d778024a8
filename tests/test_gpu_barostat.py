"""Constant pressure on the GPU (run with `-m gpu` on an MI355X): the move kernel `tmdhip_scale_groups` against numpy, and
`barostat.MonteCarloBarostat` through `attempt` and `Integrator(..., barostat=...)` against the oracle, the host model of
tests/_barostat.py, the ideal-gas law and the invariants of a rejected move."""

import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import _barostat as B
from _golden import GoldenParameters, PREC, load
from oracle import torchmd_oracle as orc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WATER_TERMS = ["lj", "electrostatics", "bonds", "angles"]
# the suite's bars against the oracle (tests/test_gpu_parity.py: FTOL, ERTOL, EFAC)
FTOL = {"f64": 1e-8, "f32": 3e-4}
ERTOL = {"f64": 1e-10, "f32": 2e-5}
EFAC = 3
# bond length (relative) of constrained dynamics (tests/test_gpu_constraints.py: CONS_TOL)
CONS_TOL = {"f32": 3e-5, "f64": 1e-10}
HIGH_P = 1.0e6  # bar: P dV of a 1 % volume change is hundreds of kcal/mol, which decides a move whatever the energies do
ACCEPT_SHRINK, REJECT_GROW, ACCEPT_STAY = (0.0, 0.0), (1.0 - 1e-12, 0.999999), (0.5, 0.0)  # (u_volume, u_accept) at HIGH_P


def _dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _water291(prec, R=1, seed=0, barostat=None, gamma=1.0):
    from torchmd_amd.forces import Forces
    from torchmd_amd.integrator import Integrator, maxwell_boltzmann
    from torchmd_amd.systems import System

    g = load("water291")
    dt = PREC[prec]
    par = GoldenParameters(g, dt)
    s = System(291, R, dt, _dev())
    s.set_positions(g["pos"][:, :, None])
    s.set_box(g["box"])
    torch.manual_seed(seed)
    s.set_velocities(maxwell_boltzmann(par.masses, 300.0, 1).repeat(R, 1, 1))
    kw = dict(cutoff=7.3, rfa=True)
    f = Forces(par, terms=WATER_TERMS, **kw)
    U = f.compute(s.pos, s.box, s.forces)
    torch.manual_seed(seed + 1)
    integ = Integrator(s, f, 1.0, _dev(), gamma=gamma, T=300.0, barostat=barostat)
    return g, par, kw, s, f, integ, U


def _water_box(nside, prec, seed=0, barostat=None, pme=False, constraints=None, timestep=1.0):
    from torchmd_amd.builders import tip3p_box, water_forcefield
    from torchmd_amd.forces import Forces
    from torchmd_amd.integrator import Integrator, maxwell_boltzmann
    from torchmd_amd.parameters import Parameters
    from torchmd_amd.systems import System

    dt = PREC[prec]
    mol, pos, box = tip3p_box(nside, seed=seed)
    par = Parameters(water_forcefield(mol), mol, WATER_TERMS, precision=dt)
    s = System(mol.numAtoms, 1, dt, _dev())
    s.set_positions(pos[:, :, None])
    s.set_box(box)
    torch.manual_seed(seed)
    s.set_velocities(maxwell_boltzmann(par.masses, 300.0, 1))
    f = Forces(par, terms=WATER_TERMS, **(dict(cutoff=9.0, pme=True) if pme else dict(cutoff=9.0, rfa=True)))
    U = f.compute(s.pos, s.box, s.forces)
    torch.manual_seed(seed + 1)
    integ = Integrator(s, f, timestep, _dev(), gamma=1.0, T=300.0, barostat=barostat, constraints=constraints)
    return mol, par, box, s, f, integ, U


def _barostat(streams, pressure=HIGH_P, frequency=10**9):
    """A barostat whose per-replica random numbers are prescribed: `streams[r]` = the (u_volume, u_accept) pairs of replica r."""
    from torchmd_amd.barostat import MonteCarloBarostat

    bar = MonteCarloBarostat(pressure, 300.0, frequency=frequency, seed=1)
    bar.rng = [B.ListStream([u for pair in st for u in pair]) for st in streams]
    return bar


def _oracle(par, pos, box_edges, kw):
    p = torch.as_tensor(pos)[None]
    edges = np.asarray(box_edges, dtype=np.float64)
    pairs = orc.candidate_pairs(p[0].double().numpy(), edges, kw["cutoff"] + 1.0, orc.exclusion_pairs(par))
    bt = torch.diag(torch.tensor(edges).to(p.dtype))[None]
    pots, F, _ = orc.compute(par, p, bt, WATER_TERMS, pairs=pairs, **kw)
    return pots[0], F[0]


# ----------------------------------------------------------------------------- 1. the kernel against numpy
@pytest.mark.timeout(300)
@pytest.mark.parametrize("prec", ["f64", "f32"])
def test_scale_kernel_against_numpy(prec):
    from torchmd_amd.barostat import scale_groups

    dt = PREC[prec]
    rng = np.random.default_rng(11)
    sizes = [1, 3, 4, 64, 65, 3100] + [int(v) for v in rng.choice([1, 3, 4, 64, 65], size=40)]
    N = sum(sizes)
    perm = rng.permutation(N)  # members of a group are scattered over the atom range, ascending within the group
    off = np.zeros(len(sizes) + 1, dtype=np.int32)
    off[1:] = np.cumsum(sizes)
    mem = np.concatenate([np.sort(perm[off[g]:off[g + 1]]) for g in range(len(sizes))]).astype(np.int32)
    centres = rng.uniform(0, 50.0, size=(len(sizes), 3))
    x = np.empty((2, N, 3))
    for r in range(2):
        for g in range(len(sizes)):
            x[r, mem[off[g]:off[g + 1]]] = centres[g] + rng.normal(scale=2.0 + r, size=(sizes[g], 3))
    pos0 = torch.as_tensor(x).to(dt).to(_dev()).contiguous()
    scale = np.array([[1.0, 1.0, 1.0], [1.0031, 0.9987, 1.0102]])
    o_d, m_d = torch.as_tensor(off, device=_dev()), torch.as_tensor(mem, device=_dev())

    def run():
        p, saved = pos0.clone(), torch.full_like(pos0, float("nan"))
        scale_groups(p, scale, o_d, m_d, True, saved=saved)
        return p, saved

    p, saved = run()
    p2, saved2 = run()
    assert torch.equal(p, p2) and torch.equal(saved, saved2)  # no atomics, fixed order: same bits
    assert torch.equal(saved, pos0)
    assert torch.equal(p[0], pos0[0])  # scale exactly 1: not touched
    x0 = pos0.cpu().double().numpy()  # the stored (rounded) input
    ref = x0.copy()
    for r in range(2):
        for g in range(len(sizes)):
            a = mem[off[g]:off[g + 1]]
            ref[r, a] += (scale[r] - 1.0) * x0[r, a].mean(axis=0)
    got = p.cpu().double().numpy()
    big = max(np.abs(ref).max(), np.abs(x0).max())
    # storage rounding of a coordinate of magnitude `big`: fp32 one ulp; fp64 a few ulp (the kernel sums 3 100 members lane by
    # lane, numpy pairwise: the means differ by a few ulp of the coordinate magnitude before the result is rounded)
    bar = np.finfo(np.float32).eps * big if prec == "f32" else 8 * np.finfo(np.float64).eps * big
    err = np.abs(got - ref).max()
    # intra-group distances: every atom of a group gets the same shift, rounded once per atom
    worst = 0.0
    for g in range(len(sizes)):
        a = mem[off[g]:off[g + 1]][:200]
        if len(a) > 1:
            d0 = np.linalg.norm(x0[1, a][:, None] - x0[1, a][None], axis=-1)
            d1 = np.linalg.norm(got[1, a][:, None] - got[1, a][None], axis=-1)
            worst = max(worst, np.abs(d1 - d0).max())
    print(f"scale kernel {prec}: max|x - numpy| = {err:.3e} (bar {bar:.3e}), intra-group distances change by {worst:.3e}")
    assert err <= bar, (err, bar)
    assert worst <= bar, (worst, bar)
    assert not np.array_equal(got[1], x0[1])
    # without a saved copy
    p3 = pos0.clone()
    scale_groups(p3, scale, o_d, m_d, True)
    assert torch.equal(p3, p)


# ----------------------------------------------------------------------------- 2. a rejected move restores everything
@pytest.mark.timeout(600)
@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("system", ["water291", "box16"])
def test_rejected_move_restores_everything_and_the_run_goes_on(system, prec):
    """After a rejected move pos, box, forces and vel are what they were, bit for bit, and the run continues as a twin run
    does that lost its Verlet list at the same step (`invalidate_lists`): a rejected move costs the state its list, and a
    list rebuilt at another step orders the fp sums differently.  Bit for bit on the cell-list path in both precisions; the
    all-pairs context (water291) is not reproducible to the bit from run to run, see the comment at its bar."""
    def make(barostat):
        if system == "water291":
            _, _, _, s, f, integ, _ = _water291(prec, seed=3, barostat=barostat)
        else:
            _, _, _, s, f, integ, _ = _water_box(16, prec, seed=3, barostat=barostat)
        return s, f, integ

    bar = _barostat([[REJECT_GROW]])
    s, f, integ = make(bar)
    _, pot, _ = integ.step(25)
    before = [t.clone() for t in (s.pos, s.box, s.forces, s.vel)]
    rec = bar.attempt(s, f, pot)
    assert not rec["accepted"][0] and rec["V_new"][0] > rec["V"][0] and rec["w"][0] > 100.0, rec
    assert bar.attempts[0] == 1 and bar.accepted[0] == 0
    for name, a, b in zip(("pos", "box", "forces", "vel"), before, (s.pos, s.box, s.forces, s.vel)):
        assert torch.equal(a, b), name
    out_a = integ.step(50)

    s2, f2, integ2 = make(None)
    integ2.step(25)
    same = all(torch.equal(a, b) for a, b in zip(before, (s2.pos, s2.box, s2.forces, s2.vel)))
    # the twin starts the 50 steps from the very same state (a no-op where two runs of 25 steps give the same bits)
    for a, b in zip(before, (s2.pos, s2.box, s2.forces, s2.vel)):
        b.copy_(a)
    f2.invalidate_lists(s2.pos)
    out_b = integ2.step(50)
    dx = (s.pos - s2.pos).abs().max().item()
    print(f"{system} {prec}: twin identical after its own 25 steps: {same}; 50 steps after a rejected move against the twin that dropped its list: max|dx| = {dx:.3e}, "
          f"algorithm {f.stats(s.pos)['algorithm']}, Epot {out_a[1][0]:.6f} / {out_b[1][0]:.6f}")
    assert f.stats(s.pos)["algorithm"] == ("allpairs" if system == "water291" else "celllist")
    assert torch.equal(s.box, s2.box)
    if system == "box16":
        assert same
        assert torch.equal(s.pos, s2.pos) and torch.equal(s.vel, s2.vel) and torch.equal(s.forces, s2.forces)
    else:
        # The all-pairs kernel combines partial forces with floating-point atomics (tests/test_gpu_integrator.py,
        # test_gpu_constraints.py): two runs of the SAME 25 steps already differ in their last bits (`same` is False here,
        # with or without a barostat), so no twin can be bit-identical.  What the trial box leaves behind is nothing: there
        # is no list in this context.  Bars of a re-run instead: fp64 the suite's 1e-9 A.  fp32 has no bar in the suite, so
        # from the formats: the forces of two runs agree within the suite's fp32 force bar dF = 3e-4 kcal/mol/A (FTOL); a
        # force error held for n steps moves the lightest atom (m_H = 1.008) by at most n^2/2 * dF * dt^2 / m_H, and every
        # step rounds the stored coordinate (|x| <= 17 A) once: 50^2/2 * 3e-4 * (1/48.88821)^2 / 1.008 + 50 * 2^-23 * 17
        #   = 1.56e-4 + 1.0e-4 = 2.6e-4 A.  (Observed: 1.1e-14 A in fp64, 5.7e-6 A in fp32.)
        n, dt = 50, 1.0 / 48.88821
        bar_x = 1e-9 if prec == "f64" else n * n / 2 * FTOL["f32"] * dt * dt / 1.008 + n * np.finfo(np.float32).eps * 17.0
        assert dx <= bar_x, (dx, bar_x)


# ----------------------------------------------------------------------------- 3. an accepted move against the oracle
@pytest.mark.timeout(600)
@pytest.mark.parametrize("prec", ["f64", "f32"])
def test_accepted_move_against_the_oracle(prec):
    from torchmd_amd.barostat import BAR_TO_KCAL_MOL_A3
    from torchmd_amd.integrator import BOLTZMAN

    bar = _barostat([[ACCEPT_SHRINK]])
    g, par, kw, s, f, integ, U = _water291(prec, barostat=bar)
    pos0, box0, vel0 = s.pos.clone(), s.box.clone(), s.vel.clone()
    rec = bar.attempt(s, f, U)
    assert rec["accepted"][0] and bar.accepted[0] == 1 and rec["V_new"][0] < rec["V"][0]
    assert bar.ngroups == 97 and torch.equal(s.vel, vel0)
    e0 = np.diagonal(box0[0].cpu().double().numpy())
    e1 = np.diagonal(s.box[0].cpu().double().numpy())

    def bound(pots):
        return sum(ERTOL[prec] * EFAC * max(1.0, abs(pots[t])) for t in WATER_TERMS)

    old, _ = _oracle(par, pos0[0].cpu(), e0, kw)
    new, Fnew = _oracle(par, s.pos[0].cpu(), e1, kw)
    Uo, Un = sum(old[t] for t in WATER_TERMS), sum(new[t] for t in WATER_TERMS)
    ferr = (s.forces[0].cpu() - Fnew).abs().max().item()
    print(f"water291 {prec}: U {rec['U'][0]:.6f} (oracle {Uo:.6f}), U' {rec['U_new'][0]:.6f} (oracle {Un:.6f}), max|dF| at the new state {ferr:.3e}")
    assert abs(rec["U"][0] - Uo) <= bound(old), (rec["U"][0], Uo)
    assert abs(rec["U_new"][0] - Un) <= bound(new), (rec["U_new"][0], Un)
    assert ferr <= FTOL[prec], ferr
    # the box is s * the old box, s = (V'/V)^(1/3), to the rounding of the box tensor
    sfac = (rec["V_new"][0] / rec["V"][0]) ** (1.0 / 3.0)
    assert abs(rec["V"][0] - e0.prod()) <= 1e-12 * e0.prod() and abs(rec["V_new"][0] - e1.prod()) <= 1e-12 * e1.prod()
    assert np.abs(e1 - sfac * e0).max() <= 4 * np.finfo(np.float32 if prec == "f32" else np.float64).eps * e0.max()
    assert abs(rec["V_new"][0] - (rec["V"][0] - 0.01 * rec["V"][0])) <= (1e-6 if prec == "f32" else 1e-12) * rec["V"][0]
    off = s.box[0].clone()
    off.diagonal().zero_()
    assert not off.any()
    # w from the record
    kT = BOLTZMAN * 300.0
    w = (rec["U_new"][0] - rec["U"][0]) + HIGH_P * BAR_TO_KCAL_MOL_A3 * (rec["V_new"][0] - rec["V"][0]) - 97 * kT * np.log(rec["V_new"][0] / rec["V"][0])
    assert abs(w - rec["w"][0]) <= 1e-12 * abs(w) and w < 0
    # the molecules moved rigidly, their centres by (s - 1) * centre
    x0, x1 = pos0[0].cpu().double().numpy().reshape(97, 3, 3), s.pos[0].cpu().double().numpy().reshape(97, 3, 3)
    ulp = np.finfo(np.float32 if prec == "f32" else np.float64).eps * np.abs(x0).max()
    assert np.abs((x1 - x0) - (e1 / e0 - 1.0) * x0.mean(axis=1, keepdims=True)).max() <= 4 * ulp
    # and through the integrator: step() returns U' and the run goes on from the scaled state
    bar2 = _barostat([[ACCEPT_SHRINK]], frequency=10)
    _, _, _, s2, f2, integ2, _ = _water291(prec, barostat=bar2)
    V0 = float(np.prod(np.diagonal(s2.box[0].cpu().double().numpy())))
    _, pot, _ = integ2.step(10)
    assert bar2.attempts[0] == 1 and bar2.last["accepted"][0] and pot[0] == bar2.last["U_new"][0]
    assert abs(float(np.prod(np.diagonal(s2.box[0].cpu().double().numpy()))) - 0.99 * V0) < 1e-5 * V0
    fresh = torch.zeros_like(s2.forces)
    f2.compute(s2.pos, s2.box, fresh)
    assert (fresh - s2.forces).abs().max().item() <= FTOL[prec]
    _, pot, _ = integ2.step(5)
    assert np.isfinite(pot).all() and bar2.attempts[0] == 1


# ----------------------------------------------------------------------------- 4. the ideal gas
@pytest.mark.timeout(900)
def test_ideal_gas_obeys_pv_equals_n_plus_one_kt():
    """N = 64 non-interacting atoms (LJ epsilon = 0, no charges: U = 0), 300 K, P such that (N + 1) k_B T / P = 27 000 A^3,
    8 000 attempts from 20 000 A^3 (no MD in between: positions do not enter), first fifth discarded.  The volume density is
    Gamma(N + 1, k_B T / P): <V> = 27 000 within 5 standard errors (from 20 block averages; the host model stayed within 3.8
    over 40 seeds), sigma_V / <V> within 15 % of 1 / sqrt(65); and the chain equals the host model driven by the same random
    numbers, volume for volume, to 1e-9 relative."""
    from torchmd_amd.barostat import MonteCarloBarostat
    from torchmd_amd.builders import Topology
    from torchmd_amd.forcefields.ff_yaml import YamlForceField
    from torchmd_amd.forces import Forces
    from torchmd_amd.parameters import Parameters
    from torchmd_amd.systems import System

    N, T, target, nattempts, seed = 64, 300.0, 27000.0, 8000, 17
    P = (N + 1) * B.BOLTZMAN * T / target / B.BAR
    edge = 20000.0 ** (1.0 / 3.0)
    ff = {"atomtypes": ["X"], "lj": {"X": {"sigma": 3.0, "epsilon": 0.0}}, "electrostatics": {"X": {"charge": 0.0}}, "masses": {"X": 10.0}}
    mol = Topology(atomtype=np.full(N, "X", dtype=object), charge=np.zeros(N, dtype=np.float32), masses=np.full(N, 10.0, dtype=np.float32))
    par = Parameters(YamlForceField(mol, ff), mol, ["lj"], precision=torch.float64)
    s = System(N, 1, torch.float64, _dev())
    g = (np.arange(4) + 0.5) * edge / 4
    s.set_positions(np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3)[:, :, None])
    s.set_box(np.array([edge] * 3))
    f = Forces(par, terms=["lj"], cutoff=9.0)
    U = f.compute(s.pos, s.box, s.forces)
    assert U[0] == 0.0
    bar = MonteCarloBarostat(P, T, seed=seed)
    vols, flags = np.empty(nattempts), np.zeros(nattempts, dtype=bool)
    for i in range(nattempts):
        rec = bar.attempt(s, f, U)
        assert rec["U_new"][0] == 0.0
        flags[i] = rec["accepted"][0]
        vols[i] = rec["V_new"][0] if flags[i] else rec["V"][0]
    assert bar.ngroups == N and bar.attempts[0] == nattempts and bar.accepted[0] == flags.sum()
    assert abs(float(np.prod(np.diagonal(s.box[0].cpu().numpy()))) - vols[-1]) <= 1e-12 * vols[-1]
    model, mflags = B.volume_chain([edge] * 3, N, P, T, nattempts, B.philox_stream(seed, 0))
    rel = np.abs(vols / model - 1.0).max()
    mean, se, width = B.block_stats(vols)
    print(f"ideal gas, {nattempts} attempts: <V> = {mean:.1f} A^3 ({(mean - target) / se:+.2f} block standard errors of {se:.1f}), "
          f"sigma/<V> = {width:.4f} (1/sqrt(65) = {1 / np.sqrt(N + 1):.4f}), acceptance {flags.mean():.2f}, max rel. deviation from the host model {rel:.2e}")
    assert np.array_equal(flags, mflags) and rel <= 1e-9, rel
    assert abs(mean - target) <= 5.0 * se, (mean, se)
    assert abs(width * np.sqrt(N + 1) - 1.0) <= 0.15, width
    # the atoms followed the box: still the same lattice in box fractions
    frac = s.pos[0].cpu().numpy() / np.diagonal(s.box[0].cpu().numpy())
    assert np.abs(frac - (np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3) / edge)).max() < 1e-9


# ----------------------------------------------------------------------------- 5. replicas are independent
@pytest.mark.timeout(600)
@pytest.mark.parametrize("prec", ["f64", "f32"])
def test_replicas_are_independent(prec):
    streams = [[ACCEPT_SHRINK], [REJECT_GROW], [ACCEPT_STAY]]
    bar = _barostat(streams)
    g, par, kw, s, f, integ, U = _water291(prec, R=3, barostat=bar)
    pos0, box0, F0 = s.pos.clone(), s.box.clone(), s.forces.clone()
    rec = bar.attempt(s, f, U)
    assert list(rec["accepted"]) == [True, False, True], rec
    assert list(bar.attempts) == [1, 1, 1] and list(bar.accepted) == [1, 0, 1]
    assert torch.equal(s.pos[1], pos0[1]) and torch.equal(s.box[1], box0[1]) and torch.equal(s.forces[1], F0[1])
    assert torch.equal(s.pos[2], pos0[2]) and torch.equal(s.box[2], box0[2])  # dV = 0: scale exactly 1
    assert not torch.equal(s.pos[0], pos0[0])
    for r in range(3):
        alone = _barostat([streams[r]])
        _, _, _, s1, f1, _, U1 = _water291(prec, R=1, barostat=alone)
        rec1 = alone.attempt(s1, f1, U1)
        assert rec1["accepted"][0] == rec["accepted"][r]
        assert torch.equal(s1.pos[0], s.pos[r]) and torch.equal(s1.box[0], s.box[r]), r
        assert rec1["V"][0] == rec["V"][r] and rec1["V_new"][0] == rec["V_new"][r]
        # (a three-replica context may sum in another order than a one-replica one: the suite's energy bar, not bits)
        for key in ("U", "U_new"):
            assert abs(rec1[key][0] - rec[key][r]) <= ERTOL[prec] * EFAC * max(1.0, abs(rec1[key][0])), (r, key)
        assert (s1.forces[0] - s.forces[r]).abs().max().item() <= FTOL[prec]


# ----------------------------------------------------------------------------- 6. constraints and PME
@pytest.mark.timeout(900)
@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_composes_with_constraints_and_pme(prec):
    """12 288-atom water box, rigid water, PME, Langevin 300 K, 1 bar, a move every 25 steps, 500 steps at 2 fs."""
    import _constraints as H
    from torchmd_amd.barostat import MonteCarloBarostat
    from torchmd_amd.constraints import find_constraints

    bar = MonteCarloBarostat(1.0, 300.0, frequency=25, seed=5)
    mol, par, box, s, f, integ, _ = _water_box(16, prec, seed=2, barostat=bar, pme=True, constraints="water", timestep=2.0)
    for _ in range(5):
        ek, pot, T = integ.step(100)
        assert np.isfinite(ek).all() and np.isfinite(pot).all()
    assert bar.attempts[0] == 20
    cs = find_constraints(par.masses, par.bond_params, par.angle_params, "water")
    pairs, d = cs.pairs()
    dr, _ = H.residuals(s.pos[0].cpu().double().numpy(), s.vel[0].cpu().double().numpy(), pairs, d)
    e = np.diagonal(s.box[0].cpu().double().numpy())
    rho = mol.numAtoms / 3 * 18.0154 / 6.02214076e23 / (e.prod() * 1e-24)
    print(f"tip3p_box(16) {prec}, rigid, PME, 1 bar, 500 steps at 2 fs: {bar.accepted[0]} of {bar.attempts[0]} moves accepted, "
          f"box {box[0]:.3f} -> {e[0]:.3f} A, density {rho:.4f} g/cm^3, worst bond error {dr:.2e}, T = {T[0]:.1f} K")
    assert 1 <= bar.accepted[0] <= 19, (bar.accepted, bar.attempts)  # at least one move accepted and one rejected
    assert dr <= CONS_TOL[prec], dr
    assert e[0] == e[1] == e[2] and e[0] != box[0]  # still cubic, and it moved
    assert f.stats(s.pos)["pme_evaluations"] > 0


# ----------------------------------------------------------------------------- 7. off means off
_CHILD = r"""
import json, os, sys
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
import numpy as np, torch, yaml
import test_gpu_driver as D
from _golden import load

def run(barostat):
    from torchmd_amd.builders import tip3p_box, water_forcefield
    from torchmd_amd.forces import Forces
    from torchmd_amd.integrator import Integrator, maxwell_boltzmann
    from torchmd_amd.parameters import Parameters
    from torchmd_amd.systems import System
    dev = torch.device("cuda:0")
    terms = ["lj", "electrostatics", "bonds", "angles"]
    mol, pos, box = tip3p_box(12, seed=1)
    par = Parameters(water_forcefield(mol), mol, terms, precision=torch.float32)
    s = System(mol.numAtoms, 1, torch.float32, dev)
    s.set_positions(pos[:, :, None]); s.set_box(box)
    torch.manual_seed(1)
    s.set_velocities(maxwell_boltzmann(par.masses, 300.0, 1))
    f = Forces(par, terms=terms, cutoff=9.0, rfa=True)
    f.compute(s.pos, s.box, s.forces)
    torch.manual_seed(2)
    kw = {} if barostat is None else {"barostat": barostat}
    Integrator(s, f, 1.0, dev, gamma=1.0, T=300.0, **kw).step(100)
    st = f.stats(s.pos)
    return {"n_rebuilds": st["n_rebuilds"], "n_compute": st["n_compute"], "algorithm": st["algorithm"], "pos": float(s.pos.double().sum())}

out = {"off": run(None), "module_after_off": "torchmd_amd.barostat" in sys.modules}
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
open(os.path.join(TMP, "conf.yaml"), "w").write(yaml.safe_dump(conf))
driver.main(["--conf", os.path.join(TMP, "conf.yaml")])
out["module_after_run_py"] = "torchmd_amd.barostat" in sys.modules
out["files"] = sorted(os.listdir(os.path.join(TMP, "log")))
out["header"] = open(os.path.join(TMP, "log", "monitor_0.csv")).readline().strip()
from torchmd_amd.barostat import MonteCarloBarostat
out["never"] = run(MonteCarloBarostat(1.0, 300.0, frequency=10**6, seed=1))
conf.update(barostat_pressure=1.0, barostat_frequency=25, log_dir=os.path.join(TMP, "log_npt"))
open(os.path.join(TMP, "conf_npt.yaml"), "w").write(yaml.safe_dump(conf))
driver.main(["--conf", os.path.join(TMP, "conf_npt.yaml")])
out["files_npt"] = sorted(os.listdir(os.path.join(TMP, "log_npt")))
out["header_npt"] = open(os.path.join(TMP, "log_npt", "monitor_0.csv")).readline().strip()
out["box_shape"] = list(np.load(os.path.join(TMP, "log_npt", "output_box_0.npy")).shape)
print("RESULT " + json.dumps(out))
"""


@pytest.mark.timeout(900)
def test_off_means_off(tmp_path):
    code = f"ROOT = {ROOT!r}\nTMP = {str(tmp_path)!r}\n" + _CHILD
    res = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=800, cwd=ROOT)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-4000:]
    out = json.loads(next(ln for ln in res.stdout.splitlines() if ln.startswith("RESULT "))[7:])
    print(out)
    assert out["module_after_off"] is False and out["module_after_run_py"] is False
    assert out["files"] == ["input.yaml", "monitor_0.csv", "output_0.npy"], out["files"]
    assert out["header"] == "iter,ns,epot,ekin,etot,T,t"
    # a barostat that never attempts leaves the run what it was: same launches, same rebuilds, same trajectory
    assert out["off"]["algorithm"] == "celllist"
    assert out["never"] == out["off"], (out["never"], out["off"])
    # and with the two keys on: the box file and the volume column
    assert out["files_npt"] == ["input.yaml", "monitor_0.csv", "output_0.npy", "output_box_0.npy"], out["files_npt"]
    assert out["header_npt"] == "iter,ns,epot,ekin,etot,T,volume,t" and out["box_shape"] == [2, 3]
