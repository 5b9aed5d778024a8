"""Hamiltonian replica exchange on the device: tmdhip_restraint_states against the numpy model with the rows of
the tables permuted, and `HamiltonianExchange` inside `Integrator.step` against a twin that makes the same library calls by hand.

Bars.  Cross energies against the model: the bar tests/test_gpu_restraints.py holds the evaluation's energies to, M eps64 |E| per
entry for sums of M non-negative terms taken in another order; the diagonal against tmdhip_restraint_apply, a second call, and
every trajectory against its twin: bit for bit.  Returned energies against a second evaluation: tests/test_gpu_parity.py's
relative bars.  NVE: §22's bar, twice the spread of the run without exchange."""

import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import _hrex as H
from _exchange import Counting
from _golden import PREC

pytestmark = pytest.mark.gpu

NP = {"f32": np.float32, "f64": np.float64}
EPS64 = np.finfo(np.float64).eps
WATER_TERMS = ["lj", "electrostatics", "bonds", "angles"]
FTOL = {"f64": 1e-8, "f32": 3e-4}  # tests/test_gpu_parity.py: forces, energies (relative, x EFAC)
ERTOL = {"f64": 1e-10, "f32": 2e-5}
EFAC = 3
LAMBDAS = np.array([[1.0, 1.0], [1.0, 0.5], [1.0, 0.0], [0.5, 0.0]])  # four states of the schedule (lambda_vdw, lambda_elec)
SOLUTE = [300, 301, 302]  # one water (the 192-atom box: atoms 30 .. 32)
BETA300 = 1.0 / (H.BOLTZMAN * 300.0)


def _dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int32 if a.dtype == np.float32 else np.int64)


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def _stream(dev):
    return C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


# ----------------------------------------------------------------------------- the kernel
def _context(mass, rs, prec, R):
    from torchmd_amd.forces import Forces

    f = Forces(H.BarePar(mass, PREC[prec]), terms=[], restraints=rs)
    eng = f._engine(torch.zeros(R, len(mass), 3, dtype=PREC[prec], device=_dev()))
    eng.sync_restraints(rs)
    return f, eng


def _states(eng, p, boxes, R):
    from torchmd_amd import _lib as L

    out = np.full((R, R, 2), -7.0)
    L.check(eng.lib.tmdhip_restraint_states(eng.ctx, C.c_void_p(p.data_ptr()), _dp(boxes), _dp(out), _stream(p.device)),
            "tmdhip_restraint_states")
    return out


def _run_energy(eng, R):
    from torchmd_amd import _lib as L

    out = np.full((R, 2), -7.0)
    L.check(eng.lib.tmdhip_restraint_energy(eng.ctx, _dp(out), _stream(_dev())), "tmdhip_restraint_energy")
    return out


@pytest.mark.parametrize("prec", ["f32", "f64"])
@pytest.mark.parametrize("nrows", [1, 255, 256, 257, 600])
@pytest.mark.parametrize("R", [1, 2, 16, 17, 33])
def test_restraint_states_against_the_model_with_rows_permuted(R, nrows, prec):
    from torchmd_amd import _lib as L

    pos, boxes, mass, rs = H.states_case(R, nrows)
    pos = pos.astype(NP[prec]).astype(np.float64)  # the model sees the positions the device holds
    f, eng = _context(mass, rs, prec, R)
    p = torch.as_tensor(pos, dtype=PREC[prec]).to(_dev()).contiguous()
    boxes = np.ascontiguousarray(boxes)
    before = _run_energy(eng, R)
    got = _states(eng, p, boxes, R)
    want = H.cross_model(rs, pos, boxes)
    nterm = rs.npos + rs.ndist
    err = np.abs(got - want)
    rel = (err / np.where(want != 0, np.abs(want), 1.0)).max()
    print(f"{prec} R={R} rows={nrows}: max |E - model| / |E| = {rel:.2e} (bar {nterm * EPS64:.2e}), largest entry {np.abs(want).max():.3e}")
    assert (err <= nterm * EPS64 * np.abs(want)).all(), np.argwhere(err > nterm * EPS64 * np.abs(want))[:5]
    assert (want.sum(axis=2) > 0.0).mean() > 0.5  # (k = 0 may switch off all of a row of one entry, not most rows)
    if R > 1:
        assert np.abs(want[:, 0] - want[:, 1]).max() > 0.0  # (the rows differ: a kernel that took the replica's own row would show)
    # the diagonal has the bits of the evaluation's energies
    e = torch.full((R, 2), -1.0, dtype=torch.float64, device=_dev())
    L.check(eng.lib.tmdhip_restraint_apply(eng.ctx, C.c_void_p(p.data_ptr()), _dp(boxes), C.c_void_p(), C.c_void_p(), C.c_void_p(), 0.0,
                                           C.c_void_p(e.data_ptr()), _stream(p.device)), "tmdhip_restraint_apply")
    assert np.array_equal(_bits(got[np.arange(R), np.arange(R)]), _bits(e.cpu().numpy()))
    # two calls: the same bits; and the row tmdhip_restraint_energy reads is as it was
    assert np.array_equal(_bits(_states(eng, p, boxes, R)), _bits(got))
    assert np.array_equal(_bits(_run_energy(eng, R)), _bits(before))


def test_restraint_states_without_restraints_and_refusals():
    from torchmd_amd import _lib as L
    from torchmd_amd.restraints import Restraints

    R = 3
    pos, boxes, mass, rs = H.states_case(R, 20)
    f, eng = _context(mass, Restraints(R), "f64", R)
    p = torch.as_tensor(pos).to(_dev()).contiguous()
    assert (_states(eng, p, boxes, R) == 0.0).all()  # no tables in place: zeros, nothing launched
    out = np.full((R, R, 2), -7.0)
    st = _stream(p.device)
    for args in ((None, C.c_void_p(p.data_ptr()), _dp(boxes), _dp(out)), (eng.ctx, C.c_void_p(), _dp(boxes), _dp(out)),
                 (eng.ctx, C.c_void_p(p.data_ptr()), None, _dp(out)), (eng.ctx, C.c_void_p(p.data_ptr()), _dp(boxes), None)):
        assert eng.lib.tmdhip_restraint_states(*args, st) < 0 and "null argument" in L.last_error()
    assert (out == -7.0).all()
    # tables handed over, taken away again: zeros again (the workspace went with the state)
    eng.sync_restraints(rs)
    assert np.abs(_states(eng, p, boxes, R)).min() > 0.0
    eng.sync_restraints(Restraints(R))
    assert (_states(eng, p, boxes, R) == 0.0).all()
    with pytest.raises(ValueError, match="needs restraints"):
        from torchmd_amd.forces import Forces

        Forces(H.BarePar(mass, torch.float64), terms=[]).restraint_energies(p, torch.zeros(R, 3, 3, device=_dev()))


# ----------------------------------------------------------------------------- TIP3P with one water as the solute
_WATER = {}


def _water(prec, nside):
    from torchmd_amd.builders import tip3p_box, water_forcefield
    from torchmd_amd.parameters import Parameters

    if (prec, nside) not in _WATER:
        mol, pos, box = tip3p_box(nside, seed=21)
        par = Parameters(water_forcefield(mol), mol, WATER_TERMS, precision=PREC[prec])
        _WATER[prec, nside] = (mol, np.asarray(pos, dtype=np.float64), np.asarray(box, dtype=np.float64), par)
    return _WATER[prec, nside]


def _vel0(mol, R, T):
    from torchmd_amd.builders import water_forcefield
    from torchmd_amd.integrator import maxwell_boltzmann
    from torchmd_amd.parameters import Parameters

    torch.manual_seed(5)
    return maxwell_boltzmann(Parameters(water_forcefield(mol), mol, WATER_TERMS, precision=torch.float64).masses, T, R)


def _solute(pos):
    return SOLUTE if len(pos) > SOLUTE[-1] else [30, 31, 32]


def _pair_of_oxygens(pos, box):
    """Two oxygens outside the solute, 4 to 6 A apart (inside half the smallest box)."""
    L = np.asarray(box).reshape(-1)[:3]
    ox = np.arange(0, len(pos), 3)
    d = pos[ox] - pos[0]
    r = np.linalg.norm(d - L * np.rint(d / L), axis=1)
    j = next(int(ox[k]) for k in np.argsort(r) if 4.0 < r[k] < 6.0 and ox[k] not in _solute(pos))
    return (0, j), float(r[ox == j][0])


def _terms(pos, box, R, k=40.0):
    """`Alchemical` with the first R states of LAMBDAS and one distance restraint with R targets 0.3 A apart."""
    from torchmd_amd.alchemy import Alchemical
    from torchmd_amd.restraints import Restraints

    pair, r = _pair_of_oxygens(pos, box)
    al = Alchemical(_solute(pos), LAMBDAS[:R, 0], LAMBDAS[:R, 1])
    rs = Restraints(R).add_distance([pair], np.array([[r - 0.3 + 0.3 * q] for q in range(R)]), k)
    return al, rs


CASES = {
    # fp64, all pairs: the 648-atom box; fp32, the fused pair + step launch on the cell list: §19's 2 187-atom box, cutoff 7
    "f64-allpairs": dict(prec="f64", nside=6, kw=dict(cutoff=9.0, rfa=True, switch_dist=7.5, algorithm="allpairs")),
    "f32-fused-list": dict(prec="f32", nside=9, kw=dict(cutoff=7.0, rfa=True)),
    # fp64, all pairs, where two runs give the same bits: 192 atoms (L = 12.4 A), run with TMDHIP_ALLPAIRS_WAVES=1
    "f64-allpairs-1split": dict(prec="f64", nside=4, kw=dict(cutoff=6.0, rfa=True, switch_dist=5.0, algorithm="allpairs")),
}


def _build(case, R, exchange=None, T0=300.0, dt=1.0, langevin=True, terms=True, **integ_kw):
    from torchmd_amd.forces import Forces
    from torchmd_amd.integrator import Integrator
    from torchmd_amd.systems import System

    c = CASES[case] if isinstance(case, str) else case
    mol, pos, box, par = _water(c["prec"], c["nside"])
    al, rs = _terms(pos, box, R) if terms else (None, None)
    s = System(mol.numAtoms, R, PREC[c["prec"]], _dev())
    s.set_positions(np.repeat(pos[:, :, None], R, axis=2))
    s.set_box(box)
    s.set_velocities(_vel0(mol, R, T0).to(PREC[c["prec"]]))
    f = Forces(par, terms=WATER_TERMS, **c["kw"], **(dict(alchemical=al, restraints=rs) if terms else {}))
    f.compute(s.pos, s.box, s.forces)
    torch.manual_seed(77)  # (the integrator draws the seed of its noise stream)
    integ = Integrator(s, f, dt, _dev(), **(dict(gamma=1.0, T=300.0) if langevin else {}), exchange=exchange, **integ_kw)
    return s, f, integ, al, rs


def _state(s):
    return [getattr(s, k).cpu().numpy().copy() for k in ("pos", "vel", "forces")]


def _same_bits(a, b):
    """Positions, velocities and forces of two runs, bit for bit (what differs is printed)."""
    same = True
    for name, x, y in zip(("pos", "vel", "forces"), a, b):
        if not np.array_equal(_bits(x), _bits(y)):
            d = np.abs(x.astype(np.float64) - y.astype(np.float64))
            print(f"{name} differ: max {d.max():.3e} at {np.unravel_index(np.argmax(d), d.shape)}, {np.count_nonzero(d)} of {d.size} entries")
            same = False
    return same


def _pin_lanes(case, monkeypatch):
    if case == "f32-fused-list":
        # the engine's energies meet in 256 slots per replica by atomic additions: at 4 lanes per atom (137 pair waves) a slot
        # receives one addend of a kind and the sums do not depend on the order of arrival
        monkeypatch.setenv("TMDHIP_LPA", "4")
        monkeypatch.setenv("TMDHIP_VSKIN", "0")


def _check_path(case, f, s):
    st = f.stats(s.pos)
    if case == "f32-fused-list":
        assert st["algorithm"] == "celllist" and st["steps_in_pair_launch"] > 0, st
    else:
        assert st["algorithm"] == "allpairs", st




def _reference_forces(case, R):
    """A second `Forces`, a context of its own, whose tables stay in state order: row a is state a."""
    from torchmd_amd.forces import Forces

    c = CASES[case] if isinstance(case, str) else case
    mol, pos, box, par = _water(c["prec"], c["nside"])
    al, rs = _terms(pos, box, R)
    return Forces(par, terms=WATER_TERMS, alchemical=al, restraints=rs, **c["kw"])


def _forced(frequency, **kw):
    from torchmd_amd.hrex import HamiltonianExchange

    hx = HamiltonianExchange(frequency=frequency, seed=3, **kw)
    hx.rng = Counting(0.0)  # u = 0 < exp(Delta): every tried pair is accepted
    return hx


def _cut_run(case, R, cuts, **kw):
    """The run without exchange=, cut like the run under test: (state, the last call's result)."""
    s, f, integ, al, rs = _build(case, R, None, **kw)
    out = None
    for n in cuts:
        out = integ.step(n)
    return _state(s), out


# ----------------------------------------------------------------------------- the control's matrix
@pytest.mark.parametrize("case", ["f64-allpairs", "f32-fused-list"])
def test_the_controls_matrix_is_the_sum_made_by_hand(case, monkeypatch):
    """Four states (1,1), (1,0.5), (1,0), (0.5,0) of one water and four targets of one distance restraint, three forced attempts:
    every matrix the control decided on equals, bit for bit, alchemical_energies + the restraint states of a second context
    whose tables are in state order — also after the slots have moved, when the device rows of the run are no longer."""
    _pin_lanes(case, monkeypatch)
    R, rows = 4, np.arange(4)
    hx = _forced(10, keep_matrices=True)
    s, f, integ, al, rs = _build(case, R, hx)
    assert hx.terms == [rs, al] and hx.beta == BETA300  # (Langevin's T)
    eng = f._engine(s.pos)
    seen, inner = [], hx.cross_matrix

    def cross(system, forces):
        e0 = _run_energy(eng, R)
        m = inner(system, forces)
        seen.append(dict(pos=system.pos.detach().clone(), held=hx.states.copy(), M=m, e0=e0, e1=_run_energy(eng, R)))
        return m

    hx.cross_matrix = cross
    integ.step(30)
    _check_path(case, f, s)
    assert [h.tolist() for h in hx.history] == [[1, 0, 3, 2], [2, 0, 3, 1], [3, 1, 2, 0]] and hx.rng.count == 5
    assert hx.attempts.tolist() == [2, 1, 2] and np.array_equal(hx.accepted, hx.attempts) and len(hx.matrices) == 3
    g = _reference_forces(case, R)
    work = np.zeros(R)
    for n, a in enumerate(seen):
        cross_rs = g.restraint_energies(a["pos"], s.box)
        want = g.alchemical_energies(a["pos"], s.box, LAMBDAS) + cross_rs.sum(axis=2)
        print(f"{case} attempt {n}: beta M =\n{BETA300 * a['M']}")
        assert np.array_equal(_bits(a["M"]), _bits(want)) and np.array_equal(hx.matrices[n], BETA300 * a["M"])
        assert np.abs(np.diff(want, axis=1)).min() > 1e-6  # (the states differ for every slot)
        # the run's own restraint energies are the entries of the states the slots held, and the call left them alone
        assert np.array_equal(_bits(cross_rs[rows, a["held"]]), _bits(a["e0"])) and np.array_equal(_bits(a["e1"]), _bits(a["e0"]))
        assert a["e0"][:, 1].min() > 0.0
        work += a["M"][rows, hx.history[n]] - a["M"][rows, a["held"]]
    assert np.array_equal(hx.work(), work) and np.abs(work).min() > 0.0
    assert np.array_equal(hx.record["M"], seen[-1]["M"]) and hx.record["states"].tolist() == [3, 1, 2, 0]


# ----------------------------------------------------------------------------- trajectories, bit for bit
# Where two runs of the same steps give the same bits: on the cell-list path, which stores its forces, with
# the lanes per atom pinned so that every energy slot receives one addend of a kind (`_pin_lanes`); and on the all-pairs path
# only when every atom's force has two addends (its pair sum and its bonded sum: TMDHIP_ALLPAIRS_WAVES=1, one j range per
# atom) and the launch has at most 256 waves per replica (192 atoms).  That knob is read once per process, so the all-pairs
# cases run in a process of their own (`test_fp64_all_pairs_bit_for_bit`), which calls the same three functions.
def _twin_check(case):
    """`step(2 x frequency)` with every tried pair accepted against the twin without exchange= that makes, after every batch,
    the two cross-energy calls, the decision of tests/_hrex.py, the setters and compute() by hand."""
    R, freq = 4, 10
    hx = _forced(freq)
    s, f, integ, al, rs = _build(case, R, hx)
    out = integ.step(2 * freq)
    _check_path(case, f, s)
    assert hx.nattempts == 2 and hx.states.tolist() == [2, 0, 3, 1] and np.array_equal(hx.accepted, hx.attempts)
    s2, f2, integ2, al2, rs2 = _build(case, R, None)
    r0, k0 = rs2.dist_r0.copy(), rs2.dist_k.copy()
    states = list(range(R))
    for n in range(2):
        out2 = integ2.step(freq)
        M = f2.alchemical_energies(s2.pos, s2.box, LAMBDAS) + f2.restraint_energies(s2.pos, s2.box).sum(axis=2)[:, np.argsort(states)]
        states, acc, delta = H.decide(M.tolist(), states, n % 2, [0.0, 0.0], BETA300)
        assert acc.all()
        states = states.tolist()
        al2.set_lambdas(LAMBDAS[states, 0], LAMBDAS[states, 1])
        rs2.set_distance_targets(r0[states])
        rs2.set_strengths(distance_k=k0[states])
        pot2 = f2.compute(s2.pos, s2.box, s2.forces)
    assert states == hx.states.tolist()
    assert _same_bits(_state(s), _state(s2))
    assert np.array_equal(_bits(out[0]), _bits(out2[0])) and list(out[1]) == list(pot2) and np.array_equal(out[2], out2[2])
    assert np.array_equal(np.stack(al.lambdas(R), axis=1), LAMBDAS[states]) and np.array_equal(rs.dist_r0, r0[states])
    # (and the swaps matter: the run without them is another trajectory)
    plain, _ = _cut_run(case, R, (freq, freq))
    assert not np.array_equal(_bits(plain[0]), _bits(_state(s)[0]))


def _no_swap_check(case, R=4):
    """`decide` patched so that no swap is accepted: the cross-energy launches between the batches leave no trace.  (With one
    replica no pair is tried to begin with.)"""
    from torchmd_amd.hrex import HamiltonianExchange

    hx = HamiltonianExchange(frequency=10, seed=3)
    s, f, integ, al, rs = _build(case, R, hx)
    inner = hx.decide

    def decide(M):
        states, accepted, delta, pairs, u = inner(M)
        return hx.states.copy(), np.zeros(len(pairs), dtype=bool), delta, pairs, u

    hx.decide = decide
    integ.step(20)
    out = integ.step(5)
    _check_path(case, f, s)
    assert hx.nattempts == 2 and hx.accepted.sum() == 0 and hx.work().tolist() == [0.0] * R and hx.states.tolist() == list(range(R))
    assert hx.attempts.tolist() == ([1, 1, 1] if R == 4 else []) and hx.record["M"].shape == (R, R)
    assert al.version == 1 and np.isfinite(hx.record["M"]).all()
    plain, out0 = _cut_run(case, R, (10, 10, 5))
    assert _same_bits(_state(s), plain)
    assert np.array_equal(_bits(out[0]), _bits(out0[0])) and list(out[1]) == list(out0[1])


def _returned_check(case, exact):
    """After an attempt that moved a slot the potential energies `step` returns are compute()'s at the final state and
    `systems.forces` are that call's forces — `exact`: bit for bit, else at the bars of tests/test_gpu_parity.py (force and
    energy atomics: DESIGN §11) — and they are not those of the assignment before."""
    R = 4
    prec = CASES[case]["prec"]
    hx = _forced(10)
    s, f, integ, al, rs = _build(case, R, hx)
    vel_seen = []
    inner = hx.attempt

    def attempt(system, forces, epot=None):
        vel_seen.append(system.vel.clone())
        return inner(system, forces, epot)

    hx.attempt = attempt
    out = integ.step(10)
    assert hx.states.tolist() == [1, 0, 3, 2] and torch.equal(s.vel, vel_seen[0]) and integ.kinetic_source is None
    F2 = torch.zeros_like(s.pos)
    tot = np.asarray(f.compute(s.pos, s.box, F2))
    got = np.asarray(out[1])
    print(f"{case}: |U returned - U compute| = {np.abs(got - tot).max():.3e}, |F left - F compute| = {(s.forces - F2).abs().max().item():.3e}")
    if exact:
        assert np.array_equal(_bits(got), _bits(tot)) and torch.equal(s.forces, F2)
    else:
        assert (np.abs(got - tot) <= ERTOL[prec] * EFAC * np.maximum(1.0, np.abs(tot))).all()
        assert (s.forces - F2).abs().max().item() <= FTOL[prec]
    # ... and not those of the assignment before it: a second context that still holds state r in slot r
    g = _reference_forces(case, R)
    Fg = torch.zeros_like(s.pos)
    old = np.asarray(g.compute(s.pos, s.box, Fg))
    print(f"{case}: U(new) - U(old) per slot = {got - old}, max |dF| = {(s.forces - Fg).abs().max().item():.3e}")
    # (neighbouring states differ by several k_B T = 0.6 kcal/mol and by a restraint force of k x 0.3 A = 12 kcal/mol/A)
    assert np.abs(got - old).min() > 0.5 and (s.forces - Fg).abs().max().item() > 1e3 * FTOL[prec]
    # the gap is the work the control booked
    assert np.abs((got - old) - hx.work()).max() <= ERTOL[prec] * EFAC * np.maximum(1.0, np.abs(old)).max()


def test_forced_acceptance_equals_the_twin_that_makes_the_calls_by_hand_fp32_fused_list(monkeypatch):
    _pin_lanes("f32-fused-list", monkeypatch)
    _twin_check("f32-fused-list")


def test_no_swap_accepted_is_the_run_without_exchange_fp32_fused_list(monkeypatch):
    _pin_lanes("f32-fused-list", monkeypatch)
    _no_swap_check("f32-fused-list")


def test_one_replica_is_the_run_without_exchange(monkeypatch):
    _pin_lanes("f32-fused-list", monkeypatch)
    _no_swap_check("f32-fused-list", R=1)


def test_returned_energies_and_forces_are_those_of_the_new_assignment_fp32_fused_list(monkeypatch):
    _pin_lanes("f32-fused-list", monkeypatch)
    _returned_check("f32-fused-list", exact=True)


def test_returned_energies_and_forces_are_those_of_the_new_assignment_fp64_all_pairs():
    _returned_check("f64-allpairs", exact=False)


def all_pairs_checks():
    """What `test_fp64_all_pairs_bit_for_bit` runs in its child process."""
    assert os.environ.get("TMDHIP_ALLPAIRS_WAVES") == "1"
    _twin_check("f64-allpairs-1split")
    _no_swap_check("f64-allpairs-1split")
    _returned_check("f64-allpairs-1split", exact=True)
    print("ALL_PAIRS_OK")


def test_fp64_all_pairs_bit_for_bit():
    """The three checks above in fp64 on the all-pairs path, in a process of its own (see the comment above `_twin_check`)."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = (f"import sys; sys.path.insert(0, {os.path.join(root, 'tests')!r}); sys.path.insert(0, {root!r}); "
            "import test_gpu_hrex as T; T.all_pairs_checks()")
    res = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, cwd=root,
                         env=dict(os.environ, TMDHIP_ALLPAIRS_WAVES="1"))
    print(res.stdout[-3000:])
    assert res.returncode == 0 and "ALL_PAIRS_OK" in res.stdout, res.stdout[-3000:] + res.stderr[-4000:]


def test_nve_conserves_kinetic_plus_potential_minus_work():
    """NVE, fp64, 200 steps of 0.25 fs, forced swaps every 20 steps.  The spread of E_kin + E_pot - work over the ten calls, the
    largest of the four slots, is at most twice that of the run without exchange on the same start (§22's bar); without the
    work it misses that bar by more than 10x."""
    case = dict(prec="f64", nside=6, kw=dict(cutoff=9.0, rfa=True, switch_dist=7.5, switch_mode="exact", algorithm="allpairs"))
    R = 4
    spread = {}
    for name in ("plain", "exchange"):
        hx = _forced(20, temperature=300.0) if name == "exchange" else None
        s, f, integ, al, rs = _build(case, R, hx, T0=150.0, dt=0.25, langevin=False)
        e, raw = [], []
        for _ in range(10):
            ek, ep, _ = integ.step(20)
            w = hx.work() if hx is not None else np.zeros(R)
            raw.append(np.asarray(ek, dtype=np.float64) + np.asarray(ep))
            e.append(raw[-1] - w)
        spread[name] = (np.max(e, axis=0) - np.min(e, axis=0)).max()
        if hx is not None:
            spread["without work"] = (np.max(raw, axis=0) - np.min(raw, axis=0)).max()
            assert hx.nattempts == 10 and np.array_equal(hx.accepted, hx.attempts) and np.abs(hx.work()).max() > 0.1
    print(f"NVE, 200 steps of 0.25 fs: spread plain {spread['plain']:.3e}, with exchange {spread['exchange']:.3e}, "
          f"without the work {spread['without work']:.3e} kcal/mol")
    assert spread["exchange"] <= 2 * spread["plain"]
    assert spread["without work"] > 10 * 2 * spread["plain"]


def test_rigid_waters_under_exchange():
    """constraints="water" at 2 fs: the swaps go through, the returned energies are compute()'s, the waters keep their shape
    (the constraint solver's own tolerance, tests/test_gpu_constraints.py: 1e-10 relative in fp64)."""
    R = 4
    hx = _forced(10)
    s, f, integ, al, rs = _build("f64-allpairs", R, hx, dt=2.0, constraints="water")
    out = integ.step(20)
    assert hx.nattempts == 2 and hx.states.tolist() == [2, 0, 3, 1]
    F2 = torch.zeros_like(s.pos)
    tot = np.asarray(f.compute(s.pos, s.box, F2))
    assert np.abs(np.asarray(out[1]) - tot).max() <= ERTOL["f64"] * EFAC * np.abs(tot).max() and np.isfinite(out[0]).all()
    cs = integ.constraints
    w, d0 = np.asarray(cs.waters), np.asarray(cs.water_dist)
    want = np.stack([d0[:, 0], d0[:, 0], d0[:, 1]], axis=1)
    for r in range(R):
        p = s.pos[r].cpu().double().numpy()
        d = np.stack([np.linalg.norm(p[w[:, 0]] - p[w[:, 1]], axis=1), np.linalg.norm(p[w[:, 0]] - p[w[:, 2]], axis=1),
                      np.linalg.norm(p[w[:, 1]] - p[w[:, 2]], axis=1)], axis=1)
        assert np.abs(d / want - 1.0).max() <= 1e-10


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
np.savez(os.path.join(TMP, "restraints.npz"), dist_pair=np.array([[3, 12]]), dist_r0=np.array([[4.0], [4.5]]), dist_k=np.array([20.0]))
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
side = dict(alchemical={"atoms": [30, 31, 32], "lambda_vdw": [1.0, 1.0], "lambda_elec": [1.0, 0.5]}, restraints=os.path.join(TMP, "restraints.npz"))
go("log", **side)
out["module_after_off"] = "torchmd_amd.hrex" in sys.modules
go("log_hx", hamiltonian_exchange={"frequency": 10, "seed": 3, "keep_matrices": True}, **side)
out["json"] = json.load(open(os.path.join(TMP, "log_hx", "hamiltonian_exchange.json")))
out["u"] = np.load(os.path.join(TMP, "log_hx", "hrex_u.npy")).tolist()
out["states"] = np.load(os.path.join(TMP, "log_hx", "hrex_states.npy")).tolist()
print("RESULT " + json.dumps(out))
"""


def test_run_py_with_and_without_the_mapping(tmp_path):
    import json

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = f"ROOT = {root!r}\nTMP = {str(tmp_path)!r}\n" + _CHILD
    res = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, cwd=root)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-4000:]
    out = json.loads(next(ln for ln in res.stdout.splitlines() if ln.startswith("RESULT "))[7:])
    files = ["input.yaml"] + [f"monitor_{k}.csv" for k in range(2)] + [f"output_{k}.npy" for k in range(2)]
    assert out["module_after_off"] is False  # off means off: without the key the module is never imported
    assert out["log"]["files"] == files
    assert out["log_hx"]["files"] == sorted(files + ["hamiltonian_exchange.json", "hrex_states.npy", "hrex_u.npy"])
    head = "iter,ns,epot,ekin,etot,T,restraints,alchemical,dudl_vdw,dudl_elec,t"
    assert all(rows[0] == head and len(rows) == 3 for rows in out["log"]["rows"])
    u, states, js = np.array(out["u"]), np.array(out["states"]), out["json"]
    assert u.shape == (4, 2, 2) and np.isfinite(u).all() and states.shape == (4, 2)
    assert all(sorted(row) == [0, 1] for row in states.tolist())
    assert js["frequency"] == 10 and js["seed"] == 3 and abs(js["temperature"] - 300.0) < 1e-9 and js["attempts"] == [2]
    assert 0 <= js["accepted"][0] <= 2 and js["states"] == states[-1].tolist()
    for k, rows in enumerate(out["log_hx"]["rows"]):
        assert rows[0] == head.replace("T,", "T,state,") and len(rows) == 3
        vals = np.array([[float(x) for x in r.split(",")] for r in rows[1:]])
        assert np.isfinite(vals).all()
        assert vals[:, 6].tolist() == [states[1][k], states[3][k]]  # the state the slot holds when the row is written
