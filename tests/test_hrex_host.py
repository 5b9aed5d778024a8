"""The Hamiltonian exchange without a GPU: the decision against a brute-force transcription, the acceptance rate
of two harmonic windows against its closed form, the random stream, the snapshots and assignments of `Alchemical` and
`Restraints` against the permutation made by hand, every refusal, the exports, the header, and the control's place in the one
schedule loop (`Integrator.run_schedule` with a fake segment runner, as tests/test_schedule_host.py drives it)."""

import math
import os

import numpy as np
import pytest
import torch

import _hrex as H
from _exchange import Counting

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BETA300 = 1.0 / (H.BOLTZMAN * 300.0)


def _forces(**kw):
    from _golden import GoldenParameters, load
    from torchmd_amd.forces import Forces

    g = load("water291")
    return g, Forces(GoldenParameters(g, torch.float32), terms=["lj", "electrostatics", "bonds", "angles"], cutoff=7.3, rfa=True, **kw)


def _integrator(R, term=None, exchange=None, forces_kw=None, **kw):
    """An integrator on the host whose Forces never evaluates: `compute` is replaced by a recorder; `term` (a host side term of
    tests/_hrex.py) sits in the restraints' slot."""
    from torchmd_amd.integrator import Integrator
    from torchmd_amd.systems import System

    g, f = _forces(**(forces_kw or {}))
    if term is not None:
        f.restraints = term
    f.computed = []

    def compute(pos, box, forces):
        f.computed.append([t.version for t in (f.restraints, f.alchemical) if t is not None])
        forces.fill_(float(len(f.computed)))
        return [100.0 * len(f.computed) + r for r in range(pos.shape[0])]

    f.compute = compute
    s = System(291, R, torch.float32, "cpu")
    s.set_box(g["box"])
    return Integrator(s, f, 1.0, "cpu", exchange=exchange, **kw), f, s


def _runner(it, log=None, before=None):
    """What `_step_body` does to the step count (tests/test_schedule_host.py), after `before()` has placed the replicas."""

    def run(n):
        if log is not None:
            log.append(("segment", n))
        it._nstep += max(n, 0)
        if before is not None:
            before()
        R = it.systems.pos.shape[0]
        return (np.zeros(R, dtype=np.float32), [float(it._nstep)] * R, np.zeros(R))

    return run


# ----------------------------------------------------------------------------- the decision
@pytest.mark.parametrize("R", [1, 2, 3, 8, 17])
def test_decisions_equal_the_brute_force_transcription(R):
    from torchmd_amd.hrex import hamiltonian_decisions

    rng = np.random.default_rng(100 + R)
    seen = {True: 0, False: 0}
    for trial in range(40):
        M = rng.normal(0.0, 1.5 / BETA300, (R, R))
        states = rng.permutation(R)
        for parity in (0, 1):
            pairs = H.pairs_of(parity, R)
            u = rng.random(len(pairs))
            new, acc, delta, got_pairs = hamiltonian_decisions(M, states, parity, u, BETA300)
            want, wacc, wdelta = H.decide(M.tolist(), states.tolist(), parity, u.tolist(), BETA300)
            assert np.array_equal(new, want) and np.array_equal(acc, wacc) and got_pairs.tolist() == [list(p) for p in pairs]
            assert np.array_equal(delta, wdelta)  # (the same expression in the same order)
            assert sorted(new.tolist()) == list(range(R)) and got_pairs.shape == (len(pairs), 2)
            assert np.array_equal(states, np.asarray(states))  # (the input is not changed)
            for a in acc:
                seen[bool(a)] += 1
            # an accepted pair has traded, a rejected pair has not, nobody else has moved
            slot = {int(s): r for r, s in enumerate(states)}
            for (a, b), ok in zip(pairs, acc):
                assert (new[slot[a]], new[slot[b]]) == ((b, a) if ok else (a, b))
            untried = [r for r in range(R) if all(states[r] not in p for p in pairs)]
            assert all(new[r] == states[r] for r in untried)
    if R > 1:
        assert seen[True] > 10 and seen[False] > 10  # (both branches were taken)


@pytest.mark.parametrize("R", [2, 3, 8, 17])
def test_equal_matrix_accepts_everything_and_nan_rejects(R):
    from torchmd_amd.hrex import hamiltonian_decisions

    rng = np.random.default_rng(R)
    states = rng.permutation(R)
    for parity in (0, 1):
        n = len(H.pairs_of(parity, R))
        u = np.full(n, 1.0 - 2.0**-53)  # the largest number the generator can return
        new, acc, delta, pairs = hamiltonian_decisions(np.full((R, R), 3.25), states, parity, u, BETA300)
        assert acc.all() and (delta == 0.0).all()
        slot = np.argsort(states)
        for a, b in pairs:
            assert new[slot[a]] == b and new[slot[b]] == a
        if n:
            # one NaN in the row of the slot that holds state `parity`: the pair it belongs to is rejected even with u = 0
            M = np.full((R, R), 3.25)
            M[slot[parity], parity + 1] = np.nan
            new, acc, delta, pairs = hamiltonian_decisions(M, states, parity, np.zeros(n), BETA300)
            assert not acc[0] and np.isnan(delta[0]) and acc[1:].all()
            assert new[slot[parity]] == parity and new[slot[parity + 1]] == parity + 1


def test_decision_refusals():
    from torchmd_amd.hrex import hamiltonian_decisions

    M = np.zeros((4, 4))
    with pytest.raises(ValueError, match="u needs as many"):
        hamiltonian_decisions(M, [0, 1, 2, 3], 0, [0.5], BETA300)
    with pytest.raises(ValueError, match="u needs as many"):
        hamiltonian_decisions(M, [0, 1, 2, 3], 1, [0.5, 0.5], BETA300)
    with pytest.raises(ValueError, match="permutation"):
        hamiltonian_decisions(M, [0, 1, 1, 3], 0, [0.5, 0.5], BETA300)
    with pytest.raises(ValueError, match="permutation"):
        hamiltonian_decisions(np.zeros((3, 4)), [0, 1, 2, 3], 0, [0.5, 0.5], BETA300)
    new, acc, delta, pairs = hamiltonian_decisions(np.zeros((1, 1)), [0], 0, [], BETA300)
    assert new.tolist() == [0] and len(acc) == 0 and pairs.shape == (0, 2)


# ----------------------------------------------------------------------------- the acceptance rate, exactly
@pytest.mark.parametrize("d", [0.2, 0.5, 1.0])
def test_acceptance_of_two_harmonic_windows(d):
    """Two windows of strength k = 10 kcal/mol/A^2 with centres d apart at 300 K; before every attempt each slot is drawn from
    the Boltzmann distribution of the window it holds.  20 000 tried pairs (the odd attempts of two replicas try none);
    the acceptance must be erfc(sqrt(beta k) d / 2) within 5 binomial standard deviations."""
    from torchmd_amd.hrex import HamiltonianExchange

    k, ntried = 10.0, 20000
    term = H.Windows([1.0, 1.0 + d], k)
    hx = HamiltonianExchange(frequency=1, temperature=300.0, seed=17)
    it, f, s = _integrator(2, term, hx)
    sigma = math.sqrt(1.0 / (BETA300 * k))
    rng = np.random.default_rng(int(1000 * d))

    def place():
        s.pos[:, 0, 0] = torch.as_tensor(term.centres + sigma * rng.standard_normal(2), dtype=s.pos.dtype)

    it.run_schedule(2 * ntried, [hx], _runner(it, before=place))
    p = H.acceptance_of_two_windows(BETA300, k, d)
    rate = hx.accepted[0] / hx.attempts[0]
    sd = math.sqrt(p * (1.0 - p) / ntried)
    print(f"d = {d}: acceptance {rate:.5f}, exact {p:.5f}, {abs(rate - p) / sd:.2f} standard deviations")
    assert hx.nattempts == 2 * ntried and hx.attempts.tolist() == [ntried]
    assert abs(rate - p) <= 5 * sd
    # the bookkeeping of the same run: every accepted swap was assigned and evaluated once, and nothing else was
    assert len(term.assigned) == len(f.computed) == hx.accepted[0] and term.version == hx.accepted[0]
    assert sorted(hx.states.tolist()) == [0, 1] and hx.states.tolist() == hx.history[-1].tolist()
    assert np.allclose(np.sort(term.centres), [1.0, 1.0 + d]) and term.centres[0] == [1.0, 1.0 + d][hx.states[0]]


# ----------------------------------------------------------------------------- the random stream
@pytest.mark.parametrize("R", [1, 2, 5, 8])
def test_stream_position_depends_on_the_number_of_attempts_only(R):
    from torchmd_amd.controls import philox_stream
    from torchmd_amd.hrex import HamiltonianExchange

    nattempts = 7
    after = []
    for kind in ("accepts", "rejects"):
        # accepts: every state is as good as any other; rejects: a slot is far better off where it is, whatever u says
        M = np.zeros((R, R)) if kind == "accepts" else 1e6 * (1.0 - np.eye(R))
        term = H.Constant(M)
        hx = HamiltonianExchange(frequency=3, temperature=300.0, seed=5)
        it, f, s = _integrator(R, term, hx)
        it.run_schedule(3 * nattempts, [hx], _runner(it))
        assert hx.nattempts == nattempts
        if kind == "rejects":
            assert hx.accepted.sum() == 0 and hx.states.tolist() == list(range(R)) and not f.computed and not term.assigned
        elif R > 1:
            assert np.array_equal(hx.accepted, hx.attempts) and hx.accepted.sum() > 0
        after.append(hx.rng.random())
    ndraws = sum(len(H.pairs_of(n % 2, R)) for n in range(nattempts))
    fresh = philox_stream(5, 0)
    for _ in range(ndraws):
        fresh.random()
    assert after[0] == after[1] == fresh.random()


# ----------------------------------------------------------------------------- snapshots and assignments of the real terms
def _alchemical(R):
    from torchmd_amd.alchemy import Alchemical

    lv = np.linspace(1.0, 0.0, R)
    return Alchemical([0, 1, 2], lv, np.zeros(R))


def _restraints(R):
    from torchmd_amd.restraints import Restraints

    rng = np.random.default_rng(3)
    rs = Restraints(R)
    rs.add_position([0, 150], rng.normal(0.0, 1.0, (R, 2, 3)), rng.uniform(1.0, 50.0, (R, 2)))
    rs.add_distance([[3, 12], [6, 30], [9, 60]], rng.uniform(2.0, 6.0, (R, 3)), rng.uniform(1.0, 90.0, (R, 3)))
    return rs


def test_snapshot_and_assignment_equal_the_permutation_by_hand():
    from torchmd_amd.hrex import HamiltonianExchange

    R = 5
    al, rs = _alchemical(R), _restraints(R)
    lam0 = np.stack(al.lambdas(R), axis=1)
    tables0 = [t.copy() for t in (rs.pos_ref, rs.pos_k, rs.dist_r0, rs.dist_k)]
    assert np.array_equal(al.exchange_parameters(R), lam0)
    snap = rs.exchange_parameters(R)
    assert all(np.array_equal(snap[n], t) for n, t in zip(("pos_ref", "pos_k", "dist_r0", "dist_k"), tables0))
    snap["dist_r0"][0, 0] = -1.0  # (a copy: the term's own table is not the snapshot)
    assert rs.dist_r0[0, 0] == tables0[2][0, 0]
    # nothing per replica: nothing to trade
    from torchmd_amd.alchemy import Alchemical
    from torchmd_amd.restraints import Restraints

    assert Alchemical([0, 1, 2], 0.5, 0.0).exchange_parameters(R) is None and Restraints(R).exchange_parameters(R) is None
    assert Alchemical([0, 1, 2], 0.5, 0.0).exchange_parameters(1).tolist() == [[0.5, 0.0]]

    hx = HamiltonianExchange(frequency=10, temperature=300.0, seed=1)
    it, f, s = _integrator(R, None, hx, forces_kw=dict(alchemical=al, restraints=rs))
    assert hx.terms == [rs, al] and hx.states.tolist() == list(range(R)) and hx.beta == BETA300
    # the terms' device halves replaced: all states equally good, u = 0
    Ms = {rs: np.arange(R * R, dtype=np.float64).reshape(R, R), al: np.zeros((R, R))}
    rs.cross_energies = lambda owner, pos, box, snapshot: Ms[rs]
    al.cross_energies = lambda owner, pos, box, snapshot: Ms[al]
    hx.beta = 0.0  # (every Delta is 0: accepted)
    hx.rng = Counting(0.0)
    states = list(range(R))
    want_history = [[1, 0, 3, 2, 4], [2, 0, 4, 1, 3], [3, 1, 4, 0, 2]]
    versions = (rs.version, al.version)
    for n in range(3):
        out = it.run_schedule(10, [hx], _runner(it))
        states = want_history[n]
        assert hx.states.tolist() == states and hx.history[-1].tolist() == states
        assert np.array_equal(np.stack(al.lambdas(R), axis=1), lam0[states])
        for got, want in zip((rs.pos_ref, rs.pos_k, rs.dist_r0, rs.dist_k), H.permute_restraints(rs, tables0, states)):
            assert np.array_equal(got, want)
        # one version bump per term and attempt (one upload at the next evaluation), and the evaluation came after both
        assert (rs.version, al.version) == (versions[0] + n + 1, versions[1] + n + 1)
        assert f.computed[-1] == [rs.version, al.version] and len(f.computed) == n + 1
        assert out[1] == [100.0 * (n + 1) + r for r in range(R)]  # the potential energies of that evaluation
        assert torch.equal(s.forces, torch.full_like(s.forces, float(n + 1)))
        assert np.array_equal(hx.record["M"], Ms[rs]) and hx.record["accepted"].all() and hx.record["states"].tolist() == states
    assert hx.rng.count == 2 + 2 + 2 and hx.attempts.tolist() == [2, 1, 2, 1] and np.array_equal(hx.accepted, hx.attempts)
    # work: the sum over attempts of M[r][new] - M[r][old]
    work, old = np.zeros(R), list(range(R))
    for new in want_history:
        work += np.array([Ms[rs][r, new[r]] - Ms[rs][r, old[r]] for r in range(R)])
        old = new
    assert np.array_equal(hx.work(), work)
    # the restraints' own map from slot rows to states follows the assignment
    assert hx.snapshots[0]["state_of_slot"].tolist() == want_history[-1]


def test_restraint_columns_are_mapped_from_slot_rows_to_states():
    """tmdhip_restraint_states answers by the row of the device table, which belongs to a slot; the exchange asks by state."""
    R = 4
    rs = _restraints(R)
    snap = rs.exchange_parameters(R)
    states = [2, 0, 3, 1]
    rs.assign_states(snap, states)

    class Owner:
        def restraint_energies(self, pos, box):
            # entry [i, k] = 10 i + (the state that slot k holds), split over (position, distance)
            e = np.array([[10.0 * i + states[k] for k in range(R)] for i in range(R)])
            return np.stack([0.25 * e, 0.75 * e], axis=2)

    M = rs.cross_energies(Owner(), None, None, snap)
    assert np.array_equal(M, np.array([[10.0 * i + a for a in range(R)] for i in range(R)]))


def test_a_change_from_outside_raises_at_the_next_attempt():
    from torchmd_amd.hrex import HamiltonianExchange

    R = 3
    for who in ("alchemical", "restraints"):
        al, rs = _alchemical(R), _restraints(R)
        hx = HamiltonianExchange(frequency=10, temperature=300.0, seed=1)
        it, f, s = _integrator(R, None, hx, forces_kw=dict(alchemical=al, restraints=rs))
        rs.cross_energies = al.cross_energies = lambda owner, pos, box, snapshot: np.zeros((R, R))
        it.run_schedule(10, [hx], _runner(it))
        assert hx.nattempts == 1 and hx.states.tolist() == [1, 0, 2]
        if who == "alchemical":
            al.set_lambdas([1.0, 0.5, 0.0], [0.0, 0.0, 0.0])
        else:
            rs.set_distance_targets(rs.dist_r0 + 0.5)
        with pytest.raises(RuntimeError, match=f"{who} parameters were changed"):
            it.run_schedule(10, [hx], _runner(it))
        assert hx.nattempts == 1


# ----------------------------------------------------------------------------- refusals
def test_refusals():
    from torchmd_amd.barostat import MonteCarloBarostat
    from torchmd_amd.hrex import HamiltonianExchange
    from torchmd_amd.metadynamics import Metadynamics
    from torchmd_amd.restraints import Restraints
    from torchmd_amd.thermostat import VelocityRescale

    def hx(**kw):
        return HamiltonianExchange(**{"frequency": 10, "temperature": 300.0, "seed": 1, **kw})

    def distances(R):
        return Restraints(R).add_distance([[3, 12]], np.linspace(3.0, 4.0, R)[:, None], 10.0)

    for bad in (0, -5, 2.5, True, "10", None):
        with pytest.raises(ValueError, match="frequency"):
            hx(frequency=bad)
    for bad in (0.0, -300.0, np.inf, [300.0, 310.0]):
        with pytest.raises(ValueError, match="temperature"):
            hx(temperature=bad)
    with pytest.raises(ValueError, match="batch"):
        _integrator(2, H.Windows([1.0, 2.0], 10.0), hx(), batch=torch.zeros(291, dtype=torch.long))
    with pytest.raises(ValueError, match="barostat"):
        _integrator(2, None, hx(), forces_kw=dict(restraints=distances(2)), gamma=1.0, T=300.0,
                    barostat=MonteCarloBarostat(1.0, 300.0, frequency=25, seed=2))
    # no exchangeable side term: none at all, one coupling shared by all replicas, restraints without entries
    from torchmd_amd.alchemy import Alchemical

    for kw in ({}, dict(alchemical=Alchemical([0, 1, 2], 0.5, 0.0)), dict(restraints=Restraints(2))):
        with pytest.raises(ValueError, match="side term that holds parameters per replica"):
            _integrator(2, None, hx(), forces_kw=kw)
    # a snapshot whose number of rows is not the number of replicas
    with pytest.raises(ValueError, match="3 replicas"):
        _integrator(2, None, hx(), forces_kw=dict(restraints=distances(3)))
    with pytest.raises(ValueError, match="3 couplings for 2 replicas"):
        _integrator(2, None, hx(), forces_kw=dict(alchemical=_alchemical(3)))
    with pytest.raises(ValueError, match="3 windows for 2 replicas"):
        _integrator(2, H.Windows([1.0, 2.0, 3.0], 10.0), hx())
    # the temperature: given, Langevin's, the thermostat's one common target; a ladder and none at all are refused
    assert _integrator(2, H.Windows([1.0, 2.0], 10.0), hx(temperature=250.0), gamma=1.0, T=300.0)[0].exchange.beta == 1.0 / (H.BOLTZMAN * 250.0)
    assert _integrator(2, H.Windows([1.0, 2.0], 10.0), hx(temperature=None), gamma=1.0, T=310.0)[0].exchange.beta == 1.0 / (H.BOLTZMAN * 310.0)
    for target in (320.0, [320.0, 320.0]):
        it = _integrator(2, H.Windows([1.0, 2.0], 10.0), hx(temperature=None), thermostat=VelocityRescale(target, seed=1))[0]
        assert it.exchange.beta == 1.0 / (H.BOLTZMAN * 320.0)
    with pytest.raises(ValueError, match="ladder of distinct temperatures"):
        _integrator(2, H.Windows([1.0, 2.0], 10.0), hx(temperature=None), thermostat=VelocityRescale([300.0, 320.0], seed=1))
    with pytest.raises(ValueError, match="needs a temperature"):
        _integrator(2, H.Windows([1.0, 2.0], 10.0), hx(temperature=None))
    # metadynamics refuses any exchange through its own entry
    md = Metadynamics([("distance", (0, 3))], sigma=0.2, height=0.1, frequency=20, temperature=300.0, grid_min=1.0, grid_max=9.0,
                      nreplicas=2)
    with pytest.raises(ValueError, match="exchange"):
        _integrator(2, None, hx(), forces_kw=dict(restraints=distances(2), metadynamics=md))
    # one replica is allowed and tries no pair
    one = hx()
    it, f, s = _integrator(1, H.Windows([1.0], 10.0), one)
    it.run_schedule(30, [one], _runner(it))
    assert one.nattempts == 3 and len(one.attempts) == 0 and one.states.tolist() == [0] and not f.computed
    assert one.record["M"].shape == (1, 1) and one.record["pairs"].shape == (0, 2) and one.work().tolist() == [0.0]
    # an attempt before the control belongs to an integrator
    with pytest.raises(RuntimeError, match="no integrator"):
        hx().attempt(s, f)


def test_run_py_refusals(tmp_path):
    import yaml

    from torchmd_amd import run as driver

    def conf(**kw):
        path = tmp_path / "conf.yaml"
        path.write_text(yaml.safe_dump(dict(kw, log_dir=str(tmp_path))))  # (get_args echoes the configuration into log_dir)
        return ["--conf", str(path)]

    ok = driver.get_args(conf(hamiltonian_exchange={"frequency": 20, "seed": 3, "temperature": 300.0, "keep_matrices": True}))
    assert ok.hamiltonian_exchange["frequency"] == 20 and driver.get_args(conf()).hamiltonian_exchange is None
    with pytest.raises(ValueError, match="unknown keys"):
        driver.get_args(conf(hamiltonian_exchange={"frequency": 20, "period": 3}))
    with pytest.raises(ValueError, match="two exchanges"):
        driver.get_args(conf(hamiltonian_exchange={"frequency": 20}, exchange_frequency=20, thermostat="csvr",
                             thermostat_temperature=[300.0, 310.0], langevin_temperature=0))
    with pytest.raises(ValueError, match="mapping"):
        driver.get_args(conf(hamiltonian_exchange=20))


# ----------------------------------------------------------------------------- the surface
def test_exports_and_import_rules():
    import subprocess
    import sys

    import torchmd_amd
    from torchmd_amd.hrex import HamiltonianExchange

    assert torchmd_amd.HamiltonianExchange is HamiltonianExchange and "HamiltonianExchange" in torchmd_amd.__all__
    # lazily: the package, the integrator and the controls' module come without it
    code = ("import sys; import torchmd_amd, torchmd_amd.integrator, torchmd_amd.controls, torchmd_amd.run; "
            "assert 'torchmd_amd.hrex' not in sys.modules; torchmd_amd.HamiltonianExchange; assert 'torchmd_amd.hrex' in sys.modules")
    res = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd=ROOT, timeout=300)
    assert res.returncode == 0, res.stderr[-2000:]
    src = open(os.path.join(ROOT, "torchmd_amd", "hrex.py")).read()
    assert "isinstance(t" not in src and "Alchemical)" not in src and "Restraints)" not in src  # no test on the kind of term
    assert "hrex" not in open(os.path.join(ROOT, "torchmd_amd", "controls.py")).read()
    # the protocol's defaults: not exchangeable
    from torchmd_amd._lib import SideTerm

    assert SideTerm().exchange_parameters(4) is None
    for name in ("cross_energies", "assign_states"):
        with pytest.raises(NotImplementedError):
            getattr(SideTerm(), name)(None, None) if name == "assign_states" else getattr(SideTerm(), name)(None, None, None, None)


def test_header_declares_the_symbol_and_abi_11():
    from torchmd_amd import _lib as L

    text = open(os.path.join(ROOT, "include", "tmdhip.h")).read()
    assert "tmdhip_restraint_states(" in text and "#define TMDHIP_ABI_VERSION 11" in text
    assert L.ABI_VERSION == 11 and len(L.SIGNATURES["tmdhip_restraint_states"][1]) == 5


# ----------------------------------------------------------------------------- its place in the schedule
def test_the_control_acts_at_rank_two_between_barostat_and_deposition():
    from torchmd_amd.hrex import HamiltonianExchange

    class Recorder:
        def __init__(self, name, frequency, rank, log):
            self.name, self.frequency, self.rank, self.log = name, frequency, rank, log

        def after_segment(self, integrator, out):
            self.log.append((self.name, integrator._nstep))
            return out

    log = []
    hx = HamiltonianExchange(frequency=40, temperature=300.0, seed=1)
    it, f, s = _integrator(2, H.Constant(np.zeros((2, 2))), hx)
    hx.rng = Counting(0.0)
    inner = hx.attempt

    def attempt(system, forces, epot=None):
        log.append(("exchange", it._nstep))
        return inner(system, forces, epot)

    hx.attempt = attempt
    assert hx.rank == 2
    controls = [Recorder("deposition", 20, 3, log), hx, Recorder("barostat", 25, 1, log), Recorder("thermostat", 10, 0, log)]
    out = it.run_schedule(200, controls, _runner(it, log))
    at200 = [e for e in log if e[1] == 200 and e[0] != "segment"]
    assert at200 == [("thermostat", 200), ("barostat", 200), ("exchange", 200), ("deposition", 200)]
    assert [e[1] for e in log if e[0] == "exchange"] == [40, 80, 120, 160, 200] and hx.nattempts == 5
    # attempts 0, 2 and 4 try the one pair and move both slots: the potential returned is that of the evaluation after the
    # last one, the kinetic energies are as the segment left them and nobody is named the kinetic source
    assert hx.attempts.tolist() == [3] and hx.accepted.tolist() == [3] and len(f.computed) == 3
    assert out[1] == [300.0, 301.0] and out[0].dtype == np.float32 and it.kinetic_source is None
    # an attempt that moves nothing hands `out` on as it came
    again = it.run_schedule(40, controls, _runner(it, log))
    assert hx.nattempts == 6 and len(f.computed) == 3 and again[1] == [240.0, 240.0]
