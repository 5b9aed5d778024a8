"""The one schedule loop of `Integrator.step` without a GPU ("Adding a scheduled control"): `Integrator.run_schedule`
driven with a recording segment runner and recording controls, against a model that walks the steps one at a time; and the
rule for the kinetic energy that `step` returns, on the `after_segment` of the five real controls with their device halves
replaced by recorders."""

import numpy as np
import pytest
import torch

FREQ = {"thermostat": 10, "barostat": 25, "exchange": 40, "metadynamics": 20}
RANK = {"thermostat": 0, "barostat": 1, "exchange": 2, "metadynamics": 3}
CALLS = (7, 13, 30, 1, 49, 100, 0, 40)
COMBINATIONS = ((), ("thermostat",), ("barostat",), ("metadynamics",), ("thermostat", "barostat"), ("thermostat", "exchange"),
                ("thermostat", "metadynamics"))


def _integrator(R=2, **kw):
    from _golden import GoldenParameters, load
    from torchmd_amd.forces import Forces
    from torchmd_amd.integrator import Integrator
    from torchmd_amd.systems import System

    g = load("water291")
    f = Forces(GoldenParameters(g, torch.float32), terms=["lj", "electrostatics", "bonds", "angles"], cutoff=7.3, rfa=True)
    s = System(291, R, torch.float32, "cpu")
    s.set_box(g["box"])
    return Integrator(s, f, 1.0, "cpu", **kw)


class Recorder:
    """A control that does nothing but say when it was called."""

    def __init__(self, name, log, it):
        self.name, self.frequency, self.rank, self.log, self.it = name, FREQ[name], RANK[name], log, it

    def after_segment(self, integrator, out):
        assert integrator is self.it
        self.log.append((self.name, self.it._nstep))
        return out


def _runner(it, log):
    """What `_step_body` does to the step count, and a return value that says which segment it was."""

    def run(n):
        log.append(("segment", n))
        it._nstep += max(n, 0)
        return (np.full(2, float(it._nstep), dtype=np.float32), [float(it._nstep)] * 2, np.full(2, 0.5 * it._nstep))

    return run


def _model(nstep, niter, names, acting=None):
    """The log of one call, one step at a time: a segment closes where a multiple of some frequency is reached or where the
    call ends; those whose multiple it is act in rank order."""
    if not names or niter <= 0:
        return [("segment", niter)]
    log, start = [], nstep
    for step in range(nstep + 1, nstep + niter + 1):
        due = [n for n in sorted(names, key=RANK.get) if step % FREQ[n] == 0]
        if due or step == nstep + niter:
            log.append(("segment", step - start))
            log += [(n, step) for n in due if acting is None or n in acting]
            start = step
    return log


@pytest.mark.parametrize("names", COMBINATIONS, ids=lambda c: "+".join(c) or "none")
def test_the_loop_equals_the_step_by_step_model(names):
    it, log = _integrator(), []
    run = _runner(it, log)
    controls = [Recorder(n, log, it) for n in reversed(names)]  # (handed over in the wrong order: the loop sorts by rank)
    nstep = 0
    for niter in CALLS:
        del log[:]
        out = it.run_schedule(niter, controls, run)
        assert log == _model(nstep, niter, names), (names, nstep, niter)
        nstep += niter
        assert it._nstep == nstep
        # the recorders change nothing: what the last segment returned is what the call returns
        assert out[1] == [float(nstep)] * 2 and out[0].dtype == np.float32 and it.kinetic_source is None
        if not names or niter == 0:
            assert log == [("segment", niter)]  # exactly one runner call, no cuts
    assert nstep == 240


def test_rank_order_where_all_four_coincide():
    it, log = _integrator(), []
    controls = [Recorder(n, log, it) for n in ("metadynamics", "exchange", "barostat", "thermostat")]
    it.run_schedule(200, controls, _runner(it, log))
    assert log == _model(0, 200, tuple(FREQ))
    assert log[-5:] == [("segment", 10), ("thermostat", 200), ("barostat", 200), ("exchange", 200), ("metadynamics", 200)]
    assert [e for e in log if e[1] == 100 and e[0] != "segment"] == [("thermostat", 100), ("barostat", 100), ("metadynamics", 100)]


# ----------------------------------------------------------------------------- the real controls, their device halves recorded
K_TH, K_EX, K_CR = np.array([11.25, 12.5]), np.array([21.25, 22.5]), np.array([31.25, 32.5])


def _real_controls(log):
    """The five kinds of action with `apply` / `attempt` / `deposit` replaced: each logs itself and leaves the record its
    kernel would (host tensors: `run_schedule` reads them back like device ones)."""
    from torchmd_amd import _lib as L
    from torchmd_amd.barostat import MonteCarloBarostat
    from torchmd_amd.crescale import CRescaleBarostat
    from torchmd_amd.exchange import ReplicaExchange
    from torchmd_amd.metadynamics import Metadynamics
    from torchmd_amd.thermostat import VelocityRescale

    th = VelocityRescale(300.0, frequency=FREQ["thermostat"], seed=1)
    mc = MonteCarloBarostat(1.0, 300.0, frequency=FREQ["barostat"], seed=2)
    cr = CRescaleBarostat(1.0, 300.0, frequency=FREQ["barostat"], seed=3)
    ex = ReplicaExchange(FREQ["exchange"], seed=4)
    md = Metadynamics([("distance", (0, 3))], sigma=0.2, height=0.1, frequency=FREQ["metadynamics"], temperature=300.0,
                      grid_min=1.0, grid_max=9.0, nreplicas=2)
    it = _integrator(thermostat=th)
    assert [c.rank for c in (th, mc, cr, ex, md)] == [0, 1, 1, 2, 3]

    def th_apply(system, masses, dt, ndof):
        assert system is it.systems and masses is it.masses and dt == it.dt and ndof == it._thermostat_ndof == 3 * 291
        log.append(("thermostat", it._nstep))
        th._record = torch.zeros(2, L.THERMOSTAT_RECORD_DOUBLES, dtype=torch.float64)
        th._record[:, L.THERMOSTAT_K_AFTER] = torch.as_tensor(K_TH)

    def mc_attempt(system, forces, epot):
        assert system is it.systems and forces is it.forces
        log.append(("mc", it._nstep, list(epot)))
        return {"U": np.asarray(epot, dtype=np.float64), "U_new": np.array([-1.5, -2.5]), "accepted": np.array([True, False])}

    def cr_apply(system, forces, masses, dt, epot, ekin):
        assert system is it.systems and forces is it.forces and masses is it.masses and dt == it.dt
        log.append(("crescale", it._nstep, list(epot), ekin))
        return {"K_after": K_CR.copy(), "U_new": np.array([-3.5, -4.5])}

    def ex_attempt(system, masses, thermostat, epot):
        assert system is it.systems and masses is it.masses and thermostat is th
        log.append(("exchange", it._nstep, list(epot)))
        ex._record = torch.zeros(2, L.EXCHANGE_RECORD_DOUBLES, dtype=torch.float64)
        ex._record[:, L.EXCHANGE_K_AFTER] = torch.as_tensor(K_EX)

    def md_deposit(system):
        assert system is it.systems
        log.append(("deposit", it._nstep))

    def reads(c, name, kinetic):
        c.kinetic = lambda: (log.append(("read", name)), kinetic())[1]

    reads(th, "thermostat", th.kinetic), reads(ex, "exchange", ex.kinetic)
    th.apply, mc.attempt, cr.apply, ex.attempt, md.deposit = th_apply, mc_attempt, cr_apply, ex_attempt, md_deposit
    return it, dict(th=th, mc=mc, cr=cr, ex=ex, md=md)


def _split(log):
    """(what ran and acted, what was read back)."""
    return [e for e in log if e[0] != "read"], [e for e in log if e[0] == "read"]


def _kinetic(it, K):
    """(Ekin, T) that `step` returns for the record `K`: cast to the run's precision, the temperature of the cast."""
    Ekin = K.astype(np.float32)
    return Ekin, it._temperature(Ekin)


def test_a_frozen_deposition_cuts_but_does_not_act():
    log = []
    it, c = _real_controls(log)
    c["md"].frozen = True
    it.run_schedule(50, [c["md"]], _runner(it, log))
    assert log == [("segment", 20), ("segment", 20), ("segment", 10)] == _model(0, 50, ("metadynamics",), acting=())
    c["md"].frozen = False
    it.run_schedule(50, [c["md"]], _runner(it, log))
    assert log[3:] == [("segment", 10), ("deposit", 60), ("segment", 20), ("deposit", 80), ("segment", 20), ("deposit", 100)]


@pytest.mark.parametrize("last", ("thermostat", "mc", "crescale", "thermostat+crescale", "exchange", "deposit", "nothing"))
def test_the_kinetic_energy_returned_is_that_of_the_last_actor(last):
    """Calls on a fresh integrator that end on a step where `last` is the last to act (frequencies 10 / 25 / 40 / 20)."""
    log = []
    it, c = _real_controls(log)
    run = _runner(it, log)
    plain = lambda n: (np.full(2, float(n), dtype=np.float32), [float(n)] * 2, np.full(2, 0.5 * n))  # noqa: E731 (the runner's)
    if last == "thermostat":  # 30: on the thermostat's multiple only
        out = it.run_schedule(30, [c["th"], c["mc"]], run)
        acts, read = _split(log)
        want = _kinetic(it, K_TH) + (plain(30)[1],)
        assert acts[-1] == ("thermostat", 30)
    elif last == "mc":  # 50: thermostat, then the Monte Carlo move, which leaves the kinetic source as it is
        out = it.run_schedule(50, [c["th"], c["mc"]], run)
        acts, read = _split(log)
        want = _kinetic(it, K_TH) + ([-1.5, 50.0],)  # (U_new where accepted)
        assert acts[-2:] == [("thermostat", 50), ("mc", 50, [50.0, 50.0])]
    elif last == "crescale":  # 25: the barostat alone, its own K_after
        out = it.run_schedule(25, [c["th"], c["cr"]], run)
        acts, read = _split(log)
        want = _kinetic(it, K_CR) + ([-3.5, -4.5],)
        assert acts[-1][:3] == ("crescale", 25, [25.0, 25.0]) and np.array_equal(acts[-1][3], plain(25)[0])
    elif last == "thermostat+crescale":  # 50: the thermostat's source is cleared by the rescaling after it
        out = it.run_schedule(50, [c["th"], c["cr"]], run)
        acts, read = _split(log)
        want = _kinetic(it, K_CR) + ([-3.5, -4.5],)
        assert [e[:2] for e in acts[-2:]] == [("thermostat", 50), ("crescale", 50)]
    elif last == "exchange":  # 40: thermostat, then the exchange
        out = it.run_schedule(40, [c["th"], c["ex"]], run)
        acts, read = _split(log)
        want = _kinetic(it, K_EX) + (plain(40)[1],)
        assert acts[-2:] == [("thermostat", 40), ("exchange", 40, [40.0, 40.0])]
    elif last == "deposit":  # 20: thermostat, then the deposition, which changes nothing
        out = it.run_schedule(20, [c["th"], c["md"]], run)
        acts, read = _split(log)
        want = _kinetic(it, K_TH) + (plain(20)[1],)
        assert acts[-2:] == [("thermostat", 20), ("deposit", 20)]
    else:  # 43: the thermostat and the exchange acted on interior segments; the last one ended on nothing
        out = it.run_schedule(43, [c["th"], c["ex"]], run)
        acts, read = _split(log)
        want = (plain(43)[0], plain(43)[2], plain(43)[1])
        assert acts[-2:] == [("exchange", 40, [40.0, 40.0]), ("segment", 3)]
    # one record is read back, after everything else, where a kinetic source is left; none where it is not
    reader = {"thermostat": "thermostat", "mc": "thermostat", "exchange": "exchange", "deposit": "thermostat"}.get(last)
    assert read == ([("read", reader)] if reader else []) and (not reader or log[-1] == ("read", reader))
    Ekin, T, pot = want
    assert out[0].dtype == np.float32 and np.array_equal(out[0], Ekin) and np.array_equal(out[2], T) and list(out[1]) == pot
    assert it.kinetic_source is None  # (nothing of this call is left for the next one)
