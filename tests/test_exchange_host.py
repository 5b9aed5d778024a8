"""Temperature replica exchange without a GPU: the decision function of torchmd_amd/exchange.py against the model
of tests/_exchange.py and against the canonical distribution it must leave invariant, how `Integrator.step` is cut under three
schedules, what is refused, and `temperature_ladder`."""

import numpy as np
import pytest

import _exchange as M


def _decide(*a):
    from torchmd_amd.exchange import exchange_decisions

    return exchange_decisions(*a)


# ----------------------------------------------------------------------------- the decision
def test_a_cold_rung_with_the_higher_energy_always_swaps():
    T = [300.0, 400.0]
    for u in (0.0, 0.5, 1.0 - 2.0**-53):
        # slot 0 on the cold rung holds the higher energy: Delta = (beta_cold - beta_hot) (U_cold - U_hot) > 0
        rungs, acc, delta, pairs = _decide([-90.0, -100.0], T, [0, 1], 0, [u])
        assert list(rungs) == [1, 0] and acc.tolist() == [True] and delta[0] > 0 and pairs.tolist() == [[0, 1]]
        # the same with the slots the other way round: what counts is the rung, not the slot
        rungs, acc, delta, _ = _decide([-100.0, -90.0], T, [1, 0], 0, [u])
        assert list(rungs) == [0, 1] and acc.tolist() == [True] and delta[0] > 0
    want = (1.0 / (M.BOLTZMAN * 300.0) - 1.0 / (M.BOLTZMAN * 400.0)) * 10.0
    assert delta[0] == want
    # the other sign: accepted only below exp(Delta)
    p = np.exp(-want)
    for u, ok in ((0.0, True), (np.nextafter(p, 0), True), (np.nextafter(p, 1), False), (0.999, False)):
        rungs, acc, delta, _ = _decide([-100.0, -90.0], T, [0, 1], 0, [u])
        assert delta[0] == -want and acc.tolist() == [ok] and list(rungs) == ([1, 0] if ok else [0, 1])


def test_parity_pairing():
    want = {(1, 0): [], (1, 1): [], (2, 0): [[0, 1]], (2, 1): [], (3, 0): [[0, 1]], (3, 1): [[1, 2]],
            (4, 0): [[0, 1], [2, 3]], (4, 1): [[1, 2]], (5, 1): [[1, 2], [3, 4]]}
    rng = np.random.default_rng(4)
    for (R, parity), pairs in want.items():
        T = 300.0 * 1.1 ** np.arange(R)
        start = rng.permutation(R)
        U = rng.normal(-100.0, 5.0, R)
        rungs, acc, delta, got = _decide(U, T, start, parity, np.zeros(len(pairs)))  # (u = 0: every pair swaps)
        assert got.tolist() == pairs and got.shape == (len(pairs), 2) and acc.all() and len(delta) == len(pairs)
        assert sorted(rungs) == list(range(R))
        moved = {a for p in pairs for a in p}
        for slot in range(R):
            if start[slot] in moved:
                a = start[slot]
                assert rungs[slot] == (a + 1 if [a, a + 1] in pairs else a - 1)
            else:
                assert rungs[slot] == start[slot]
        assert list(start) == list(start.copy())  # (the input is not changed)
        with pytest.raises(ValueError):
            _decide(U, T, start, parity, np.zeros(len(pairs) + 1))
    with pytest.raises(ValueError):
        _decide([0.0, 0.0], [300.0, 310.0], [0, 0], 0, [0.5])  # (no permutation)


def test_decisions_equal_the_model_and_rungs_stay_a_permutation():
    rng = np.random.default_rng(5)
    for R in (2, 3, 4, 7):
        T = 300.0 * 1.15 ** np.arange(R)
        rungs = rng.permutation(R)
        seen = [0, 0]
        for k in range(300):
            U = rng.normal(-50.0, 3.0, R)
            u = rng.random(len(M.pairs_of(k % 2, R)))
            before = rungs.copy()
            new, acc, delta, pairs = _decide(U, T, rungs, k % 2, u)
            mr, ma, md = M.decide(U, T, rungs, k % 2, u)
            assert np.array_equal(new, mr) and np.array_equal(acc, ma) and np.array_equal(delta, md)
            assert np.array_equal(rungs, before) and sorted(new) == list(range(R))
            seen = [seen[0] + int(acc.sum()), seen[1] + int((~acc).sum())]
            rungs = new
        assert min(seen) > 20  # (both outcomes were exercised)


def test_one_draw_per_tried_pair_and_underflow():
    from torchmd_amd.exchange import ReplicaExchange
    from torchmd_amd.thermostat import VelocityRescale

    ex = ReplicaExchange(frequency=5, seed=1)
    assert ex.frequency == 5 and ex.seed == 1 and ex.rungs is None and ex.last is None and ex.work() is None and ex.history == []
    # exp(Delta) underflows to zero: rejected for every u, 0.0 included, and no exception
    T = [300.0, 301.0]
    rungs, acc, delta, _ = _decide([-1e9, 1e9], T, [0, 1], 0, [0.0])
    assert delta[0] < -745.0 and acc.tolist() == [False] and list(rungs) == [0, 1]
    rungs, acc, delta, _ = _decide([1e9, -1e9], T, [0, 1], 0, [0.999])  # exp would overflow: never evaluated
    assert delta[0] > 745.0 and acc.tolist() == [True]
    # the stream of a seeded object: Philox keyed (seed, 0)
    g = np.random.Generator(np.random.Philox(key=np.array([1, 0], dtype=np.uint64)))
    assert [ex.rng.random() for _ in range(3)] == [g.random() for _ in range(3)]
    # the host half of an attempt (`decide`) draws one number per tried pair even where Delta >= 0 makes it needless
    for R, npairs in ((1, (0, 0)), (2, (1, 0)), (3, (1, 1)), (4, (2, 1)), (5, (2, 2))):
        ex = ReplicaExchange(frequency=5, seed=1)
        ex.rng = M.Counting(0.5)
        ex.bind(VelocityRescale(list(300.0 + 10.0 * np.arange(R))), R)
        assert ex.rungs.tolist() == list(range(R)) and len(ex.attempts) == R - 1 == len(ex.accepted)
        for k in range(4):
            before = ex.rng.count
            # cold rungs hold the higher energies: Delta >= 0 for every pair
            rungs, acc, delta, pairs, u = ex.decide(-100.0 - 5.0 * ex.rungs)
            assert ex.rng.count - before == npairs[k % 2] == len(pairs) == len(u) and acc.all() and (delta >= 0).all()
            assert pairs.tolist() == [list(p) for p in M.pairs_of(k % 2, R)] and (u == 0.5).all()
            ex.rungs, ex.nattempts = rungs, ex.nattempts + 1  # (what `attempt` does with it)
        assert ex.rng.count == 2 * sum(npairs)
    with pytest.raises(RuntimeError, match="rungs"):
        ex.bind(VelocityRescale([300.0, 310.0]), 2)


# ----------------------------------------------------------------------------- the distribution it must leave alone
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_exchange_leaves_the_canonical_distribution_invariant(seed):
    """Four rungs at 300 / 330 / 363 / 400 K.  Every round draws the energy of every slot afresh from the canonical
    distribution of the temperature the slot holds, U = k_B T Gamma(10) (a system of 20 harmonic degrees of freedom), then
    attempts an exchange; the energies collected by rung after the exchange must still be canonical at the rung's temperature:
    <U> = 10 k_B T_a and Var U = 10 (k_B T_a)^2, within four block standard errors (40 000 rounds of alternating parity, the
    first fifth dropped, 20 blocks).  A wrong sign or a wrong beta in Delta shifts both."""
    T = np.array([300.0, 330.0, 363.0, 400.0])
    R, rounds, shape = 4, 40000, 10.0
    rng = np.random.default_rng(seed)
    rungs = np.arange(R)
    by_rung = np.zeros((rounds, R))
    tried, taken = np.zeros(R - 1), np.zeros(R - 1)
    for k in range(rounds):
        U = M.BOLTZMAN * T[rungs] * rng.standard_gamma(shape, R)
        rungs, acc, delta, pairs = _decide(U, T, rungs, k % 2, rng.random(len(M.pairs_of(k % 2, R))))
        by_rung[k, rungs] = U
        tried[pairs[:, 0]] += 1
        taken[pairs[acc, 0]] += 1
    worst = 0.0
    for a in range(R):
        kT = M.BOLTZMAN * T[a]
        mean, emean, var, evar = M.block_statistics(by_rung[rounds // 5:, a])
        dev = max(abs(mean - shape * kT) / emean, abs(var - shape * kT * kT) / evar)
        worst = max(worst, dev)
        print(f"seed {seed} rung {a} ({T[a]:.0f} K): <U> = {mean:.5f} +- {emean:.5f} (expected {shape * kT:.5f}), "
              f"Var U = {var:.6f} +- {evar:.6f} (expected {shape * kT * kT:.6f}): {dev:.2f} standard errors")
        assert abs(mean - shape * kT) <= 4 * emean and abs(var - shape * kT * kT) <= 4 * evar, (a, mean, emean, var, evar)
    rate = taken / tried
    print(f"seed {seed}: worst deviation {worst:.2f} standard errors, acceptance {rate}")
    assert (rate > 0.05).all() and (rate < 0.95).all(), rate


# ----------------------------------------------------------------------------- cutting step() under three schedules
def test_step_is_cut_at_the_union_of_three_schedules():
    from torchmd_amd.integrator import cut_schedules

    freqs = (10, 25, 40)
    nstep, events = 0, {0: [], 1: [], 2: []}
    for niter in (7, 13, 30, 1, 49, 100, 3, 22, 25, 150):
        segs = cut_schedules(nstep, niter, freqs)
        assert sum(n for n, _ in segs) == niter and all(n > 0 for n, _ in segs)
        done = 0
        for n, hit in segs:
            done += n
            assert len(hit) == 3
            for k, f in enumerate(freqs):
                assert hit[k] == ((nstep + done) % f == 0)
                if hit[k]:
                    events[k].append(nstep + done)
        assert all(any(hit) for _, hit in segs[:-1])  # no needless cuts
        nstep += niter
    assert nstep == 400
    for k, f in enumerate(freqs):
        assert events[k] == list(range(f, 401, f))


# ----------------------------------------------------------------------------- what is refused
def test_refusals_and_the_ladder(tmp_path):
    import torch

    import torchmd_amd
    from _golden import GoldenParameters, load
    from torchmd_amd import run as driver
    from torchmd_amd.barostat import MonteCarloBarostat
    from torchmd_amd.exchange import ReplicaExchange, temperature_ladder
    from torchmd_amd.forces import Forces
    from torchmd_amd.integrator import Integrator
    from torchmd_amd.systems import System
    from torchmd_amd.thermostat import VelocityRescale

    assert torchmd_amd.ReplicaExchange is ReplicaExchange and torchmd_amd.temperature_ladder is temperature_ladder
    assert ReplicaExchange().frequency == 500
    for bad in (0, -5, 2.5, "10", None):
        with pytest.raises(ValueError, match="frequency"):
            ReplicaExchange(frequency=bad)
    assert ReplicaExchange(frequency=20.0).frequency == 20

    g = load("water291")
    par = GoldenParameters(g, torch.float32)
    f = Forces(par, terms=["lj", "electrostatics", "bonds", "angles"], cutoff=7.3, rfa=True)
    s = System(291, 3, torch.float32, "cpu")
    s.set_box(g["box"])
    lad = [280.0, 300.0, 320.0]
    it = Integrator(s, f, 1.0, "cpu", thermostat=VelocityRescale(lad), exchange=ReplicaExchange(20))
    assert it.exchange.frequency == 20 and Integrator(s, f, 1.0, "cpu").exchange is None
    with pytest.raises(ValueError, match="VelocityRescale"):  # no thermostat
        Integrator(s, f, 1.0, "cpu", exchange=ReplicaExchange(20))
    with pytest.raises(ValueError, match="VelocityRescale"):  # Langevin
        Integrator(s, f, 1.0, "cpu", gamma=1.0, T=300.0, exchange=ReplicaExchange(20))
    with pytest.raises(ValueError, match="sequence"):  # one temperature for all
        Integrator(s, f, 1.0, "cpu", thermostat=VelocityRescale(300.0), exchange=ReplicaExchange(20))
    with pytest.raises(ValueError, match="replicas"):  # a ladder of the wrong length
        Integrator(s, f, 1.0, "cpu", thermostat=VelocityRescale([280.0, 300.0]), exchange=ReplicaExchange(20))
    for notup in ([280.0, 320.0, 300.0], [300.0, 300.0, 320.0], [320.0, 300.0, 280.0]):
        with pytest.raises(ValueError, match="increasing"):
            Integrator(s, f, 1.0, "cpu", thermostat=VelocityRescale(notup), exchange=ReplicaExchange(20))
    with pytest.raises(ValueError, match="batch"):
        Integrator(s, f, 1.0, "cpu", batch=torch.zeros(291, dtype=torch.int64), thermostat=VelocityRescale(lad),
                   exchange=ReplicaExchange(20))
    bar = MonteCarloBarostat(1.0, 300.0)
    with pytest.raises(ValueError, match="barostat"):
        Integrator(s, f, 1.0, "cpu", thermostat=VelocityRescale(lad), barostat=bar, exchange=ReplicaExchange(20))
    with pytest.raises(ValueError, match="barostat"):  # (equal temperatures pass the thermostat's own check of a barostat)
        Integrator(s, f, 1.0, "cpu", thermostat=VelocityRescale([300.0] * 3), barostat=bar, exchange=ReplicaExchange(20))
    ex = ReplicaExchange(20)
    ex.frequency = 2.5  # (set after construction)
    with pytest.raises(ValueError, match="frequency"):
        Integrator(s, f, 1.0, "cpu", thermostat=VelocityRescale(lad), exchange=ex)

    # the ladder: exact end points, a constant ratio
    t = temperature_ladder(300.0, 400.0, 4)
    assert t[0] == 300.0 and t[-1] == 400.0 and len(t) == 4 and (np.diff(t) > 0).all()
    assert np.allclose(t[1:] / t[:-1], (400.0 / 300.0) ** (1.0 / 3.0), rtol=1e-14)
    assert np.allclose(t, [300.0, 330.19, 363.42, 400.0], atol=0.01)
    assert temperature_ladder(300.0, 300.0, 1).tolist() == [300.0] and temperature_ladder(280.0, 320.0, 2).tolist() == [280.0, 320.0]
    for bad in ((300.0, 400.0, 0), (400.0, 300.0, 3), (0.0, 300.0, 3), (300.0, 300.0, 2), (300.0, 400.0, 2.5)):
        with pytest.raises(ValueError):
            temperature_ladder(*bad)
    Integrator(s, f, 1.0, "cpu", thermostat=VelocityRescale(temperature_ladder(280.0, 320.0, 3)), exchange=ReplicaExchange(20))

    # run.py: the keys, their defaults, and what they need
    base = ["--log-dir", str(tmp_path / "a"), "--steps", "100", "--output-period", "10"]
    args = driver.get_args(base)
    assert args.exchange_frequency is None and args.exchange_seed is None
    csvr = ["--thermostat", "csvr", "--thermostat-temperature", "280,300"]
    args = driver.get_args(base + csvr + ["--exchange-frequency", "50", "--exchange-seed", "7"])
    assert args.exchange_frequency == 50 and args.exchange_seed == 7
    conf = tmp_path / "conf.yaml"
    conf.write_text(f"thermostat: csvr\nthermostat_temperature: [280, 300, 320]\nexchange_frequency: 40\nsteps: 100\n"
                    f"output_period: 10\nlog_dir: {tmp_path / 'b'}\n")
    args = driver.get_args(["--conf", str(conf)])
    assert args.exchange_frequency == 40 and args.exchange_seed is None
    with pytest.raises(ValueError, match="csvr"):
        driver.get_args(base + ["--exchange-frequency", "50"])
    with pytest.raises(ValueError, match="list"):
        driver.get_args(base + ["--thermostat", "csvr", "--thermostat-temperature", "300", "--exchange-frequency", "50"])
    with pytest.raises(ValueError, match="positive"):
        driver.get_args(base + csvr + ["--exchange-frequency", "0"])
