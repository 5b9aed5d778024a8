"""CPU tests (no GPU) of the Monte Carlo barostat: the C symbol, the acceptance arithmetic, how `Integrator.step` is cut
into segments, the host model of the volume chain against the ideal-gas law, and the driver's two configuration keys."""

import os
import re

import numpy as np
import pytest

import _barostat as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_scale_groups_is_exported_and_the_abi_constant_matches():
    from torchmd_amd import _lib

    header = open(os.path.join(ROOT, "include", "tmdhip.h")).read()
    assert "tmdhip_scale_groups" in set(re.findall(r"\b(tmdhip_[a-z0-9_]+)\s*\(", header))
    assert int(re.search(r"#define\s+TMDHIP_ABI_VERSION\s+(\d+)", header).group(1)) == _lib.ABI_VERSION == 11
    assert "tmdhip_scale_groups" in _lib.SIGNATURES
    lib = _lib.load()
    assert hasattr(lib, "tmdhip_scale_groups") and lib.tmdhip_abi_version() == _lib.ABI_VERSION
    # argument validation happens before any HIP call
    assert lib.tmdhip_scale_groups(7, 1, 1, None, None, None, 1, None, None, 0, None) < 0 and "dtype" in _lib.last_error()
    assert lib.tmdhip_scale_groups(_lib.F32, 1, 3, None, None, None, 1, None, None, 0, None) < 0 and "null" in _lib.last_error()
    assert lib.tmdhip_scale_groups(_lib.F32, 0, 3, None, None, None, 1, None, None, 0, None) < 0


def test_acceptance_weight_by_hand():
    from torchmd_amd import barostat as bar
    from torchmd_amd.integrator import BOLTZMAN

    # 1 bar = 1e5 J/m^3 = 1e5 * 1e-30 J/A^3; per mole and in kcal: N_A * 1e-25 / 4184
    factor = 6.02214076e23 * 1e-25 / 4184.0
    assert abs(factor - 1.4393e-5) < 1e-9
    assert abs(bar.BAR_TO_KCAL_MOL_A3 - factor) <= 1e-12 * factor
    assert BOLTZMAN == 0.001987191
    # a compression of 100 A^3 at 1 000 bar, 300 K, 216 molecules, the energy rising by 2.5 kcal/mol:
    #   dU = 2.5;  P dV = 1000 * 1.43932618546845e-5 * (-100) = -1.43932618546845
    #   ln(V'/V) = ln(269/270) = -(x + x^2/2 + x^3/3 + x^4/4 + ...), x = 1/270:
    #     0.0037037037037 + 0.0000068587106 + 0.0000000169351 + 0.0000000000470 = 0.0037105793964
    #   N kT ln(V'/V) = 216 * 0.5961573 * (-0.0037105793964) = 128.7699768 * (-0.0037105793964) = -0.4778112228
    #   w = 2.5 - 1.4393261855 + 0.4778112228 = 1.5384850373
    U, Un, V, Vn, N, P, T = -2000.0, -1997.5, 27000.0, 26900.0, 216, 1000.0, 300.0
    kT = 0.001987191 * 300.0
    assert abs(kT - 0.5961573) < 1e-12
    x = 1.0 / 270.0
    ln = -sum(x ** k / k for k in range(1, 12))
    assert abs(ln + 0.0037105793964) < 1e-12
    by_hand = 2.5 + 1000.0 * factor * (-100.0) - 216 * kT * ln
    assert abs(by_hand - 1.5384850373) < 1e-9
    w = bar.acceptance_weight(U, Un, V, Vn, N, P, T)
    assert abs(w - by_hand) <= 1e-12 * abs(by_hand), (w, by_hand)
    # an expansion of an ideal gas at the pressure where V is the most probable volume of exp(-w/kT) V^0: w ~ 0 to first order
    N, V = 64, 27000.0
    P = N * kT / V / factor
    w = bar.acceptance_weight(0.0, 0.0, V, V + 1.0, N, P, T)
    assert abs(w - (N * kT / V - N * kT * np.log1p(1.0 / V))) <= 1e-12 * N * kT / V
    assert 0 < w < 1e-6
    # vectorised over replicas, as `attempt` uses it
    w2 = bar.acceptance_weight(np.array([U, 0.0]), np.array([Un, 0.0]), np.array([27000.0, V]), np.array([Vn, V + 1.0]), np.array([216, 64]),
                               np.array([1000.0, P]), T)
    assert abs(w2[0] - by_hand) <= 1e-12 * abs(by_hand) and abs(w2[1] - w) <= 1e-12 * w


def test_step_is_cut_on_multiples_of_the_frequency():
    from torchmd_amd.integrator import cut_segments

    for nstep in (0, 7, 25):
        for niter in (1, 20, 25, 60):
            segs = cut_segments(nstep, niter, 25)
            assert sum(n for n, _ in segs) == niter and all(n > 0 for n, _ in segs)
            at, attempts = nstep, []
            for n, attempt in segs:
                at += n
                assert attempt == (at % 25 == 0), (nstep, niter, segs)
                if attempt:
                    attempts.append(at)
            # every multiple of 25 in (nstep, nstep + niter] is hit, and nothing else
            assert attempts == [m for m in range(nstep + 1, nstep + niter + 1) if m % 25 == 0], (nstep, niter, segs)
    assert cut_segments(0, 60, 25) == [(25, True), (25, True), (10, False)]
    assert cut_segments(7, 20, 25) == [(18, True), (2, False)]
    assert cut_segments(25, 1, 25) == [(1, False)]


def test_host_model_of_the_volume_chain_obeys_the_ideal_gas_law():
    """PV = (N + 1) k_B T for N non-interacting molecules under this barostat: the density of V is Gamma(N + 1, kT/P)."""
    N, T, target = 64, 300.0, 27000.0
    P = (N + 1) * B.BOLTZMAN * T / target / B.BAR
    edge = 20000.0 ** (1.0 / 3.0)
    worst, widths = 0.0, []
    for seed in range(6):
        vols, flags = B.volume_chain([edge] * 3, N, P, T, 8000, np.random.default_rng(seed))
        mean, se, width = B.block_stats(vols)
        worst = max(worst, abs(mean - target) / se)
        widths.append(width)
        assert 0.2 < flags.mean() < 0.8  # the step size adapts towards 25-75 % acceptance
    print(f"host model, 6 seeds: worst |<V> - 27000| = {worst:.2f} block standard errors, sigma/<V> = {min(widths):.4f} .. {max(widths):.4f}")
    assert worst <= 5.0
    assert all(abs(w * np.sqrt(N + 1) - 1.0) <= 0.15 for w in widths)
    # the barostat's own per-replica stream: replica r's numbers do not depend on the replicas beside it
    a, b = B.philox_stream(5, 1), B.philox_stream(5, 1)
    assert [a.random() for _ in range(4)] == [b.random() for _ in range(4)]
    assert B.philox_stream(5, 0).random() != B.philox_stream(5, 1).random()


def test_barostat_constructor_and_run_py_keys(tmp_path):
    from torchmd_amd import run as driver
    from torchmd_amd.barostat import MonteCarloBarostat

    with pytest.raises(ValueError):
        MonteCarloBarostat(1.0, 0.0)
    with pytest.raises(ValueError):
        MonteCarloBarostat(1.0, 300.0, frequency=0)
    b = MonteCarloBarostat(1.0, 300.0, seed=3)
    assert b.frequency == 25 and b.seed == 3 and b.pressure_bar == 1.0 and b.last is None

    base = ["--log-dir", str(tmp_path / "a"), "--steps", "100", "--output-period", "10"]
    args = driver.get_args(base)
    assert args.barostat_pressure is None and args.barostat_frequency == 25
    args = driver.get_args(base + ["--barostat-pressure", "1.5", "--barostat-frequency", "50"])
    assert args.barostat_pressure == 1.5 and args.barostat_frequency == 50
    conf = tmp_path / "conf.yaml"
    conf.write_text(f"barostat_pressure: 1\nbarostat_frequency: 10\nsteps: 100\noutput_period: 10\nlog_dir: {tmp_path / 'b'}\n")
    args = driver.get_args(["--conf", str(conf)])
    assert args.barostat_pressure == 1.0 and isinstance(args.barostat_pressure, float) and args.barostat_frequency == 10
    with pytest.raises(ValueError):
        driver.get_args(base + ["--barostat-pressure", "1", "--barostat-frequency", "-5"])
    with pytest.raises(ValueError):
        driver.get_args(base + ["--barostat-frequency", "0"])


def test_integrator_refuses_what_the_barostat_cannot_serve():
    import torch

    from _golden import GoldenParameters, load
    from torchmd_amd.barostat import MonteCarloBarostat
    from torchmd_amd.forces import Forces
    from torchmd_amd.integrator import Integrator
    from torchmd_amd.systems import System

    g = load("water291")
    par = GoldenParameters(g, torch.float32)
    f = Forces(par, terms=["lj", "electrostatics", "bonds", "angles"], cutoff=7.3, rfa=True)
    s = System(291, 1, torch.float32, "cpu")
    s.set_box(g["box"])
    bar = MonteCarloBarostat(1.0, 300.0)
    with pytest.raises(ValueError, match="thermostat"):
        Integrator(s, f, 1.0, "cpu", barostat=bar)  # no T
    Integrator(s, f, 1.0, "cpu", gamma=1.0, T=300.0, barostat=bar)
    s.set_box(np.array([0.0, 0.0, 0.0]))
    with pytest.raises(ValueError, match="periodic"):
        Integrator(s, f, 1.0, "cpu", gamma=1.0, T=300.0, barostat=bar)

    class Duck:
        def compute(self, pos, box, forces):
            return [0.0]

    s.set_box(g["box"])
    s.set_masses(par.masses.reshape(-1))
    with pytest.raises(ValueError, match="Forces"):
        Integrator(s, Duck(), 1.0, "cpu", gamma=1.0, T=300.0, barostat=bar)
