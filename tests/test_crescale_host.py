"""The stochastic cell-rescaling barostat without a GPU: the host build of crescale_math.h against the numpy model
of tests/_crescale.py, the model's Euler chain for an ideal gas against the analytic NPT volume distribution, the units, what
Python refuses, and the random streams.

Bars.  Header against model: the same IEEE operations up to the association of a product and the last bit of exp / sqrt: 4 eps64
of the magnitude of the terms.  A molecule moved by the header's loops against the model's vectorised sums: the shift is formed
from at most 65 addends, (n + 4) eps64 max|x| on top of one rounding to the storage precision.

Euler chain (64 atoms, (N + 1) kT / P0 = 27 000 A^3, beta = 1 / P0, dt_p / tau_p = 0.1, Langevin gamma dt_p = 1, 80 000
applications, first fifth discarded, seed 0): <V> / 27 000 - 1 = +0.0019 (block error 0.0034), sigma_V / <V> = 0.1287 (block
error 0.0010) against 1 / sqrt(65) = 0.1240.  Each must lie within 4 of its own block standard errors plus 0.5 % of the analytic
value.  The bar of the width has no room to spare: the Euler step of eps widens the distribution by a bias of O(dt_p / tau_p),
here +0.0047, that no longer run removes, against a bar of 0.0048 of which 0.0042 is the block error (a longer run narrows the
bar, not the bias).  The run is deterministic (numpy's seeded Generator); a change of the model's draw order or of numpy's
streams can move the estimate across the bar without anything being wrong."""

import ctypes as C
import os
import shutil
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import _crescale as M

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "torchmd_amd", "csrc")
EPS64 = np.finfo(np.float64).eps
SRC = os.path.join(HERE, "crescale_math_host.cpp")


def _toolchain():
    from torchmd_amd import _build

    cxx = next((c for c in (os.environ.get("CXX"), "g++", "c++", "clang++") if c and shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler (CXX, g++, c++, clang++) found: crescale_math.h is not checked on the CPU")
    try:
        hipcc = _build._hipcc()
    except RuntimeError:
        hipcc = None
    inc = None
    for root in ((os.path.dirname(os.path.dirname(os.path.realpath(hipcc))),) if hipcc else ()) + ("/opt/rocm",):
        if os.path.exists(os.path.join(root, "include", "hip", "hip_runtime.h")):
            inc = os.path.join(root, "include")
            break
    if inc is None:
        pytest.skip("the HIP headers (hip/hip_runtime.h) of a ROCm installation were not found: crescale_math.h is not checked on the CPU")
    return [cxx, "-std=c++17", "-O2", "-ffp-contract=off", "-D__HIP_PLATFORM_AMD__", f"-I{inc}", f"-I{CSRC}"]


@pytest.fixture(scope="module")
def cm(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("crescale_math") / "libcrescale_math_host.so")
    cmd = _toolchain() + ["-fPIC", "-shared", SRC, "-o", out]
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, " ".join(cmd) + "\n" + res.stdout + res.stderr
    lib = C.CDLL(out)
    dp, fp = C.POINTER(C.c_double), C.POINTER(C.c_float)
    lib.cm_delta_eps.restype = lib.cm_mu.restype = lib.cm_shift_pos.restype = lib.cm_shift_vel.restype = C.c_double
    lib.cm_delta_eps.argtypes = [C.c_double] * 7 + [C.c_int]
    lib.cm_mu.argtypes = [C.c_double]
    lib.cm_shift_pos.argtypes = lib.cm_shift_vel.argtypes = [C.c_double] * 3
    lib.cm_move_f64.restype = lib.cm_move_f32.restype = None
    lib.cm_move_f64.argtypes = [C.c_int, dp, dp, dp, dp, dp]
    lib.cm_move_f32.argtypes = [C.c_int, fp, fp, fp, dp, dp]
    return lib


def _p(a, t):
    return a.ctypes.data_as(C.POINTER(t))


# ---------------------------------------------------------------- the compiled header
def test_header_step_of_ln_v_equals_model(cm):
    rng = np.random.default_rng(0)
    worst = 0.0
    for _ in range(2000):
        beta = 10.0 ** rng.uniform(2, 5)  # A^3 mol / kcal: 4.5e-5 / bar is 3.1e3
        dtt = 10.0 ** rng.uniform(-3, -0.5)
        p0, pint = rng.normal() * 1e-3, rng.normal() * 1e-2
        kT, vol, xi = rng.uniform(0.2, 1.0), 10.0 ** rng.uniform(3, 7), rng.normal()
        for stochastic in (0, 1):
            want = M.delta_eps(p0, pint, vol, kT, beta, dtt, xi, bool(stochastic))
            got = cm.cm_delta_eps(beta, dtt, p0, pint, kT, vol, xi, stochastic)
            scale = beta * dtt * (abs(p0) + abs(pint)) + stochastic * np.sqrt(2 * kT * beta * dtt / vol) * abs(xi)
            worst = max(worst, abs(got - want) / (EPS64 * scale))
            de = float(np.clip(want, -0.5, 0.5))
            worst = max(worst, abs(cm.cm_mu(de) - M.mu_of(de)) / (EPS64 * M.mu_of(de)))
        # without noise the draw does not matter
        assert cm.cm_delta_eps(beta, dtt, p0, pint, kT, vol, xi, 0) == cm.cm_delta_eps(beta, dtt, p0, pint, kT, vol, -7.0, 0)
        s, sm, smx = rng.uniform(0.9, 1.1), rng.uniform(1, 500), rng.normal() * 1e4
        worst = max(worst, abs(cm.cm_shift_pos(s, smx, sm) - (s - 1.0) * (smx / sm)) / (EPS64 * abs((s - 1.0) * smx / sm)))
        worst = max(worst, abs(cm.cm_shift_vel(s, smx, sm) - (1.0 / s - 1.0) * (smx / sm)) / (EPS64 * abs((1.0 / s - 1.0) * smx / sm)))
    print(f"header against model: worst {worst:.2f} eps64 of the scale")
    assert worst <= 4
    assert cm.cm_mu(0.0) == 1.0 and cm.cm_shift_pos(1.0, 123.0, 4.0) == 0.0 and cm.cm_shift_vel(1.0, 123.0, 4.0) == 0.0


def _ulp(x, dtype):
    return np.spacing(np.abs(np.asarray(x, dtype=np.float64)).astype(dtype)).astype(np.float64)


def _check_move(n, pos, vel, mass, s, got_pos, got_vel, k, dtype, massless=()):
    """`got_*` against the model for one molecule: one rounding plus the summation error of the shift; K against the model."""
    off, mem = np.array([0, n]), np.arange(n)
    wp, wv = M.rescale_molecules(pos, vel, mass, s, off, mem)
    tol_p = _ulp(wp, dtype) * (dtype != np.float64) + (n + 4) * EPS64 * np.abs(pos).max()
    tol_v = _ulp(wv, dtype) * (dtype != np.float64) + (n + 4) * EPS64 * np.abs(vel).max()
    assert (np.abs(got_pos - wp) <= tol_p).all() and (np.abs(got_vel - wv) <= tol_v).all()
    for a in massless:
        assert np.array_equal(got_vel[a], vel[a])
    kb, sb = M.kinetic(mass, vel)
    ka, sa = M.kinetic(mass, got_vel)
    assert abs(k[0] - kb) <= (n + 4) * EPS64 * sb and abs(k[1] - ka) <= (n + 4) * EPS64 * sa
    # rigid: distance vectors and relative velocities inside the molecule change by roundings only
    for new, old, dt in ((got_pos, pos, dtype), (got_vel, vel, dtype)):
        w = [a for a in range(n) if a not in massless] if new is got_vel else list(range(n))
        d_new, d_old = new[w] - new[w[0]], old[w] - old[w[0]]
        assert (np.abs(d_new - d_old) <= 2 * _ulp(np.abs(old).max(), dt) + (n + 4) * EPS64 * np.abs(old).max()).all()


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_header_moves_a_molecule_as_the_model(cm, dtype):
    rng = np.random.default_rng(1)
    for n, massless in ((1, ()), (3, ()), (4, (3,)), (64, ()), (65, ())):
        pos = rng.uniform(0, 40, (n, 3)).astype(dtype)
        vel = (rng.normal(size=(n, 3)) * 0.01).astype(dtype)
        mass = rng.uniform(1, 16, n).astype(dtype)
        mass[list(massless)] = 0
        vel[list(massless)] = np.inf  # (what a Maxwell-Boltzmann draw leaves on a massless row: never read)
        s = np.array([1.002, 0.9991, 1.0])
        gp, gv, k = pos.copy(), vel.copy(), np.zeros(2)
        t = C.c_double if dtype == np.float64 else C.c_float
        (cm.cm_move_f64 if dtype == np.float64 else cm.cm_move_f32)(n, _p(gp, t), _p(gv, t), _p(mass, t), _p(s, C.c_double), _p(k, C.c_double))
        safe = vel.astype(np.float64).copy()
        safe[list(massless)] = 0.0
        got_v = gv.astype(np.float64)
        assert all(np.isinf(got_v[a]).all() for a in massless)
        got_v[list(massless)] = 0.0
        _check_move(n, pos.astype(np.float64), safe, mass.astype(np.float64), s, gp.astype(np.float64), got_v, k, dtype, massless)
        assert np.array_equal(gp[:, 2], pos[:, 2])  # a factor of exactly 1 shifts by exactly 0
        # all three factors 1: nothing moves, K_after is K_before
        gp2, gv2, one = pos.copy(), vel.copy(), np.ones(3)
        (cm.cm_move_f64 if dtype == np.float64 else cm.cm_move_f32)(n, _p(gp2, t), _p(gv2, t), _p(mass, t), _p(one, C.c_double), _p(k, C.c_double))
        assert np.array_equal(gp2, pos) and np.array_equal(gv2, vel) and k[0] == k[1]


def test_stand_alone_program_under_the_host_sanitizers(tmp_path):
    """crescale_math_host.cpp with its own main, built with -fsanitize=address,undefined where the compiler has them (a plain
    build otherwise), run as a process of its own; its output is checked against the model."""
    base = _toolchain() + ["-DCRESCALE_HOST_MAIN", "-g", SRC, "-o", str(tmp_path / "crescale_host")]
    res = subprocess.run(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"], capture_output=True, text=True)
    sanitized = res.returncode == 0
    if not sanitized:
        res = subprocess.run(base, capture_output=True, text=True)
        assert res.returncode == 0, res.stdout + res.stderr
    # (the leak checker needs ptrace, which a container may not grant: bounds, use after free and undefined behaviour are what is asked)
    run = subprocess.run([str(tmp_path / "crescale_host")], capture_output=True, text=True, timeout=60,
                         env={**os.environ, "ASAN_OPTIONS": "detect_leaks=0"})
    print("sanitizers:", sanitized)
    assert run.returncode == 0 and not run.stderr.strip(), run.stderr
    lines = run.stdout.strip().splitlines()
    de, mu = (float.fromhex(x) for x in lines[0].split())
    want = M.delta_eps(1.4e-5, -3.0e-3, 27000.0, 0.596, 3000.0, 0.02, 0.7)
    assert abs(de - want) <= 4 * EPS64 * abs(want) and abs(mu - M.mu_of(want)) <= 4 * EPS64
    state = 12345

    def nxt():
        nonlocal state
        state = (state * 6364136223846793005 + 1442695040888963407) % 2**64
        return (state >> 11) / 9007199254740992.0

    s = np.array([1.001, 0.9985, 1.0])
    assert [int(line.split()[0]) for line in lines[1:]] == [1, 3, 4, 65]
    for line in lines[1:]:
        tok = line.split()
        n = int(tok[0])
        vals = np.array([float.fromhex(x) for x in tok[1:]])
        assert len(vals) == 6 * n + 2
        pos, vel, mass = np.zeros((n, 3)), np.zeros((n, 3)), np.zeros(n)
        for a in range(n):
            mass[a] = 0.0 if (n == 4 and a == 3) else 1.0 + 15.0 * nxt()
            for c in range(3):
                pos[a, c] = 40.0 * nxt()
                vel[a, c] = 0.02 * (nxt() - 0.5)
        _check_move(n, pos, vel, mass, s, vals[: 3 * n].reshape(n, 3), vals[3 * n: 6 * n].reshape(n, 3), vals[6 * n:], np.float64,
                    massless=(3,) if n == 4 else ())


# ---------------------------------------------------------------- the model's chain
def test_euler_chain_of_an_ideal_gas_samples_the_npt_volume_distribution():
    N, V0 = 64, 27000.0
    v = M.ideal_gas_chain(80000, natoms=N, mean_volume=V0, dt_over_tau=0.1, gamma_dt=1.0, seed=0)
    mean, se, rel, rel_se = M.block_stats(v[len(v) // 5:], 10)
    want_rel = 1.0 / np.sqrt(N + 1)
    print(f"<V> / {V0:.0f} - 1 = {mean / V0 - 1:+.4f} (block error {se / V0:.4f}); sigma / <V> = {rel:.4f} (block error {rel_se:.4f}), "
          f"analytic {want_rel:.4f}")
    assert abs(mean - V0) <= 4 * se + 0.005 * V0
    assert abs(rel - want_rel) <= 4 * rel_se + 0.005 * want_rel


# ---------------------------------------------------------------- units
def test_units():
    from torchmd_amd import crescale as X
    from torchmd_amd.barostat import BAR_TO_KCAL_MOL_A3
    from torchmd_amd.integrator import BOLTZMAN, PICOSEC2TIMEU, TIMEFACTOR

    # 1 bar = 1e5 Pa = 1e5 J / m^3 = 1e-25 J / A^3; kcal/mol = 4184 J / N_A
    assert abs(BAR_TO_KCAL_MOL_A3 - 1e5 * 1e-30 * 6.02214076e23 / 4184.0) <= 2 * EPS64 * BAR_TO_KCAL_MOL_A3
    assert M.BAR_TO_KCAL_MOL_A3 == BAR_TO_KCAL_MOL_A3 and M.BOLTZMAN == BOLTZMAN and M.PICOSEC2TIMEU == PICOSEC2TIMEU
    b = X.CRescaleBarostat([1.0, 250.0], 300.0, tau=2.0, compressibility=4.5e-5, frequency=10)
    p0, kT, beta = b.targets(2)
    assert np.array_equal(p0, np.array([1.0, 250.0]) * BAR_TO_KCAL_MOL_A3) and np.array_equal(kT, np.full(2, BOLTZMAN * 300.0))
    assert np.array_equal(beta, np.full(2, 4.5e-5 / BAR_TO_KCAL_MOL_A3))
    # beta P is a pure number: 4.5e-5 / bar times 1000 bar
    assert abs(beta[0] * 1000.0 * BAR_TO_KCAL_MOL_A3 - 0.045) <= 4 * EPS64
    # 10 steps of 2 fs against 2 ps: dt_p / tau_p = 0.01, whatever the integrator's time unit is
    dt = 2.0 / TIMEFACTOR
    assert abs(b.dt_over_tau(dt) - 0.01) <= 4 * EPS64 * 0.01
    # the package's step of ln V is the model's, bit for bit (the integrator test compares runs for equality)
    rng = np.random.default_rng(2)
    for stochastic in (True, False):
        a = [rng.normal(size=5) * 1e-3, rng.normal(size=5) * 1e-2, rng.uniform(1e3, 1e6, 5), rng.uniform(0.3, 0.9, 5),
             rng.uniform(1e3, 1e4, 5), 0.02, rng.normal(size=5)]
        assert np.array_equal(X.delta_epsilon(*a, stochastic), M.delta_eps(*a, stochastic))
    # water at 1000 bar above target, dt_p / tau_p = 0.01: the box grows by beta dP dt_p / tau_p / 3 = 1.5e-4 per edge
    mu = M.mu(1.0, 1001.0 * BAR_TO_KCAL_MOL_A3, 27000.0, 300.0, 4.5e-5, 2.0, 10, dt, 0.0, stochastic=False)
    assert abs(mu - 1.0 - 1.5e-4) < 2e-8


# ---------------------------------------------------------------- Python
def test_constructor_and_public_surface(tmp_path):
    import torchmd_amd
    from torchmd_amd import _lib, run as driver
    from torchmd_amd.crescale import CRescaleBarostat

    assert torchmd_amd.CRescaleBarostat is CRescaleBarostat and "CRescaleBarostat" in torchmd_amd.__all__
    b = CRescaleBarostat(1.0, 300.0, seed=3)
    assert (b.tau, b.frequency, b.stochastic, b.seed, b.applications) == (1.0, 10, True, 3, 0)
    assert b.compressibilities.tolist() == [4.5e-5] and b.last is None and b.work() is None and b.rng is None
    for bad in (dict(pressure_bar=np.nan), dict(temperature=0.0), dict(temperature=[300.0, -1.0]), dict(compressibility=0.0),
                dict(compressibility=[4.5e-5, np.inf]), dict(tau=0.0), dict(tau=np.nan), dict(frequency=0), dict(frequency=2.5),
                dict(pressure_bar=[]), dict(temperature=[[300.0]])):
        with pytest.raises(ValueError):
            CRescaleBarostat(**{**dict(pressure_bar=1.0, temperature=300.0), **bad})
    assert CRescaleBarostat(-50.0, 300.0).pressures_bar.tolist() == [-50.0]  # (tension is a valid target)
    with pytest.raises(ValueError, match="3 replicas"):
        CRescaleBarostat([1.0, 2.0], 300.0).targets(3)
    assert "tmdhip_rescale_molecules" in _lib.SIGNATURES and "tmdhip_rescale_molecules_workspace" in _lib.SIGNATURES
    assert _lib.ABI_VERSION == 11
    header = open(os.path.join(os.path.dirname(HERE), "include", "tmdhip.h")).read()
    assert "tmdhip_rescale_molecules(" in header and "#define TMDHIP_ABI_VERSION 11" in header
    # run.py: the keys and their defaults
    base = ["--log-dir", str(tmp_path / "a"), "--steps", "100", "--output-period", "10"]
    args = driver.get_args(base)
    assert (args.barostat, args.barostat_tau, args.barostat_compressibility, args.barostat_pressure) == ("montecarlo", 1.0, 4.5e-5, None)
    args = driver.get_args(base + ["--barostat", "crescale", "--barostat-tau", "0.5", "--barostat-compressibility", "5e-5",
                                   "--barostat-pressure", "1"])
    assert (args.barostat, args.barostat_tau, args.barostat_compressibility, args.barostat_pressure) == ("crescale", 0.5, 5e-5, 1.0)
    conf = tmp_path / "conf.yaml"
    conf.write_text(f"barostat: crescale\nbarostat_pressure: 1\nbarostat_tau: 2\nsteps: 100\noutput_period: 10\nlog_dir: {tmp_path / 'b'}\n")
    args = driver.get_args(["--conf", str(conf)])
    assert args.barostat == "crescale" and args.barostat_tau == 2.0 and isinstance(args.barostat_tau, float)
    with pytest.raises(ValueError, match="barostat must be"):
        driver.get_args(base + ["--barostat", "berendsen"])


def _water291(R=1, **extra):
    from _golden import GoldenParameters, load
    from torchmd_amd.forces import Forces
    from torchmd_amd.systems import System

    g = load("water291")
    par = GoldenParameters(g, torch.float32)
    f = Forces(par, terms=["lj", "electrostatics", "bonds", "angles"], cutoff=7.3, rfa=True, **extra)
    s = System(291, R, torch.float32, "cpu")
    s.set_box(g["box"])
    return g, par, f, s


def test_integrator_refuses_what_the_barostat_cannot_serve():
    from torchmd_amd.crescale import CRescaleBarostat
    from torchmd_amd.domain import DomainSet
    from torchmd_amd.exchange import ReplicaExchange
    from torchmd_amd.integrator import Integrator
    from torchmd_amd.metadynamics import Metadynamics
    from torchmd_amd.restraints import Restraints
    from torchmd_amd.thermostat import VelocityRescale

    g, par, f, s = _water291(2)

    def bar(**kw):
        return CRescaleBarostat(**{**dict(pressure_bar=1.0, temperature=300.0, seed=1), **kw})

    # what is served: Langevin, a rescaling thermostat, a ladder that the barostat's temperatures equal, no thermostat without noise
    Integrator(s, f, 1.0, "cpu", gamma=1.0, T=300.0, barostat=bar())
    Integrator(s, f, 1.0, "cpu", thermostat=VelocityRescale(300.0), barostat=bar())
    it = Integrator(s, f, 1.0, "cpu", thermostat=VelocityRescale([290.0, 310.0]), barostat=bar(temperature=[290.0, 310.0],
                                                                                                pressure_bar=[1.0, 100.0]))
    assert it.barostat.virial_driven and it._virial_barostat
    Integrator(s, f, 1.0, "cpu", barostat=bar(stochastic=False))
    # what is not
    with pytest.raises(ValueError, match="thermostat"):
        Integrator(s, f, 1.0, "cpu", barostat=bar())  # noise without a bath
    with pytest.raises(ValueError, match="thermostat"):
        Integrator(s, f, 1.0, "cpu", gamma=0.0, T=300.0, barostat=bar())  # a Langevin temperature without friction is no bath
    with pytest.raises(ValueError, match="temperatures must equal"):
        Integrator(s, f, 1.0, "cpu", gamma=1.0, T=310.0, barostat=bar())
    with pytest.raises(ValueError, match="temperatures must equal"):
        Integrator(s, f, 1.0, "cpu", thermostat=VelocityRescale([290.0, 310.0]), barostat=bar())
    with pytest.raises(ValueError, match="2 replicas"):
        Integrator(s, f, 1.0, "cpu", gamma=1.0, T=300.0, barostat=bar(pressure_bar=[1.0, 2.0, 3.0]))
    with pytest.raises(ValueError, match="batch"):
        Integrator(s, f, 1.0, "cpu", gamma=1.0, T=300.0, batch=torch.zeros(291, dtype=torch.int64), barostat=bar())
    with pytest.raises(ValueError, match="exchange"):
        Integrator(s, f, 1.0, "cpu", thermostat=VelocityRescale([290.0, 310.0]), barostat=bar(temperature=[290.0, 310.0]),
                   exchange=ReplicaExchange(20))
    md = Metadynamics(("distance", (0, 3)), sigma=0.25, height=1.0, frequency=10, temperature=300.0, bias_factor=5.0, grid_min=1.0,
                      grid_max=9.0, grid_bins=64, nreplicas=2)
    with pytest.raises(ValueError, match="metadynamics"):
        Integrator(s, _water291(2, metadynamics=md)[2], 1.0, "cpu", gamma=1.0, T=300.0, barostat=bar())
    rs = Restraints(2)
    rs.add_distance(np.array([[0, 3]]), [3.0], [10.0])
    Integrator(s, _water291(2, restraints=rs)[2], 1.0, "cpu", gamma=1.0, T=300.0, barostat=bar())  # distance restraints scale with the box
    rs.add_position([0], np.asarray(g["pos"], dtype=np.float64).reshape(-1, 3)[[0]], 10.0)
    with pytest.raises(ValueError, match="position restraints"):
        Integrator(s, _water291(2, restraints=rs)[2], 1.0, "cpu", gamma=1.0, T=300.0, barostat=bar())

    class Duck:
        def compute(self, pos, box, forces):
            return [0.0, 0.0]

    s.set_masses(par.masses.reshape(-1))
    with pytest.raises(ValueError, match="Forces"):
        Integrator(s, Duck(), 1.0, "cpu", gamma=1.0, T=300.0, barostat=bar())
    dd = DomainSet(np.asarray(g["box"], dtype=np.float64).reshape(-1)[:3], 2, torch.device("cpu"), torch.float32, ["lj"], 7.3, dry=True)
    with pytest.raises(ValueError, match="DomainSet"):
        Integrator(s, dd, 1.0, "cpu", gamma=1.0, T=300.0, barostat=bar())
    with pytest.raises(ValueError, match="Forces"):
        bar().apply(s, Duck(), s.masses, 0.02, [0.0, 0.0], [0.0, 0.0])
    with pytest.raises(ValueError, match="vmap"):
        torch.vmap(lambda q: bar().apply(SimpleNamespace(pos=q, box=s.box, vel=q), f, s.masses, 0.02, [0.0, 0.0], [0.0, 0.0]))(
            torch.zeros(2, 2, 291, 3))
    s.set_box(np.array([0.0, 0.0, 0.0]))
    with pytest.raises(ValueError, match="periodic"):
        Integrator(s, f, 1.0, "cpu", gamma=1.0, T=300.0, barostat=bar())


def test_everything_check_molecules_refuses_is_refused():
    """An exclusion that spans two molecules (here: all bonds dropped from the topology the molecules are read from, the
    exclusions kept) has no molecular virial."""
    from torchmd_amd.crescale import CRescaleBarostat
    from torchmd_amd.integrator import Integrator

    g, par, f, s = _water291(1)
    f._excl_csr = (np.array([0, 1] + [1] * 290, dtype=np.int32), np.array([5], dtype=np.int32))  # atoms 0 and 5: two waters
    f._molecule_table = None
    with pytest.raises(ValueError, match="two molecules"):
        Integrator(s, f, 1.0, "cpu", gamma=1.0, T=300.0, barostat=CRescaleBarostat(1.0, 300.0))


def test_the_generators_advance_also_without_noise_and_do_not_depend_on_the_neighbours(monkeypatch):
    """`stochastic=False` draws its xi all the same, so switching the noise on later continues one chain; a replica's stream is
    keyed (seed, replica).  The draw is made by `apply` before anything is launched: here every launch is replaced."""
    from torchmd_amd import crescale as X

    class Stop(Exception):
        pass

    def draws(stochastic, R, n):
        b = X.CRescaleBarostat(1.0, 300.0, stochastic=stochastic, seed=11)
        b.rng = [np.random.Generator(np.random.Philox(key=np.array([b.seed, r], dtype=np.uint64))) for r in range(R)]
        return b, [[g.standard_normal() for g in b.rng] for _ in range(n)]

    _, a = draws(True, 3, 4)
    _, c = draws(True, 1, 4)
    assert [row[0] for row in a] == [row[0] for row in c] and a[0][0] != a[0][1]
    want = M.mu(1.0, 2e-3, 27000.0, 300.0, 4.5e-5, 1.0, 10, 0.04, 0.0, stochastic=False)
    assert want == M.mu(1.0, 2e-3, 27000.0, 300.0, 4.5e-5, 1.0, 10, 0.04, 5.0, stochastic=False) != \
        M.mu(1.0, 2e-3, 27000.0, 300.0, 4.5e-5, 1.0, 10, 0.04, 5.0, stochastic=True)
    # through `apply`, with the device work replaced: the pressure is handed in, the launch stops the call
    import torchmd_amd.forces as F

    class Fake(F.Forces):
        def __init__(self):
            pass

        def _molecules(self):
            return np.array([0, 1, 2], dtype=np.int32), np.array([0, 1], dtype=np.int32), None

        def _pressure_terms(self, pos, box, vel=None, masses=None):
            out = np.zeros((1, 8))
            out[0, 6], out[0, 7] = 1000.0, 2e-3
            return out

    seen = {}

    def stop(pos, vel, m, scale, *rest):
        seen["scale"] = np.array(scale)
        raise Stop

    def setup(self, system, forces):
        if self.rng is None:
            self.rng = [np.random.Generator(np.random.Philox(key=np.array([self.seed, 0], dtype=np.uint64)))]
        self._molecules = (None, None, None, False)
        self._work = np.zeros(1)

    monkeypatch.setattr(X, "rescale_molecules", stop)
    monkeypatch.setattr(X.CRescaleBarostat, "_setup", setup)
    sysm = SimpleNamespace(pos=torch.zeros(1, 2, 3, dtype=torch.float64), vel=torch.zeros(1, 2, 3, dtype=torch.float64),
                           box=torch.eye(3, dtype=torch.float64)[None] * 10.0)
    for stochastic in (False, True):
        b = X.CRescaleBarostat(1.0, 300.0, stochastic=stochastic, seed=11)
        twin = np.random.Generator(np.random.Philox(key=np.array([11, 0], dtype=np.uint64)))
        for _ in range(3):
            xi = twin.standard_normal()
            with pytest.raises(Stop):
                b.apply(sysm, Fake(), torch.ones(2, dtype=torch.float64), 0.04, [0.0])
            mu = M.mu(1.0, 2e-3, 1000.0, 300.0, 4.5e-5, 1.0, 10, 0.04, xi, stochastic=stochastic)
            assert np.array_equal(seen["scale"], (mu * np.full((1, 3), 10.0)) / 10.0)
        assert b.rng[0].standard_normal() == twin.standard_normal()  # three draws were made, noise or not
