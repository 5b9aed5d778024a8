"""The velocity-rescaling thermostat without a GPU: its scale factor (torchmd_amd/csrc/thermostat_math.h, compiled for the
host) against the numpy model of tests/_thermostat.py, the model's own chain against the canonical distribution, how
`Integrator.step` is cut under two schedules, and what is refused.

tests/thermostat_math_host.cpp wraps the header behind a C interface; a module-scoped fixture compiles it with the system C++
compiler (-ffp-contract=off) against the HIP headers, as tests/test_cons_math_host.py does.  The formula is a handful of
IEEE operations (+, *, /, sqrt, all correctly rounded) in one stated order, so host build and model must agree bit for
bit; the closed forms (c = 0, c = 1) hold to a few roundings, bars stated where they are asserted."""

import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import _thermostat as M

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "torchmd_amd", "csrc")
EPS = np.finfo(np.float64).eps


def _rocm_include():
    from torchmd_amd import _build

    try:
        hipcc = _build._hipcc()
    except RuntimeError:
        return None
    for root in (os.path.dirname(os.path.dirname(os.path.realpath(hipcc))), "/opt/rocm"):
        if os.path.exists(os.path.join(root, "include", "hip", "hip_runtime.h")):
            return os.path.join(root, "include")
    return None


@pytest.fixture(scope="module")
def tm(tmp_path_factory):
    cxx = next((c for c in (os.environ.get("CXX"), "g++", "c++", "clang++") if c and shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler (CXX, g++, c++, clang++) found: thermostat_math.h is not checked on the CPU")
    inc = _rocm_include()
    if inc is None:
        pytest.skip("the HIP headers (hip/hip_runtime.h) of a ROCm installation were not found: thermostat_math.h is not checked on the CPU")
    out = str(tmp_path_factory.mktemp("thermostat_math") / "libthermostat_math_host.so")
    cmd = [cxx, "-std=c++17", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-D__HIP_PLATFORM_AMD__", f"-I{inc}", f"-I{CSRC}",
           os.path.join(HERE, "thermostat_math_host.cpp"), "-o", out]
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, " ".join(cmd) + "\n" + res.stdout + res.stderr
    lib = C.CDLL(out)
    lib.tm_alpha.restype = C.c_double
    lib.tm_alpha.argtypes = [C.c_double] * 6
    lib.tm_kinetic.restype = C.c_double
    lib.tm_kinetic.argtypes = [C.POINTER(C.c_double), C.c_int, C.POINTER(C.c_double)]
    return lib


# ----------------------------------------------------------------------------- the formula
def test_alpha_equals_the_model(tm):
    rng = np.random.default_rng(1)
    for _ in range(2000):
        nf = float(rng.integers(2, 20000))
        T = rng.uniform(1.0, 1000.0)
        kbar = 0.5 * nf * M.BOLTZMAN * T
        K = kbar * rng.uniform(0.01, 10.0)
        c = rng.choice([0.0, 1.0, rng.uniform(0, 1), 1.0 - 1e-12, 1e-12])
        r1, s = M.draw(rng, int(nf))
        assert tm.tm_alpha(K, kbar, nf, c, r1, s) == M.alpha(K, kbar, nf, c, r1, s), (K, kbar, nf, c, r1, s)


def test_kinetic_equals_the_model(tm):
    rng = np.random.default_rng(2)
    for remove in (0, 1):
        for _ in range(200):
            m = rng.uniform(1, 16, 30)
            v = rng.standard_normal((30, 3)) + rng.uniform(-2, 2)
            sums = np.array([m.sum(), *(m[:, None] * v).sum(axis=0), (m * (v * v).sum(axis=1)).sum()])
            vcm = np.zeros(3)
            K = tm.tm_kinetic(sums.ctypes.data_as(C.POINTER(C.c_double)), remove, vcm.ctypes.data_as(C.POINTER(C.c_double)))
            Km, vm = M.kinetic(sums[0], sums[1:4], sums[4], bool(remove))
            assert K == Km and list(vcm) == list(vm)
            # the identity behind it: K is the kinetic energy of v - V_cm, to the rounding of the two terms of the difference
            direct = 0.5 * (m * ((v - vcm) ** 2).sum(axis=1)).sum()
            assert abs(K - direct) <= 64 * EPS * 0.5 * sums[4]
    # no mass, or a kinetic energy that rounding made negative: K = 0, V_cm = 0
    vcm = np.ones(3)
    z = np.zeros(5)
    assert tm.tm_kinetic(z.ctypes.data_as(C.POINTER(C.c_double)), 1, vcm.ctypes.data_as(C.POINTER(C.c_double))) == 0.0 and not vcm.any()
    one = np.array([1.0, 1.0, 0.0, 0.0, 1.0 - EPS])  # (sum m v^2 a rounding below (sum m) V_cm^2)
    assert tm.tm_kinetic(one.ctypes.data_as(C.POINTER(C.c_double)), 1, vcm.ctypes.data_as(C.POINTER(C.c_double))) == 0.0


def test_alpha_edges(tm):
    rng = np.random.default_rng(3)
    nf, T = 63.0, 300.0
    kT = M.BOLTZMAN * T
    kbar = 0.5 * nf * kT
    for _ in range(500):
        r1, s = M.draw(rng, 63)
        got = []
        for K in (1e-3 * kbar, 0.7 * kbar, kbar, 40.0 * kbar):
            # c = 0: K_after = (k_B T / 2) (R1^2 + S) whatever K was: four roundings (two products, a quotient, alpha^2 K after a
            # square root): 8 eps
            a = tm.tm_alpha(K, kbar, nf, 0.0, r1, s)
            want = 0.5 * kT * (r1 * r1 + s)
            assert abs(a * a * K - want) <= 8 * EPS * want, (K, a * a * K, want)
            got.append(a * a * K)
            # c = 1: exactly 1
            assert tm.tm_alpha(K, kbar, nf, 1.0, r1, s) == 1.0
        assert max(got) - min(got) <= 16 * EPS * max(got)
        # K = 0 (and what is not a positive number): 1
        for K in (0.0, -0.0, -1.0, float("nan")):
            assert tm.tm_alpha(K, kbar, nf, 0.9, r1, s) == 1.0
    # alpha^2 = (sqrt(c) + R1 sqrt((1 - c) Kbar / (N_f K)))^2 + (1 - c) Kbar S / (N_f K): with S = 0 and R1 at the root of the
    # square it is zero in exact arithmetic and may come out negative: clamped, never a NaN
    seen_clamp = False
    for c in np.linspace(0.05, 0.95, 181):
        for K in kbar * np.array([0.3, 1.0, 1.7, 3.1]):
            r1 = -np.sqrt(c) / np.sqrt((1.0 - c) * kbar / (nf * K))
            nk = nf * K
            a2 = c + ((1.0 - c) * kbar * (r1 * r1 + 0.0)) / nk + 2.0 * r1 * np.sqrt((c * (1.0 - c) * kbar) / nk)
            a = tm.tm_alpha(K, kbar, nf, c, r1, 0.0)
            assert a >= 0.0 and a <= 1e-7 and np.isfinite(a), (c, K, a)
            if a2 < 0:
                seen_clamp = True
                assert a == 0.0
    assert seen_clamp  # (the clamp was exercised)


# ----------------------------------------------------------------------------- the model's chain
def test_model_chain_samples_the_canonical_distribution():
    """Free particles, N_f = 63, c = 0.9, 8 000 applications per temperature, the first fifth dropped: <K> = N_f k_B T / 2 and
    Var K = N_f (k_B T)^2 / 2, each within four block standard errors (20 blocks of 320 applications; the chain's
    autocorrelation time is 1 / (1 - c) = 10 applications).  The GPU test repeats this chain with the same seed."""
    K = M.model_chain()
    assert K.shape == (4, 8000)
    for r, T in enumerate(M.CHAIN_T):
        mean, emean, var, evar, wmean, wvar = M.chain_statistics(K[r], T)
        print(f"T = {T:.0f} K: <K> = {mean:.4f} +- {emean:.4f} (expected {wmean:.4f}), Var K = {var:.4f} +- {evar:.4f} (expected {wvar:.4f})")
        assert abs(mean - wmean) <= 4 * emean, (T, mean, wmean, emean)
        assert abs(var - wvar) <= 4 * evar, (T, var, wvar, evar)
        assert emean < 0.02 * wmean and evar < 0.15 * wvar  # (the errors themselves are small: the bound is not loose)
    # a replica's chain does not depend on its neighbours
    g = M.generators(M.CHAIN_SEED, 4)[2]
    h = M.generators(M.CHAIN_SEED, 3)[2]
    assert M.draw(g, 63) == M.draw(h, 63)


# ----------------------------------------------------------------------------- cutting step() under two schedules
def test_step_is_cut_at_the_union_of_two_schedules():
    from torchmd_amd.integrator import cut_schedules, cut_segments

    nstep, events = 0, {0: [], 1: []}
    for niter in (7, 13, 30, 1, 49, 100, 3, 22, 25):
        segs = cut_schedules(nstep, niter, (10, 25))
        assert sum(n for n, _ in segs) == niter and all(n > 0 for n, _ in segs)
        done = 0
        for n, hit in segs:
            done += n
            for k, f in enumerate((10, 25)):
                assert hit[k] == ((nstep + done) % f == 0)
                if hit[k]:
                    events[k].append(nstep + done)
        # no needless cuts: every segment but the last ends on an event
        assert all(any(hit) for _, hit in segs[:-1])
        nstep += niter
    assert nstep == 250
    assert events[0] == list(range(10, 251, 10)) and events[1] == list(range(25, 251, 25))
    # one schedule: what cut_segments gives
    for nstep, niter in ((0, 50), (3, 21), (9, 1), (10, 5)):
        assert cut_schedules(nstep, niter, (10,)) == [(n, (hit,)) for n, hit in cut_segments(nstep, niter, 10)]


# ----------------------------------------------------------------------------- what is refused
def test_constructor_and_run_py_keys(tmp_path):
    import torchmd_amd
    from torchmd_amd import run as driver
    from torchmd_amd.thermostat import VelocityRescale

    assert torchmd_amd.VelocityRescale is VelocityRescale
    for bad in (dict(temperature=0.0), dict(temperature=[300.0, -1.0]), dict(temperature=300.0, tau=-1.0),
                dict(temperature=300.0, frequency=0), dict(temperature=300.0, frequency=2.5), dict(temperature=[])):
        with pytest.raises(ValueError):
            VelocityRescale(**bad)
    t = VelocityRescale(300.0, seed=5)
    assert t.tau == 0.1 and t.frequency == 10 and t.remove_com and t.seed == 5 and t.last is None and t.heat() is None
    assert t.temperature == 300.0 and list(t.targets(3)) == [300.0] * 3
    assert t.degrees_of_freedom(66) == 63 and VelocityRescale(300.0, remove_com=False).degrees_of_freedom(66) == 66
    # c = exp(-frequency dt / tau): tau in ps, dt in the integrator's units
    dt = 2.0 / M.TIMEFACTOR
    assert t.decay(dt) == pytest.approx(np.exp(-10 * 0.002 / 0.1), rel=1e-12)
    assert VelocityRescale(300.0, tau=0).decay(dt) == 0.0
    lad = VelocityRescale([280.0, 300.0, 320.0])
    assert lad.temperature is None and list(lad.targets(3)) == [280.0, 300.0, 320.0]
    with pytest.raises(ValueError, match="replicas"):
        lad.targets(2)
    with pytest.raises(ValueError, match="degrees of freedom"):
        t.degrees_of_freedom(4)

    base = ["--log-dir", str(tmp_path / "a"), "--steps", "100", "--output-period", "10"]
    args = driver.get_args(base)
    assert args.thermostat is None
    args = driver.get_args(base + ["--thermostat", "csvr", "--thermostat-tau", "0.5", "--thermostat-frequency", "20",
                                   "--thermostat-temperature", "280,300"])
    assert args.thermostat == "csvr" and args.thermostat_tau == 0.5 and args.thermostat_frequency == 20
    assert args.thermostat_temperature == [280.0, 300.0] and args.remove_com is True
    conf = tmp_path / "conf.yaml"
    conf.write_text(f"thermostat: csvr\nthermostat_temperature: [280, 300, 320]\nremove_com: false\nsteps: 100\noutput_period: 10\n"
                    f"log_dir: {tmp_path / 'b'}\n")
    args = driver.get_args(["--conf", str(conf)])
    assert args.thermostat_temperature == [280.0, 300.0, 320.0] and args.remove_com is False and args.thermostat_frequency == 10
    with pytest.raises(ValueError):
        driver.get_args(base + ["--thermostat", "berendsen"])
    with pytest.raises(ValueError, match="Langevin"):
        driver.get_args(base + ["--thermostat", "csvr", "--langevin-temperature", "300"])


def test_integrator_refuses_what_the_thermostat_cannot_serve():
    import torch

    from _golden import GoldenParameters, load
    from torchmd_amd.barostat import MonteCarloBarostat
    from torchmd_amd.forces import Forces
    from torchmd_amd.integrator import Integrator
    from torchmd_amd.systems import System
    from torchmd_amd.thermostat import VelocityRescale

    g = load("water291")
    par = GoldenParameters(g, torch.float32)
    f = Forces(par, terms=["lj", "electrostatics", "bonds", "angles"], cutoff=7.3, rfa=True)
    s = System(291, 3, torch.float32, "cpu")
    s.set_box(g["box"])
    th = VelocityRescale(300.0)
    it = Integrator(s, f, 1.0, "cpu", thermostat=th)
    assert it.thermostat is th and it._thermostat_ndof == 3 * 291
    with pytest.raises(ValueError, match="Langevin"):
        Integrator(s, f, 1.0, "cpu", gamma=1.0, T=300.0, thermostat=th)
    with pytest.raises(ValueError, match="Langevin"):
        Integrator(s, f, 1.0, "cpu", gamma=1.0, thermostat=th)
    with pytest.raises(ValueError, match="batch"):
        Integrator(s, f, 1.0, "cpu", batch=torch.zeros(291, dtype=torch.int64), thermostat=th)
    with pytest.raises(ValueError, match="replicas"):
        Integrator(s, f, 1.0, "cpu", thermostat=VelocityRescale([280.0, 300.0]))
    Integrator(s, f, 1.0, "cpu", thermostat=VelocityRescale([280.0, 300.0, 320.0]))
    bar = MonteCarloBarostat(1.0, 300.0)
    with pytest.raises(ValueError, match="ladder"):
        Integrator(s, f, 1.0, "cpu", thermostat=VelocityRescale([280.0, 300.0, 320.0]), barostat=bar)
    # one common temperature under a barostat is fine: it is the barostat's thermostat
    Integrator(s, f, 1.0, "cpu", thermostat=VelocityRescale(300.0), barostat=bar)
    Integrator(s, f, 1.0, "cpu", thermostat=VelocityRescale([300.0, 300.0, 300.0]), barostat=bar)
    # with constraints the count is the constraint set's
    fc = Forces(par, terms=["lj", "electrostatics"], cutoff=7.3, rfa=True)
    ic = Integrator(s, fc, 2.0, "cpu", constraints="water", thermostat=VelocityRescale(300.0))
    assert ic._thermostat_ndof == ic.constraints.ndof() == 6 * 97
