"""The generalized-Born implicit solvent without a GPU: the numpy model (`_gb.py`) against central differences of
its own energy, its limits and invariants, the host build of gb_math.h against the model pair by pair and atom by atom, the
same source as a stand-alone program under the address and undefined-behaviour sanitizers, the default radii, and what the
Python layer refuses.

Bars.  Finite differences: 10 |FD(h) - FD(h/2)| + 1e-9 per component at h = 1e-5; the energies of the differences are
evaluated by the same model code in extended precision (numpy longdouble), because in float64 the rounding of an energy of
order 10^2, eps64 E / h ~ 4e-9, is larger than the bar's floor.  Header against model: 8 eps64 times the sum of the absolute
addends for the double instantiation (at most 8 roundings on the path to any addend differ between numpy's order of operations
and the header's), and 32 eps32 for the float instantiation: the constant c of the GPU bars, counted in DESIGN §21 from the
roundings on the path to the worst addend of t (about 28 half-ulps on (r/4)(u^2 - l^2), 17 on ln(u/l))."""

import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import _gb as M

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "torchmd_amd", "csrc")
EPS64 = np.finfo(np.float64).eps
EPS32 = np.finfo(np.float32).eps
LD = np.longdouble
C_HOST = 8   # eps64 per unit of sum |addends|, double instantiation against the model
C_REAL = 32  # eps_R per unit of sum |addends|: the constant of the fp32 bars


def _fd_forces(pos, q, rad, sc, h, **kw):
    num = np.zeros_like(pos)
    for i in range(len(pos)):
        for c in range(3):
            p, m = pos.copy(), pos.copy()
            p[i, c] += h
            m[i, c] -= h
            num[i, c] = float(-(M.energy(p, q, rad, sc, work=LD, **kw) - M.energy(m, q, rad, sc, work=LD, **kw)) / (2 * h))
    return num


# ----------------------------------------------------------------------------- the model against itself
def test_model_forces_are_minus_the_gradient_of_its_energy():
    pos, q, rad, sc = M.cluster(40, 5, edge=7.0)
    o = M.evaluate(pos, q, rad, sc)
    assert (o["regimes"][1:] > 0).all(), o["regimes"]  # separate, overlapping and engulfed pairs all occur
    a, b = _fd_forces(pos, q, rad, sc, 1e-5), _fd_forces(pos, q, rad, sc, 5e-6)
    bar = 10 * np.abs(a - b) + 1e-9
    err = np.abs(a - o["F"])
    print(f"max |F - FD| = {err.max():.2e}, worst err / bar = {(err / bar).max():.2f}, regimes {o['regimes']}")
    assert (err <= bar).all()


def test_model_single_ion():
    for r in (1.2, 1.85, 2.5):
        o = M.evaluate(np.zeros((1, 3)), [0.7], [r], [0.8], surface_tension=0.0)
        want = -0.5 * M.KE * (1.0 - 1.0 / 78.5) * 0.49 / (r - 0.09)
        assert abs(o["B"][0] - (r - 0.09)) <= 4 * EPS64 * (r - 0.09)
        assert abs(o["E_gb"] - want) <= 4 * EPS64 * abs(want)
        assert o["F"].tolist() == [[0.0, 0.0, 0.0]]


def test_model_two_far_ions_are_coulomb_screened():
    q, rad, sc = np.array([0.8, -0.5]), np.array([1.5, 1.7]), np.array([0.85, 0.72])
    for dist in (1e3, 1e5):
        pos = np.array([[0.0, 0.0, 0.0], [dist, 0.0, 0.0]])
        o = M.evaluate(pos, q, rad, sc, surface_tension=0.0)
        rho = rad - M.OFFSET
        p = -M.KE * (1.0 - 1.0 / 78.5)
        self_terms = 0.5 * p * (q * q / rho).sum()
        cross = o["E_gb"] - self_terms
        # descreening falls off as sigma^3 / r^4 and exp(-D) vanishes: B -> rho, f -> r
        assert np.abs(o["B"] / rho - 1.0).max() < 10.0 / dist ** 4 * 1e3
        coulomb = M.KE * q[0] * q[1] / dist
        assert abs(cross - p * q[0] * q[1] / dist) <= 1e-9 * abs(coulomb) + 8 * EPS64 * abs(self_terms)
        # vacuum Coulomb + GB cross term = Coulomb / eps_out
        assert abs((coulomb + cross) - coulomb / 78.5) <= 1e-9 * abs(coulomb) + 8 * EPS64 * abs(self_terms)


def test_model_no_net_force_no_net_torque_and_gamma_zero():
    pos, q, rad, sc = M.cluster(65, 2)
    o = M.evaluate(pos, q, rad, sc)
    F = o["F"]
    scale = np.abs(F).sum()
    assert np.abs(F.sum(axis=0)).max() <= 16 * EPS64 * scale
    assert np.abs(np.cross(pos, F).sum(axis=0)).max() <= 16 * EPS64 * scale * np.abs(pos).max()
    o0 = M.evaluate(pos, q, rad, sc, surface_tension=0.0)
    assert o0["E_sa"] == 0.0 and o0["E_gb"] == o["E_gb"] and o["E_sa"] > 0.0
    assert np.array_equal(o0["B"], o["B"])


def test_model_fp32_convention_only_changes_the_pair_vector():
    pos, q, rad, sc = M.cluster(65, 2)
    p32 = pos.astype(np.float32).astype(np.float64)
    a = M.evaluate(p32, q, rad, sc, dtype=np.float32)
    b = M.evaluate(p32, q, rad, sc)
    # d formed in float32 differs from d formed in float64 by eps32 / 2 relative: well inside 32 eps32 S
    ob = M.evaluate(p32, q, rad, sc, bounds=True)
    assert (np.abs(a["I"] - b["I"]) <= C_REAL * EPS32 * ob["S_I"]).all() and not np.array_equal(a["I"], b["I"])


# ----------------------------------------------------------------------------- the compiled header
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


def _toolchain():
    cxx = next((c for c in (os.environ.get("CXX"), "g++", "c++", "clang++") if c and shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler (CXX, g++, c++, clang++) found: gb_math.h is not checked on the CPU")
    inc = _rocm_include()
    if inc is None:
        pytest.skip("the HIP headers (hip/hip_runtime.h) of a ROCm installation were not found: gb_math.h is not checked on the CPU")
    return cxx, inc


@pytest.fixture(scope="module")
def gm(tmp_path_factory):
    cxx, inc = _toolchain()
    out = str(tmp_path_factory.mktemp("gb_math") / "libgb_math_host.so")
    cmd = [cxx, "-std=c++17", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-D__HIP_PLATFORM_AMD__", f"-I{inc}", f"-I{CSRC}",
           os.path.join(HERE, "gb_math_host.cpp"), "-o", out]
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, " ".join(cmd) + "\n" + res.stdout + res.stderr
    lib = C.CDLL(out)
    d, f = C.c_double, C.c_float
    dp, fp = C.POINTER(d), C.POINTER(f)
    for name in ("gb_t_f64", "gb_t3_f64"):
        getattr(lib, name).restype, getattr(lib, name).argtypes = d, [d, d, d]
    for name in ("gb_t_f32", "gb_t3_f32"):
        getattr(lib, name).restype, getattr(lib, name).argtypes = f, [f, f, f]
    lib.gb_pair_f64.restype, lib.gb_pair_f64.argtypes = None, [d, d, d, d, dp]
    lib.gb_pair_f32.restype, lib.gb_pair_f32.argtypes = None, [f, f, f, f, fp]
    lib.gb_born.restype, lib.gb_born.argtypes = None, [d, d, dp]
    lib.gb_chain.restype, lib.gb_chain.argtypes = None, [d, d, d, d, d, dp]
    lib.gb_all_f64.restype, lib.gb_all_f64.argtypes = None, [C.c_int, dp, dp, dp, dp, dp, d, dp, dp, dp]
    return lib


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def _pair_cases():
    """(r, rho_i, sigma_j): random pairs in all regimes, and r at the regime boundaries rho = |r - sigma| and rho = r + sigma
    exactly and one ulp to either side."""
    rng = np.random.default_rng(11)
    names = list(M.RADII)
    cases = []
    for _ in range(400):
        a, b = names[rng.integers(len(names))], names[rng.integers(len(names))]
        cases.append((float(rng.uniform(0.2, 12.0)), M.RADII[a] - M.OFFSET, M.SCALES[b] * (M.RADII[b] - M.OFFSET)))
    for rho, sig in ((1.11, 1.3736), (1.61, 0.9435), (1.11, 1.6416), (1.71, 1.1592), (1.46, 1.0)):
        for r0 in (rho + sig, sig - rho, rho - sig):  # |r - sigma| = rho from outside / inside; r + sigma = rho
            if r0 > 0.05:
                for r in (np.nextafter(r0, 0.0), r0, np.nextafter(r0, np.inf)):
                    cases.append((float(r), rho, sig))
    return cases


def test_header_pair_functions_against_the_model(gm):
    worst = {"t64": 0.0, "t3_64": 0.0, "t32": 0.0, "t3_32": 0.0}
    regimes = set()
    for r, rho, sig in _pair_cases():
        terms, reg = M.pair_t(r, rho, sig)
        regimes.add(int(reg))
        t, S = float(sum(terms)), float(sum(abs(x) for x in terms))
        t3s = M.pair_t3(r, rho, sig)
        t3, S3 = float(sum(t3s)), float(sum(abs(x) for x in t3s))
        got, got3 = gm.gb_t_f64(r, rho, sig), gm.gb_t3_f64(r, rho, sig)
        assert abs(got - t) <= C_HOST * EPS64 * S, (r, rho, sig, got, t)
        assert abs(got3 - t3) <= C_HOST * EPS64 * S3, (r, rho, sig, got3, t3)
        if S > 0:
            worst["t64"] = max(worst["t64"], abs(got - t) / (EPS64 * S))
        if S3 > 0:
            worst["t3_64"] = max(worst["t3_64"], abs(got3 - t3) / (EPS64 * S3))
        # the float instantiation on the float-rounded arguments, against the model on the same numbers
        rf, rhof, sigf = (float(np.float32(v)) for v in (r, rho, sig))
        terms, _ = M.pair_t(rf, rhof, sigf)
        t, S = float(sum(terms)), float(sum(abs(x) for x in terms))
        t3s = M.pair_t3(rf, rhof, sigf)
        t3, S3 = float(sum(t3s)), float(sum(abs(x) for x in t3s))
        got, got3 = gm.gb_t_f32(rf, rhof, sigf), gm.gb_t3_f32(rf, rhof, sigf)
        # (one ulp of r across a boundary flips the regime of one side only: both are continuous there, the bar holds)
        assert abs(got - t) <= C_REAL * EPS32 * max(S, 1.0 / rhof), (rf, rhof, sigf, got, t)
        assert abs(got3 - t3) <= C_REAL * EPS32 * max(S3, 1.0 / rhof ** 2), (rf, rhof, sigf, got3, t3)
        if S > 0:
            worst["t32"] = max(worst["t32"], abs(got - t) / (EPS32 * S))
        if S3 > 0:
            worst["t3_32"] = max(worst["t3_32"], abs(got3 - t3) / (EPS32 * S3))
    assert regimes == {0, 1, 2, 3}
    print("worst multiples of eps S:", {k: round(v, 2) for k, v in worst.items()})


def test_header_pair_energy_and_closes_against_the_model(gm):
    rng = np.random.default_rng(12)
    out = (C.c_double * 3)()
    out32 = (C.c_float * 3)()
    for k in range(300):
        r2 = 0.0 if k < 5 else float(rng.uniform(0.1, 15.0)) ** 2
        pqq, Bi, Bj = float(rng.uniform(-200, 200)), float(rng.uniform(1.1, 6.0)), float(rng.uniform(1.1, 6.0))
        if k < 5:
            Bj = Bi
        D = r2 / (4 * Bi * Bj)
        ex = np.exp(-D)
        f2 = r2 + Bi * Bj * ex
        G = pqq / np.sqrt(f2)
        g = -G * (1 - 0.25 * ex) / f2
        h = -0.5 * G * ex * (1 + D) / f2
        gm.gb_pair_f64(r2, pqq, Bi, Bj, out)
        # f2 is a sum of two positive addends, the rest products: relative bars (D's rounding enters exp as D eps)
        rel = (C_HOST + 2 * D) * EPS64
        assert abs(out[0] - G) <= rel * abs(G) and abs(out[1] - g) <= rel * abs(g) and abs(out[2] - h) <= rel * abs(h) + 1e-300
        a32 = [float(np.float32(v)) for v in (r2, pqq, Bi, Bj)]
        D = a32[0] / (4 * a32[2] * a32[3])
        ex = np.exp(-D)
        f2 = a32[0] + a32[2] * a32[3] * ex
        G = a32[1] / np.sqrt(f2)
        gm.gb_pair_f32(*a32, out32)
        rel = (C_REAL + 2 * D) * EPS32
        assert abs(out32[0] - G) <= rel * abs(G)
        assert abs(out32[1] + G * (1 - 0.25 * ex) / f2) <= rel * abs(G / f2)
        assert abs(out32[2] + 0.5 * G * ex * (1 + D) / f2) <= rel * abs(G / f2) * ex * (1 + D) + 1e-30
        if k < 5:  # the self term: G = pqq / B, h B = -pqq / (2 B^2)
            assert abs(out[0] - pqq / Bi) <= 4 * EPS64 * abs(pqq / Bi) and abs(out[2] * Bi + 0.5 * pqq / Bi ** 2) <= 8 * EPS64 * abs(pqq / Bi ** 2)
    o2 = (C.c_double * 2)()
    for k in range(200):
        radius = float(rng.choice(list(M.RADII.values())))
        I = float(rng.uniform(0.0, 0.6))
        B, c, T = M.born_close(np.array([I]), np.array([radius]))
        gm.gb_born(I, radius, o2)
        # B = 1 / (1/rho - T/r): the bar is on the difference's addends
        S = B[0] ** 2 * (1.0 / (radius - M.OFFSET) + abs(T[0]) / radius)
        assert abs(o2[0] - B[0]) <= C_HOST * EPS64 * S
        # c = rho P (1 - T^2) / r: the addends of P = 1 - 1.6 psi + 14.55 psi^2, of 1 - T^2 (it cancels as T -> 1), and T's
        # argument Q = psi - 0.8 psi^2 + 4.85 psi^3 through dT = (1 - T^2) dQ
        rho = radius - M.OFFSET
        psi, t = rho * I, abs(T[0])
        P, Pabs, Qabs = 1 - 1.6 * psi + 14.55 * psi ** 2, 1 + 1.6 * psi + 14.55 * psi ** 2, psi + 0.8 * psi ** 2 + 4.85 * psi ** 3
        Sc = rho / radius * (Pabs * (1 - t * t) + abs(P) * (1 + t * t) + abs(P) * 2 * t * (1 - t * t) * Qabs)
        assert abs(o2[1] - c[0]) <= C_HOST * EPS64 * Sc
        sa, bsum = float(rng.uniform(0.0, 0.7)), float(rng.uniform(-30, 30))
        esa = sa * (radius / B[0]) ** 6
        b = (bsum - 6 * esa / B[0]) * B[0] ** 2 * c[0]
        gm.gb_chain(bsum, radius, sa, B[0], c[0], o2)
        assert abs(o2[0] - esa) <= C_HOST * EPS64 * esa
        assert abs(o2[1] - b) <= C_HOST * EPS64 * (abs(bsum) + 6 * esa / B[0]) * B[0] ** 2 * abs(c[0])


def test_header_whole_structure_against_the_model(gm):
    pos, q, rad, sc = M.cluster(65, 2)
    o = M.evaluate(pos, q, rad, sc, bounds=True)
    n = len(pos)
    sa = 4 * np.pi * 0.0054 * (rad + 1.4) ** 2
    B, F, E = np.zeros(n), np.zeros((n, 3)), np.zeros(2)
    qs = q * np.sqrt(M.KE)
    gm.gb_all_f64(n, _dp(np.ascontiguousarray(pos)), _dp(qs), _dp(rad), _dp(sc), _dp(sa), -(1.0 - 1.0 / 78.5), _dp(B), _dp(F), _dp(E))
    u = (C_HOST + o["M"]) * EPS64  # per-addend roundings and the sums' own
    print(f"B {np.abs(B - o['B']).max():.1e} E {abs(E[0] - o['E_gb']):.1e} {abs(E[1] - o['E_sa']):.1e} F {np.abs(F - o['F']).max():.1e}")
    assert (np.abs(B - o["B"]) <= u * o["S_B"]).all()
    assert abs(E[0] - o["E_gb"]) <= u * o["S_Egb"] and abs(E[1] - o["E_sa"]) <= u * o["S_Esa"]
    assert (np.abs(F - o["F"]).max(axis=1) <= u * o["S_F"]).all()


def test_header_as_a_program_runs_clean_under_the_sanitizers(tmp_path):
    cxx, inc = _toolchain()
    exe = str(tmp_path / "gb_math_main")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-ffp-contract=off", "-DGB_MATH_MAIN",
           "-D__HIP_PLATFORM_AMD__", f"-I{inc}", f"-I{CSRC}", os.path.join(HERE, "gb_math_host.cpp"), "-o", exe]
    res = subprocess.run(cmd, capture_output=True, text=True)
    if res.returncode != 0 and "sanitize" in (res.stdout + res.stderr):
        pytest.skip("the host compiler has no address / undefined-behaviour sanitizer runtime")
    assert res.returncode == 0, " ".join(cmd) + "\n" + res.stdout + res.stderr
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and run.stdout.strip().endswith("ok") and "runtime error" not in run.stderr and "Sanitizer" not in run.stderr, (
        run.stdout + run.stderr)


# ----------------------------------------------------------------------------- the Python layer
def _thrombin_parameters():
    import torch

    import _golden as G

    g = G.load("thrombin")
    return g, G.GoldenParameters(g, torch.float64)


def test_default_radii_on_thrombin():
    from torchmd_amd.implicit import GeneralizedBorn, elements_from_masses

    g, par = _thrombin_parameters()
    el = elements_from_masses(par.masses.numpy())
    assert None not in el and set(el) == {"H", "C", "N", "O", "S", "Cl"}
    gb = GeneralizedBorn.from_parameters(par)
    assert gb.natoms == 4676
    el = np.array(el)
    on_n = gb.radii[el == "H"] == 1.3
    assert on_n.any() and not on_n.all() and set(gb.radii[el == "H"]) == {1.2, 1.3}
    for e, r in (("C", 1.7), ("N", 1.55), ("O", 1.5), ("S", 1.8), ("Cl", 1.7)):
        assert (gb.radii[el == e] == r).all()
    for e, s in (("H", 0.85), ("C", 0.72), ("N", 0.79), ("O", 0.85), ("S", 0.96), ("Cl", 0.8)):
        assert (gb.scale[el == e] == s).all()
    # every H with the larger radius has a bond to a nitrogen
    bonds = g["par_bond_idx"].reshape(-1, 2)
    partner_is_n = np.zeros(len(el), dtype=bool)
    for a, b in bonds:
        partner_is_n[a] |= el[b] == "N"
        partner_is_n[b] |= el[a] == "N"
    assert np.array_equal(gb.radii == 1.3, (el == "H") & partner_is_n)


def test_recorded_thrombin_model_is_the_model():
    """tests/golden/thrombin_gb.npz (what the GPU test compares with) against the model's first pass, which is what fits in a few
    seconds here: the Born radii of both conventions bit for bit, and the bounds; the energies and forces of the file follow from
    them through the same `evaluate` that the small-cluster tests check."""
    import _golden as G

    ref = G.load(M.THROMBIN_GOLDEN)
    pos, q, rad, sc = M.thrombin_inputs()
    p32 = pos.astype(np.float32).astype(np.float64)
    for tag, dt in (("f64", np.float64), ("f32", np.float32)):
        o = M.evaluate(p32, q, rad, sc, dtype=dt, born_only=True)
        assert np.array_equal(o["B"], ref[tag + "_B"])
        if tag == "f64":
            assert np.array_equal(o["S_B"], ref["S_B"]) and np.array_equal(o["regimes"], ref["regimes"])
    assert ref["f64_F"].shape == (4676, 3) and int(ref["M"]) == 7 * 4675 + 8
    assert np.abs(ref["f64_F"].sum(axis=0)).max() <= 16 * EPS64 * np.abs(ref["f64_F"]).sum()
    assert 0 < np.abs(ref["f32_F"] - ref["f64_F"]).max() <= C_REAL * EPS32 * ref["S_F"].max()


def test_public_surface_and_refusals():
    import inspect

    import torch

    import torchmd_amd
    from torchmd_amd.domain import DomainSet
    from torchmd_amd.forces import Forces
    from torchmd_amd.implicit import GeneralizedBorn
    from torchmd_amd.integrator import Integrator

    assert torchmd_amd.GeneralizedBorn is GeneralizedBorn and "GeneralizedBorn" in torchmd_amd.__all__
    assert "implicit_solvent" in inspect.signature(Forces.__init__).parameters
    for bad in (dict(radii=[1.5, 0.09], scale=[0.8, 0.8]), dict(radii=[1.5, np.nan], scale=[0.8, 0.8]), dict(radii=[1.5, 1.5], scale=[0.8, -0.1]),
                dict(radii=[1.5, 1.5], scale=[0.8]), dict(radii=[1.5], scale=[0.8], solute_dielectric=0.0),
                dict(radii=[1.5], scale=[0.8], solvent_dielectric=-1.0), dict(radii=[1.5], scale=[0.8], surface_tension=-1.0)):
        with pytest.raises(ValueError):
            GeneralizedBorn(**bad)
    _, par = _thrombin_parameters()
    gb = GeneralizedBorn.from_parameters(par)
    terms = ["electrostatics", "lj"]
    with pytest.raises(ValueError, match="4676"):
        Forces(par, terms=terms, implicit_solvent=GeneralizedBorn([1.5] * 10, [0.8] * 10))
    with pytest.raises(ValueError, match="GeneralizedBorn"):
        Forces(par, terms=terms, implicit_solvent="obc2")
    with pytest.raises(ValueError, match="pme"):
        Forces(par, terms=terms, cutoff=9.0, pme=True, implicit_solvent=gb)
    with pytest.raises(ValueError, match="rfa"):
        Forces(par, terms=terms, cutoff=9.0, rfa=True, implicit_solvent=gb)

    from torchmd_amd.vsites import VirtualSites

    vs = VirtualSites(np.zeros(0, dtype=np.int64), np.zeros((0, 3), dtype=np.int64), np.zeros((0, 3)))  # (even an empty table)
    with pytest.raises(ValueError, match="virtual_sites"):
        Forces(par, terms=terms, virtual_sites=vs, implicit_solvent=gb)
    with pytest.raises(ValueError, match="implicit_solvent"):
        DomainSet(np.full(3, 30.0), 2, "cpu", None, ["lj"], 9.0, dry=True, implicit_solvent=gb)
    # a cutoff on the vacuum terms is allowed; the box, the pressure and vmap are refused before any device work
    f = Forces(par, terms=terms, cutoff=9.0, implicit_solvent=gb)
    Forces(par, terms=terms, cutoff=None, implicit_solvent=gb)
    with pytest.raises(ValueError, match="open boundaries"):
        f._gb_box(np.array([[30.0, 30.0, 30.0]]))
    f._gb_box(np.zeros((3, 3)))
    pos = torch.zeros(1, 4676, 3, dtype=torch.float64)
    with pytest.raises(ValueError, match="implicit_solvent"):
        f.virial(pos, torch.zeros(1, 3, 3, dtype=torch.float64))
    with pytest.raises(ValueError, match="vmap"):
        torch.vmap(lambda p: f.compute(p, torch.zeros(1, 3, 3, dtype=torch.float64), None, toNumpy=False))(pos[None])
    with pytest.raises(ValueError, match="born_radii"):
        Forces(par, terms=terms).born_radii()

    # the integrator's refusals: atom groups and any barostat (looked at before anything touches a device)
    class Duck:
        pass

    integ = Integrator.__new__(Integrator)
    integ.forces = f
    integ.batch, integ.barostat = torch.zeros(4676, dtype=torch.long), None
    with pytest.raises(ValueError, match="batch"):
        integ._check_side_terms()
    integ.batch, integ.barostat = None, Duck()
    with pytest.raises(ValueError, match="barostat"):
        integ._check_side_terms()
    integ.barostat = None
    integ._check_side_terms()
