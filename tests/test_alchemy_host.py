"""Alchemical decoupling without a GPU: the numpy model (`_alchemy.py`) against central differences of its own
energy in x, lambda_vdw and lambda_elec; the host build of alchemy_math.h against the model pair by pair, in double and in
float; its special cases; the same source as a stand-alone program under the address and undefined-behaviour sanitizers; the
host logic (CSR builder, refusals, the null class staying unmerged) and what the Python layer refuses.

Bars.  Finite differences: 10 |FD(h) - FD(h/2)| + floor per component, h = 1e-5.  The floor is the rounding of the two
float64 energies of a difference: each carries at most eps64 S_E (S_E: the sum of the absolute addends of the energy, which the
model returns), so their difference over 2 h carries at most eps64 S_E / h; the floor is 4 eps64 S_E / h (FD(h) and FD(h/2)
each once, the second with half the step).
Header against model: (c eps) sum|addends|.  c is counted in half-ulps on the path to the worst addend, which is
2 A / r^18 alpha sigma^6 sw of dU/dlambda_vdw at lambda_vdw = 1: 1/sqrt (2), 1/r^2 (5), 1/r^6 (17), 1/r^12 (35), times
(-2 A / r^6 + B) (19 + 35 + 1 = 55), times alpha A / B (3), times sw (22: r, r - r_s amplified by r / (r_c - r_s) <= 6, the
polynomial) = 80 half-ulps = 40 eps, taken as C_REAL = 48.  The float instantiation is compared at 48 eps32; the double one at
C_HOST = 96 eps64, because there the model's own float64 rounding (at most as large) stands on the other side."""

import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import _alchemy as M

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "torchmd_amd", "csrc")
EPS64 = np.finfo(np.float64).eps
EPS32 = np.finfo(np.float32).eps
C_REAL = 48
C_HOST = 96
CUT, SWD = 9.0, 7.5


def _model_kwargs(sysd, **kw):
    return dict(box=sysd["box"], atoms=sysd["atoms"], q=sysd["q"], cls=sysd["cls"], A=sysd["A"], B=sysd["B"], excl=sysd["excl"],
                pairs14=sysd["pairs14"], scee=sysd["scee"], **kw)


# ----------------------------------------------------------------------------- the model against itself
@pytest.mark.parametrize("lv,le,rfa,swd", [(0.5, 0.0, True, SWD), (1.0, 0.6, True, SWD), (0.25, 0.0, False, None), (1.0, 1.0, False, SWD)])
def test_model_against_finite_differences(lv, le, rfa, swd):
    sysd = M.chain_system(5, 40, seed=3, edge=20.0)
    kw = _model_kwargs(sysd, alpha=0.5, cutoff=CUT, switch_dist=swd, rfa=rfa)
    pos = sysd["pos"]
    o = M.evaluate(pos, lv=lv, le=le, **kw)
    S_E = o["S_E"][:3].sum()

    def fd(h):
        num = np.zeros_like(pos)
        for i in list(range(5)) + [5, 9, 17, 30]:
            for c in range(3):
                p, m = pos.copy(), pos.copy()
                p[i, c] += h
                m[i, c] -= h
                num[i, c] = -(M.total_energy(p, lv, le, **kw) - M.total_energy(m, lv, le, **kw)) / (2 * h)
        return num

    a, b = fd(1e-5), fd(5e-6)
    rows = list(range(5)) + [5, 9, 17, 30]
    bar = 10 * np.abs(a - b) + 4 * EPS64 * S_E / 1e-5
    err = np.abs(a - o["F"])[rows]
    print(f"lv {lv} le {le}: max |F - FD| = {err.max():.2e}, worst err / bar = {(err / bar[rows]).max():.2f}")
    assert (err <= bar[rows]).all()
    # dU/dlambda: central differences in lambda of the cross energy (one-sided range kept inside [0, 1]; the staging rule is a
    # refusal of the package, not of the mathematics)
    for which, name in ((0, "dv"), (1, "de")):
        def e_at(x):
            l = [lv, le]
            l[which] = x
            return M.total_energy(pos, l[0], l[1], **kw)

        x0 = [lv, le][which]
        vals = []
        for h in (1e-5, 5e-6):
            lo, hi = x0 - h, x0 + h
            if hi > 1.0 or lo < 0.0:
                vals = None
                break
            vals.append((e_at(hi) - e_at(lo)) / (2 * h))
        if vals is None:
            continue
        bar = 10 * abs(vals[0] - vals[1]) + 4 * EPS64 * S_E / 1e-5
        assert abs(o[name] - vals[0]) <= bar, (name, o[name], vals)


def test_model_limits():
    sysd = M.chain_system(3, 30, seed=1, edge=20.0)
    kw = _model_kwargs(sysd, alpha=0.5, cutoff=CUT, switch_dist=SWD, rfa=True)
    o0 = M.evaluate(sysd["pos"], lv=0.0, le=0.0, **kw)
    assert o0["E_lj"] == 0.0 and o0["E_el"] == 0.0
    env = np.arange(3, sysd["N"])
    assert not o0["F"][env].any()  # the environment feels nothing of a decoupled solute
    o1 = M.evaluate(sysd["pos"], lv=1.0, le=1.0, **kw)
    oa = M.evaluate(sysd["pos"], lv=1.0, le=1.0, **{**kw, "alpha": 0.0})
    assert o1["E_lj"] == oa["E_lj"] and np.array_equal(o1["F"], oa["F"])  # at full coupling alpha does not enter


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
        pytest.skip("no host C++ compiler (CXX, g++, c++, clang++) found: alchemy_math.h is not checked on the CPU")
    inc = _rocm_include()
    if inc is None:
        pytest.skip("the HIP headers (hip/hip_runtime.h) of a ROCm installation were not found: alchemy_math.h is not checked on the CPU")
    return cxx, inc


@pytest.fixture(scope="module")
def am(tmp_path_factory):
    cxx, inc = _toolchain()
    out = str(tmp_path_factory.mktemp("alchemy_math") / "libalchemy_math_host.so")
    cmd = [cxx, "-std=c++17", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-D__HIP_PLATFORM_AMD__", f"-I{inc}", f"-I{CSRC}",
           os.path.join(HERE, "alchemy_math_host.cpp"), "-o", out]
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, " ".join(cmd) + "\n" + res.stdout + res.stderr
    lib = C.CDLL(out)
    d, f, dp, fp = C.c_double, C.c_float, C.POINTER(C.c_double), C.POINTER(C.c_float)
    ip = C.POINTER(C.c_int32)
    lib.alch_pair_f64.restype, lib.alch_pair_f64.argtypes = None, [dp, d, d, d, d, d, d, dp]
    lib.alch_pair_f32.restype, lib.alch_pair_f32.argtypes = None, [dp, f, f, f, f, f, f, fp]
    lib.alch_lj_at_f64.restype, lib.alch_lj_at_f64.argtypes = d, [dp, d, d, d, d]
    lib.alch_pair14_f64.restype, lib.alch_pair14_f64.argtypes = None, [d, d, d, dp]
    lib.alch_pair14_f32.restype, lib.alch_pair14_f32.argtypes = None, [f, f, f, fp]
    lib.alch_validate_c.restype, lib.alch_validate_c.argtypes = None, [C.c_long, C.c_long, C.c_long, ip, dp, dp, d, C.c_char_p, C.c_int]
    lib.alch_closed_c.restype, lib.alch_closed_c.argtypes = None, [C.c_long, C.c_long, ip, ip, C.c_long, C.c_int, C.c_char_p, C.c_int]
    lib.alch_csr_c.restype = C.c_long
    lib.alch_csr_c.argtypes = [C.c_long, ip, ip, ip, dp, ip, C.c_int, dp, dp, C.c_long, ip, dp, C.c_int, ip, ip, ip, dp, C.c_long]
    return lib


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def _ip(a):
    return a.ctypes.data_as(C.POINTER(C.c_int32))


def _cfg(swd, rfa, alpha, reference, parts=3):
    krf, crf = M.rf_consts(CUT) if rfa else (0.0, 0.0)
    return np.array([swd or 0.0, CUT, krf, crf, alpha, float(reference), float(rfa), float(parts)])


def _pair_cases():
    """(r, qq, A, B): random distances from deep inside the core to the cutoff, r at the switching distance and the cutoff
    exactly and one ulp to either side, over three LJ pairs (one with A = 0) and both charge signs."""
    rng = np.random.default_rng(5)
    ljs = [(582000.0, 595.0), (1.2e5, 150.0), (0.0, 0.0)]
    rs = list(rng.uniform(0.3, CUT, 150)) + list(rng.uniform(SWD, CUT, 50))
    for r0 in (SWD, CUT):
        rs += [np.nextafter(r0, 0.0), r0, np.nextafter(r0, np.inf)]
    return [(float(r), float(rng.choice([-1.0, 1.0]) * rng.uniform(5, 120)), *ljs[k % 3]) for k, r in enumerate(rs)]


@pytest.mark.parametrize("lv,le", [(1.0, 1.0), (1.0, 0.3), (0.7, 0.0), (0.5, 0.0), (0.05, 0.0), (0.0, 0.0)])
@pytest.mark.parametrize("swd,rfa,reference", [(SWD, True, 0), (SWD, False, 1), (None, True, 0)])
def test_header_pair_against_the_model(am, lv, le, swd, rfa, reference):
    cfg = _cfg(swd, rfa, 0.5, reference)
    worst = {"f64": 0.0, "f32": 0.0}
    o64, o32 = np.zeros(4), np.zeros(4, dtype=np.float32)
    for r, qq, A, B in _pair_cases():
        r2 = r * r
        m = M.pair(np.array([r2]), qq, A, B, lv, le, 0.5, cutoff=CUT, switch_dist=swd, rfa=rfa, reference_switch=bool(reference))
        want = np.array([m["ulj"][0], m["gel"][0], m["dv"][0], m["fs"][0]])
        S = np.array([m["a_ulj"][0], m["a_gel"][0], m["a_dv"][0], m["a_fs"][0]])
        am.alch_pair_f64(_dp(cfg), r2, qq, A, B, lv, le, _dp(o64))
        assert (np.abs(o64 - want) <= C_HOST * EPS64 * S).all(), (r, qq, A, B, o64, want, S)
        worst["f64"] = max(worst["f64"], float((np.abs(o64 - want) / np.where(S > 0, S, 1)).max() / EPS64))
        r2f = np.float32(r2)
        m = M.pair(np.array([float(r2f)]), float(np.float32(qq)), float(np.float32(A)), float(np.float32(B)), float(np.float32(lv)),
                   float(np.float32(le)), float(np.float32(0.5)), cutoff=CUT, switch_dist=swd, rfa=rfa, reference_switch=bool(reference))
        want = np.array([m["ulj"][0], m["gel"][0], m["dv"][0], m["fs"][0]])
        S = np.array([m["a_ulj"][0], m["a_gel"][0], m["a_dv"][0], m["a_fs"][0]])
        am.alch_pair_f32(_dp(cfg), r2f, qq, A, B, lv, le, o32.ctypes.data_as(C.POINTER(C.c_float)))
        assert (np.abs(o32.astype(np.float64) - want) <= C_REAL * EPS32 * S).all(), (r, qq, A, B, o32, want, S)
        worst["f32"] = max(worst["f32"], float((np.abs(o32 - want) / np.where(S > 0, S, 1)).max() / EPS32))
    print(f"lv {lv} le {le} switch {swd} rfa {rfa}: worst |header - model| / sum|addends| = {worst['f64']:.1f} eps64, {worst['f32']:.1f} eps32")


def test_header_special_cases(am):
    cfg = _cfg(SWD, True, 0.5, 0)
    o = np.zeros(4)
    A, B = 582000.0, 595.0
    # r = 0 at lv < 1: finite energy, zero force, no charge part
    for lv in (0.0, 0.3, 0.999):
        am.alch_pair_f64(_dp(cfg), 0.0, 55.0, A, B, lv, 0.0, _dp(o))
        s = 0.5 * (A / B) * (1 - lv)
        assert np.isfinite(o).all() and o[3] == 0.0 and o[1] == 0.0
        assert abs(o[0] - lv * (A / s**2 - B / s)) <= 8 * EPS64 * lv * (A / s**2 + B / s)
    # lambda = 0 gives exactly 0 energy and force at every distance
    for r in (0.0, 0.5, 3.0, 8.2, CUT):
        am.alch_pair_f64(_dp(cfg), r * r, 55.0, A, B, 0.0, 0.0, _dp(o))
        assert o[0] == 0.0 and o[3] == 0.0
        assert am.alch_lj_at_f64(_dp(cfg), r * r, A, B, 0.0) == 0.0
    # lv = 1: the plain 12-6 sequence of operations on 1/r (pair_terms), alpha does not enter the energy or the force
    for r in (2.9, 3.7, 5.0, 8.0, 8.9):
        r2 = r * r
        rinv = 1.0 / np.sqrt(r2)
        rinv2 = rinv * rinv
        rinv6 = rinv2 * rinv2 * rinv2
        elj = (A * rinv6 - B) * rinv6
        f = (-12.0 * A * rinv6 + 6.0 * B) * rinv6 * rinv
        rr = r2 * rinv
        if rr > SWD:
            t = (rr - SWD) * (1.0 / (CUT - SWD))
            sw = 1.0 + t * t * t * (-10.0 + t * (15.0 - t * 6.0))
            dsw = t * t * (-30.0 + t * (60.0 - t * 30.0)) * (1.0 / (CUT - SWD))
            f = sw * f + elj * dsw * 1.0
            elj *= sw
        cfg_lj = _cfg(SWD, True, 0.5, 0, parts=1)
        am.alch_pair_f64(_dp(cfg_lj), r2, 0.0, A, B, 1.0, 1.0, _dp(o))
        assert o[0] == elj and o[3] == f * rinv, (r, o, elj, f * rinv)
        o2 = np.zeros(4)
        am.alch_pair_f64(_dp(_cfg(SWD, True, 0.0, 0, parts=1)), r2, 0.0, A, B, 1.0, 1.0, _dp(o2))
        assert o2[0] == o[0] and o2[3] == o[3]
    # the foreign-energy form agrees with the pair function at the same state
    for lv in (0.2, 0.8, 1.0):
        for r in (1.0, 4.0, 8.5):
            am.alch_pair_f64(_dp(cfg), r * r, 0.0, A, B, lv, 0.0, _dp(o))
            got = am.alch_lj_at_f64(_dp(cfg), r * r, A, B, lv)
            assert abs(got - o[0]) <= C_HOST * EPS64 * (lv * (A / r**12 + B / r**6) + abs(o[0]))
    # the 1-4 Coulomb term
    am.alch_pair14_f64(6.25, 40.0, 1.2, _dp(o))
    assert abs(o[0] - 40.0 / 2.5 / 1.2) <= 4 * EPS64 * o[0] and abs(o[1] + o[0] / 6.25) <= 4 * EPS64 * o[0]


def test_header_under_the_sanitizers(tmp_path):
    cxx, inc = _toolchain()
    exe = str(tmp_path / "alchemy_math_main")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-DALCHEMY_MATH_MAIN", "-D__HIP_PLATFORM_AMD__", f"-I{inc}", f"-I{CSRC}", os.path.join(HERE, "alchemy_math_host.cpp"), "-o", exe]
    res = subprocess.run(cmd, capture_output=True, text=True)
    if res.returncode != 0 and ("sanitize" in res.stderr or "asan" in res.stderr.lower()):
        pytest.skip("the host compiler has no address / UB sanitizer runtime")
    assert res.returncode == 0, " ".join(cmd) + "\n" + res.stdout + res.stderr
    run = subprocess.run([exe], capture_output=True, text=True)
    print(run.stdout)
    assert run.returncode == 0 and run.stdout.strip().endswith("ok"), run.stdout + run.stderr


# ----------------------------------------------------------------------------- host logic
def test_csr_builder(am):
    sysd = M.chain_system(6, 4, seed=2)
    n, ns = sysd["N"], 6
    atoms = np.arange(ns, dtype=np.int32)
    ex = {(int(a), int(b)) for a, b in sysd["excl"]} | {(int(b), int(a)) for a, b in sysd["excl"]}
    rows = [sorted(b for (a, b) in ex if a == i) for i in range(n)]
    eoff = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int32)
    eidx = np.array([b for r in rows for b in r] or [0], dtype=np.int32)
    qs = np.ascontiguousarray(sysd["q"][:ns] * np.sqrt(M.KE))
    cls = np.ascontiguousarray(sysd["cls"][:ns].astype(np.int32))
    T = sysd["A"].shape[0]
    tA, tB = np.ascontiguousarray(sysd["A"].reshape(-1)), np.ascontiguousarray(sysd["B"].reshape(-1))
    p14 = np.ascontiguousarray(sysd["pairs14"].astype(np.int32))
    scee = np.ascontiguousarray(sysd["scee"])
    cap = 256
    off, partner, kind, prm = np.zeros(ns + 1, np.int32), np.zeros(cap, np.int32), np.zeros(cap, np.int32), np.zeros((cap, 4))
    for f32 in (0, 1):
        ne = am.alch_csr_c(ns, _ip(atoms), _ip(eoff), _ip(eidx), _dp(qs), _ip(cls), T, _dp(tA), _dp(tB), len(p14), _ip(p14), _dp(scee), f32,
                           _ip(off), _ip(partner), _ip(kind), _dp(prm), cap)
        want = {}
        for a in range(ns):
            row = [(b, 0) for b in range(ns) if b != a and (a, b) not in ex]
            row += [(int(j if i == a else i), 1) for i, j in p14 if a in (i, j)]
            want[a] = row
        assert ne == sum(len(r) for r in want.values()) and off[ns] == ne
        for a in range(ns):
            got = [(int(partner[e]), int(kind[e])) for e in range(off[a], off[a + 1])]
            assert got == want[a], (a, got, want[a])
            for e in range(off[a], off[a + 1]):
                b = int(partner[e])
                qq = float(np.float32(qs[a]) * np.float32(qs[b])) if f32 else qs[a] * qs[b]
                assert prm[e, 0] == qq
                if kind[e] == 0:
                    assert prm[e, 1] == sysd["A"][cls[a], cls[b]] and prm[e, 2] == sysd["B"][cls[a], cls[b]]
                else:
                    assert prm[e, 3] == 1.2
    # n = 1: one empty row
    ne = am.alch_csr_c(1, _ip(atoms[:1]), _ip(eoff), _ip(eidx), _dp(qs), _ip(cls), T, _dp(tA), _dp(tB), 0, _ip(p14), _dp(scee), 0, _ip(off),
                       _ip(partner), _ip(kind), _dp(prm), cap)
    assert ne == 0 and off[0] == 0 and off[1] == 0


def test_c_refusals(am):
    msg = C.create_string_buffer(256)

    def validate(natoms, atoms, lv, le, alpha):
        atoms = np.asarray(atoms, dtype=np.int32)
        lv, le = np.asarray(lv, dtype=np.float64), np.asarray(le, dtype=np.float64)
        am.alch_validate_c(natoms, len(lv), len(atoms), _ip(atoms), _dp(lv), _dp(le), alpha, msg, 256)
        return msg.value.decode()

    assert validate(10, [1, 2], [1.0, 0.5], [1.0, 0.0], 0.5) == ""
    assert "out of range" in validate(10, [1, 10], [1.0], [1.0], 0.5)
    assert "out of range" in validate(10, [-1], [1.0], [1.0], 0.5)
    assert "twice" in validate(10, [3, 3], [1.0], [1.0], 0.5)
    assert "[0, 1]" in validate(10, [3], [1.5], [0.0], 0.5)
    assert "[0, 1]" in validate(10, [3], [1.0], [-0.1], 0.5)
    assert "[0, 1]" in validate(10, [3], [float("nan")], [0.0], 0.5)
    assert "soft core" in validate(10, [3], [1.0, 0.9], [1.0, 0.1], 0.5)
    assert "alpha" in validate(10, [3], [1.0], [1.0], -0.1)

    def closed(atoms, idx, width):
        atoms, idx = np.asarray(atoms, dtype=np.int32), np.asarray(idx, dtype=np.int32)
        am.alch_closed_c(10, len(atoms), _ip(atoms), _ip(idx), len(idx) // width, width, msg, 256)
        return msg.value.decode()

    assert closed([0, 1, 2], [0, 1, 1, 2, 4, 5], 2) == ""
    assert "joins the solute" in closed([0, 1, 2], [0, 1, 2, 3], 2)
    assert "joins the solute" in closed([0, 1, 2], [0, 1, 2, 1, 2, 5], 3)
    assert "joins the solute" in closed([0, 1, 2, 3], [4, 1, 2, 3], 4)


def test_python_refusals_and_the_null_class():
    from torchmd_amd import Alchemical
    from torchmd_amd.alchemy import append_null_class, check_closed
    from torchmd_amd.forces import merge_lj_types

    for bad in (dict(atoms=[1, 1]), dict(atoms=[-1]), dict(atoms=[]), dict(atoms=[0], lambda_vdw=1.1), dict(atoms=[0], lambda_elec=-0.1),
                dict(atoms=[0], lambda_vdw=0.5, lambda_elec=0.5), dict(atoms=[0], lambda_vdw=[1.0, 0.9], lambda_elec=[1.0, 0.1]),
                dict(atoms=[0], alpha=-1.0), dict(atoms=[0], lambda_vdw=[1.0, 1.0, 1.0], lambda_elec=[1.0, 1.0])):
        with pytest.raises(ValueError):
            Alchemical(**bad)
    al = Alchemical([5, 3, 4], lambda_vdw=[1.0, 0.5], lambda_elec=[1.0, 0.0])
    assert al.atoms.tolist() == [3, 4, 5]
    v0 = al.version
    al.set_lambdas([1.0, 0.25], 0.0)
    assert al.version > v0 and al.lambdas(2)[0].tolist() == [1.0, 0.25] and al.lambdas(2)[1].tolist() == [0.0, 0.0]
    with pytest.raises(ValueError):
        al.lambdas(3)
    with pytest.raises(ValueError):
        al.set_lambdas(0.5, 0.5)
    assert Alchemical([0]).lambdas(4)[0].tolist() == [1.0] * 4
    # closure
    check_closed([0, 1, 2], 6, {"bond": np.array([[0, 1], [1, 2], [3, 4]])})
    with pytest.raises(ValueError, match="closed under the topology"):
        check_closed([0, 1, 2], 6, {"bond": np.array([[0, 1], [2, 3]])})
    with pytest.raises(ValueError, match="closed under the topology"):
        check_closed([0, 1, 2], 6, {"angle": np.array([[1, 2, 3]])})
    # the null class: a water-like table whose hydrogen row is all zero; the solute's class must not merge with it
    A = np.array([[5.0e5, 0.0, 3.0e5], [0.0, 0.0, 0.0], [3.0e5, 0.0, 2.0e5]])
    B = np.array([[600.0, 0.0, 400.0], [0.0, 0.0, 0.0], [400.0, 0.0, 300.0]])
    types = np.array([0, 1, 1, 0, 1, 1, 2, 2])
    Am, Bm, tm, _ = merge_lj_types(A, B, types)
    A2, B2, t2, cls = append_null_class(Am, Bm, tm, [6, 7])
    assert A2.shape == (Am.shape[0] + 1,) * 2 and not A2[-1].any() and not B2[:, -1].any()
    assert t2[6] == t2[7] == Am.shape[0] and t2[1] != t2[6] and (t2[:6] == tm[:6]).all()
    assert (cls == tm[[6, 7]]).all() and (A2[:-1, :-1] == Am).all()
    # a water as the solute among waters: its hydrogens leave the charged all-zero class for the null class
    A2, B2, t2, cls = append_null_class(Am, Bm, tm, [3, 4, 5])
    assert t2[4] == t2[5] == t2[3] == Am.shape[0] and t2[1] == tm[1] != t2[4] and cls.tolist() == tm[[3, 4, 5]].tolist()


def test_domain_decomposition_refuses_a_solute():
    from torchmd_amd import Alchemical
    from torchmd_amd.domain import DomainSet

    with pytest.raises(ValueError, match="alchemical"):
        DomainSet(np.full(3, 30.0), 2, "cpu", None, ["lj"], 9.0, dry=True, alchemical=Alchemical([0]))
