"""The arithmetic of the constrained MD step (torchmd_amd/csrc/cons_math.h: settle_water, shake_cluster<2..5>,
cons_velocities) compiled for the host and held to the fp64 reference of tests/_constraints.py — no GPU.

tests/cons_math_host.cpp wraps the header behind a C interface; a module-scoped fixture compiles it with the system C++
compiler (-ffp-contract=off, as the kernel's `#pragma clang fp contract(off)`) against the HIP headers of the ROCm
installation torchmd_amd/_build.py uses, and loads it with ctypes.  Without a host compiler or the HIP headers the module
skips and says so.

Bars: SETTLE against iterated SHAKE (tol 1e-14) 1e-12 A — the two solve the same equations, and their measured distance
is 1.4e-14 A at coordinates of up to 60 A (two ulps of 7e-15 A); a wrong formula misses by ~1e-3 A.  At
displacements of sigma >= 0.2 A per coordinate the closed form and the iteration may land on different roots of the same
equations, so there the contract of a `true` return is asserted instead."""

import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import _constraints as H
from _bonded_systems import _rotation

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "torchmd_amd", "csrc")
DP = C.POINTER(C.c_double)

# d_OH, d_HH: TIP3P, TIP4P-Ew (0.9572 A, 104.52 deg), SPC (1.0 A, 1.633 A), an H2S-like 1.34 A / 92 deg
GEOMETRIES = {
    "tip3p": (0.9572, 1.5139),
    "tip4pew": (0.9572, 2 * 0.9572 * np.sin(np.deg2rad(104.52) / 2)),
    "spc": (1.0, 1.633),
    "h2s": (1.34, 2 * 1.34 * np.sin(np.deg2rad(92.0) / 2)),
}
HEAVY = (15.9994, 32.06)
HYDROGEN = (1.008, 2.014, 3.024)
CLUSTER_HEAVY = (12.011, 14.007, 15.999, 32.06)


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
def cm(tmp_path_factory):
    cxx = next((c for c in (os.environ.get("CXX"), "g++", "c++", "clang++") if c and shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler (CXX, g++, c++, clang++) found: cons_math.h is not checked on the CPU")
    inc = _rocm_include()
    if inc is None:
        pytest.skip("the HIP headers (hip/hip_runtime.h) of a ROCm installation were not found: cons_math.h is not checked on the CPU")
    out = str(tmp_path_factory.mktemp("cons_math") / "libcons_math_host.so")
    cmd = [cxx, "-std=c++17", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-D__HIP_PLATFORM_AMD__", f"-I{inc}", f"-I{CSRC}",
           os.path.join(HERE, "cons_math_host.cpp"), "-o", out]
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, " ".join(cmd) + "\n" + res.stdout + res.stderr
    lib = C.CDLL(out)
    lib.cm_settle.argtypes = [DP, DP, C.c_double, C.c_double, C.c_double, C.c_double]
    lib.cm_shake.argtypes = [C.c_int, DP, DP, DP, DP, C.c_double, C.c_int]
    lib.cm_velocities.argtypes = [C.c_int, C.c_int, DP, DP, DP]
    return lib


def _p(a):
    assert a.dtype == np.float64 and a.flags.c_contiguous
    return a.ctypes.data_as(DP)


def settle(cm, b4, xp, mO, mH, dOH, dHH):
    """settle_water on [S, 3, 3] arrays: (result, ok [S])."""
    out, ok = np.ascontiguousarray(xp, dtype=np.float64).copy(), np.zeros(len(xp), dtype=bool)
    b4 = np.ascontiguousarray(b4, dtype=np.float64)
    for s in range(len(out)):
        ok[s] = cm.cm_settle(_p(b4[s]), _p(out[s]), mO, mH, dOH, dHH) == 1
    return out, ok


def _centres(rng, n, rmax):
    u = rng.standard_normal((n, 3))
    return u / np.linalg.norm(u, axis=1, keepdims=True) * rng.uniform(0, rmax, (n, 1))


def water_samples(rng, n, dOH, dHH, sigma, rmax=60.0):
    """n rigid molecules (O, H1, H2) at the geometry, randomly rotated, centres up to rmax from the origin, and the same
    with every coordinate displaced by a Gaussian of width sigma: (b4, xp) [n, 3, 3]."""
    h = np.sqrt(dOH * dOH - 0.25 * dHH * dHH)
    mol = np.array([[0.0, 0.0, 0.0], [0.5 * dHH, h, 0.0], [-0.5 * dHH, h, 0.0]])
    b4 = np.stack([mol @ _rotation(rng).T for _ in range(n)]) + _centres(rng, n, rmax)[:, None, :]
    return b4, b4 + sigma * rng.standard_normal(b4.shape)


def _water_units(n, dOH, dHH):
    return [(np.arange(3 * s, 3 * s + 3), [(0, 1, dOH), (0, 2, dOH), (1, 2, dHH)]) for s in range(n)]


def _lengths(x):
    return np.stack([np.linalg.norm(x[:, 0] - x[:, 1], axis=1), np.linalg.norm(x[:, 0] - x[:, 2], axis=1),
                     np.linalg.norm(x[:, 1] - x[:, 2], axis=1)], axis=1)


# ----------------------------------------------------------------------------- settle_water
NSAMPLE = 50  # per geometry x heavy mass x hydrogen mass x sigma: 24 x 3 x 50 = 3 600 molecules


@pytest.mark.parametrize("geom", list(GEOMETRIES))
def test_settle_equals_shake(cm, geom):
    dOH, dHH = GEOMETRIES[geom]
    worst = 0.0
    for gi, mO in enumerate(HEAVY):
        for hi, mH in enumerate(HYDROGEN):
            for si, sigma in enumerate((0.01, 0.05, 0.1)):
                rng = np.random.default_rng([list(GEOMETRIES).index(geom), gi, hi, si])
                b4, xp = water_samples(rng, NSAMPLE, dOH, dHH, sigma)
                got, ok = settle(cm, b4, xp, mO, mH, dOH, dHH)
                assert ok.all(), (geom, mO, mH, sigma, np.flatnonzero(~ok))  # (no sample dropped)
                m = np.tile([mO, mH, mH], NSAMPLE)
                ref = H.shake(xp.reshape(-1, 3).copy(), b4.reshape(-1, 3), m, _water_units(NSAMPLE, dOH, dHH))
                err = np.abs(got.reshape(-1, 3) - ref).max()
                worst = max(worst, err)
                assert err <= 1e-12, (geom, mO, mH, sigma, err)
    print(f"settle_water vs host SHAKE (1e-14), {geom}: max|dx| = {worst:.2e} A")


def test_settle_leaves_a_rigid_molecule_alone(cm):
    rng = np.random.default_rng(11)
    for geom, (dOH, dHH) in GEOMETRIES.items():
        b4, _ = water_samples(rng, 8, dOH, dHH, 0.0)
        got, ok = settle(cm, b4, b4.copy(), 15.9994, 1.008, dOH, dHH)
        assert ok.all() and np.abs(got - b4).max() <= 1e-13, (geom, np.abs(got - b4).max())


@pytest.mark.parametrize("sigma", [0.2, 0.3])
def test_settle_contract_when_far_from_the_geometry(cm, sigma):
    """Whatever root the closed form picks, a `true` return is a valid constrained position: finite, the three lengths
    held, the centre of mass kept, and every mass-weighted displacement in the plane of the old molecule (a sum of
    constraint forces along the old bonds)."""
    ntrue = ntotal = 0
    for gi, (geom, (dOH, dHH)) in enumerate(GEOMETRIES.items()):
        for hi, (mO, mH) in enumerate([(15.9994, 1.008), (32.06, 1.008), (15.9994, 3.024), (32.06, 2.014)]):
            rng = np.random.default_rng([int(sigma * 10), gi, hi])
            b4, xp = water_samples(rng, 100, dOH, dHH, sigma)
            got, ok = settle(cm, b4, xp, mO, mH, dOH, dHH)
            finite = np.isfinite(got).all(axis=(1, 2))
            assert not (ok & ~finite).any(), (geom, mO, mH, "a non-finite result reported as settled")
            ntrue += int(ok.sum())
            ntotal += len(ok)
            g, x0, u = got[ok], b4[ok], xp[ok]
            ln = _lengths(g)
            assert np.abs(ln - [dOH, dOH, dHH]).max() <= 1e-9, (geom, mO, mH, np.abs(ln - [dOH, dOH, dHH]).max())
            m = np.array([mO, mH, mH])[None, :, None]
            com = lambda y: (m * y).sum(axis=1) / m.sum()
            assert np.abs(com(g) - com(u)).max() <= 1e-9, (geom, mO, mH)
            nrm = np.cross(x0[:, 1] - x0[:, 0], x0[:, 2] - x0[:, 0])
            nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
            off = np.abs(np.einsum("sak,sk->sa", m * (g - u), nrm)).max()
            assert off <= 1e-9, (geom, mO, mH, off)
    assert ntrue >= 0.8 * ntotal, (ntrue, ntotal)  # (the contract above is not vacuous)
    print(f"settle_water at sigma = {sigma} A: {ntrue} of {ntotal} settled, all within the contract")


# ----------------------------------------------------------------------------- shake_cluster, cons_velocities
def cluster_samples(rng, n, na, sigma, rmax=30.0):
    """n clusters of na atoms: heavy atom (mass from CLUSTER_HEAVY) first, na - 1 hydrogens on bonds of 0.95 - 1.12 A in
    directions at least ~70 degrees apart; (ref, x, masses [n, na], d [n, na])."""
    tet = np.array([[1, 1, 1], [1, -1, -1], [-1, 1, -1], [-1, -1, 1]]) / np.sqrt(3.0)
    ref, mass, d = np.zeros((n, na, 3)), np.zeros((n, na)), np.zeros((n, na))
    for s in range(n):
        dirs = tet[rng.permutation(4)[: na - 1]] + 0.15 * rng.standard_normal((na - 1, 3))
        dirs /= np.linalg.norm(dirs, axis=1, keepdims=True)
        d[s, 1:] = rng.uniform(0.95, 1.12, na - 1)
        ref[s, 1:] = (dirs * d[s, 1:, None]) @ _rotation(rng).T
        mass[s] = [rng.choice(CLUSTER_HEAVY)] + [1.008] * (na - 1)
    ref += _centres(rng, n, rmax)[:, None, :]
    return ref, ref + sigma * rng.standard_normal(ref.shape), mass, d


def _cluster_units(n, na, d):
    return [(np.arange(na * s, na * s + na), [(0, k, d[s, k]) for k in range(1, na)]) for s in range(n)]


def shake_cluster(cm, ref, x, mass, d, tol, max_iter):
    out, ok = np.ascontiguousarray(x).copy(), np.zeros(len(x), dtype=bool)
    im = np.ascontiguousarray(1.0 / mass)
    for s in range(len(out)):
        rc = cm.cm_shake(ref.shape[1], _p(np.ascontiguousarray(ref[s])), _p(out[s]), _p(im[s]), _p(np.ascontiguousarray(d[s])), tol, max_iter)
        assert rc in (0, 1)
        ok[s] = rc == 1
    return out, ok


@pytest.mark.parametrize("na", [2, 3, 4, 5])
def test_shake_cluster(cm, na):
    rng = np.random.default_rng(100 + na)
    n = 60
    ref, x, mass, d = cluster_samples(rng, n, na, 0.05)
    host = H.shake(x.reshape(-1, 3).copy(), ref.reshape(-1, 3), mass.reshape(-1), _cluster_units(n, na, d)).reshape(n, na, 3)
    tight, _ = shake_cluster(cm, ref, x, mass, d, 1e-14, 1000)
    err = np.abs(tight - host).max()
    assert err <= 1e-12, (na, err)
    # the production setting: relative bond error <= tolerance, and it says so
    prod, ok = shake_cluster(cm, ref, x, mass, d, 1e-10, 200)
    rel = np.abs(np.linalg.norm(prod[:, 1:] - prod[:, :1], axis=2) - d[:, 1:]) / d[:, 1:]
    assert ok.all() and rel.max() <= 1e-10, (na, rel.max())
    # one sweep of a displaced cluster is not convergence
    _, ok1 = shake_cluster(cm, ref, x, mass, d, 1e-10, 1)
    assert not ok1.any(), na
    print(f"shake_cluster<{na}>: max|dx| vs host at tol 1e-14 = {err:.2e} A, at tol 1e-10 |x - host| = {np.abs(prod - host).max():.2e} A, "
          f"bond error {rel.max():.2e}")


@pytest.mark.parametrize("na,water", [(2, False), (3, False), (4, False), (5, False), (3, True)])
def test_cons_velocities(cm, na, water):
    rng = np.random.default_rng(200 + na + 10 * water)
    n = 60
    if water:
        x = np.concatenate([water_samples(rng, n // 4, *g, 0.0)[0] for g in GEOMETRIES.values()])
        mass = np.stack([[rng.choice(HEAVY)] + [rng.choice(HYDROGEN)] * 2 for _ in range(n)])
        pairs = [(0, 1, 0.0), (0, 2, 0.0), (1, 2, 0.0)]
    else:
        x, _, mass, _ = cluster_samples(rng, n, na, 0.0)
        pairs = [(0, k, 0.0) for k in range(1, na)]
    v = rng.standard_normal(x.shape)
    us = [(np.arange(na * s, na * s + na), pairs) for s in range(n)]
    host = H.project(x.reshape(-1, 3), v.reshape(-1, 3).copy(), mass.reshape(-1), us).reshape(n, na, 3)
    got = np.ascontiguousarray(v).copy()
    im = np.ascontiguousarray(1.0 / mass)
    for s in range(n):
        assert cm.cm_velocities(na, int(water), _p(np.ascontiguousarray(x[s])), _p(got[s]), _p(im[s])) == 0
    vmax = np.abs(v).max()
    assert np.abs(got - host).max() <= 1e-13 * vmax, np.abs(got - host).max()
    worst = 0.0
    for a, b, _ in pairs:
        r, dv = x[:, a] - x[:, b], got[:, a] - got[:, b]
        along = np.abs(np.einsum("sk,sk->s", r, dv)) / (np.linalg.norm(r, axis=1) * np.linalg.norm(v, axis=2).max(axis=1))
        worst = max(worst, along.max())
    assert worst <= 1e-13, worst
    dp = np.abs(((got - v) * mass[:, :, None]).sum(axis=1)).max()
    assert dp <= 1e-13, dp
    print(f"cons_velocities na = {na} water = {water}: max|dv| vs host = {np.abs(got - host).max():.2e}, r.dv/(|r||v|) = {worst:.2e}, "
          f"momentum change {dp:.2e}")
