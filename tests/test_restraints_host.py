"""Harmonic restraints without a GPU: the numpy model (`Restraints.energy_forces`) against central finite
differences of its own energy, the host build of restraint_math.h against the model, the per-atom rows, what is refused, and
the splitting that keeps the restraint out of the step kernels, checked in double.

Bars.  Finite differences: h = 1e-5 A on energies of order 10^2 with third derivatives of order k / r: truncation ~1e-10
relative, rounding eps64 E / h ~ 1e-9: 1e-6 relative (to the largest force component of the case) holds with room.  Host build
against model: the same IEEE operations up to the association of a few products: 4 eps64 relative per component.  Splitting: the
two schemes are the same real arithmetic; every step adds a few roundings of size eps64 max|x| to each coordinate, and the
stiffest spring here turns an error over by |k| dt^2 / m < 1 per step, so 64 eps64 steps max|x| bounds the difference."""

import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import _restraints as M
from torchmd_amd.restraints import Restraints, build_rows, min_image

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "torchmd_amd", "csrc")
EPS64 = np.finfo(np.float64).eps


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
def rm(tmp_path_factory):
    cxx = next((c for c in (os.environ.get("CXX"), "g++", "c++", "clang++") if c and shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler (CXX, g++, c++, clang++) found: restraint_math.h is not checked on the CPU")
    inc = _rocm_include()
    if inc is None:
        pytest.skip("the HIP headers (hip/hip_runtime.h) of a ROCm installation were not found: restraint_math.h is not checked on the CPU")
    out = str(tmp_path_factory.mktemp("restraint_math") / "librestraint_math_host.so")
    cmd = [cxx, "-std=c++17", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-D__HIP_PLATFORM_AMD__", f"-I{inc}", f"-I{CSRC}",
           os.path.join(HERE, "restraint_math_host.cpp"), "-o", out]
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, " ".join(cmd) + "\n" + res.stdout + res.stderr
    lib = C.CDLL(out)
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    lib.rm_position.restype = C.c_double
    lib.rm_position.argtypes = [dp, dp, dp, C.c_double, dp]
    lib.rm_distance.restype = C.c_double
    lib.rm_distance.argtypes = [dp, dp, dp, C.c_double, C.c_double, dp]
    lib.rm_validate.restype = C.c_int
    lib.rm_validate.argtypes = [C.c_int64] * 4 + [ip, dp, dp, ip, dp, dp, C.c_char_p, C.c_int]
    lib.rm_rows.restype = C.c_int
    lib.rm_rows.argtypes = [C.c_int64, C.c_int64, ip, ip, ip, ip, ip]
    return lib


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def _ip(a):
    return a.ctypes.data_as(C.POINTER(C.c_int32))


# the edge cases of the issue: (name, box, x_i, x_j or reference, r0)
L = 20.0
CASES = [
    ("inside", [L, L, L], [3.0, 4.0, 5.0], [4.5, 2.0, 6.0], 1.5),
    ("across a face", [L, L, L], [0.3, 4.0, 19.6], [19.5, 5.0, 0.2], 2.0),
    ("zero box", [0.0, 0.0, 0.0], [0.3, 4.0, 19.6], [19.5, 5.0, 0.2], 12.0),
    ("one open axis", [L, 0.0, L], [0.3, -14.0, 19.6], [19.5, 15.0, 0.2], 3.0),
    ("r < r0", [L, L, L], [3.0, 4.0, 5.0], [3.5, 4.2, 5.1], 4.0),
]


def _pair_restraints(a, b, r0):
    rs = Restraints(1)
    rs.add_distance([[0, 1]], r0, 37.0)
    rs.add_position([0], np.asarray([b]), 11.0)
    return rs, np.asarray([[a, b]], dtype=np.float64)


# ----------------------------------------------------------------------------- the model
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_model_forces_are_minus_the_gradient_of_its_energy(case):
    _, box, a, b, r0 = case
    rs, pos = _pair_restraints(a, b, r0)
    E, F = rs.energy_forces(pos, box)
    h = 1e-5
    num = np.zeros((2, 3))
    for i in range(2):
        for c in range(3):
            p, m = pos.copy(), pos.copy()
            p[0, i, c] += h
            m[0, i, c] -= h
            num[i, c] = -(rs.energy_forces(p, box)[0].sum() - rs.energy_forces(m, box)[0].sum()) / (2 * h)
    scale = np.abs(F).max()
    assert scale > 1.0
    assert np.abs(num - F[0]).max() <= 1e-6 * scale, (num, F[0])
    assert np.abs(F[0].sum(axis=0) - F[0, 0] - F[0, 1]).max() == 0.0
    # the distance restraint alone: equal and opposite, bit for bit
    rd = Restraints(1)
    rd.add_distance([[0, 1]], r0, 37.0)
    Fd = rd.energy_forces(pos, box)[1][0]
    assert np.array_equal(Fd[0], -Fd[1])


def test_model_coincident_pair_zero_strength_and_replicas():
    rs = Restraints(2)
    rs.add_distance([[0, 1], [1, 2]], [[1.5, 2.0], [2.5, 3.0]], [[10.0, 0.0], [20.0, 30.0]])
    pos = np.zeros((2, 3, 3))
    pos[:, 2] = [1.0, 2.0, 2.0]  # r = 3 from the coincident pair 0, 1
    E, F = rs.energy_forces(pos, [L, L, L])
    assert np.all(F[:, 0] == 0.0)  # r = 0: no direction, no force
    assert E[0, 1] == 0.5 * 10.0 * 1.5 ** 2  # ... and E = k r0^2 / 2; the k = 0 entry adds nothing
    assert np.all(F[0] == 0.0)
    assert E[1, 1] == 0.5 * 20.0 * 2.5 ** 2 + 0.0  # r = r0 = 3 in replica 1
    assert np.all(E[:, 0] == 0.0)
    with pytest.raises(ValueError, match="replicas"):
        rs.energy_forces(pos[:1], [L, L, L])


def test_min_image():
    d = min_image([[19.5, -10.5, 9.9], [29.0, 0.0, -29.0]], [20.0, 0.0, 20.0])
    assert np.allclose(d, [[-0.5, -10.5, 9.9], [9.0, 0.0, -9.0]], atol=1e-12)


# ----------------------------------------------------------------------------- the compiled header
def test_header_equals_model(rm):
    worst = 0.0
    for _, box, a, b, r0 in CASES + [("coincident", [L, L, L], [1.0, 2.0, 3.0], [1.0, 2.0, 3.0], 2.0)]:
        rs, pos = _pair_restraints(a, b, r0)
        box = np.asarray(box, dtype=np.float64)
        xa, xb = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
        f = np.zeros(3)
        rd = Restraints(1)
        rd.add_distance([[0, 1]], r0, 37.0)
        Ed, Fd = rd.energy_forces(pos, box)
        e = rm.rm_distance(_dp(xa), _dp(xb), _dp(box), 37.0, float(r0), _dp(f))
        for got, want in list(zip(f, Fd[0, 0])) + [(e, Ed[0, 1])]:
            assert abs(got - want) <= 4 * EPS64 * abs(want), (got, want)
            worst = max(worst, abs(got - want) / abs(want) if want else 0.0)
        rp = Restraints(1)
        rp.add_position([0], np.asarray([b]), 11.0)
        Ep, Fp = rp.energy_forces(pos, box)
        e = rm.rm_position(_dp(xa), _dp(xb), _dp(box), 11.0, _dp(f))
        for got, want in list(zip(f, Fp[0, 0])) + [(e, Ep[0, 0])]:
            assert abs(got - want) <= 4 * EPS64 * abs(want), (got, want)
    print(f"largest relative deviation header - model: {worst:.2e}")


def test_rows_of_an_atom_in_five_distance_restraints_and_a_position_restraint(rm):
    pos_atoms = np.array([12, 7, 3], dtype=np.int32)
    pairs = np.array([[7, 1], [2, 7], [7, 12], [9, 7], [4, 5], [7, 3]], dtype=np.int32)
    atoms, off, ent = build_rows(pos_atoms, pairs)
    assert list(atoms) == [1, 2, 3, 4, 5, 7, 9, 12]
    row = ent[off[5]:off[6]]  # atom 7: its position entry, then its distance entries by restraint index, with the sign of its end
    assert row.tolist() == [[0, 1, -1, 0], [1, 0, 1, 1], [1, 1, 2, -1], [1, 2, 12, 1], [1, 3, 9, -1], [1, 5, 3, 1]]
    assert ent[off[2]:off[3]].tolist() == [[0, 2, -1, 0], [1, 5, 7, -1]]  # atom 3
    assert ent[off[7]:off[8]].tolist() == [[0, 0, -1, 0], [1, 2, 7, -1]]  # atom 12
    assert off[-1] == len(pos_atoms) + 2 * len(pairs)
    # the library's builder gives the same rows
    n = len(pos_atoms) + 2 * len(pairs)
    a2, o2, e2 = np.zeros(n, np.int32), np.zeros(n + 1, np.int32), np.zeros((n, 4), np.int32)
    nrows = rm.rm_rows(len(pos_atoms), len(pairs), _ip(pos_atoms), _ip(np.ascontiguousarray(pairs)), _ip(a2), _ip(o2), _ip(e2))
    assert nrows == len(atoms) and np.array_equal(a2[:nrows], atoms) and np.array_equal(o2[:nrows + 1], off) and np.array_equal(e2, ent)


# ----------------------------------------------------------------------------- what is refused
def _validate(rm, natoms, nrep, pos_atom, pos_ref, pos_k, pairs, r0, k):
    pos_atom = np.ascontiguousarray(pos_atom, dtype=np.int32)
    pairs = np.ascontiguousarray(pairs, dtype=np.int32).reshape(-1, 2)
    arrs = [np.ascontiguousarray(a, dtype=np.float64) for a in (pos_ref, pos_k, r0, k)]
    why = C.create_string_buffer(256)
    rm.rm_validate(natoms, nrep, len(pos_atom), len(pairs), _ip(pos_atom), _dp(arrs[0]), _dp(arrs[1]), _ip(pairs), _dp(arrs[2]),
                   _dp(arrs[3]), why, 256)
    return why.value.decode()


def test_library_refusals(rm):
    ok = dict(natoms=10, nrep=2, pos_atom=[1, 4], pos_ref=np.zeros((2, 2, 3)), pos_k=np.ones((2, 2)), pairs=[[0, 1], [1, 9]],
              r0=np.ones((2, 2)), k=np.ones((2, 2)))
    assert _validate(rm, **ok) == ""
    assert _validate(rm, **{**ok, "k": np.zeros((2, 2))}) == ""  # k = 0: an entry switched off
    bad = {
        "bad size": {"natoms": 0},
        "out of range": {"pos_atom": [1, 10]},
        "index out of range": {"pairs": [[0, 1], [1, -1]]},
        "must differ": {"pairs": [[0, 1], [9, 9]]},
        "second position entry": {"pos_atom": [4, 4]},
        "finite k": {"pos_k": [[1.0, -1.0], [1.0, 1.0]]},
        "finite k >= 0": {"k": [[1.0, 1.0], [np.inf, 1.0]]},
        "finite r0": {"r0": [[1.0, 1.0], [1.0, -0.5]]},
        "r0 >= 0": {"r0": [[np.nan, 1.0], [1.0, 1.0]]},
        "finite reference": {"pos_ref": np.full((2, 2, 3), np.nan)},
    }
    for expect, change in bad.items():
        why = _validate(rm, **{**ok, **change})
        assert expect in why, (expect, why)


def test_python_refusals():
    rs = Restraints(2)
    with pytest.raises(ValueError):
        Restraints(0)
    with pytest.raises(ValueError, match="differ"):
        rs.add_distance([[3, 3]], 1.0, 1.0)
    with pytest.raises(ValueError, match="finite"):
        rs.add_distance([[3, 4]], -1.0, 1.0)
    with pytest.raises(ValueError, match="finite"):
        rs.add_distance([[3, 4]], 1.0, np.nan)
    with pytest.raises(ValueError, match=r"\[2,1\]"):
        rs.add_distance([[3, 4]], [[1.0], [2.0], [3.0]], 1.0)
    with pytest.raises(ValueError, match="reference"):
        rs.add_position([1], np.zeros((3, 1, 3)), 1.0)
    with pytest.raises(ValueError, match="finite"):
        rs.add_position([1], np.full((1, 3), np.inf), 1.0)
    rs.add_position([1, 2], np.zeros((2, 3)), [1.0, 2.0])
    with pytest.raises(ValueError, match="one position restraint"):
        rs.add_position([2], np.zeros((1, 3)), 1.0)
    rs.add_distance([[3, 4]], [[1.0], [2.0]], 5.0)
    assert rs.npos == 2 and rs.ndist == 1 and rs.dist_r0.tolist() == [[1.0], [2.0]] and rs.pos_k.shape == (2, 2)
    v = rs.version
    rs.set_distance_targets([[1.5], [2.5]])
    rs.set_position_reference(np.ones((2, 2, 3)))
    rs.set_strengths(position_k=3.0, distance_k=[[1.0], [0.0]])
    assert rs.version == v + 3 and rs.dist_k.tolist() == [[1.0], [0.0]]
    # what a Forces checks: indices, massless atoms, virtual sites
    rs.check(5, np.ones(5))
    with pytest.raises(ValueError, match="beyond"):
        rs.check(4)
    with pytest.raises(ValueError, match="no mass"):
        rs.check(5, np.array([1.0, 1.0, 0.0, 1.0, 1.0]))

    class Sites:
        nsites = 1
        sites = np.array([4])

    with pytest.raises(ValueError, match="virtual site"):
        rs.check(5, np.ones(5), Sites())


def test_public_surface_and_forces_keyword():
    import inspect

    import torchmd_amd
    from torchmd_amd.forces import Forces

    assert torchmd_amd.Restraints is Restraints and "Restraints" in torchmd_amd.__all__
    params = list(inspect.signature(Forces.__init__).parameters)
    assert params[-1] == "restraints"
    from torchmd_amd.domain import DomainSet

    with pytest.raises(ValueError, match="restraints"):
        DomainSet(np.full(3, 30.0), 2, "cpu", None, ["lj"], 9.0, dry=True, restraints=Restraints(1))


# ----------------------------------------------------------------------------- the splitting
@pytest.mark.parametrize("gdt", [0.0, 0.05])
def test_impulse_scheme_equals_restraint_inside_the_force(gdt):
    toy = M.Toy()
    dt = 0.02
    gamma = gdt / dt
    cuts = (1, 4, 7)
    steps = sum(cuts)
    xi, vi, fi = M.run_cut(M.run_inside, toy, cuts, dt, gamma)
    assert np.abs(xi - toy.x0).max() > 0.05  # (something happened)
    bar_x = 64 * EPS64 * steps * np.abs(xi).max()
    bar_v = 64 * EPS64 * steps * max(np.abs(vi).max(), np.abs(xi).max() / dt / steps)
    xs, vs, fs = M.run_cut(M.run_impulse, toy, cuts, dt, gamma)
    dx, dv = np.abs(xs - xi).max(), np.abs(vs - vi).max()
    print(f"gamma dt = {gdt}: |dx| = {dx:.2e} (bar {bar_x:.2e}), |dv| = {dv:.2e} (bar {bar_v:.2e})")
    assert dx <= bar_x and dv <= bar_v
    assert np.abs(fs - fi).max() <= 64 * EPS64 * steps * np.abs(fi).max()  # the force buffer carries F_r across calls
    # the cuts do not matter either
    x1, v1, _ = M.run_cut(M.run_impulse, toy, (12,), dt, gamma)
    assert np.abs(x1 - xi).max() <= bar_x and np.abs(v1 - vi).max() <= bar_v
    # controls: dt/2 in place of dt, and (with friction) the compensation left out, miss the bar by more than 10^3
    xh, _, _ = M.run_cut(M.run_impulse, toy, cuts, dt, gamma, interior_kick=0.5 * dt / (1.0 - gamma * dt))
    assert np.abs(xh - xi).max() > 1e3 * bar_x
    if gdt:
        xn, _, _ = M.run_cut(M.run_impulse, toy, cuts, dt, gamma, interior_kick=dt)
        print(f"  compensation left out: |dx| = {np.abs(xn - xi).max():.2e}")
        assert np.abs(xn - xi).max() > 1e3 * bar_x
