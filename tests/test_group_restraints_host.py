"""Group restraints without a GPU: the numpy model (`GroupRestraints.energy_forces`) against central finite
differences of its own energy, the host build of group_math.h against the model, invariances of both, single-atom groups against
`Restraints` and the oracle's angle term, the rows, what is refused, the exchange of windows and the Boresch correction.

Bars.  Finite differences: h = 1e-5 A on energies of order 10^2 with third derivatives of order k / r: truncation ~1e-10
relative, rounding eps64 E / h ~ 1e-9: 1e-6 relative to the largest force component of the case (the bar and the reasoning of
tests/test_restraints_host.py).  Host build against model, one restraint on given centres: the same IEEE operations in the same
order, 4 eps64 relative per component.  The whole walk against the model: the centres are summed in member order there and
pairwise in numpy, n eps64 x 8 A per centre, amplified by at most 8 / 2 through an arm: 64 n eps64 max|F|.  A box vector added
to one atom: 64 eps64 relative.  Net force of one restraint: 16 eps64 sum|F|; net torque in the zero box likewise with
sum |x||F|.  The oracle's angle term in double: another formula for the same force, 1e-10 relative (tests/test_gpu_parity.py's
fp64 bar).  Boresch: 0.03 kcal/mol against a quadrature of the six factors (the Gaussian approximation itself is off by 0.017
at these parameters; a slipped factor 2 or a missing sine is 0.4 or more)."""

import ctypes as C
import os
import shutil
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest

import _group_restraints as M
from torchmd_amd.group_restraints import ANGLE, DIHEDRAL, DISTANCE, GroupRestraints, restraint_terms
from torchmd_amd.restraints import Restraints

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "torchmd_amd", "csrc")
EPS64 = np.finfo(np.float64).eps
L = 20.0


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
def gm(tmp_path_factory):
    cxx = next((c for c in (os.environ.get("CXX"), "g++", "c++", "clang++") if c and shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler (CXX, g++, c++, clang++) found: group_math.h is not checked on the CPU")
    inc = _rocm_include()
    if inc is None:
        pytest.skip("the HIP headers (hip/hip_runtime.h) of a ROCm installation were not found: group_math.h is not checked on the CPU")
    out = str(tmp_path_factory.mktemp("group_math") / "libgroup_math_host.so")
    cmd = [cxx, "-std=c++17", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-D__HIP_PLATFORM_AMD__", f"-I{inc}", f"-I{CSRC}",
           os.path.join(HERE, "group_math_host.cpp"), "-o", out]
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, " ".join(cmd) + "\n" + res.stdout + res.stderr
    lib = C.CDLL(out)
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    lib.gm_restraint.restype = C.c_double
    lib.gm_restraint.argtypes = [C.c_int, dp, dp, C.c_double, C.c_double, C.c_double, dp]
    lib.gm_validate.restype = C.c_int
    lib.gm_validate.argtypes = [C.c_int64, C.c_int64, C.c_int64, ip, ip, dp, C.c_int64, ip, ip, dp, dp, dp, C.c_char_p, C.c_int]
    lib.gm_rows.restype = C.c_int
    lib.gm_rows.argtypes = [C.c_int64, ip, ip, C.c_int64, ip, ip, ip, ip, ip, ip, ip]
    lib.gm_normalise.restype = None
    lib.gm_normalise.argtypes = [C.c_int64, ip, dp, dp]
    lib.gm_energy_forces.restype = None
    lib.gm_energy_forces.argtypes = [C.c_int64, dp, dp, C.c_int64, ip, ip, dp, C.c_int64, ip, ip, dp, dp, dp, dp, dp, dp]
    return lib


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def _ip(a):
    return a.ctypes.data_as(C.POINTER(C.c_int32))


def _tables(gr):
    """The arrays of the descriptor, kept alive by the caller: off, atoms, W, kind, groups, target, k, flat."""
    return gr.descriptor()[1]


def _header(gm, gr, pos, box):
    """(E [R,3], F [R,N,3], centres [R,G,3]) of the host build's whole walk."""
    pos = np.ascontiguousarray(gr._positions(pos))
    R, N = pos.shape[:2]
    boxes = np.ascontiguousarray(gr._boxes(box, R))
    off, atoms, W, kind, groups, target, k, flat = _tables(gr)
    E, F, X = np.zeros((R, 3)), np.zeros((R, N, 3)), np.zeros((R, gr.ngroups, 3))
    for r in range(R):
        t, kk, fl = (np.ascontiguousarray(a[r]) for a in (target, k, flat))
        gm.gm_energy_forces(N, _dp(pos[r]), _dp(boxes[r]), gr.ngroups, _ip(off), _ip(atoms), _dp(W), gr.nrestraints, _ip(kind), _ip(groups),
                            _dp(t), _dp(kk), _dp(fl), _dp(X[r]), _dp(E[r]), _dp(F[r]))
    return E, F, X


# ----------------------------------------------------------------------------- the cases
def _cloud(rng, centre, n, radius=2.0):
    return np.asarray(centre) + rng.uniform(-radius, radius, (n, 3))


def _case(name):
    """(GroupRestraints of one replica, pos [N,3], box [3]); every angle between consecutive arms within [0.3, pi - 0.3]."""
    rng = np.random.default_rng(sum(map(ord, name)))
    box = np.array([L, L, L])
    centres = np.array([[3.0, 4.0, 5.0], [7.0, 8.5, 4.0], [11.0, 5.0, 8.0], [13.0, 10.0, 12.0], [6.0, 12.0, 10.0]])
    sizes = [1, 2, 40, 5, 3]
    gr = GroupRestraints(1)
    wrap = True
    if name == "zero box":
        box, wrap = np.zeros(3), False
    if name == "one open axis":
        box = np.array([L, 0.0, L])
        centres = centres + np.array([0.0, -30.0, 0.0])
    if name == "wrapped group":
        centres = centres + np.array([L - 11.5, 0.0, L - 8.5])  # the group of 40 lies across two faces
    pos, members = [], []
    for c, n in zip(centres, sizes):
        members.append(np.arange(len(pos), len(pos) + n))
        pos.extend(_cloud(rng, c, n))
    pos = np.asarray(pos)
    if name == "an atom in three groups":
        members[1] = np.array([members[1][0], members[2][3]])
        members[3] = np.concatenate([members[3], [members[2][3]]])
        pos[members[2][3]] = 0.5 * (centres[1] + centres[3])
    mass = rng.uniform(1.0, 16.0, len(pos))
    for i, m in enumerate(members):
        gr.add_group(rng.permutation(m), weights=rng.uniform(0.5, 2.0, len(m)) if i == 3 else None)
    gr.masses = mass
    if wrap:
        for c in range(3):
            if box[c] != 0.0:
                pos[:, c] -= box[c] * np.floor(pos[:, c] / box[c])  # every atom on its own
    if name == "dihedral across the wrap":
        # phi = -3.0 on four single atoms, phi0 = 3.0: delta = -6 + 2 pi
        pos = np.array([[1.0, 0.0, 0.0], [0.0, 0.0, 0.0], [0.0, 0.0, 1.5], [np.cos(-3.0), np.sin(-3.0), 1.5]]) * 2.0 + 5.0
        gr = GroupRestraints(1)
        g = [gr.add_group([i], weights=[1.0]) for i in range(4)]
        gr.add_dihedral(g, 3.0, 40.0)
        phi = gr.values(pos, box)[0, 0]
        assert abs(abs(phi) - 3.0) < 1e-12  # (whichever sign the convention gives: the target is the other one)
        gr.set_targets(-phi)
        return gr, pos, box
    if name == "a group named by four restraints":
        gr.add_distance((2, 0), 6.0, 50.0)
        gr.add_angle((1, 2, 3), 1.3, 60.0)
        gr.add_dihedral((0, 1, 2, 3), 0.4, 30.0)
        gr.add_dihedral((4, 3, 2, 0), -1.0, 30.0)
    else:
        gr.add_distance((0, 2), 7.0, 50.0)
        gr.add_angle((0, 1, 2), 1.2, 60.0)
        gr.add_dihedral((0, 1, 2, 3), 0.4, 30.0)
        gr.add_distance((3, 4), 5.0, 20.0, flat=0.3)
    if name.startswith("flat"):
        s = gr.values(pos, box)[0]
        off = {"flat inside": -0.3, "flat edge side": 1e-3, "flat outside": 0.5}[name]
        flat = np.array([0.4, 0.2, 0.3, 0.25])
        sign = np.array([1.0, -1.0, 1.0, -1.0])
        gr.set_flat(flat)
        gr.set_targets(s - sign * (flat + off))
        if name == "flat inside":  # (one entry outside, so that there is a force to compare with)
            t = gr.target.copy()
            t[0, 0] = s[0] - 1.0
            gr.set_targets(t)
    si = M.sines(gr, pos, box)
    assert si.min() > np.sin(0.3), (name, si)
    assert gr.check_extent(pos, box)
    return gr, pos, box


CASES = ["groups of 1, 2 and 40", "wrapped group", "zero box", "one open axis", "an atom in three groups",
         "a group named by four restraints", "flat inside", "flat edge side", "flat outside", "dihedral across the wrap"]


# ----------------------------------------------------------------------------- the model
@pytest.mark.parametrize("name", CASES)
def test_model_forces_are_minus_the_gradient_of_its_energy(name):
    gr, pos, box = _case(name)
    E, F = gr.energy_forces(pos, box)
    h = 1e-5
    at = gr.atoms()
    num = np.zeros((len(at), 3))
    for n, i in enumerate(at):
        for c in range(3):
            p, m = pos.copy(), pos.copy()
            p[i, c] += h
            m[i, c] -= h
            num[n, c] = -(gr.energy_forces(p, box)[0].sum() - gr.energy_forces(m, box)[0].sum()) / (2 * h)
    scale = np.abs(F).max()
    print(f"{name}: E = {E[0]}, max|F| = {scale:.3f}, |FD - F| = {np.abs(num - F[0, at]).max():.2e}")
    assert scale > (0.01 if name == "flat edge side" else 1.0)  # (k x 1e-3 just outside the flat bottom)
    assert np.abs(num - F[0, at]).max() <= 1e-6 * scale
    others = np.setdiff1d(np.arange(len(pos)), at)
    assert not F[0, others].any()
    if name == "flat inside":
        assert E[0, 1] == 0.0 and E[0, 2] == 0.0  # inside the flat bottom: no energy
    if name == "dihedral across the wrap":
        assert abs(np.sqrt(2 * E[0, 2] / 40.0) - (2 * np.pi - 6.0)) < 1e-12


def test_model_switched_off_entries_and_singular_geometries():
    gr = GroupRestraints(2)
    g = [gr.add_group([i], weights=[1.0]) for i in range(4)]
    gr.add_distance((g[0], g[1]), 1.5, [10.0, 0.0])
    gr.add_angle((g[0], g[1], g[2]), 1.0, 20.0)
    gr.add_dihedral(g, 0.5, 30.0)
    pos = np.zeros((2, 4, 3))
    pos[:, 1] = [1.0, 0.0, 0.0]
    pos[:, 2] = [3.0, 0.0, 0.0]  # collinear with 0 and 1: sin theta = 0, and a degenerate dihedral
    pos[:, 3] = [3.0, 1.0, 0.0]
    pos[1, 0] = pos[1, 1]  # r = 0 in replica 1 (switched off there anyway), a zero arm of the angle
    E, F = gr.energy_forces(pos, np.zeros(3))
    assert E[0, 0] == 0.5 * 10.0 * 0.25 and E[1, 0] == 0.0
    assert E[0, 1] == 0.5 * 20.0 * (np.pi - 1.0) ** 2  # theta = pi: no direction, the energy of the formula
    assert np.isfinite(E).all() and np.isfinite(F).all()
    assert not F[1].any()  # every geometry of replica 1 is singular or off
    assert np.array_equal(F[0, 0], [-5.0, 0.0, 0.0]) and np.array_equal(F[0, 1], [5.0, 0.0, 0.0]) and not F[0, 2:].any()  # (r < r0: apart)


# ----------------------------------------------------------------------------- the header
def test_header_restraint_equals_the_model(gm):
    rng = np.random.default_rng(2)
    worst = 0.0
    for trial in range(300):
        kind = trial % 3
        box = [np.array([L, L, L]), np.zeros(3), np.array([L, 0.0, L])][(trial // 3) % 3]
        X = np.ascontiguousarray(rng.uniform(0.0, L, (4, 3)))
        s0 = rng.uniform(0.2, 3.0) * (1.0 if kind != DIHEDRAL else rng.choice([-1.0, 1.0]))
        k, flat = rng.uniform(1.0, 100.0), rng.choice([0.0, 0.1])
        e, F, _ = restraint_terms(kind, X[: kind + 2], box, s0, k, flat)
        G = np.zeros((4, 3))
        eh = gm.gm_restraint(kind, _dp(X), _dp(np.ascontiguousarray(box)), s0, k, flat, _dp(G))
        rel = np.abs(G - F) / np.maximum(np.abs(F), 1e-300)
        worst = max(worst, rel[F != 0].max() if (F != 0).any() else 0.0, abs(eh - e) / max(abs(e), 1e-300))
        assert np.all(np.abs(G - F) <= 4 * EPS64 * np.abs(F)) and abs(eh - e) <= 4 * EPS64 * abs(e), (trial, kind)
    print(f"header against model, 300 restraints: worst relative difference {worst / EPS64:.2f} eps64")


@pytest.mark.parametrize("name", CASES)
def test_header_walk_equals_the_model(gm, name):
    gr, pos, box = _case(name)
    E, F = gr.energy_forces(pos, box)
    Eh, Fh, Xh = _header(gm, gr, pos, box)
    nmax = max(len(a) for a in gr.group_atoms)
    bar = 64 * nmax * EPS64 * np.abs(F).max()
    print(f"{name}: |F_header - F_model| = {np.abs(Fh - F).max():.2e} (bar {bar:.2e})")
    assert np.abs(Fh - F).max() <= bar
    assert np.abs(Xh - gr.centres(pos, box)).max() <= nmax * EPS64 * 8.0 + 4 * EPS64 * np.abs(Xh).max()
    assert np.abs(Eh - E).max() <= 64 * nmax * EPS64 * np.abs(E).sum() + bar


# ----------------------------------------------------------------------------- invariances
def _evaluators(gm):
    return {"model": lambda gr, pos, box: gr.energy_forces(pos, box), "header": lambda gr, pos, box: _header(gm, gr, pos, box)[:2]}


@pytest.mark.parametrize("which", ["model", "header"])
def test_a_box_vector_on_any_one_atom_changes_nothing(gm, which):
    ev = _evaluators(gm)[which]
    gr, pos, box = _case("wrapped group")
    E, F = ev(gr, pos, box)
    worst = 0.0
    for g, at in enumerate(gr.group_atoms):
        for a in {int(at[0]), int(at[-1]), int(at[len(at) // 2])}:  # the anchor, and two others
            for c in range(3):
                for sign in (-1.0, 1.0):
                    p = pos.copy()
                    p[a, c] += sign * box[c]
                    E2, F2 = ev(gr, p, box)
                    worst = max(worst, np.abs(F2 - F).max() / np.abs(F).max(), np.abs(E2 - E).max() / np.abs(E).max())
    print(f"{which}: a box vector on one atom moves energies and forces by {worst / EPS64:.1f} eps64 relative")
    assert worst <= 64 * EPS64


@pytest.mark.parametrize("which", ["model", "header"])
def test_every_restraint_has_no_net_force_and_no_net_torque(gm, which):
    ev = _evaluators(gm)[which]
    for name in ("groups of 1, 2 and 40", "wrapped group", "zero box", "an atom in three groups"):
        full, pos, box = _case(name)
        for m in range(full.nrestraints):
            one = GroupRestraints(1)
            for g in range(full.ngroups):
                one.add_group(full.group_atoms[g], full.group_weights[g])
            one.masses = full.masses
            kind = int(full.kind[m])
            one._add(kind, full.groups[m, : kind + 2], full.target[:, m], full.k[:, m], 0.0)
            F = ev(one, pos, box)[1][0]
            assert np.abs(F).max() > 0.01
            assert np.abs(F.sum(axis=0)).max() <= 16 * EPS64 * np.abs(F).sum(), (which, name, m)
            if name == "zero box":
                torque = np.cross(pos, F)
                scale = (np.linalg.norm(pos, axis=1) * np.linalg.norm(F, axis=1)).sum()
                assert np.abs(torque.sum(axis=0)).max() <= 16 * EPS64 * scale, (which, m, torque.sum(axis=0), scale)


# ----------------------------------------------------------------------------- single-atom groups
def test_single_atom_distance_is_the_distance_restraint():
    rng = np.random.default_rng(5)
    for box in (np.array([L, L, L]), np.zeros(3), np.array([L, 0.0, L])):
        pos = rng.uniform(0.0, L, (1, 6, 3))
        rs, gr = Restraints(1), GroupRestraints(1)
        g = [gr.add_group([i], weights=[3.0]) for i in range(6)]
        for i, j in ((0, 1), (2, 1), (4, 5), (0, 5)):
            r0, k = rng.uniform(1.0, 12.0), rng.uniform(5.0, 90.0)
            rs.add_distance([[i, j]], r0, k)
            gr.add_distance((g[i], g[j]), r0, k)
        (Er, Fr), (Eg, Fg) = rs.energy_forces(pos, box), gr.energy_forces(pos, box)
        assert np.all(np.abs(Fg - Fr) <= 4 * EPS64 * np.abs(Fr)) and abs(Eg[0, 0] - Er[0, 1]) <= 4 * EPS64 * Er[0, 1]


def test_single_atom_angle_is_the_oracles_angle_term():
    import torch
    from _golden import box_tensor, load, pos_tensor
    from oracle import torchmd_oracle as orc

    g = load("water291")
    pos = np.asarray(g["pos"], dtype=np.float64).reshape(-1, 3)
    box = np.asarray(g["box"], dtype=np.float64).reshape(-1)[:3]
    triples = [(0, 30, 60), (3, 150, 9), (27, 1, 2), (288, 12, 100)]
    rng = np.random.default_rng(6)
    k, th0 = rng.uniform(20.0, 100.0, 4), rng.uniform(0.5, 2.5, 4)
    gr = GroupRestraints(1)
    for (a, b, c), kk, t in zip(triples, k, th0):
        gr.add_angle([gr.add_group([i], weights=[1.0]) for i in (a, b, c)], t, kk)
    assert M.sines(gr, pos, box).min() > 0.2
    E, F = gr.energy_forces(pos, box)
    par = SimpleNamespace(nonbonded_params=None, bond_params=None, dihedral_params=None, improper_params=None, nonbonded_14_params=None,
                          angle_params={"idx": torch.tensor(triples), "map": torch.stack([torch.arange(4), torch.arange(4)], dim=1),
                                        "params": torch.tensor(np.stack([0.5 * k, th0], axis=1))})
    opot, oF, _ = orc.compute(par, pos_tensor(pos, 1, torch.float64), box_tensor(box, 1, torch.float64), ["angles"])
    print(f"angle restraints on water291: E = {E[0, 1]:.9f} (oracle {opot[0]['angles']:.9f}), |dF| = {np.abs(F[0] - oF[0].numpy()).max():.2e}")
    assert np.abs(F).max() > 10.0
    assert np.abs(F[0] - oF[0].numpy()).max() <= 1e-10 * np.abs(F).max()
    assert abs(E[0, 1] - opot[0]["angles"]) <= 1e-10 * E[0, 1] and E[0, 0] == 0.0 and E[0, 2] == 0.0


# ----------------------------------------------------------------------------- plumbing
def test_rows_from_python_and_from_the_c_builder_are_identical(gm):
    for gr in (_case("an atom in three groups")[0], _case("a group named by four restraints")[0], M.kernel_case()[3]):
        off, atoms, W, kind, groups = _tables(gr)[:5]
        nm, M4 = len(atoms), 4 * gr.nrestraints
        use_off, use = np.zeros(gr.ngroups + 1, np.int32), np.zeros((M4, 2), np.int32)
        rows, mem_off, mem = np.zeros(nm, np.int32), np.zeros(nm + 1, np.int32), np.zeros((nm, 2), np.int32)
        n = gm.gm_rows(gr.ngroups, _ip(off), _ip(atoms), gr.nrestraints, _ip(kind), _ip(groups), _ip(use_off), _ip(use), _ip(rows),
                       _ip(mem_off), _ip(mem))
        p_use_off, p_use, p_atoms, p_mem_off, p_mem = gr.build_rows()
        assert n == len(p_atoms) and np.array_equal(rows[:n], p_atoms) and np.array_equal(mem_off[: n + 1], p_mem_off)
        assert np.array_equal(use_off, p_use_off) and np.array_equal(use[: use_off[-1]], p_use)
        assert np.array_equal(mem[: mem_off[n]], p_mem)
        assert (np.diff(p_atoms) > 0).all()
        for t in range(n):  # an atom's memberships by ascending group, a group's restraints by ascending index
            assert (np.diff(p_mem[p_mem_off[t] : p_mem_off[t + 1], 0]) > 0).all()
        for g in range(gr.ngroups):
            assert (np.diff(p_use[p_use_off[g] : p_use_off[g + 1], 0]) > 0).all()
        w = np.zeros(nm)
        gm.gm_normalise(gr.ngroups, _ip(off), _dp(W), _dp(w))
        assert np.array_equal(w, np.concatenate([gr.weights(g) for g in range(gr.ngroups)]))
    three = _case("an atom in three groups")[0]
    shared = int(three.group_atoms[1][1])
    _, _, p_atoms, p_mem_off, p_mem = three.build_rows()
    t = int(np.searchsorted(p_atoms, shared))
    assert p_mem[p_mem_off[t] : p_mem_off[t + 1], 0].tolist() == [1, 2, 3]


def test_what_the_c_validation_refuses(gm):
    gr = _case("a group named by four restraints")[0]
    N = 51

    def why(change=None, natoms=N, nrep=1):
        keep = [a.copy() for a in _tables(gr)]
        if change:
            change(keep)
        off, atoms, W, kind, groups, target, k, flat = keep
        buf = C.create_string_buffer(256)
        n = gm.gm_validate(natoms, nrep, len(off) - 1, _ip(off), _ip(atoms), _dp(W), len(kind), _ip(kind), _ip(groups), _dp(target), _dp(k),
                           _dp(flat), buf, 256)
        return buf.value.decode() if n else ""

    def poke(index, where, value):
        def change(keep):
            keep[index].reshape(-1)[where] = value
        return change

    assert why() == ""
    assert "empty" in why(poke(0, 1, 0))
    assert "named twice" in why(poke(1, 2, gr.group_atoms[1][0]))
    assert "out of range" in why(poke(1, 0, N)) and "out of range" in why(poke(1, 0, -1)) and "out of range" in why(natoms=10)
    for bad in (0.0, -1.0, np.nan, np.inf):
        assert "weights" in why(poke(2, 5, bad))
    assert "a group is named twice" in why(poke(4, 1, 2))  # the distance (2, 0) -> (2, 2)
    assert "wrong number of groups" in why(poke(4, 2, 1)) and "wrong number of groups" in why(poke(4, 4 + 2, -1))
    assert "group index out of range" in why(poke(4, 0, 5))
    assert "unknown kind" in why(poke(3, 0, 3))
    for bad in (-1.0, np.nan, np.inf):
        assert "finite k" in why(poke(6, 1, bad)) and "finite flat" in why(poke(7, 1, bad))
    assert "finite target" in why(poke(5, 0, np.nan)) and "finite target" in why(poke(5, 2, np.inf))
    assert "[0, pi]" in why(poke(5, 1, 3.2)) and "[0, pi]" in why(poke(5, 1, -0.1))
    assert why(poke(5, 2, -7.0)) == ""  # (a dihedral target is any finite number)


def test_what_python_refuses():
    gr = GroupRestraints(2)
    with pytest.raises(ValueError, match="whole number"):
        GroupRestraints(0)
    with pytest.raises(ValueError, match="non-empty"):
        gr.add_group([])
    with pytest.raises(ValueError, match="named twice"):
        gr.add_group([1, 2, 1])
    with pytest.raises(ValueError, match="non-negative"):
        gr.add_group([1, -2])
    for bad in ([1.0, 0.0], [1.0, -1.0], [1.0, np.nan], [1.0, np.inf], [1.0]):
        with pytest.raises(ValueError, match="weights"):
            gr.add_group([1, 2], weights=bad)
    a, b, c, d = (gr.add_group([i, i + 10]) for i in range(4))
    with pytest.raises(ValueError, match="named twice"):
        gr.add_distance((a, a), 1.0, 1.0)
    with pytest.raises(ValueError, match="wrong number of groups"):
        gr.add_angle((a, b), 1.0, 1.0)
    with pytest.raises(ValueError, match="wrong number of groups"):
        gr.add_dihedral((a, b, c), 1.0, 1.0)
    with pytest.raises(ValueError, match="out of range"):
        gr.add_distance((a, 4), 1.0, 1.0)
    for bad in (-1.0, np.nan, np.inf):
        with pytest.raises(ValueError, match="k must be finite"):
            gr.add_distance((a, b), 1.0, bad)
        with pytest.raises(ValueError, match="flat must be finite"):
            gr.add_distance((a, b), 1.0, 1.0, flat=bad)
    with pytest.raises(ValueError, match="target must be finite"):
        gr.add_dihedral((a, b, c, d), np.nan, 1.0)
    with pytest.raises(ValueError, match=r"\[0, pi\]"):
        gr.add_angle((a, b, c), 3.2, 1.0)
    with pytest.raises(ValueError, match="scalar or"):
        gr.add_distance((a, b), [1.0, 2.0, 3.0], 1.0)
    assert gr.nrestraints == 0 and gr.descriptor()[0].enable == 0
    i = gr.add_distance((a, b), [1.0, 2.0], 5.0)
    j = gr.add_angle((a, b, c), 1.0, [0.0, 3.0], flat=0.1)
    assert (i, j) == (0, 1) and gr.k.tolist() == [[5.0, 0.0], [5.0, 3.0]] and gr.groups.tolist() == [[0, 1, -1, -1], [0, 1, 2, -1]]
    with pytest.raises(ValueError, match=r"\[0, pi\]"):
        gr.set_targets([[1.0, 4.0], [1.0, 1.0]])
    # what a Forces refuses: an index beyond the system, a massless member, a virtual site; groups without weights need masses
    with pytest.raises(ValueError, match="needs masses"):
        gr.energy_forces(np.zeros((2, 20, 3)), np.zeros(3))
    with pytest.raises(ValueError, match="beyond the system"):
        gr.check(13)
    m = np.ones(20)
    m[11] = 0.0
    with pytest.raises(ValueError, match="no mass"):
        gr.check(20, m)
    with pytest.raises(ValueError, match="virtual site"):
        gr.check(20, np.ones(20), SimpleNamespace(nsites=1, sites=[12]))
    v = gr.version
    gr.check(20, np.ones(20))
    assert gr.version == v + 1  # (the default weights arrived: one upload)
    gr.check(20, np.ones(20))
    assert gr.version == v + 1
    assert set(gr.refusals) == {"vmap", "batch", "barostat", "pressure", "update_atoms", "domain"}
    assert gr.refusal("exchange") is None and gr.side_width == 3 and gr.side_name == "group_restraints"
    from torchmd_amd import forces

    assert forces.SIDE_TERMS[-1] == "group_restraints"
    import torchmd_amd
    from torchmd_amd.domain import DomainSet

    assert torchmd_amd.GroupRestraints is GroupRestraints and "GroupRestraints" in torchmd_amd.__all__
    with pytest.raises(ValueError, match="group restraints cannot be domain-decomposed"):
        DomainSet(np.full(3, 30.0), 2, "cpu", None, ["lj"], 9.0, dry=True, group_restraints=gr)


def test_check_extent():
    gr = GroupRestraints(1)
    gr.add_group([0, 1, 2], weights=[1.0, 1.0, 1.0])
    box = np.array([L, L, 0.0])
    pos = np.array([[1.0, 1.0, 1.0], [19.0, 3.0, 500.0], [4.0, 18.0, -300.0]])  # whole across two faces, open along z
    assert gr.check_extent(pos, box)
    pos[1, 0] = 11.0  # half an edge from the anchor
    assert not gr.check_extent(pos, box)
    pos[1, 0] = 10.9
    assert gr.check_extent(pos, box) and gr.check_extent(pos[None], box[None])


def test_exchange_round_trip_restores_the_tables_bit_for_bit():
    pos, box, mass, gr = M.kernel_case(R=4, seed=5)
    before = (gr.target.copy(), gr.k.copy(), gr.flat.copy())
    with pytest.raises(ValueError, match="4 replicas"):
        gr.exchange_parameters(3)
    snap = gr.exchange_parameters(4)
    perm = np.array([2, 0, 3, 1])
    v = gr.version
    gr.assign_states(snap, perm)
    assert gr.version == v + 1 and np.array_equal(snap["state_of_slot"], perm)
    assert np.array_equal(gr.target, before[0][perm]) and np.array_equal(gr.k, before[1][perm]) and np.array_equal(gr.flat, before[2][perm])
    E = gr.energy_forces(pos, box)[0]
    gr.assign_states(snap, np.arange(4))
    assert gr.version == v + 2
    for a, b in zip((gr.target, gr.k, gr.flat), before):
        assert a.tobytes() == b.tobytes()
    assert GroupRestraints(4).exchange_parameters(4) is None
    assert not np.array_equal(E, gr.energy_forces(pos, box)[0])


def test_from_npz_rebuilds_the_tables(tmp_path):
    pos, box, mass, gr = M.kernel_case(R=3)
    off, atoms, W, kind, groups, target, k, flat = _tables(gr)
    path = str(tmp_path / "gr.npz")
    np.savez(path, group_off=off, member_atom=atoms, member_weight=W, kind=kind, groups=groups, target=target, k=k, flat=flat)
    back = GroupRestraints.from_npz(path, 3)
    for a, b in zip(_tables(back), _tables(gr)):
        assert np.array_equal(a, b)
    np.savez(path, group_off=off, member_atom=atoms, kind=kind, groups=groups, target=target[0], k=7.0)
    back = GroupRestraints.from_npz(path, 3)
    assert back.group_weights[0] is None and (back.k == 7.0).all() and (back.flat == 0.0).all() and np.array_equal(back.target[2], target[0])
    assert back.monitor_columns() == ("group_restraints",)


# ----------------------------------------------------------------------------- the Boresch set
def test_boresch_set_and_its_standard_state_correction():
    from torchmd_amd.integrator import BOLTZMAN

    T, K, r0 = 300.0, 20.0, 6.0
    thA, thB = np.pi / 2 + 0.3, np.pi / 2 - 0.3
    gr = GroupRestraints.boresch(2, receptor=(10, 11, 12), ligand=(40, 41, 42), r0=r0, theta_a0=thA, theta_b0=thB, phi_a0=0.5,
                                 phi_b0=-1.0, phi_c0=2.0, k_r=K, k_theta=K, k_phi=K)
    assert [a.tolist() for a in gr.group_atoms] == [[10], [11], [12], [40], [41], [42]]
    assert gr.kind.tolist() == [DISTANCE, ANGLE, ANGLE, DIHEDRAL, DIHEDRAL, DIHEDRAL]
    assert gr.groups.tolist() == [[0, 3, -1, -1], [1, 0, 3, -1], [0, 3, 4, -1], [2, 1, 0, 3], [1, 0, 3, 4], [0, 3, 4, 5]]
    got = gr.boresch_standard_state(T)
    kT = BOLTZMAN * T
    x = np.linspace(0.0, 1.0, 200001)

    def integral(f, lo, hi):  # composite Simpson
        y = f(lo + (hi - lo) * x)
        return (hi - lo) / (len(x) - 1) / 3.0 * (y[0] + y[-1] + 4.0 * y[1:-1:2].sum() + 2.0 * y[2:-1:2].sum())

    Z = integral(lambda r: r * r * np.exp(-0.5 * K * (r - r0) ** 2 / kT), 0.0, r0 + 10.0)
    for t0 in (thA, thB):
        Z *= integral(lambda t: np.sin(t) * np.exp(-0.5 * K * (t - t0) ** 2 / kT), 0.0, np.pi)
    Z *= integral(lambda d: np.exp(-0.5 * K * d * d / kT), -np.pi, np.pi) ** 3
    want = -kT * np.log(8.0 * np.pi**2 * 1660.5392 / Z)
    print(f"Boresch correction: analytic {got[0]:.4f}, quadrature {want:.4f} kcal/mol")
    assert got.shape == (2,) and got[0] == got[1] and abs(got[0] - want) <= 0.03
    assert -12.0 < got[0] < -5.0
    gr.set_flat(0.1)
    with pytest.raises(ValueError, match="flat = 0"):
        gr.boresch_standard_state(T)
    with pytest.raises(ValueError, match="not built by"):
        M.kernel_case()[3].boresch_standard_state(T)
