"""The pressure observable without a GPU: the numpy model of tests/_pressure.py against central differences of
its own energy under rigid molecular scaling, its reciprocal-space part against central differences of
`_ewald.pme_reciprocal`'s energy, the host build of virial_math.h against the model, and what Python refuses.

Bars.  Finite differences of the model: eps is halved from 1e-5 until the model counts the same pairs at 1 -+ eps, 1 -+ eps / 2
and 1 (an unswitched cutoff makes U jump, a reaction field makes dU/dr jump); the bar is 10 |FD(eps) - FD(eps / 2)| + 64 eps64 S,
the one of the GPU test.  Host build against model: the same IEEE operations up to the association of a product: 4 eps64 of
|f_a| (|d_a| / 2 + |delta_a|) per pair.  Translation of whole molecules by box multiples: 64 eps64 S."""

import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

import _ewald as E
import _pressure as M

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "torchmd_amd", "csrc")
EPS64 = np.finfo(np.float64).eps
WATER_TERMS = ["lj", "electrostatics", "bonds", "angles"]
CASES = {
    "lj_rf": (("lj", "electrostatics"), dict(rfa=True)),
    "coul": (("electrostatics",), dict()),
    "lj_sw_exact": (("lj",), dict(switch_dist=5.0, switch_mode="exact")),
    "repulsion": (("repulsion",), dict()),
}
CUTOFF = 6.0
_SYS = {}


def _water(nside=4, seed=6):
    from torchmd_amd.builders import tip3p_box, water_forcefield
    from torchmd_amd.forces import build_exclusion_csr
    from torchmd_amd.parameters import Parameters

    if (nside, seed) not in _SYS:
        mol, pos, box = tip3p_box(nside, seed=seed)
        par = Parameters(water_forcefield(mol), mol, WATER_TERMS, precision=torch.float64)
        excl = build_exclusion_csr(mol.numAtoms, par.get_exclusions(("bonds", "angles", "1-4")))
        _SYS[(nside, seed)] = (np.asarray(pos, dtype=np.float64), np.asarray(box, dtype=np.float64), par, excl, mol)
    return _SYS[(nside, seed)]


@pytest.mark.parametrize("case", list(CASES))
def test_model_virial_is_minus_the_derivative_of_its_energy_under_rigid_molecular_scaling(case):
    pos, box, par, excl, _ = _water()
    terms, opts = CASES[case]
    sysm = M.system_of(par, terms, excl)
    m = M.nonbonded_model(pos, box, sysm, terms, CUTOFF, **opts)
    assert m.npairs > 5000
    for a in range(3):
        def at(lam):
            s = np.ones(3)
            s[a] = lam
            r = M.nonbonded_model(*M.scale_molecules(pos, box, sysm, s), sysm, terms, CUTOFF, **opts)
            return r.U, r.npairs

        eps = 1e-5
        for _ in range(12):
            v = {k: at(1.0 + k * eps) for k in (-1.0, -0.5, 0.5, 1.0)}
            if all(x[1] == m.npairs for x in v.values()):
                break
            eps /= 2
        else:
            pytest.fail("no eps with a constant pair count")
        fd1, fd2 = -(v[1.0][0] - v[-1.0][0]) / (2 * eps), -(v[0.5][0] - v[-0.5][0]) / eps
        bar = 10 * abs(fd1 - fd2) + 64 * EPS64 * m.S[a]
        print(f"{case} axis {a}: eps {eps:.3g}, W = {m.W[a]!r}, FD = {fd1!r}, |d| = {abs(m.W[a] - fd1):.2e}, bar {bar:.2e}")
        assert abs(m.W[a] - fd1) <= bar and abs(m.W[a]) > 100 * bar


def test_reciprocal_model_against_differences_of_pme_reciprocal():
    pos, box, par, excl, _ = _water()
    sysm = M.system_of(par, ("electrostatics",), excl)
    sysm.charges = sysm.charges.copy()
    sysm.charges[0] += 0.7  # a net charge: the background has a value
    beta, grid, order = 0.35, (15, 17, 19), 5
    m = M.reciprocal_model(pos, box, sysm, beta, grid, order)
    assert abs(m.background) > 0.1
    for a in range(3):
        s = np.ones(3)
        eps = 1e-6
        # box and ALL positions scaled: the modes' part alone
        s[a] = 1 + eps
        ep = E.pme_reciprocal(pos * s, sysm.charges, box * s, beta, grid, order)[0]
        s[a] = 1 - eps
        em = E.pme_reciprocal(pos * s, sysm.charges, box * s, beta, grid, order)[0]
        fd = -(ep - em) / (2 * eps)
        print(f"axis {a}: modes {m.modes[a]!r}, FD {fd!r}")
        assert abs(fd - m.modes[a]) <= 1e-7 * m.S_modes[a]
        # box and molecule centres scaled: modes - delta . F
        s[a] = 1 + eps
        ep = E.pme_reciprocal(*M.scale_molecules(pos, box, sysm, s)[:1], sysm.charges, box * s, beta, grid, order)[0]
        s[a] = 1 - eps
        em = E.pme_reciprocal(*M.scale_molecules(pos, box, sysm, s)[:1], sysm.charges, box * s, beta, grid, order)[0]
        fd = -(ep - em) / (2 * eps)
        assert abs(fd - (m.modes[a] + m.correction[a])) <= 1e-7 * (m.S_modes[a] + m.S_dF[a])
    # the background: E ~ 1 / V
    V = np.prod(box)
    assert abs(m.background - (-E.KE * np.pi * sysm.charges.sum() ** 2 / (2 * V * beta**2))) <= 4 * EPS64 * abs(m.background)


def test_molecules_of_one_molecular_and_atomic_virial_agree():
    from torchmd_amd.builders import argon_forcefield, lj_box
    from torchmd_amd.forces import build_exclusion_csr
    from torchmd_amd.parameters import Parameters

    mol, pos, box = lj_box(5, seed=2)
    par = Parameters(argon_forcefield(mol), mol, ["lj"], precision=torch.float64)
    sysm = M.system_of(par, ("lj",), build_exclusion_csr(mol.numAtoms, []))
    assert len(sysm.off) - 1 == mol.numAtoms
    m = M.nonbonded_model(pos, box, sysm, ("lj",), 7.0)
    # the atomic virial sum_{i<j} f_ij,a d_ij,a, written out
    p = np.asarray(pos, dtype=np.float64)
    i, j = np.triu_indices(len(p), k=1)
    d = p[i] - p[j]
    d -= box * np.rint(d / box)
    r = np.sqrt((d * d).sum(axis=1))
    keep = r <= 7.0
    A, B = sysm.A[0, 0], sysm.B[0, 0]
    dEdr = -12 * A / r**13 + 6 * B / r**7
    W = (-(dEdr / r)[:, None] * d * d)[keep].sum(axis=0)
    assert keep.sum() == m.npairs and (np.abs(W - m.W) <= 64 * EPS64 * m.S).all()


@pytest.mark.parametrize("case", ["lj_rf", "coul"])
def test_translating_whole_molecules_by_box_multiples_leaves_the_virial(case):
    pos, box, par, excl, _ = _water()
    terms, opts = CASES[case]
    sysm = M.system_of(par, terms, excl)
    m = M.nonbonded_model(pos, box, sysm, terms, CUTOFF, **opts)
    k = np.random.default_rng(4).integers(-3, 4, size=(len(sysm.off) - 1, 3)).astype(np.float64)
    m2 = M.nonbonded_model(pos + (k * box)[sysm.mol_of], box, sysm, terms, CUTOFF, **opts)
    print(f"{case}: |dW| = {np.abs(m.W - m2.W)}, bar {64 * EPS64 * m.S}")
    assert m2.npairs == m.npairs and (np.abs(m.W - m2.W) <= 64 * EPS64 * m.S).all()
    # and it is not the atomic virial: moving single atoms of a molecule by a box edge changes delta, and W with it
    broken = pos.copy()
    broken[1::3] += box
    assert np.abs(M.nonbonded_model(broken, box, sysm, terms, CUTOFF, **opts).W - m.W).max() > 1.0


# ---------------------------------------------------------------- the compiled header
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
def vm(tmp_path_factory):
    cxx = next((c for c in (os.environ.get("CXX"), "g++", "c++", "clang++") if c and shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler (CXX, g++, c++, clang++) found: virial_math.h is not checked on the CPU")
    inc = _rocm_include()
    if inc is None:
        pytest.skip("the HIP headers (hip/hip_runtime.h) of a ROCm installation were not found: virial_math.h is not checked on the CPU")
    out = str(tmp_path_factory.mktemp("virial_math") / "libvirial_math_host.so")
    cmd = [cxx, "-std=c++17", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-D__HIP_PLATFORM_AMD__", f"-I{inc}", f"-I{CSRC}",
           os.path.join(HERE, "virial_math_host.cpp"), "-o", out]
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, " ".join(cmd) + "\n" + res.stdout + res.stderr
    lib = C.CDLL(out)
    dp, fp, ip = C.POINTER(C.c_double), C.POINTER(C.c_float), C.POINTER(C.c_int32)
    lib.vm_pair_f64.restype = lib.vm_pair_f32.restype = lib.vm_finish.restype = None
    lib.vm_pair_f64.argtypes = [dp, C.c_double, dp, dp]
    lib.vm_pair_f32.argtypes = [fp, C.c_float, dp, dp]
    lib.vm_mode_factor.restype = C.c_double
    lib.vm_mode_factor.argtypes = [C.c_double] * 3
    lib.vm_finish.argtypes = [dp] * 4
    lib.vm_validate.restype = C.c_int
    lib.vm_validate.argtypes = [C.c_int64, C.c_int64, ip, ip, ip, C.c_char_p, C.c_int]
    return lib


def _p(a, t):
    return a.ctypes.data_as(C.POINTER(t))


def test_header_pair_contribution_equals_model(vm):
    rng = np.random.default_rng(0)
    worst = 0.0
    for _ in range(2000):
        d = rng.uniform(-9, 9, 3)
        delta = rng.uniform(-1, 1, 3) * rng.choice([0.0, 1.0, 30.0])
        fs = rng.normal() * 10.0 ** rng.integers(-3, 3)
        w = rng.normal(size=3)
        want = w + (-(d * fs)) * (0.5 * d - delta)
        got = w.copy()
        vm.vm_pair_f64(_p(d, C.c_double), fs, _p(delta, C.c_double), _p(got, C.c_double))
        scale = np.abs(w) + np.abs(d * fs) * (0.5 * np.abs(d) + np.abs(delta))
        worst = max(worst, (np.abs(got - want) / (EPS64 * scale)).max())
        # fp32: the force component is rounded in float as the pair kernels form it, everything after that in double
        d32, fs32 = d.astype(np.float32), np.float32(fs)
        f32 = -(d32 * fs32)
        assert f32.dtype == np.float32
        want32 = w + f32.astype(np.float64) * (0.5 * d32.astype(np.float64) - delta)
        got32 = w.copy()
        vm.vm_pair_f32(_p(d32, C.c_float), fs32, _p(delta, C.c_double), _p(got32, C.c_double))
        worst = max(worst, (np.abs(got32 - want32) / (EPS64 * scale)).max())
    print(f"header against model: worst {worst:.2f} eps64 of the scale")
    assert worst <= 4


def test_header_sums_a_model_system(vm):
    """The header's pair contribution over every ordered pair of a small box reproduces the model's W."""
    pos, box, par, excl, _ = _water(3, 2)
    terms, opts = CASES["lj_rf"]
    sysm = M.system_of(par, terms, excl)
    cutoff = 4.5
    m = M.nonbonded_model(pos, box, sysm, terms, cutoff, **opts)
    _, delta, _ = M.molecule_centres(pos, sysm.mass, sysm.off, sysm.mem, sysm.mol_of)
    from _pair_reference import ELEC_FACTOR, pair_partials

    n = len(pos)
    keys = set(M._exclusion_keys(excl, n).tolist())
    w = np.zeros(3)
    count = 0
    for i in range(n):
        for j in range(n):
            if i == j or i * n + j in keys:
                continue
            d = M.engine_delta(pos, np.array([i]), np.array([j]), box)[0]
            r = np.sqrt((d * d).sum())
            if r > cutoff:
                continue
            qq = ELEC_FACTOR * sysm.charges[i] * sysm.charges[j]
            _, fpart, _, _ = pair_partials(np.array([r]), sysm.A[sysm.types[i], sysm.types[j]], sysm.B[sysm.types[i], sysm.types[j]],
                                           np.array([qq]), terms, cutoff=cutoff, **opts)
            fs = float(sum(fpart)[0] / r)
            vm.vm_pair_f64(_p(np.ascontiguousarray(d), C.c_double), fs, _p(np.ascontiguousarray(delta[i]), C.c_double), _p(w, C.c_double))
            count += 1
    assert count == 2 * m.npairs
    print(f"header over {count} ordered pairs: |dW| = {np.abs(w - m.W)}, bar {(64 + count) * EPS64 * m.S}")
    assert (np.abs(w - m.W) <= (64 + count) * EPS64 * m.S).all()


def test_header_mode_factor_and_finish(vm):
    rng = np.random.default_rng(1)
    for _ in range(200):
        f = rng.uniform(-0.5, 0.5, 3)
        m2, beta = float((f * f).sum()), float(rng.uniform(0.2, 0.5))
        for a in range(3):
            want = 1.0 - 2.0 * (1.0 + np.pi**2 * m2 / beta**2) * f[a] ** 2 / m2
            assert abs(vm.vm_mode_factor(m2, float(f[a] ** 2), beta) - want) <= 4 * EPS64 * (1 + abs(want))
    # isotropic modes: the three factors sum to 3 - 2 (1 + pi^2 m^2 / beta^2), the trace of Essmann's eq. 2.20
    assert abs(sum(vm.vm_mode_factor(0.03, 0.01, 0.3) for _ in range(3)) - (3 - 2 * (1 + np.pi**2 * 0.03 / 0.09))) < 1e-12
    kin, w, box, out = np.array([1.0, 2.0, 3.0]), np.array([-4.0, 5.5, 0.25]), np.array([10.0, 11.0, 12.5]), np.zeros(8)
    vm.vm_finish(_p(kin, C.c_double), _p(w, C.c_double), _p(box, C.c_double), _p(out, C.c_double))
    assert np.array_equal(out[:3], kin) and np.array_equal(out[3:6], w) and out[6] == 1375.0
    assert abs(out[7] - (kin.sum() + w.sum()) / (3 * 1375.0)) <= 4 * EPS64 * abs(out[7])


def _validate(vm, natoms, off, mem):
    off, mem = np.asarray(off, dtype=np.int32), np.asarray(mem, dtype=np.int32)
    mol_of = np.full(natoms, -7, dtype=np.int32)
    why = C.create_string_buffer(256)
    vm.vm_validate(natoms, len(off) - 1, _p(off, C.c_int32), _p(mem, C.c_int32), _p(mol_of, C.c_int32), why, 256)
    return why.value.decode(), mol_of


def test_library_refusals_of_a_molecule_table(vm):
    why, mol_of = _validate(vm, 5, [0, 2, 3, 5], [3, 0, 2, 4, 1])
    assert why == "" and mol_of.tolist() == [0, 2, 1, 0, 2]
    assert "two molecules" in _validate(vm, 5, [0, 2, 3, 5], [3, 0, 2, 3, 1])[0]
    assert "out of range" in _validate(vm, 5, [0, 2, 3, 5], [3, 0, 2, 5, 1])[0]
    assert "out of range" in _validate(vm, 5, [0, 2, 3, 5], [3, 0, -1, 4, 1])[0]
    assert "empty" in _validate(vm, 5, [0, 2, 2, 5], [3, 0, 2, 4, 1])[0]
    assert "0 to natoms" in _validate(vm, 5, [0, 2, 3, 4], [3, 0, 2, 4, 1])[0]
    assert "0 to natoms" in _validate(vm, 5, [1, 2, 3, 5], [3, 0, 2, 4, 1])[0]
    assert "1 .. natoms" in _validate(vm, 2, [0, 1, 1, 2], [0, 1])[0]


# ---------------------------------------------------------------- Python
def test_molecule_table_and_python_refusals():
    from torchmd_amd import pressure as P
    from torchmd_amd.builders import tip4p_box
    from torchmd_amd.domain import DomainSet
    from torchmd_amd.forces import build_exclusion_csr

    off, mem, mol_of = P.molecule_table(6, np.array([[0, 1], [4, 5], [1, 2]]))
    assert off.tolist() == [0, 3, 4, 6] and mem.tolist() == [0, 1, 2, 3, 4, 5] and mol_of.tolist() == [0, 0, 0, 1, 2, 2]
    assert off.dtype == mem.dtype == mol_of.dtype == np.int32
    P.check_molecules(mol_of, build_exclusion_csr(6, [[0, 2], [4, 5]]))
    with pytest.raises(ValueError, match="two molecules"):
        P.check_molecules(mol_of, build_exclusion_csr(6, [[0, 2], [2, 3]]))
    # a virtual site belongs to its parents' molecule, also without a bond of its own
    mol, pos, box, vs = tip4p_box(2, seed=1)
    bonds = np.asarray(mol.bonds)
    bonds = bonds[~np.isin(bonds, vs.sites).any(axis=1)]
    off, mem, mol_of = P.molecule_table(mol.numAtoms, bonds, vs)
    assert np.all(np.diff(off) == 4) and np.array_equal(mol_of, np.arange(mol.numAtoms) // 4)
    P.check_molecules(mol_of, build_exclusion_csr(mol.numAtoms, vs.exclusion_pairs().tolist()), vs)
    wrong = mol_of.copy()
    wrong[vs.parents[0, 1]] = mol_of.max() + 1
    with pytest.raises(ValueError, match="virtual site"):
        P.check_molecules(wrong, build_exclusion_csr(mol.numAtoms, []), vs)
    with pytest.raises(ValueError, match="box edge"):
        P.check_edges([[10.0, 0.0, 10.0]])
    P.check_edges([[10.0, 11.0, 12.0]])
    assert abs(P.to_bar(P.BAR_TO_KCAL_MOL_A3) - 1.0) < 1e-15
    with pytest.raises(ValueError, match="domain decomposition"):
        DomainSet.pressure(None)
    with pytest.raises(ValueError, match="domain decomposition"):
        DomainSet.pressure_tensor(None)


def test_public_surface(tmp_path):
    import inspect

    from torchmd_amd import _lib, run
    from torchmd_amd.forces import Forces
    from torchmd_amd.integrator import Integrator

    assert callable(Forces.virial) and callable(Integrator.pressure) and callable(Integrator.pressure_tensor)
    for fn in (Forces.virial, Integrator.pressure, Integrator.pressure_tensor):
        doc = inspect.getdoc(fn)
        assert doc and ("external" in doc or "pressure_tensor" in doc)
    assert "tmdhip_pressure" in _lib.SIGNATURES and "tmdhip_set_molecules" in _lib.SIGNATURES
    lib = _lib.load()
    assert hasattr(lib, "tmdhip_pressure") and hasattr(lib, "tmdhip_set_molecules")
    header = open(os.path.join(os.path.dirname(HERE), "include", "tmdhip.h")).read()
    assert "tmdhip_molecule_desc" in header and C.sizeof(_lib.MoleculeDesc) == 24
    assert run.DEFAULTS["pressure"] is False
    log = ["--log-dir", str(tmp_path)]  # (get_args echoes the configuration into its log directory)
    assert run.get_args(["--pressure"] + log).pressure is True and run.get_args(log).pressure is False
