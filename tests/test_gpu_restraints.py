"""Harmonic position and distance restraints on the device: the kernel of restraint.hip against the numpy model
(`Restraints.energy_forces`), `Forces(restraints=)` against the oracle with the restraints appended to its bond list, and
`Integrator.step` under restraints — where the restraint force never enters the pair or step kernels but is applied as an
impulse between their launches — against a loop made by hand of parts that know nothing of restraints.

Bars.  Kernel against model: both sum a row's forces in double in the same order and round once on the store, so one ulp of the
dtype per component is room for the association of a product, no more; energies are sums of M non-negative terms taken in
another order: M eps64 sum|terms|.  Trajectories: fp64 within 64 eps64 x steps x max|pos| (max|vel|) of the by-hand loop, the
two being the same arithmetic up to where a_r is added; fp32 within twice the deviation of the by-hand fp32 loop from the fp64
truth, measured here — the rounding noise of the existing kernels — with a control (k halved in the model) that must miss the
bar by more than 10x."""

import ctypes as C
import os

import numpy as np
import pytest
import torch

import _restraints as M
from _golden import PREC, GoldenParameters, box_tensor, load, pos_tensor
from torchmd_amd.restraints import Restraints

pytestmark = pytest.mark.gpu

NP = {"f32": np.float32, "f64": np.float64}
EPS64 = np.finfo(np.float64).eps
WATER_TERMS = ["lj", "electrostatics", "bonds", "angles"]
FTOL = {"f64": 1e-8, "f32": 3e-4}  # tests/test_gpu_parity.py: forces, energies (relative, x EFAC)
ERTOL = {"f64": 1e-10, "f32": 2e-5}
EFAC = 3


def _dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _bits(t):
    return t.cpu().contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int64)


def _tensor(a, prec):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=PREC[prec]).to(_dev()).contiguous()


def _stream(dev):
    return C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


class _BarePar:
    """What `Forces(terms=[])` asks of its parameters: a context with atoms and no force term of its own."""

    def __init__(self, mass, dtype):
        self.masses = torch.tensor(mass, dtype=dtype)
        self.charges = torch.zeros(len(mass), dtype=dtype)
        self.nonbonded_params = None
        self.bond_params = self.angle_params = self.dihedral_params = self.improper_params = self.nonbonded_14_params = None
        self.mapped_atom_types = torch.zeros(len(mass), dtype=torch.int64)
        self.natoms = len(mass)

    def get_exclusions(self, types=("bonds", "angles", "1-4"), fullarray=False):
        return []


def _context(mass, rs, prec, R):
    """(Forces, engine) of a context that holds nothing but the restraints."""
    from torchmd_amd.forces import Forces

    f = Forces(_BarePar(mass, PREC[prec]), terms=[], restraints=rs)
    eng = f._engine(torch.zeros(R, len(mass), 3, dtype=PREC[prec], device=_dev()))
    eng.sync_restraints(rs)
    return f, eng


def _apply(eng, pos, box, forces=None, vel=None, mass=None, kick=0.0, energies=None, check=True):
    from torchmd_amd import _lib as L

    boxes = np.ascontiguousarray(np.broadcast_to(np.asarray(box, dtype=np.float64).reshape(-1, 3), (pos.shape[0], 3)))
    ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p()  # noqa: E731
    rc = eng.lib.tmdhip_restraint_apply(eng.ctx, ptr(pos), boxes.ctypes.data_as(C.POINTER(C.c_double)), ptr(forces), ptr(vel), ptr(mass),
                                        float(kick), ptr(energies), _stream(pos.device))
    return L.check(rc, "tmdhip_restraint_apply") if check else rc


def _ulp(want, prec):
    return np.spacing(np.abs(want).astype(NP[prec])).astype(np.float64)


def _kernel_against_model(prec, pos, box, mass, rs, repeats):
    R, N = pos.shape[:2]
    rng = np.random.default_rng(99)
    pos = pos.astype(NP[prec]).astype(np.float64)  # the model sees the positions the device holds
    mass = mass.astype(NP[prec]).astype(np.float64)
    f_in = rng.normal(0.0, 20.0, (R, N, 3)).astype(NP[prec]).astype(np.float64)
    v_in = rng.normal(0.0, 0.05, (R, N, 3)).astype(NP[prec]).astype(np.float64)
    kick = 0.0123
    E, F = rs.energy_forces(pos, box)
    touched = np.zeros(N, dtype=bool)
    touched[rs.atoms()] = True
    _, eng = _context(mass, rs, prec, R)
    p, m = _tensor(pos, prec), _tensor(mass, prec)

    def once(mode):
        f, v = _tensor(f_in, prec), _tensor(v_in, prec)
        e = torch.full((R, 2), -1.0, dtype=torch.float64, device=_dev())
        if mode == "finish":
            _apply(eng, p, box, forces=f, vel=v, mass=m, kick=kick, energies=e)
        elif mode == "impulse":
            _apply(eng, p, box, vel=v, mass=m, kick=kick)
        else:
            _apply(eng, p, box, forces=f, energies=e)
        return f, v, e

    f, v, e = once("finish")
    want_f = (f_in + F).astype(NP[prec]).astype(np.float64)
    want_v = (v_in + kick * F / mass[None, :, None]).astype(NP[prec]).astype(np.float64)
    got_f, got_v = f.cpu().double().numpy(), v.cpu().double().numpy()
    df = np.abs(got_f - want_f) / _ulp(want_f, prec)
    dv = np.abs(got_v - want_v) / _ulp(want_v, prec)
    print(f"{prec} R={R} N={N} rows={len(rs.atoms())}: forces {df.max():.2f} ulp, velocities {dv.max():.2f} ulp, "
          f"|E - model| = {np.abs(e.cpu().numpy() - E).max():.2e}")
    assert df.max() <= 1.0 and dv.max() <= 1.0
    assert np.abs(F[:, touched]).max() > 1.0  # (something was added)
    # rows of atoms in no restraint: never written
    assert torch.equal(_bits(f)[:, ~touched], _bits(_tensor(f_in, prec))[:, ~touched])
    assert torch.equal(_bits(v)[:, ~touched], _bits(_tensor(v_in, prec))[:, ~touched])
    # energies: M terms in another order than the model's
    nterm = rs.npos + rs.ndist
    for r in range(R):
        for c in range(2):
            assert abs(e[r, c].item() - E[r, c]) <= nterm * EPS64 * abs(E[r, c]), (r, c, e[r, c].item(), E[r, c])
    # the impulse writes the velocities only, by the same rule; the evaluation writes no velocity
    fi, vi, _ = once("impulse")
    assert torch.equal(_bits(vi), _bits(v)) and torch.equal(_bits(fi), _bits(_tensor(f_in, prec)))
    fe, ve, ee = once("evaluate")
    assert torch.equal(_bits(fe), _bits(f)) and torch.equal(_bits(ve), _bits(_tensor(v_in, prec))) and torch.equal(ee, e)
    for _ in range(repeats):  # no atomics: the same bits every time
        f2, v2, e2 = once("finish")
        assert torch.equal(_bits(f2), _bits(f)) and torch.equal(_bits(v2), _bits(v)) and torch.equal(e2, e)
    return eng


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_kernel_against_model(prec):
    pos, box, mass, rs = M.kernel_case(R=3, N=200)
    assert rs.npos == 17 and rs.ndist == 23 and rs.dist_k[1, 9] == 0.0 and rs.pos_k[1, 5] == 0.0
    _kernel_against_model(prec, pos, box, mass, rs, repeats=20)


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_kernel_many_blocks(prec):
    pos, box, mass, rs = M.big_case(N=70001, nrestrained=30000)
    _kernel_against_model(prec, pos, box, mass, rs, repeats=1)


def test_kernel_past_a_chunk_of_sixteen_replicas():
    pos, box, mass, rs = M.kernel_case(R=17, N=200, seed=12)
    _kernel_against_model("f32", pos, box, mass, rs, repeats=1)


def test_moving_a_target_replaces_the_tables():
    pos, box, mass, rs = M.kernel_case(R=3, N=200)
    f, eng = _context(mass, rs, "f64", 3)
    p = _tensor(pos, "f64")
    e = torch.zeros(3, 2, dtype=torch.float64, device=_dev())
    _apply(eng, p, box, energies=e)
    e0 = e.cpu().numpy().copy()
    rs.set_distance_targets(rs.dist_r0 + 0.5)
    eng.sync_restraints(rs)
    _apply(eng, p, box, energies=e)
    E = rs.energy_forces(pos, box)[0]
    assert np.allclose(e.cpu().numpy(), E, rtol=1e-13) and np.abs(e.cpu().numpy()[:, 1] - e0[:, 1]).min() > 1.0
    assert np.array_equal(e.cpu().numpy()[:, 0], e0[:, 0])


def test_library_refusals_launch_nothing():
    from torchmd_amd import _lib as L

    pos, box, mass, rs = M.kernel_case(R=3, N=200)
    f, eng = _context(mass, rs, "f64", 3)
    lib = eng.lib
    p = _tensor(pos, "f64")
    frc = _tensor(np.zeros_like(pos), "f64")
    before = _bits(frc).clone()

    def refused(change, expect):
        d, keep = rs.descriptor()
        change(d, keep)
        assert lib.tmdhip_set_restraints(eng.ctx, C.byref(d)) < 0
        assert expect in L.last_error(), (expect, L.last_error())

    def set_(name, value):
        return lambda d, keep: setattr(d, name, value)

    def poke(index, where, value):
        def change(d, keep):
            keep[index].reshape(-1)[where] = value
        return change

    refused(set_("struct_size", 8), "size mismatch")
    refused(set_("nreplicas", 2), "nreplicas")
    refused(set_("npos", -1), "bad size")
    refused(poke(0, 0, 200), "out of range")
    refused(poke(3, 1, -1), "out of range")
    refused(lambda d, keep: keep[3].reshape(-1, 2).__setitem__(2, [5, 5]), "must differ")
    refused(lambda d, keep: keep[0].__setitem__(1, keep[0][0]), "second position entry")
    refused(poke(2, 3, -1.0), "finite k")
    refused(poke(5, 3, np.nan), "finite k")
    refused(poke(4, 3, -0.1), "finite r0")
    refused(poke(1, 3, np.inf), "finite reference")
    # the tables in place are the ones that were accepted: the evaluation is unchanged
    e = torch.zeros(3, 2, dtype=torch.float64, device=_dev())
    _apply(eng, p, box, energies=e)
    assert np.allclose(e.cpu().numpy(), rs.energy_forces(pos, box)[0], rtol=1e-13)
    # velocities without masses, and a restrained atom without mass where masses are first seen
    v = _tensor(np.zeros_like(pos), "f64")
    assert _apply(eng, p, box, vel=v, check=False) < 0 and "masses" in L.last_error()
    m0 = mass.copy()
    m0[7] = 0.0
    assert _apply(eng, p, box, vel=v, mass=_tensor(m0, "f64"), kick=1.0, check=False) < 0 and "no mass" in L.last_error()
    assert torch.equal(_bits(v), torch.zeros_like(_bits(v))) and torch.equal(_bits(frc), before)
    # 1 - gamma dt <= 0 in tmdhip_md_run
    d = L.MdDesc()
    d.struct_size = C.sizeof(L.MdDesc)
    boxes = np.ascontiguousarray(np.tile(box, (3, 1)))
    d.niter, d.pos_dev, d.vel_dev, d.forces_dev = 2, p.data_ptr(), v.data_ptr(), frc.data_ptr()
    mt = _tensor(mass, "f64")
    d.mass_dev, d.vcoeff_dev, d.box_host = mt.data_ptr(), mt.data_ptr(), boxes.ctypes.data_as(C.c_void_p)
    d.dt, d.gamma = 0.5, 2.0
    assert lib.tmdhip_md_run(eng.ctx, C.byref(d), _stream(p.device)) < 0 and "1 - gamma dt" in L.last_error()
    torch.cuda.synchronize()
    assert torch.equal(_bits(p), _bits(_tensor(pos, "f64"))) and torch.equal(_bits(v), torch.zeros_like(_bits(v)))
    # a restrained atom that is a virtual site of the context (atom 7 of the tables, given two unrestrained parents here)
    vd = L.VsiteDesc()
    vd.struct_size = C.sizeof(L.VsiteDesc)
    vd.enable, vd.nsites = 1, 1
    pa = [a for a in range(200) if a not in set(rs.atoms().tolist())][:2]
    site, parent, weight = np.array([7], np.int32), np.array([[pa[0], pa[1], -1]], np.int32), np.array([[0.5, 0.5, 0.0]])
    assert 7 in rs.atoms()
    vd.site_host, vd.parent_host, vd.weight_host = (a.ctypes.data_as(C.c_void_p) for a in (site, parent, weight))
    L.check(lib.tmdhip_set_vsites(eng.ctx, C.byref(vd)), "tmdhip_set_vsites")
    refused(lambda d, keep: None, "virtual site")
    vd.enable = 0
    L.check(lib.tmdhip_set_vsites(eng.ctx, C.byref(vd)), "tmdhip_set_vsites")
    d, keep = rs.descriptor()
    assert lib.tmdhip_set_restraints(eng.ctx, C.byref(d)) == 0  # (the same tables, once the site is gone)
    # a context with passive atoms (what a brick of the domain decomposition is): a context of its own
    f2, eng2 = _context(mass, Restraints(3), "f64", 3)
    types, charges = np.zeros(200, np.int32), np.zeros(200, np.float64)
    L.check(lib.tmdhip_update_atoms(eng2.ctx, 200, types.ctypes.data_as(C.c_void_p), charges.ctypes.data_as(C.c_void_p), 150),
            "tmdhip_update_atoms")
    d, keep = rs.descriptor()
    assert lib.tmdhip_set_restraints(eng2.ctx, C.byref(d)) < 0 and "passive atoms" in L.last_error()
    e2 = torch.full((3, 2), -1.0, dtype=torch.float64, device=_dev())
    _apply(eng2, p, box, forces=frc, energies=e2)  # (no tables in place: nothing added, energies zero)
    assert torch.equal(_bits(frc), before) and (e2 == 0).all()
    # enable = 0 releases everything: nothing is added any more
    off = Restraints(3)
    eng.sync_restraints(off)
    _apply(eng, p, box, forces=frc, energies=e)
    assert torch.equal(_bits(frc), before) and (e == 0).all()


# ----------------------------------------------------------------------------- against the oracle
def _water291_restraints(g, R=1):
    """12 O-O distance restraints on water291, three of them across a face, all within the oracle's bond cutoff."""
    pos = np.asarray(g["pos"], dtype=np.float64).reshape(-1, 3)
    box = np.asarray(g["box"], dtype=np.float64).reshape(-1)[:3]
    ox = np.arange(0, len(pos), 3)
    d = pos[ox][:, None] - pos[ox][None]
    dm = d - box * np.rint(d / box)
    r = np.sqrt((dm * dm).sum(-1))
    crosses = np.abs(d - dm).max(-1) > 0
    ok = (r > 3.0) & (r < 6.5) & np.triu(np.ones_like(r, dtype=bool), 1)
    far, near = np.argwhere(ok & crosses), np.argwhere(ok & ~crosses)
    used, pairs = set(), []
    for cand, want in ((far, 3), (near, 9)):
        got = 0
        for i, j in cand:
            if got == want:
                break
            if i in used or j in used:
                continue
            used.update((i, j))
            pairs.append((ox[i], ox[j]))
            got += 1
        assert got == want
    rng = np.random.default_rng(4)
    rs = Restraints(R)
    rs.add_distance(np.asarray(pairs), rng.uniform(2.5, 5.0, 12), rng.uniform(20.0, 120.0, 12))
    return rs


@pytest.mark.parametrize("prec", ["f64", "f32"])
def test_forces_with_restraints_equal_the_oracle_with_extra_bonds(prec):
    from oracle import torchmd_oracle as orc
    from torchmd_amd.forces import Forces

    g = load("water291")
    dt = PREC[prec]
    par = GoldenParameters(g, dt)
    rs = _water291_restraints(g)
    f = Forces(par, terms=WATER_TERMS, cutoff=7.3, rfa=True, restraints=rs)
    p, b = pos_tensor(g["pos"], 1, dt, _dev()), box_tensor(g["box"], 1, dt, _dev())
    F = torch.full_like(p, 7.0)
    pots = f.compute(p, b, F, returnDetails=True)
    total = f.compute(p, b, torch.zeros_like(p))[0]
    # the oracle: the same system, the restraints appended to its bond list as (k / 2, r0); the pair list of the plain system
    opar = GoldenParameters(g, dt)
    nb = len(opar.bond_params["params"])
    opar.bond_params = {
        "idx": torch.cat([opar.bond_params["idx"], torch.as_tensor(rs.dist_pair, dtype=opar.bond_params["idx"].dtype)]),
        "map": torch.cat([opar.bond_params["map"], torch.stack([torch.arange(12) + len(opar.bond_params["map"]),
                                                                torch.arange(12) + nb], dim=1).to(opar.bond_params["map"].dtype)]),
        "params": torch.cat([opar.bond_params["params"],
                             torch.as_tensor(np.stack([0.5 * rs.dist_k[0], rs.dist_r0[0]], axis=1), dtype=dt)]),
    }
    pairs = orc.all_pairs(par.natoms, orc.exclusion_pairs(par))
    opots, oF, _ = orc.compute(opar, p.cpu(), b.cpu(), WATER_TERMS, pairs=pairs, cutoff=7.3, rfa=True)
    ototal = sum(opots[0][t] for t in WATER_TERMS)
    plain, _, _ = orc.compute(par, p.cpu(), b.cpu(), WATER_TERMS, pairs=pairs, cutoff=7.3, rfa=True)
    err = (F.cpu() - oF).abs().max().item()
    print(f"{prec}: max|dF| = {err:.2e}, E = {total:.6f} (oracle {ototal:.6f}), restraints {pots[0]['restraints']:.6f}")
    assert pots[0]["restraints"] > 1.0 and list(pots[0])[-1] == "restraints"
    assert err <= FTOL[prec]
    assert abs(total - ototal) <= ERTOL[prec] * EFAC * max(1.0, abs(ototal))
    assert abs(pots[0]["restraints"] - (opots[0]["bonds"] - plain[0]["bonds"])) <= ERTOL[prec] * EFAC * max(1.0, abs(opots[0]["bonds"]))
    assert abs(sum(pots[0].values()) - total) <= 1e-9 * abs(total)
    # without the keyword: no entry, and the plain total
    f0 = Forces(par, terms=WATER_TERMS, cutoff=7.3, rfa=True)
    pots0 = f0.compute(p, b, torch.zeros_like(p), returnDetails=True)
    assert "restraints" not in pots0[0]
    with pytest.raises(ValueError, match="vmap"):
        torch.vmap(lambda x: f.compute(x, b, None, toNumpy=False))(p[None])


# ----------------------------------------------------------------------------- trajectories
def _tip3p(prec, R):
    from torchmd_amd.builders import tip3p_box, water_forcefield
    from torchmd_amd.integrator import maxwell_boltzmann
    from torchmd_amd.parameters import Parameters

    mol, pos, box = tip3p_box(12, seed=21)
    par = Parameters(water_forcefield(mol), mol, WATER_TERMS, precision=PREC[prec])
    torch.manual_seed(5)
    vel0 = maxwell_boltzmann(Parameters(water_forcefield(mol), mol, WATER_TERMS, precision=torch.float64).masses, 300, R)
    return mol, np.asarray(pos, dtype=np.float64), np.asarray(box, dtype=np.float64), par, vel0


def _tip3p_restraints(pos, box, R, k=100.0):
    """Two position restraints with references displaced by 1 A, one O-O distance restraint across a face; with R replicas
    every replica has a distance target of its own."""
    p = pos[:, :, 0] if pos.ndim == 3 else pos
    L = np.asarray(box).reshape(-1)[:3]
    ox = np.arange(0, len(p), 3)
    lo = ox[np.argmin(p[ox, 0])]
    hi = ox[np.argmax(p[ox, 0])]
    d = p[lo] - p[hi]
    assert np.any(np.rint(d / L) != 0)  # across a face
    rs = Restraints(R)
    a, c = int(ox[len(ox) // 3]), int(ox[2 * len(ox) // 3])
    rs.add_position([a, c], p[[a, c]] + np.array([[1.0, 0.0, 0.0], [0.0, -0.6, 0.8]]), k)
    r = np.sqrt(np.sum((d - L * np.rint(d / L)) ** 2))
    rs.add_distance([[int(lo), int(hi)]], np.array([[r + 0.4 * (q + 1)] for q in range(R)]), k)
    return rs


def _system(mol, pos, box, vel0, prec, R):
    from torchmd_amd.systems import System

    s = System(mol.numAtoms, R, PREC[prec], _dev())
    s.set_positions(np.repeat(pos[:, :, :1], R, axis=2) if pos.ndim == 3 else np.repeat(pos[:, :, None], R, axis=2))
    s.set_box(box)
    s.set_velocities(vel0.to(PREC[prec]))
    return s


def _by_hand(case, prec, rs_model, cuts, langevin, **fkw):
    """The truth: tmdhip_first_vv, a Forces WITHOUT restraints, forces += the numpy model, tmdhip_(langevin_)second_vv."""
    from torchmd_amd import _lib as L
    from torchmd_amd.forces import Forces
    from torchmd_amd.integrator import Integrator

    mol, pos, box, par, vel0, R, terms, kw = case
    s = _system(mol, pos, box, vel0, prec, R)
    f = Forces(par, terms=terms, **kw, **fkw)
    torch.manual_seed(77)
    integ = Integrator(s, f, 1.0, _dev(), **(dict(gamma=50.0, T=300.0) if langevin else {}))
    integ._check_layout()
    lib, code, N = L.load(), L.dtype_code(s.pos.dtype), s.pos.shape[1]
    hbox = np.diagonal(s.box.cpu().double().numpy(), axis1=1, axis2=2)

    def add_restraints():
        Fr = rs_model.energy_forces(s.pos.cpu().double().numpy(), hbox)[1]
        s.forces += torch.as_tensor(Fr).to(s.forces.dtype).to(s.forces.device)

    f._compute_async(s.pos, s.box, s.forces, want_energy=False)
    add_restraints()
    st = _stream(_dev())
    for step in range(sum(cuts)):
        L.check(lib.tmdhip_first_vv(code, R, N, s.pos.data_ptr(), s.vel.data_ptr(), s.forces.data_ptr(), integ.masses.data_ptr(), integ.dt, st))
        f._compute_async(s.pos, s.box, s.forces, want_energy=False)
        add_restraints()
        if langevin:
            L.check(lib.tmdhip_langevin_second_vv(code, R, N, s.vel.data_ptr(), s.forces.data_ptr(), integ.masses.data_ptr(),
                                                  integ.vcoeff.data_ptr(), integ.dt, float(integ.gamma), integ._seed, step, st))
        else:
            L.check(lib.tmdhip_second_vv(code, R, N, s.vel.data_ptr(), s.forces.data_ptr(), integ.masses.data_ptr(), integ.dt, st))
    return s.pos.cpu().double().numpy(), s.vel.cpu().double().numpy()


def _under_test(case, prec, rs, cuts, langevin, replay=False, **fkw):
    """`Integrator.step` of a Forces WITH restraints, cut as `cuts`.  Returns positions, velocities, forces, the last
    call's result, the Forces, the System and the Integrator."""
    from torchmd_amd.forces import Forces
    from torchmd_amd.integrator import Integrator

    mol, pos, box, par, vel0, R, terms, kw = case
    s = _system(mol, pos, box, vel0, prec, R)
    f = Forces(par, terms=terms, restraints=rs, **kw, **fkw)
    f.compute(s.pos, s.box, s.forces)
    torch.manual_seed(77)
    integ = Integrator(s, f, 1.0, _dev(), **(dict(gamma=50.0, T=300.0) if langevin else {}))
    out = None
    for n in cuts:
        out = integ.step(n)
    return s.pos.cpu().double().numpy(), s.vel.cpu().double().numpy(), s.forces.cpu().double().numpy(), out, f, s, integ


def _check_return(prec, out, f, s, rs, forces, integ):
    """The potential energy the call returns is compute()'s total at the final positions, and the forces it leaves include F_r."""
    # ... and the kinetic energy it returns is that of the velocities it leaves: the finishing kick comes after the last
    # launch's own sum, which is therefore summed again (64 eps64 for the order of summation, eps32 for the cast in fp32: the
    # bound of tests/test_gpu_thermostat.py; the finishing kick changes K by far more, checked on the way)
    from torchmd_amd import _lib as L

    K = torch.zeros(s.vel.shape[0], dtype=torch.float64, device=s.vel.device)
    L.check(L.load().tmdhip_kinetic_energy(L.dtype_code(s.vel.dtype), s.vel.shape[0], s.vel.shape[1], s.vel.data_ptr(),
                                           integ.masses.data_ptr(), K.data_ptr(), _stream(s.vel.device)), "tmdhip_kinetic_energy")
    K = K.cpu().numpy()
    bound = K * (64 * EPS64 + (np.finfo(np.float32).eps if prec == "f32" else 0.0))
    assert (np.abs(np.asarray(out[0], dtype=np.float64) - K) <= bound).all(), (out[0], K)
    hbox0 = np.diagonal(s.box.cpu().double().numpy(), axis1=1, axis2=2)
    Fr0 = rs.energy_forces(s.pos.cpu().double().numpy(), hbox0)[1]
    m = integ.masses.cpu().double().numpy().reshape(1, -1, 1)
    v1 = s.vel.cpu().double().numpy()
    v0 = v1 - 0.5 * integ.dt * Fr0 / m  # the velocities before the finishing kick
    stale = np.abs(0.5 * (m * (v1 * v1 - v0 * v0)).sum(axis=(1, 2)))
    assert (stale > 10 * bound).all(), (stale, bound)  # (a sum taken before the kick would miss the bound)
    F2 = torch.zeros_like(s.pos)
    tot = f.compute(s.pos, s.box, F2)
    for r in range(s.pos.shape[0]):
        assert abs(out[1][r] - tot[r]) <= ERTOL[prec] * EFAC * max(1.0, abs(tot[r])), (r, out[1][r], tot[r])
    assert np.abs(forces - F2.cpu().double().numpy()).max() <= FTOL[prec] * 10
    hbox = np.diagonal(s.box.cpu().double().numpy(), axis1=1, axis2=2)
    Er, Fr = rs.energy_forces(s.pos.cpu().double().numpy(), hbox)
    assert np.abs(Fr).max() > 10.0 and np.allclose(f._restraint_energy, Er, rtol=1e-5)
    plain = forces - Fr  # what is left without F_r is far from the total on the restrained atoms
    assert np.abs(plain - F2.cpu().double().numpy()).max() > 10.0


CUTS = (1, 2, 7)


@pytest.mark.parametrize("langevin", [False, True], ids=["nve", "langevin"])
def test_trajectory_fp64_list_path(langevin, monkeypatch):
    monkeypatch.setenv("TMDHIP_VSKIN", "0")
    mol, pos, box, par, vel0 = _tip3p("f64", 1)
    rs = _tip3p_restraints(pos, box, 1)
    case = (mol, pos, box, par, vel0, 1, WATER_TERMS, dict(cutoff=9.0, rfa=True))
    tp, tv = _by_hand(case, "f64", rs, CUTS, langevin)
    p, v, frc, out, f, s, integ = _under_test(case, "f64", rs, CUTS, langevin)
    bar_p, bar_v = 64 * EPS64 * 10 * np.abs(tp).max(), 64 * EPS64 * 10 * np.abs(tv).max()
    print(f"fp64 list path, {'Langevin' if langevin else 'NVE'}: |dpos| = {np.abs(p - tp).max():.2e} (bar {bar_p:.2e}), "
          f"|dvel| = {np.abs(v - tv).max():.2e} (bar {bar_v:.2e})")
    assert f.stats(s.pos)["algorithm"] == "celllist" and f.stats(s.pos)["steps_in_pair_launch"] == 0
    assert np.abs(p - tp).max() <= bar_p and np.abs(v - tv).max() <= bar_v
    _check_return("f64", out, f, s, rs, frc, integ)


@pytest.mark.parametrize("langevin", [False, True], ids=["nve", "langevin"])
@pytest.mark.parametrize("R", [1, 3], ids=["lone", "batched"])
def test_trajectory_fp32_fused(R, langevin, monkeypatch):
    monkeypatch.setenv("TMDHIP_VSKIN", "0")
    mol, pos, box, par32, vel0 = _tip3p("f32", R)
    _, _, _, par64, _ = _tip3p("f64", R)
    rs = _tip3p_restraints(pos, box, R)
    if R == 3:
        assert len(set(rs.dist_r0[:, 0])) == 3
    kw = dict(cutoff=9.0, rfa=True)
    case64 = (mol, pos, box, par64, vel0, R, WATER_TERMS, kw)
    case32 = (mol, pos, box, par32, vel0, R, WATER_TERMS, kw)
    tp, tv = _by_hand(case64, "f64", rs, CUTS, langevin)
    hp, hv = _by_hand(case32, "f32", rs, CUTS, langevin)
    p, v, frc, out, f, s, integ = _under_test(case32, "f32", rs, CUTS, langevin)
    noise_p, noise_v = np.abs(hp - tp).max(), np.abs(hv - tv).max()
    dp, dv = np.abs(p - tp).max(), np.abs(v - tv).max()
    print(f"fp32 fused R={R}, {'Langevin' if langevin else 'NVE'}: |dpos| = {dp:.2e} (by hand {noise_p:.2e}), "
          f"|dvel| = {dv:.2e} (by hand {noise_v:.2e})")
    st = [f.stats(s.pos, r) for r in range(R)]
    assert all(x["steps_in_pair_launch"] >= 5 for x in st), st  # the interior steps of 2 + 7 were made by pair launches
    if R == 3:
        assert st[0]["batched_launches"] >= 5
    assert dp <= 2 * noise_p and dv <= 2 * noise_v
    # the control: the same by-hand loop with the model's k halved misses that bar by more than 10x
    half = _tip3p_restraints(pos, box, R, k=50.0)
    cp, cv = _by_hand(case32, "f32", half, CUTS, langevin)
    assert np.abs(cp - tp).max() > 10 * 2 * noise_p and np.abs(cv - tv).max() > 10 * 2 * noise_v
    _check_return("f32", out, f, s, rs, frc, integ)


def _water291_case(prec, R, **kw):
    g = load("water291")
    par = GoldenParameters(g, PREC[prec])
    pos = np.asarray(g["pos"], dtype=np.float64).reshape(-1, 3)
    box = np.asarray(g["box"], dtype=np.float64).reshape(-1)[:3]
    rng = np.random.default_rng(8)
    vel0 = torch.as_tensor(0.01 * rng.standard_normal((R, len(pos), 3)))

    class Mol:
        numAtoms = len(pos)

    return (Mol, pos, box, par, vel0, R, ["bonds", "angles", "electrostatics", "lj"], kw)


def _water291_mixed(case, R):
    pos, box = case[1], case[2]
    rs = _water291_restraints(load("water291"), R)
    rs.set_strengths(distance_k=100.0)
    rs.set_distance_targets(np.array([rs.dist_r0[0] + 0.3 * q for q in range(R)]))
    rs.add_position([0, 150], pos[[0, 150]] + np.array([[1.0, 0.0, 0.0], [0.0, 0.0, -1.0]]), 100.0)
    return rs


@pytest.mark.parametrize("langevin", [False, True], ids=["nve", "langevin"])
def test_trajectory_fp64_all_pairs_replicas_together(langevin):
    case = _water291_case("f64", 2, cutoff=7.3, rfa=True)
    rs = _water291_mixed(case, 2)
    tp, tv = _by_hand(case, "f64", rs, CUTS, langevin)
    p, v, frc, out, f, s, integ = _under_test(case, "f64", rs, CUTS, langevin)
    bar_p, bar_v = 64 * EPS64 * 10 * np.abs(tp).max(), 64 * EPS64 * 10 * np.abs(tv).max()
    print(f"fp64 all pairs x 2: |dpos| = {np.abs(p - tp).max():.2e} (bar {bar_p:.2e}), |dvel| = {np.abs(v - tv).max():.2e} (bar {bar_v:.2e})")
    assert f.stats(s.pos)["algorithm"] == "allpairs"
    assert np.abs(p - tp).max() <= bar_p and np.abs(v - tv).max() <= bar_v
    _check_return("f64", out, f, s, rs, frc, integ)


def test_trajectory_fp64_pme():
    case = _water291_case("f64", 1, cutoff=7.0, pme=True)
    case = case[:6] + (["bonds", "angles", "electrostatics", "lj"], dict(cutoff=7.0, pme=True))
    rs = _water291_mixed(case, 1)
    tp, tv = _by_hand(case, "f64", rs, CUTS, True)
    p, v, frc, out, f, s, integ = _under_test(case, "f64", rs, CUTS, True)
    bar_p, bar_v = 64 * EPS64 * 10 * np.abs(tp).max(), 64 * EPS64 * 10 * np.abs(tv).max()
    print(f"fp64 PME: |dpos| = {np.abs(p - tp).max():.2e} (bar {bar_p:.2e}), |dvel| = {np.abs(v - tv).max():.2e} (bar {bar_v:.2e})")
    assert f.stats(s.pos)["pme_evaluations"] > 0
    assert np.abs(p - tp).max() <= bar_p and np.abs(v - tv).max() <= bar_v


def test_forced_replay_repeats_the_batch(monkeypatch):
    """Rewind and replay need nothing of their own: everything is enqueued again from the snapshot."""
    monkeypatch.setenv("TMDHIP_VSKIN", "0")
    mol, pos, box, par, vel0 = _tip3p("f64", 1)
    rs = _tip3p_restraints(pos, box, 1)
    case = (mol, pos, box, par, vel0, 1, WATER_TERMS, dict(cutoff=9.0, rfa=True))
    tp, tv = _by_hand(case, "f64", rs, CUTS, True)
    p, v, frc, out, f, s, integ = _under_test(case, "f64", rs, CUTS, True)
    again = integ._step_body(CUTS[-1], replay=True)
    p2, v2 = s.pos.cpu().double().numpy(), s.vel.cpu().double().numpy()
    bar_p, bar_v = 64 * EPS64 * 10 * np.abs(tp).max(), 64 * EPS64 * 10 * np.abs(tv).max()
    assert np.abs(p2 - tp).max() <= bar_p and np.abs(v2 - tv).max() <= bar_v
    assert abs(again[1][0] - out[1][0]) <= 1e-9 * abs(out[1][0]) and abs(again[0][0] - out[0][0]) <= 1e-9 * abs(out[0][0])
    _check_return("f64", again, f, s, rs, s.forces.cpu().double().numpy(), integ)


# ----------------------------------------------------------------------------- invariants
def _water291_run(rs, R=1, prec="f64", vel_scale=0.01, **integ_kw):
    from torchmd_amd.forces import Forces
    from torchmd_amd.integrator import Integrator

    case = _water291_case(prec, R, cutoff=7.3, rfa=True)
    mol, pos, box, par, vel0, _, terms, kw = case
    s = _system(mol, pos, box, vel0 * (vel_scale / 0.01), prec, R)
    f = Forces(par, terms=terms, **kw, **({} if rs is None else {"restraints": rs}))
    f.compute(s.pos, s.box, s.forces)
    torch.manual_seed(3)
    return s, f, Integrator(s, f, 1.0, _dev(), **integ_kw)


def test_nve_energy_drift_is_that_of_the_plain_run():
    """NVE, fp64, 200 steps: the drift of E_kin + E_pot (restraints included) is at most twice that of the same run without
    restraints, measured here on the same start."""
    drift = {}
    for name in ("plain", "restrained"):
        rs = _water291_mixed(_water291_case("f64", 1), 1) if name == "restrained" else None
        s, f, integ = _water291_run(rs)
        e = []
        for _ in range(10):
            ek, ep, _ = integ.step(20)
            e.append(float(ek[0]) + ep[0])
        drift[name] = np.abs(np.asarray(e) - e[0]).max()
        if rs is not None:
            assert f._restraint_energy.sum() > 1.0
    print(f"NVE drift over 200 steps: plain {drift['plain']:.3e}, restrained {drift['restrained']:.3e} kcal/mol")
    assert drift["restrained"] <= 2 * drift["plain"]


def test_constrained_water_with_a_restrained_oxygen():
    """constraints="water" at 2 fs: the bond lengths are kept as well as without restraints (the constraint solver's own
    tolerance, tests/test_gpu_constraints.py: 1e-10 relative in fp64), and the restrained oxygen stays within
    sqrt(2 x 10 k_B T / k) of its reference.  "As well": SETTLE is analytic, so in fp64 either run's worst bond error is a few
    roundings of the positions (measured 2.9e-15 plain, 3.6e-15 restrained) and which of the two is larger is chance; the bar is
    four times the plain run's figure plus 8 eps64, which a real degradation (a kick that is not projected shows at 1e-6 and
    more) misses by orders of magnitude."""
    from torchmd_amd.builders import tip3p_box, water_forcefield
    from torchmd_amd.forces import Forces
    from torchmd_amd.integrator import BOLTZMAN, Integrator, maxwell_boltzmann
    from torchmd_amd.parameters import Parameters

    mol, pos, box = tip3p_box(6, seed=3)
    par = Parameters(water_forcefield(mol), mol, WATER_TERMS, precision=torch.float64)
    k, T = 100.0, 300.0
    atom = 3 * 40
    dev_bond = {}
    for name in ("plain", "restrained"):
        rs = None
        if name == "restrained":
            rs = Restraints(1)
            rs.add_position([atom], pos[[atom]], k)
        torch.manual_seed(9)
        vel0 = maxwell_boltzmann(par.masses, T, 1)
        s = _system(mol, np.asarray(pos, dtype=np.float64), box, vel0, "f64", 1)
        f = Forces(par, terms=WATER_TERMS, cutoff=7.0, rfa=True, **({} if rs is None else {"restraints": rs}))
        f.compute(s.pos, s.box, s.forces)
        integ = Integrator(s, f, 2.0, _dev(), gamma=1.0, T=T, constraints="water")
        far = 0.0
        for _ in range(10):
            integ.step(20)
            p = s.pos[0].cpu().double().numpy()
            if rs is not None:
                far = max(far, np.sqrt((rs.energy_forces(p[None], box)[0][0, 0]) * 2.0 / k))
        cs = integ.constraints
        w = np.asarray(cs.waters)
        d = np.stack([np.linalg.norm(p[w[:, 0]] - p[w[:, 1]], axis=1), np.linalg.norm(p[w[:, 0]] - p[w[:, 2]], axis=1),
                      np.linalg.norm(p[w[:, 1]] - p[w[:, 2]], axis=1)], axis=1)
        d0 = np.asarray(cs.water_dist)
        want = np.stack([d0[:, 0], d0[:, 0], d0[:, 1]], axis=1)
        dev_bond[name] = np.abs(d / want - 1.0).max()
    bound = np.sqrt(2 * 10 * BOLTZMAN * T / k)
    print(f"bond lengths: plain {dev_bond['plain']:.2e}, restrained {dev_bond['restrained']:.2e}; oxygen at most {far:.3f} A "
          f"from its reference (bound {bound:.3f})")
    assert dev_bond["restrained"] <= 4 * dev_bond["plain"] + 8 * EPS64
    assert 0.0 < far <= bound


def test_minimize_fire_converges_on_the_total_force():
    from torchmd_amd.minimizers import minimize_fire

    case = _water291_case("f64", 1)
    pos = case[1]
    rs = Restraints(1)
    rs.add_position([0, 150], pos[[0, 150]] + np.array([[1.0, 0.0, 0.0], [0.0, 0.0, -1.0]]), 100.0)
    s, f, _ = _water291_run(rs)
    minimize_fire(s, f, fmax=0.5, steps=5000)
    F = torch.zeros_like(s.pos)
    pots = f.compute(s.pos, s.box, F, returnDetails=True)
    fmax = F.norm(dim=2).max().item()
    moved = np.linalg.norm(s.pos[0, [0, 150]].cpu().numpy() - pos[[0, 150]], axis=1)
    print(f"FIRE: max|F_total| = {fmax:.3f}, restraint energy {pots[0]['restraints']:.3f}, restrained atoms moved {moved}")
    assert fmax <= 0.5
    assert moved.min() > 0.3  # the restraints pulled: a minimiser blind to F_r would have left the atoms in their wells


LADDER = (300.0, 302.0, 304.0, 306.0)


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_ladder_under_restraints_walks_with_every_pair_accepted(prec, monkeypatch):
    """§16's forced walk (tests/test_gpu_exchange.py::test_every_pair_accepted_walks_the_ladder) with restraints in place, every
    replica with a distance target of its own: with u = 0 the odd-even transposition reverses the four rungs in four attempts,
    the thermostat's temperatures follow, and the energies every attempt decides on are compute()'s totals at the positions
    of that moment, restraint energy included."""
    import _exchange as X
    from torchmd_amd.exchange import ReplicaExchange
    from torchmd_amd.forces import Forces
    from torchmd_amd.integrator import Integrator
    from torchmd_amd.thermostat import VelocityRescale

    monkeypatch.setenv("TMDHIP_LPA", "16")  # (as §16's test: a context picks its lanes per atom from the atoms that share a launch)
    mol, pos, box, par, _ = _tip3p(prec, 4)
    rs = _tip3p_restraints(pos, box, 4)
    from torchmd_amd.integrator import maxwell_boltzmann

    torch.manual_seed(0)
    v = torch.cat([maxwell_boltzmann(par.masses, T, 1) for T in LADDER]).double()
    m = par.masses.double().reshape(1, -1, 1)
    v = v - (m * v).sum(dim=1, keepdim=True) / m.sum()
    s = _system(mol, pos, box, v, prec, 4)
    f = Forces(par, terms=WATER_TERMS, cutoff=9.0, rfa=True, restraints=rs)
    f.compute(s.pos, s.box, s.forces)
    th, ex = VelocityRescale(list(LADDER), tau=0.1, frequency=10, seed=31), ReplicaExchange(frequency=20, seed=31)
    ex.rng = X.Counting(0.0)  # u = 0 < exp(Delta): every tried pair is accepted
    seen, inner = [], ex.attempt

    def attempt(system, masses, thermostat, epot):
        seen.append((np.asarray(epot, dtype=np.float64).copy(), system.pos.detach().clone()))
        return inner(system, masses, thermostat, epot)

    ex.attempt = attempt
    integ = Integrator(s, f, 1.0, _dev(), thermostat=th, exchange=ex)
    ek, pot, T = integ.step(80)
    assert f.stats(s.pos)["algorithm"] == "celllist" and th.applications == 8 and ex.nattempts == 4 and len(seen) == 4
    assert [h.tolist() for h in ex.history] == [[1, 0, 3, 2], [2, 0, 3, 1], [3, 1, 2, 0], [3, 2, 1, 0]]
    assert ex.rungs.tolist() == [3, 2, 1, 0] and ex.rng.count == 6
    assert ex.attempts.tolist() == [2, 2, 2] and np.array_equal(ex.accepted, ex.attempts)
    assert th.temperatures.tolist() == [306.0, 304.0, 302.0, 300.0] and ex.ladder.tolist() == list(LADDER)
    assert np.isfinite(ex.record["delta"]).all() and ex.record["accepted"].all() and ex.record["pairs"].tolist() == [[1, 2]]
    assert np.array_equal(T, integ._temperature(ek)) and np.isfinite(pot).all()
    # the energy of every attempt: a second Forces (its own context) evaluates the positions the attempt saw
    g = Forces(par, terms=WATER_TERMS, cutoff=9.0, rfa=True, restraints=rs)
    hbox = np.tile(np.asarray(box, dtype=np.float64).reshape(-1)[:3], (4, 1))
    for k, (epot, p) in enumerate(seen):
        tot = np.asarray(g.compute(p, s.box, torch.zeros_like(p)))
        er = rs.energy_forces(p.cpu().double().numpy(), hbox)[0].sum(axis=1)
        print(f"{prec} attempt {k}: U = {epot}, restraint energy {er}")
        assert (er > 1.0).all()
        assert (np.abs(epot - tot) <= ERTOL[prec] * EFAC * np.maximum(1.0, np.abs(tot))).all(), (k, epot, tot)
        assert (np.abs(epot - (tot - er)) > 2 * ERTOL[prec] * EFAC * np.abs(tot)).all()  # (without it they would miss the bar)
    assert np.array_equal(ex.record["U"], seen[-1][0])



def test_exchange_and_barostat_see_the_restraint_energy():
    from torchmd_amd.barostat import MonteCarloBarostat
    from torchmd_amd.exchange import ReplicaExchange
    from torchmd_amd.forces import Forces
    from torchmd_amd.integrator import Integrator
    from torchmd_amd.thermostat import VelocityRescale

    # a two-rung ladder: the energies the exchange decides on are compute()'s totals, restraints included
    rs = _water291_mixed(_water291_case("f64", 2), 2)
    th, ex = VelocityRescale([300.0, 310.0], tau=0.1, frequency=10, seed=2), ReplicaExchange(frequency=10, seed=2)
    s, f, integ = _water291_run(rs, R=2, thermostat=th, exchange=ex)
    integ.step(10)
    tot = f.compute(s.pos, s.box, torch.zeros_like(s.pos))
    er = f._restraint_energy.sum(axis=1)
    assert ex.record is not None and er.min() > 1.0
    assert np.allclose(ex.record["U"], tot, rtol=1e-9) and not np.allclose(ex.record["U"], np.asarray(tot) - er, rtol=1e-6)
    # the barostat under distance restraints: its U is the total; position restraints are refused
    rd = _water291_restraints(load("water291"), 1)
    bar = MonteCarloBarostat(1.0, 300.0, frequency=5, seed=1)
    s, f, integ = _water291_run(rd, gamma=1.0, T=300.0, barostat=bar)
    out = integ.step(5)
    tot = f.compute(s.pos, s.box, torch.zeros_like(s.pos))[0]
    er = float(f._restraint_energy.sum())
    seen = bar.last["U_new"][0] if bar.last["accepted"][0] else bar.last["U"][0]
    print(f"barostat: U = {seen:.6f}, compute = {tot:.6f}, restraints {er:.6f}")
    assert er > 1.0 and abs(seen - tot) <= 1e-8 * abs(tot) and abs(out[1][0] - tot) <= 1e-8 * abs(tot)
    # ... also when the position entry is added after the integrator was made: looked at again at every step
    pos0 = _water291_case("f64", 1)[1]
    rd.add_position([0], pos0[[0]], 10.0)
    before = s.pos.clone()
    with pytest.raises(ValueError, match="position restraints"):
        integ.step(5)
    assert torch.equal(s.pos, before)
    rd = _water291_restraints(load("water291"), 1)
    rp = _water291_mixed(_water291_case("f64", 1), 1)
    with pytest.raises(ValueError, match="position restraints"):
        _water291_run(rp, gamma=1.0, T=300.0, barostat=MonteCarloBarostat(1.0, 300.0, frequency=5, seed=1))
    with pytest.raises(ValueError, match="batch"):
        _water291_run(rd, batch=torch.zeros(291, dtype=torch.long))


_CHILD = r"""
import json, os, sys
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
import numpy as np, torch, yaml
import test_gpu_driver as D
from _golden import load
from torchmd_amd import run as driver
from torchmd_amd.builders import TIP3P_FF
g = load("water291")
psf, pdb, ff = (os.path.join(TMP, n) for n in ("structure.psf", "structure.pdb", "water_forcefield.yaml"))
D._write_psf(psf, g); D._write_pdb(pdb, g)
open(ff, "w").write(yaml.safe_dump(TIP3P_FF))
pos = np.asarray(g["pos"], dtype=np.float64).reshape(-1, 3)
np.savez(os.path.join(TMP, "restraints.npz"), pos_atom=np.array([0, 150]), pos_ref=pos[[0, 150]] + 1.0, pos_k=np.array([50.0, 80.0]),
         dist_pair=np.array([[3, 12]]), dist_r0=np.array([[4.0], [4.5]]), dist_k=np.array([100.0]))
conf = {"structure": [psf, pdb], "forcefield": ff, "forceterms": ["LJ", "Bonds", "Angles", "Electrostatics"], "cutoff": 7.3, "rfa": True,
        "replicas": 2, "precision": "single", "device": "cuda", "timestep": 1, "temperature": 300, "langevin_temperature": 300,
        "langevin_gamma": 1.0, "seed": 1, "steps": 40, "output_period": 20, "save_period": 0, "output": "output"}
out = {}
def go(name, **kw):
    c = dict(conf, log_dir=os.path.join(TMP, name), **kw)
    open(os.path.join(TMP, name + ".yaml"), "w").write(yaml.safe_dump(c))
    driver.main(["--conf", os.path.join(TMP, name + ".yaml")])
    log = os.path.join(TMP, name)
    out[name] = {"files": sorted(os.listdir(log)), "rows": [open(os.path.join(log, f"monitor_{k}.csv")).read().splitlines() for k in range(2)]}
go("log")
out["module_after_off"] = "torchmd_amd.restraints" in sys.modules
go("log_rs", restraints=os.path.join(TMP, "restraints.npz"))
print("RESULT " + json.dumps(out))
"""


def test_run_py_with_and_without_the_key(tmp_path):
    import json
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = f"ROOT = {root!r}\nTMP = {str(tmp_path)!r}\n" + _CHILD
    res = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, cwd=root)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-4000:]
    out = json.loads(next(ln for ln in res.stdout.splitlines() if ln.startswith("RESULT "))[7:])
    files = ["input.yaml"] + [f"monitor_{k}.csv" for k in range(2)] + [f"output_{k}.npy" for k in range(2)]
    assert out["module_after_off"] is False  # without the key the module is never imported
    assert out["log"]["files"] == files and out["log_rs"]["files"] == files
    assert all(rows[0] == "iter,ns,epot,ekin,etot,T,t" and len(rows) == 3 for rows in out["log"]["rows"])
    energies = []
    for rows in out["log_rs"]["rows"]:
        assert rows[0] == "iter,ns,epot,ekin,etot,T,restraints,t" and len(rows) == 3
        vals = np.array([[float(x) for x in r.split(",")] for r in rows[1:]])
        assert np.isfinite(vals).all() and (vals[:, 6] > 1.0).all()
        energies.append(vals[-1, 6])
    assert energies[0] != energies[1]  # a distance target of its own per replica
