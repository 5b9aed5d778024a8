"""Group restraints on the device: the kernels of group_restraint.hip against the numpy model
(`GroupRestraints.energy_forces`), `Forces(group_restraints=)` against the oracle with single-atom groups appended to its bond and
angle lists, `Integrator.step` under the term against a loop made by hand of parts that know nothing of it, the exchange of
windows, and the combinations the term allows.

Bars.  Kernel against model: one ulp of the dtype on `dtype(float64(in) + model)` plus 64 n_max eps64 max|F_model| for the centre
sums (a sum in another order is off by at most n eps64 x 8 A per centre, amplified by at most 8 / 2 through an angle's arm; in
fp32 it vanishes under the ulp; the model takes the kernel's order, `fixed_order_sum`, so the room is not needed); energies
M eps64 sum|E|.  Single-atom groups against restraint_kernel: one ulp of the dtype.
Oracle: tests/test_gpu_parity.py's bars.  Trajectories: §17's method and bars (tests/test_gpu_restraints.py): fp64 within
64 eps64 x 10 x max|pos| (max|vel|) of the by-hand loop; fp32 within twice the by-hand fp32 loop's own deviation from the fp64
truth, with a control (the model's k halved) that must miss that bar by more than 10x."""

import ctypes as C
import os

import numpy as np
import pytest
import torch

import _group_restraints as M
import test_gpu_restraints as TR
from _golden import PREC, GoldenParameters, box_tensor, load, pos_tensor
from torchmd_amd.group_restraints import GroupRestraints
from torchmd_amd.restraints import Restraints, min_image

pytestmark = pytest.mark.gpu

NP = TR.NP
EPS64 = TR.EPS64
WATER_TERMS = TR.WATER_TERMS
FTOL, ERTOL, EFAC = TR.FTOL, TR.ERTOL, TR.EFAC
_dev, _bits, _tensor, _stream, _ulp = TR._dev, TR._bits, TR._tensor, TR._stream, TR._ulp


def _context(mass, gr, prec, R, **kw):
    """(Forces, engine) of a context that holds nothing but the group restraints (and what `kw` adds)."""
    from torchmd_amd.forces import Forces

    f = Forces(TR._BarePar(mass, PREC[prec]), terms=[], group_restraints=gr, **kw)
    eng = f._engine(torch.zeros(R, len(mass), 3, dtype=PREC[prec], device=_dev()))
    gr.sync(eng, f)
    return f, eng


def _apply(eng, pos, box, forces=None, vel=None, mass=None, kick=0.0, energies=None, check=True, fn="tmdhip_group_restraint_apply"):
    from torchmd_amd import _lib as L

    boxes = np.ascontiguousarray(np.broadcast_to(np.asarray(box, dtype=np.float64).reshape(-1, 3), (pos.shape[0], 3)))
    ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p()  # noqa: E731
    rc = getattr(eng.lib, fn)(eng.ctx, ptr(pos), boxes.ctypes.data_as(C.POINTER(C.c_double)), ptr(forces), ptr(vel), ptr(mass),
                              float(kick), ptr(energies), _stream(pos.device))
    return L.check(rc, fn) if check else rc


def _kernel_against_model(prec, pos, box, mass, gr, repeats):
    R, N = pos.shape[:2]
    rng = np.random.default_rng(99)
    pos = pos.astype(NP[prec]).astype(np.float64)  # the model sees the positions the device holds
    mass = mass.astype(NP[prec]).astype(np.float64)
    f_in = rng.normal(0.0, 20.0, (R, N, 3)).astype(NP[prec]).astype(np.float64)
    v_in = rng.normal(0.0, 0.05, (R, N, 3)).astype(NP[prec]).astype(np.float64)
    kick = 0.0123
    _, eng = _context(mass, gr, prec, R)  # (hands over the masses the device holds: the default weights)
    assert np.array_equal(gr.masses, mass)
    E, F = gr.energy_forces(pos, box)
    touched = np.zeros(N, dtype=bool)
    touched[gr.atoms()] = True
    p, m = _tensor(pos, prec), _tensor(mass, prec)

    def once(mode):
        f, v = _tensor(f_in, prec), _tensor(v_in, prec)
        e = torch.full((R, 3), -1.0, dtype=torch.float64, device=_dev())
        if mode == "finish":
            _apply(eng, p, box, forces=f, vel=v, mass=m, kick=kick, energies=e)
        elif mode == "impulse":
            _apply(eng, p, box, vel=v, mass=m, kick=kick)
        else:
            _apply(eng, p, box, forces=f, energies=e)
        return f, v, e

    f, v, e = once("finish")
    nmax = max(len(a) for a in gr.group_atoms)
    slack = 64 * nmax * EPS64 * np.abs(F).max()
    want_f = (f_in + F).astype(NP[prec]).astype(np.float64)
    dV = kick * F / mass[None, :, None]
    want_v = (v_in + dV).astype(NP[prec]).astype(np.float64)
    got_f, got_v = f.cpu().double().numpy(), v.cpu().double().numpy()
    df, dv = np.abs(got_f - want_f), np.abs(got_v - want_v)
    slack_v = 64 * nmax * EPS64 * np.abs(dV).max()
    print(f"{prec} R={R} N={N} rows={len(gr.atoms())}: forces {(df / _ulp(want_f, prec)).max():.2f} ulp = {df.max():.2e} "
          f"(centre slack {slack:.2e}), velocities {(dv / _ulp(want_v, prec)).max():.2f} ulp, "
          f"|E - model| = {np.abs(e.cpu().numpy() - E).max():.2e}")
    assert (df <= _ulp(want_f, prec) + slack).all() and (dv <= _ulp(want_v, prec) + slack_v).all()
    assert np.abs(F[:, touched]).max() > 1.0  # (something was added)
    # rows of atoms in no group: never written
    assert (~touched).any()
    assert torch.equal(_bits(f)[:, ~touched], _bits(_tensor(f_in, prec))[:, ~touched])
    assert torch.equal(_bits(v)[:, ~touched], _bits(_tensor(v_in, prec))[:, ~touched])
    got_e = e.cpu().numpy()
    for r in range(R):
        assert np.abs(got_e[r] - E[r]).max() <= gr.nrestraints * EPS64 * np.abs(E[r]).sum(), (r, got_e[r], E[r])
    # the impulse writes the velocities only, by the same rule; the evaluation writes no velocity
    fi, vi, _ = once("impulse")
    assert torch.equal(_bits(vi), _bits(v)) and torch.equal(_bits(fi), _bits(_tensor(f_in, prec)))
    fe, ve, ee = once("evaluate")
    assert torch.equal(_bits(fe), _bits(f)) and torch.equal(_bits(ve), _bits(_tensor(v_in, prec))) and torch.equal(ee, e)
    for _ in range(repeats):  # no atomics: the same bits every time
        f2, v2, e2 = once("finish")
        assert torch.equal(_bits(f2), _bits(f)) and torch.equal(_bits(v2), _bits(v)) and torch.equal(e2, e)
    return eng, p, got_e


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_kernel_against_model(prec):
    pos, box, mass, gr = M.kernel_case(R=3, N=600)
    assert tuple(len(a) for a in gr.group_atoms) == M.SIZES and gr.kind.tolist() == [0] * 5 + [1] * 4 + [2] * 4
    assert (gr.k == 0).sum() == 3 and len(np.unique(gr.target[:, 0])) == 3 and (gr.flat > 0).any() and (gr.flat == 0).any()
    rows = gr.build_rows()
    assert np.diff(rows[3]).max() == 3  # one atom in three groups
    _kernel_against_model(prec, pos, box, mass, gr, repeats=20)


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_kernel_more_restraints_than_a_block_holds(prec):
    """Up to 256 restraints a block of the force kernel evaluates them once into LDS; beyond that every thread recomputes its
    own, and the energy kernel has a second block: 13 + 300 restraints."""
    pos, box, mass, gr = M.kernel_case(R=2, N=600, seed=31)
    rng = np.random.default_rng(32)
    for _ in range(300):
        a, b = rng.choice(7, 2, replace=False)
        gr.add_distance((int(a), int(b)), rng.uniform(5.0, 15.0, 2), rng.uniform(0.0, 3.0, 2), flat=rng.choice([0.0, 0.3]))
    assert gr.nrestraints == 313
    _kernel_against_model(prec, pos, box, mass, gr, repeats=2)


def test_kernel_past_a_chunk_of_sixteen_replicas():
    pos, box, mass, gr = M.kernel_case(R=17, N=600, seed=12)
    _kernel_against_model("f32", pos, box, mass, gr, repeats=1)


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_kernel_one_group_of_thirty_thousand_atoms(prec):
    pos, box, mass, gr = M.big_case(N=70001, nbig=30000)
    _kernel_against_model(prec, pos, box, mass, gr, repeats=1)


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_single_atom_groups_equal_the_restraint_kernel(prec):
    """The same pairs as distance restraints of `Restraints` and as distances between single-atom groups: the two kernels'
    forces within one ulp of the dtype."""
    pos, box, mass, rs = TR.M.kernel_case(R=3, N=200)
    keep = rs.dist_k.copy()
    rs2 = Restraints(3)
    rs2.add_distance(rs.dist_pair, rs.dist_r0, keep)
    gr = GroupRestraints(3)
    index = {}
    for i, j in rs.dist_pair:
        for a in (int(i), int(j)):
            if a not in index:
                index[a] = gr.add_group([a], weights=[1.0])
    for d, (i, j) in enumerate(rs.dist_pair):
        gr.add_distance((index[int(i)], index[int(j)]), rs.dist_r0[:, d], keep[:, d])
    pos = pos.astype(NP[prec]).astype(np.float64)
    p = _tensor(pos, prec)
    _, eng_g = _context(mass, gr, prec, 3)
    from torchmd_amd.forces import Forces

    fr = Forces(TR._BarePar(mass, PREC[prec]), terms=[], restraints=rs2)
    eng_r = fr._engine(p)
    eng_r.sync_restraints(rs2)
    f_in = np.random.default_rng(1).normal(0.0, 20.0, pos.shape).astype(NP[prec]).astype(np.float64)
    fg, fr_ = _tensor(f_in, prec), _tensor(f_in, prec)
    eg = torch.zeros(3, 3, dtype=torch.float64, device=_dev())
    er = torch.zeros(3, 2, dtype=torch.float64, device=_dev())
    _apply(eng_g, p, box, forces=fg, energies=eg)
    _apply(eng_r, p, box, forces=fr_, energies=er, fn="tmdhip_restraint_apply")
    a, b = fg.cpu().double().numpy(), fr_.cpu().double().numpy()
    print(f"{prec}: single-atom groups against restraint_kernel: {(np.abs(a - b) / _ulp(b, prec)).max():.2f} ulp")
    assert np.abs(b - f_in).max() > 1.0 and (np.abs(a - b) <= _ulp(b, prec)).all()
    assert np.allclose(eg.cpu().numpy()[:, 0], er.cpu().numpy()[:, 1], rtol=1e-13)


def test_moving_a_window_replaces_the_tables():
    pos, box, mass, gr = M.kernel_case(R=3, N=600)
    f, eng = _context(mass, gr, "f64", 3)
    p = _tensor(pos, "f64")
    e = torch.zeros(3, 3, dtype=torch.float64, device=_dev())
    _apply(eng, p, box, energies=e)
    e0 = e.cpu().numpy().copy()
    t = gr.target.copy()
    t[:, :5] += 0.5
    v = gr.version
    gr.set_targets(t)
    gr.set_strengths(gr.k * 2.0)
    gr.set_flat(0.0)
    assert gr.version == v + 3 and eng.side_seen["group_restraints"] == (id(gr), v)
    gr.sync(eng, f)
    assert eng.side_seen["group_restraints"] == (id(gr), v + 3)
    _apply(eng, p, box, energies=e)
    E = gr.energy_forces(pos, box)[0]
    assert np.allclose(e.cpu().numpy(), E, rtol=1e-11) and np.abs(e.cpu().numpy() - e0).min() > 0.1


def test_library_refusals_launch_nothing():
    from torchmd_amd import _lib as L

    pos, box, mass, gr = M.kernel_case(R=3, N=600)
    f, eng = _context(mass, gr, "f64", 3)
    lib = eng.lib
    assert lib.tmdhip_abi_version() == 11
    p = _tensor(pos, "f64")
    frc = _tensor(np.zeros_like(pos), "f64")
    before = _bits(frc).clone()

    def refused(change, expect, ctx=None):
        d, keep = gr.descriptor()
        change(d, keep)
        assert lib.tmdhip_set_group_restraints(ctx or eng.ctx, C.byref(d)) < 0
        assert expect in L.last_error(), (expect, L.last_error())

    def set_(name, value):
        return lambda d, keep: setattr(d, name, value)

    def poke(index, where, value):
        def change(d, keep):
            keep[index].reshape(-1)[where] = value
        return change

    # keep: off, atoms, W, kind, groups, target, k, flat
    refused(set_("struct_size", 8), "size mismatch")
    refused(set_("nreplicas", 2), "nreplicas")
    refused(poke(0, 1, 0), "is empty")
    refused(poke(1, 2, 578), "named twice")  # (group 1 is (578, t))
    refused(poke(1, 0, 600), "out of range")
    refused(poke(1, 0, -1), "out of range")
    refused(poke(2, 3, 0.0), "weights")
    refused(poke(2, 3, np.inf), "weights")
    refused(poke(4, 1, 0), "a group is named twice")
    refused(poke(4, 2, 3), "wrong number of groups")
    refused(poke(4, 4 * 5 + 2, -1), "wrong number of groups")
    refused(poke(6, 3, -1.0), "finite k")
    refused(poke(7, 3, np.nan), "finite flat")
    refused(poke(5, 3, np.inf), "finite target")
    refused(poke(5, 5, 3.5), "[0, pi]")
    # the tables in place are the ones that were accepted: the evaluation is unchanged
    e = torch.zeros(3, 3, dtype=torch.float64, device=_dev())
    _apply(eng, p, box, energies=e)
    assert np.allclose(e.cpu().numpy(), gr.energy_forces(pos, box)[0], rtol=1e-11)
    # velocities without masses, and a group atom without mass where masses are first seen
    v = _tensor(np.zeros_like(pos), "f64")
    assert _apply(eng, p, box, vel=v, check=False) < 0 and "masses" in L.last_error()
    m0 = mass.copy()
    m0[578] = 0.0
    assert _apply(eng, p, box, vel=v, mass=_tensor(m0, "f64"), kick=1.0, check=False) < 0 and "no mass" in L.last_error()
    assert torch.equal(_bits(v), torch.zeros_like(_bits(v))) and torch.equal(_bits(frc), before)
    # 1 - gamma dt <= 0 in tmdhip_md_run, in the term's words
    d = L.MdDesc()
    d.struct_size = C.sizeof(L.MdDesc)
    boxes = np.ascontiguousarray(np.tile(box, (3, 1)))
    d.niter, d.pos_dev, d.vel_dev, d.forces_dev = 2, p.data_ptr(), v.data_ptr(), frc.data_ptr()
    mt = _tensor(mass, "f64")
    d.mass_dev, d.vcoeff_dev, d.box_host = mt.data_ptr(), mt.data_ptr(), boxes.ctypes.data_as(C.c_void_p)
    d.dt, d.gamma = 0.5, 2.0
    assert lib.tmdhip_md_run(eng.ctx, C.byref(d), _stream(p.device)) < 0 and "group restraints need 1 - gamma dt" in L.last_error()
    torch.cuda.synchronize()
    assert torch.equal(_bits(p), _bits(_tensor(pos, "f64"))) and torch.equal(_bits(v), torch.zeros_like(_bits(v)))
    # a group atom that is a virtual site of the context
    vd = L.VsiteDesc()
    vd.struct_size = C.sizeof(L.VsiteDesc)
    vd.enable, vd.nsites = 1, 1
    site, parent, weight = np.array([578], np.int32), np.array([[590, 591, -1]], np.int32), np.array([[0.5, 0.5, 0.0]])
    vd.site_host, vd.parent_host, vd.weight_host = (a.ctypes.data_as(C.c_void_p) for a in (site, parent, weight))
    L.check(lib.tmdhip_set_vsites(eng.ctx, C.byref(vd)), "tmdhip_set_vsites")
    refused(lambda d, keep: None, "virtual site")
    vd.enable = 0
    L.check(lib.tmdhip_set_vsites(eng.ctx, C.byref(vd)), "tmdhip_set_vsites")
    d2, keep = gr.descriptor()
    assert lib.tmdhip_set_group_restraints(eng.ctx, C.byref(d2)) == 0  # (the same tables, once the site is gone)
    # a context with passive atoms (what a brick of the domain decomposition is): a context of its own
    f2, eng2 = _context(mass, GroupRestraints(3), "f64", 3)
    types, charges = np.zeros(600, np.int32), np.zeros(600, np.float64)
    L.check(lib.tmdhip_update_atoms(eng2.ctx, 600, types.ctypes.data_as(C.c_void_p), charges.ctypes.data_as(C.c_void_p), 590),
            "tmdhip_update_atoms")
    refused(lambda d, keep: None, "passive atoms", ctx=eng2.ctx)
    e2 = torch.full((3, 3), -1.0, dtype=torch.float64, device=_dev())
    _apply(eng2, p, box, forces=frc, energies=e2)  # (no tables in place: nothing added, energies zero)
    assert torch.equal(_bits(frc), before) and (e2 == 0).all()
    out = np.full((3, 3, 3), -1.0)
    L.check(lib.tmdhip_group_restraint_states(eng2.ctx, C.c_void_p(p.data_ptr()), boxes.ctypes.data_as(C.POINTER(C.c_double)),
                                              out.ctypes.data_as(C.POINTER(C.c_double)), _stream(p.device)), "states")
    assert (out == 0).all()
    assert lib.tmdhip_group_restraint_states(eng.ctx, C.c_void_p(), boxes.ctypes.data_as(C.POINTER(C.c_double)),
                                             out.ctypes.data_as(C.POINTER(C.c_double)), _stream(p.device)) < 0
    assert "null argument" in L.last_error()
    # enable = 0 releases everything: nothing is added any more
    GroupRestraints(3).sync(eng, f)
    _apply(eng, p, box, forces=frc, energies=e)
    assert torch.equal(_bits(frc), before) and (e == 0).all()


def test_what_forces_and_the_integrator_refuse():
    from torchmd_amd.forces import Forces

    pos, box, mass, gr = M.kernel_case(R=3, N=600)
    with pytest.raises(ValueError, match="must be a group_restraints.GroupRestraints"):
        Forces(TR._BarePar(mass, torch.float64), terms=[], group_restraints=Restraints(3))
    with pytest.raises(ValueError, match="beyond the system"):
        Forces(TR._BarePar(mass[:500], torch.float64), terms=[], group_restraints=gr)
    m0 = mass.copy()
    m0[578] = 0.0
    with pytest.raises(ValueError, match="no mass"):
        Forces(TR._BarePar(m0, torch.float64), terms=[], group_restraints=gr)
    f = Forces(TR._BarePar(mass, torch.float64), terms=[], group_restraints=gr)
    p, b = _tensor(pos, "f64"), box_tensor(box, 3, torch.float64, _dev())
    with pytest.raises(ValueError, match="vmap"):
        torch.vmap(lambda x: f.compute(x, b, None, toNumpy=False))(p[None])
    with pytest.raises(ValueError, match="virial of the centres"):
        f.virial(p, b)
    with pytest.raises(ValueError, match="update_atoms"):
        f.update_atoms(TR._BarePar(mass, torch.float64))
    with pytest.raises(ValueError, match="needs group_restraints="):
        Forces(TR._BarePar(mass, torch.float64), terms=[]).group_restraint_energies(p, b)


# ----------------------------------------------------------------------------- against the oracle
def _water291_single_atoms(g):
    """Four O-O distances (TR's choice: some across a face) and four O-O-O angles on single-atom groups of water291."""
    rs = TR._water291_restraints(g)
    pos = np.asarray(g["pos"], dtype=np.float64).reshape(-1, 3)
    box = np.asarray(g["box"], dtype=np.float64).reshape(-1)[:3]
    rng = np.random.default_rng(14)
    gr = GroupRestraints(1)
    single = {}

    def grp(a):
        if a not in single:
            single[a] = gr.add_group([int(a)], weights=[2.5])
        return single[a]

    pairs = [tuple(int(a) for a in p) for p in rs.dist_pair[:4]]
    d = min_image(pos[pairs[0][0]] - pos[pairs[0][1]], box)
    assert np.any(np.abs((pos[pairs[0][0]] - pos[pairs[0][1]]) - d) > 0)  # across a face
    for (i, j), r0, k in zip(pairs, rs.dist_r0[0, :4], rs.dist_k[0, :4]):
        gr.add_distance((grp(i), grp(j)), r0, k)
    ox = np.arange(0, len(pos), 3)
    triples, used = [], set()
    for b in ox:
        dm = min_image(pos[ox] - pos[b], box)
        r = np.linalg.norm(dm, axis=1)
        near = [int(a) for a in ox[np.argsort(r)[1:3]]]
        u, v = min_image(pos[near[0]] - pos[b], box), min_image(pos[near[1]] - pos[b], box)
        c = np.dot(u, v) / np.linalg.norm(u) / np.linalg.norm(v)
        if abs(c) < 0.8 and not used & {int(b), *near}:
            triples.append((near[0], int(b), near[1]))
            used |= {int(b), *near}
        if len(triples) == 4:
            break
    th0, ka = rng.uniform(1.0, 2.4, 4), rng.uniform(20.0, 120.0, 4)
    for t, a0, k in zip(triples, th0, ka):
        gr.add_angle(tuple(grp(a) for a in t), a0, k)
    return gr, pairs, triples


@pytest.mark.parametrize("prec", ["f64", "f32"])
def test_forces_with_single_atom_groups_equal_the_oracle_with_extra_bonds_and_angles(prec):
    from oracle import torchmd_oracle as orc
    from torchmd_amd.forces import Forces

    g = load("water291")
    dt = PREC[prec]
    par = GoldenParameters(g, dt)
    gr, pairs, triples = _water291_single_atoms(g)
    f = Forces(par, terms=WATER_TERMS, cutoff=7.3, rfa=True, group_restraints=gr)
    p, b = pos_tensor(g["pos"], 1, dt, _dev()), box_tensor(g["box"], 1, dt, _dev())
    F = torch.full_like(p, 7.0)
    pots = f.compute(p, b, F, returnDetails=True)
    total = f.compute(p, b, torch.zeros_like(p))[0]
    opar = GoldenParameters(g, dt)

    def extend(tab, idx, params):
        n, nb = len(idx), len(tab["params"])
        return {"idx": torch.cat([tab["idx"], torch.as_tensor(idx, dtype=tab["idx"].dtype)]),
                "map": torch.cat([tab["map"], torch.stack([torch.arange(n) + len(tab["map"]), torch.arange(n) + nb], dim=1).to(tab["map"].dtype)]),
                "params": torch.cat([tab["params"], torch.as_tensor(params, dtype=dt)])}

    opar.bond_params = extend(opar.bond_params, pairs, np.stack([0.5 * gr.k[0, :4], gr.target[0, :4]], axis=1))
    opar.angle_params = extend(opar.angle_params, triples, np.stack([0.5 * gr.k[0, 4:], gr.target[0, 4:]], axis=1))
    nb_pairs = orc.all_pairs(par.natoms, orc.exclusion_pairs(par))
    opots, oF, _ = orc.compute(opar, p.cpu(), b.cpu(), WATER_TERMS, pairs=nb_pairs, cutoff=7.3, rfa=True)
    ototal = sum(opots[0][t] for t in WATER_TERMS)
    plain, _, _ = orc.compute(par, p.cpu(), b.cpu(), WATER_TERMS, pairs=nb_pairs, cutoff=7.3, rfa=True)
    err = (F.cpu() - oF).abs().max().item()
    extra = (opots[0]["bonds"] - plain[0]["bonds"]) + (opots[0]["angles"] - plain[0]["angles"])
    print(f"{prec}: max|dF| = {err:.2e}, E = {total:.6f} (oracle {ototal:.6f}), group restraints {pots[0]['group_restraints']:.6f} ({extra:.6f})")
    assert pots[0]["group_restraints"] > 1.0 and list(pots[0])[-1] == "group_restraints"
    assert f.group_restraints.energy[0, 0] > 0.5 and f.group_restraints.energy[0, 1] > 0.5 and f.group_restraints.energy[0, 2] == 0.0
    assert err <= FTOL[prec]
    assert abs(total - ototal) <= ERTOL[prec] * EFAC * max(1.0, abs(ototal))
    assert abs(pots[0]["group_restraints"] - extra) <= ERTOL[prec] * EFAC * max(1.0, abs(opots[0]["bonds"]) + abs(opots[0]["angles"]))
    assert abs(sum(pots[0].values()) - total) <= 1e-9 * abs(total)
    pots0 = Forces(par, terms=WATER_TERMS, cutoff=7.3, rfa=True).compute(p, b, torch.zeros_like(p), returnDetails=True)
    assert "group_restraints" not in pots0[0]


# ----------------------------------------------------------------------------- trajectories
def _mixed(pos, box, R, nwat, k=100.0):
    """One centre-of-mass distance between two groups of `nwat` whole waters on either side of the x face, every replica with a
    target of its own, and one Boresch set on six oxygens near the middle of the box, every target off its present value."""
    p = pos[:, :, 0] if pos.ndim == 3 else pos
    L = np.asarray(box, dtype=np.float64).reshape(-1)[:3]
    ox = np.arange(0, len(p), 3)

    def waters_near(point, n, skip=()):
        r = np.linalg.norm(min_image(p[ox] - point, L), axis=1)
        picked = [int(a) for a in ox[np.argsort(r)] if int(a) not in skip][:n]
        return picked, np.concatenate([[a, a + 1, a + 2] for a in picked])

    wa, ga = waters_near(np.array([0.17 * L[0], 0.5 * L[1], 0.5 * L[2]]), nwat)
    wb, gb = waters_near(np.array([0.83 * L[0], 0.5 * L[1], 0.5 * L[2]]), nwat, skip=set(wa))
    near = waters_near(0.5 * L, 14, skip=set(wa) | set(wb))[0]
    rng = np.random.default_rng(17)
    best = None
    for _ in range(2000):
        six = [int(a) for a in rng.permutation(near)[:6]]
        trial = GroupRestraints.boresch(1, six[:3], six[3:], 1.0, 1.0, 1.0, 0.0, 0.0, 0.0, 1.0, 1.0, 1.0)
        s = M.sines(trial, p, L).min()
        r = trial.values(p, L)[0, 0]
        if s > 0.6 and 3.0 < r < 0.4 * L.min():
            best = six
            break
    assert best is not None
    gr = GroupRestraints(R)
    P = [gr.add_group([a], weights=[1.0]) for a in best[:3]]
    Lg = [gr.add_group([a], weights=[1.0]) for a in best[3:]]
    a, b = gr.add_group(ga), gr.add_group(gb)
    s = trial.values(p, L)[0]
    gr.add_distance((P[0], Lg[0]), s[0] + 0.5, k)
    gr.add_angle((P[1], P[0], Lg[0]), float(np.clip(s[1] + 0.3, 0.1, np.pi - 0.1)), k)
    gr.add_angle((P[0], Lg[0], Lg[1]), float(np.clip(s[2] - 0.3, 0.1, np.pi - 0.1)), k)
    gr.add_dihedral((P[2], P[1], P[0], Lg[0]), s[3] + 0.3, k)
    gr.add_dihedral((P[1], P[0], Lg[0], Lg[1]), s[4] - 0.3, k)
    gr.add_dihedral((P[0], Lg[0], Lg[1], Lg[2]), s[5] + 0.3, k)
    return gr, (a, b)


def _add_com_distance(gr, ab, par, pos, box, R, k=100.0):
    """(after the masses are known: the distance's present value needs the centres)"""
    p = pos[:, :, 0] if pos.ndim == 3 else pos
    L = np.asarray(box, dtype=np.float64).reshape(-1)[:3]
    gr.masses = par.masses.detach().cpu().double().reshape(-1).numpy()
    one = GroupRestraints(1)
    for g in range(gr.ngroups):
        one.add_group(gr.group_atoms[g], gr.group_weights[g])
    one.masses = gr.masses
    X = one.centres(p, L)[0]
    raw = X[ab[0]] - X[ab[1]]
    d = min_image(raw, L)
    assert np.any(np.abs(raw - d) > 0) and one.check_extent(p, L)  # across a face, and whole
    r = float(np.linalg.norm(d))
    gr.add_distance(ab, np.array([r + 0.4 * (q + 1) for q in range(R)]), k)
    return gr


def _tip3p_groups(pos, box, par, R, k=100.0):
    gr, ab = _mixed(pos, box, R, 10, k)
    assert len(gr.group_atoms[ab[0]]) == 30 and len(gr.group_atoms[ab[1]]) == 30
    return _add_com_distance(gr, ab, par, pos, box, R, k)


class _Halved:
    """The control: the model with every k halved."""

    def __init__(self, gr):
        self.gr = gr

    def energy_forces(self, pos, box):
        return self.gr.energy_forces(pos, box, k_scale=0.5)


def _under_test(case, prec, gr, cuts, langevin, **fkw):
    """`Integrator.step` of a Forces WITH the term, cut as `cuts`."""
    from torchmd_amd.forces import Forces
    from torchmd_amd.integrator import Integrator

    mol, pos, box, par, vel0, R, terms, kw = case
    s = TR._system(mol, pos, box, vel0, prec, R)
    f = Forces(par, terms=terms, group_restraints=gr, **kw, **fkw)
    f.compute(s.pos, s.box, s.forces)
    torch.manual_seed(77)
    integ = Integrator(s, f, 1.0, _dev(), **(dict(gamma=50.0, T=300.0) if langevin else {}))
    out = None
    for n in cuts:
        out = integ.step(n)
    return s.pos.cpu().double().numpy(), s.vel.cpu().double().numpy(), s.forces.cpu().double().numpy(), out, f, s, integ


def _check_return(prec, out, f, s, gr, forces, integ):
    """The potential energy the call returns is compute()'s total at the final positions, the forces it leaves include the
    term, and the kinetic energy it returns is that of the velocities it leaves (TR._check_return's bounds)."""
    from torchmd_amd import _lib as L

    K = torch.zeros(s.vel.shape[0], dtype=torch.float64, device=s.vel.device)
    L.check(L.load().tmdhip_kinetic_energy(L.dtype_code(s.vel.dtype), s.vel.shape[0], s.vel.shape[1], s.vel.data_ptr(),
                                           integ.masses.data_ptr(), K.data_ptr(), _stream(s.vel.device)), "tmdhip_kinetic_energy")
    K = K.cpu().numpy()
    bound = K * (64 * EPS64 + (np.finfo(np.float32).eps if prec == "f32" else 0.0))
    assert (np.abs(np.asarray(out[0], dtype=np.float64) - K) <= bound).all(), (out[0], K)
    hbox = np.diagonal(s.box.cpu().double().numpy(), axis1=1, axis2=2)
    Er, Fr = gr.energy_forces(s.pos.cpu().double().numpy(), hbox)
    m = integ.masses.cpu().double().numpy().reshape(1, -1, 1)
    v1 = s.vel.cpu().double().numpy()
    v0 = v1 - 0.5 * integ.dt * Fr / m  # the velocities before the finishing kick
    stale = np.abs(0.5 * (m * (v1 * v1 - v0 * v0)).sum(axis=(1, 2)))
    assert (stale > 10 * bound).all(), (stale, bound)  # (a sum taken before the kick would miss the bound)
    F2 = torch.zeros_like(s.pos)
    tot = f.compute(s.pos, s.box, F2)
    for r in range(s.pos.shape[0]):
        assert abs(out[1][r] - tot[r]) <= ERTOL[prec] * EFAC * max(1.0, abs(tot[r])), (r, out[1][r], tot[r])
    assert np.abs(forces - F2.cpu().double().numpy()).max() <= FTOL[prec] * 10
    assert np.abs(Fr).max() > 10.0 and np.allclose(f.group_restraints.energy, Er, rtol=1e-5, atol=1e-6)
    plain = forces - Fr  # what is left without the term is far from the total on the group atoms
    assert np.abs(plain - F2.cpu().double().numpy()).max() > 10.0


CUTS = TR.CUTS


@pytest.mark.parametrize("langevin", [False, True], ids=["nve", "langevin"])
def test_trajectory_fp64_list_path(langevin, monkeypatch):
    monkeypatch.setenv("TMDHIP_VSKIN", "0")
    mol, pos, box, par, vel0 = TR._tip3p("f64", 1)
    gr = _tip3p_groups(pos, box, par, 1)
    case = (mol, pos, box, par, vel0, 1, WATER_TERMS, dict(cutoff=9.0, rfa=True))
    tp, tv = TR._by_hand(case, "f64", gr, CUTS, langevin)
    p, v, frc, out, f, s, integ = _under_test(case, "f64", gr, CUTS, langevin)
    bar_p, bar_v = 64 * EPS64 * 10 * np.abs(tp).max(), 64 * EPS64 * 10 * np.abs(tv).max()
    print(f"fp64 list path, {'Langevin' if langevin else 'NVE'}: |dpos| = {np.abs(p - tp).max():.2e} (bar {bar_p:.2e}), "
          f"|dvel| = {np.abs(v - tv).max():.2e} (bar {bar_v:.2e})")
    assert f.stats(s.pos)["algorithm"] == "celllist" and f.stats(s.pos)["steps_in_pair_launch"] == 0
    assert np.abs(p - tp).max() <= bar_p and np.abs(v - tv).max() <= bar_v
    _check_return("f64", out, f, s, gr, frc, integ)


@pytest.mark.parametrize("langevin", [False, True], ids=["nve", "langevin"])
@pytest.mark.parametrize("R", [1, 3], ids=["lone", "batched"])
def test_trajectory_fp32_fused(R, langevin, monkeypatch):
    monkeypatch.setenv("TMDHIP_VSKIN", "0")
    mol, pos, box, par32, vel0 = TR._tip3p("f32", R)
    _, _, _, par64, _ = TR._tip3p("f64", R)
    gr = _tip3p_groups(pos, box, par64, R)
    if R == 3:
        assert len(set(gr.target[:, -1])) == 3
    kw = dict(cutoff=9.0, rfa=True)
    case64 = (mol, pos, box, par64, vel0, R, WATER_TERMS, kw)
    case32 = (mol, pos, box, par32, vel0, R, WATER_TERMS, kw)
    tp, tv = TR._by_hand(case64, "f64", gr, CUTS, langevin)
    hp, hv = TR._by_hand(case32, "f32", gr, CUTS, langevin)
    p, v, frc, out, f, s, integ = _under_test(case32, "f32", gr, CUTS, langevin)
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
    cp, cv = TR._by_hand(case32, "f32", _Halved(gr), CUTS, langevin)
    assert np.abs(cp - tp).max() > 10 * 2 * noise_p and np.abs(cv - tv).max() > 10 * 2 * noise_v
    _check_return("f32", out, f, s, gr, frc, integ)


def _water291_groups(case, R, nwat=3):
    gr, ab = _mixed(case[1], case[2], R, nwat)
    return _add_com_distance(gr, ab, case[3], case[1], case[2], R)


def test_trajectory_fp64_all_pairs_replicas_together():
    case = TR._water291_case("f64", 2, cutoff=7.3, rfa=True)
    gr = _water291_groups(case, 2)
    tp, tv = TR._by_hand(case, "f64", gr, CUTS, True)
    p, v, frc, out, f, s, integ = _under_test(case, "f64", gr, CUTS, True)
    bar_p, bar_v = 64 * EPS64 * 10 * np.abs(tp).max(), 64 * EPS64 * 10 * np.abs(tv).max()
    print(f"fp64 all pairs x 2: |dpos| = {np.abs(p - tp).max():.2e} (bar {bar_p:.2e}), |dvel| = {np.abs(v - tv).max():.2e} (bar {bar_v:.2e})")
    assert f.stats(s.pos)["algorithm"] == "allpairs"
    assert np.abs(p - tp).max() <= bar_p and np.abs(v - tv).max() <= bar_v
    _check_return("f64", out, f, s, gr, frc, integ)


def test_trajectory_fp64_pme():
    case = TR._water291_case("f64", 1, cutoff=7.0, pme=True)
    gr = _water291_groups(case, 1)
    tp, tv = TR._by_hand(case, "f64", gr, CUTS, True)
    p, v, frc, out, f, s, integ = _under_test(case, "f64", gr, CUTS, True)
    bar_p, bar_v = 64 * EPS64 * 10 * np.abs(tp).max(), 64 * EPS64 * 10 * np.abs(tv).max()
    print(f"fp64 PME: |dpos| = {np.abs(p - tp).max():.2e} (bar {bar_p:.2e}), |dvel| = {np.abs(v - tv).max():.2e} (bar {bar_v:.2e})")
    assert f.stats(s.pos)["pme_evaluations"] > 0
    assert np.abs(p - tp).max() <= bar_p and np.abs(v - tv).max() <= bar_v
    _check_return("f64", out, f, s, gr, frc, integ)


# ----------------------------------------------------------------------------- exchange
@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_cross_energies_against_the_model_and_the_runs_row(prec):
    from torchmd_amd import _lib as L

    R = 4
    pos, box, mass, gr = M.kernel_case(R=R, N=600, seed=21)
    pos = pos.astype(NP[prec]).astype(np.float64)
    f, eng = _context(mass.astype(NP[prec]).astype(np.float64), gr, prec, R)
    p, b = _tensor(pos, prec), box_tensor(box, R, PREC[prec], _dev())
    e = torch.zeros(R, 3, dtype=torch.float64, device=_dev())
    _apply(eng, p, box, energies=e)
    row = e.cpu().numpy().copy()
    cross = f.group_restraint_energies(p, b)
    assert cross.shape == (R, R, 3)
    for k in range(R):  # configuration i under row k: the model with row k in every slot
        shifted = GroupRestraints(R)
        for g in range(gr.ngroups):
            shifted.add_group(gr.group_atoms[g], gr.group_weights[g])
        shifted.masses = gr.masses
        for m in range(gr.nrestraints):
            kind = int(gr.kind[m])
            shifted._add(kind, gr.groups[m, : kind + 2], np.full(R, gr.target[k, m]), np.full(R, gr.k[k, m]), np.full(R, gr.flat[k, m]))
        E, Fm = shifted.energy_forces(pos, box)
        nmax = max(len(a) for a in gr.group_atoms)  # (M eps64 sum|E| for the order of the sum, and the centres' slack as for the forces)
        bar = gr.nrestraints * EPS64 * np.abs(E).sum(axis=1).max() + 64 * nmax * EPS64 * np.abs(Fm).max()
        assert np.abs(cross[:, k] - E).max() <= bar, (k, cross[:, k], E)
    for i in range(R):
        assert cross[i, i].tobytes() == row[i].tobytes()  # the bits of the evaluation's row
    again = f.group_restraint_energies(p, b)
    assert again.tobytes() == cross.tobytes()
    # the run's row is left alone
    run_row = np.full((R, 3), -1.0)
    L.check(eng.lib.tmdhip_group_restraint_energy(eng.ctx, run_row.ctypes.data_as(C.POINTER(C.c_double)), _stream(_dev())), "energy")
    f.group_restraint_energies(p, b)
    run_row2 = np.full((R, 3), -1.0)
    L.check(eng.lib.tmdhip_group_restraint_energy(eng.ctx, run_row2.ctypes.data_as(C.POINTER(C.c_double)), _stream(_dev())), "energy")
    assert run_row.tobytes() == run_row2.tobytes()


def test_hamiltonian_exchange_walks_the_windows_of_a_centre_of_mass_distance(monkeypatch):
    """Replica-exchange umbrella sampling on a centre-of-mass distance, without an edit to hrex.py: four windows at one
    temperature, u = 0 (every tried pair is accepted, as §16's test forces it)."""
    import _exchange as X
    from torchmd_amd.forces import Forces
    from torchmd_amd.hrex import HamiltonianExchange
    from torchmd_amd.integrator import Integrator

    R = 4
    mol, pos, box, par, vel0 = TR._tip3p("f64", R)
    gr, ab = _mixed(pos, box, R, 10)
    windows = GroupRestraints(R)
    a, b = windows.add_group(gr.group_atoms[ab[0]]), windows.add_group(gr.group_atoms[ab[1]])
    _add_com_distance(windows, (a, b), par, pos, box, R, k=40.0)
    assert len(set(windows.target[:, 0])) == 4
    s = TR._system(mol, pos, box, vel0, "f64", R)
    f = Forces(par, terms=WATER_TERMS, cutoff=9.0, rfa=True, group_restraints=windows)
    f.compute(s.pos, s.box, s.forces)
    hx = HamiltonianExchange(frequency=5, seed=3)
    hx.rng = X.Counting(0.0)
    seen, inner = [], hx.attempt

    def attempt(system, forces, epot=None):
        before = np.asarray(epot, dtype=np.float64).copy()
        tot = np.asarray(forces.compute(system.pos, system.box, torch.zeros_like(system.pos)))  # (under the old assignment)
        pot = inner(system, forces, epot)
        seen.append((before, tot, None if pot is None else np.asarray(pot, dtype=np.float64), hx.states.copy(),
                     system.pos.detach().clone(), system.forces.detach().clone()))
        return pot

    hx.attempt = attempt
    torch.manual_seed(77)
    integ = Integrator(s, f, 1.0, _dev(), gamma=1.0, T=300.0, exchange=hx)
    integ.step(20)
    assert hx.nattempts == 4 and [h.tolist() for h in hx.history] == [[1, 0, 3, 2], [2, 0, 3, 1], [3, 1, 2, 0], [3, 2, 1, 0]]
    assert np.array_equal(hx.accepted, hx.attempts)
    plain = Forces(par, terms=WATER_TERMS, cutoff=9.0, rfa=True)
    hbox = np.tile(np.asarray(box, dtype=np.float64).reshape(-1)[:3], (R, 1))
    for k, (before, tot, pot, states, p, frc) in enumerate(seen):
        # each attempt's energies are compute()'s totals at the positions of that moment
        assert (np.abs(before - tot) <= ERTOL["f64"] * EFAC * np.maximum(1.0, np.abs(tot))).all(), (k, before, tot)
        # after the accepted swap the forces are the plain forces plus the model's under the new assignment
        assert pot is not None
    # ... and the forces and energies it leaves: the plain forces plus the model's under each recorded assignment
    snap = hx.snapshots[0]
    assert np.array_equal(windows.target[:, 0], snap["target"][hx.states, 0]) and hx.states.tolist() == [3, 2, 1, 0]
    for k, (before, tot, pot, states, p, frc) in enumerate(seen):
        model = GroupRestraints(R)
        for g in range(windows.ngroups):
            model.add_group(windows.group_atoms[g])
        model.masses = windows.masses
        model.add_distance((0, 1), snap["target"][states, 0], snap["k"][states, 0], snap["flat"][states, 0])
        Er, Fr = model.energy_forces(p.cpu().numpy(), hbox)
        F0 = torch.zeros_like(p)
        e0 = np.asarray(plain.compute(p, s.box, F0))
        assert np.abs(frc.cpu().numpy() - (F0.cpu().numpy() + Fr)).max() <= FTOL["f64"] * 10 and np.abs(Fr).max() > 1.0, k
        assert (np.abs(pot - (e0 + Er.sum(axis=1))) <= ERTOL["f64"] * EFAC * np.abs(pot)).all(), k


# ----------------------------------------------------------------------------- invariants and allowed combinations
def _water291_run(gr, R=1, prec="f64", vel_scale=0.01, fkw=None, **integ_kw):
    from torchmd_amd.forces import Forces
    from torchmd_amd.integrator import Integrator

    case = TR._water291_case(prec, R, cutoff=7.3, rfa=True)
    mol, pos, box, par, vel0, _, terms, kw = case
    s = TR._system(mol, pos, box, vel0 * (vel_scale / 0.01), prec, R)
    f = Forces(par, terms=terms, **kw, **(fkw or {}), **({} if gr is None else {"group_restraints": gr}))
    f.compute(s.pos, s.box, s.forces)
    torch.manual_seed(3)
    return s, f, Integrator(s, f, 1.0, _dev(), **integ_kw)


def test_nve_energy_drift_is_that_of_the_plain_run():
    """NVE, fp64, 200 steps on water291: the drift of E_kin + E_pot (the term included) is at most twice the plain run's."""
    drift = {}
    for name in ("plain", "restrained"):
        gr = _water291_groups(TR._water291_case("f64", 1), 1) if name == "restrained" else None
        s, f, integ = _water291_run(gr)
        e = []
        for _ in range(10):
            ek, ep, _ = integ.step(20)
            e.append(float(ek[0]) + ep[0])
        drift[name] = np.abs(np.asarray(e) - e[0]).max()
        if gr is not None:
            assert f.group_restraints.energy.sum() > 1.0
    print(f"NVE drift over 200 steps: plain {drift['plain']:.3e}, with group restraints {drift['restrained']:.3e} kcal/mol")
    assert drift["restrained"] <= 2 * drift["plain"]


def test_constrained_water_with_group_atoms_inside_the_molecules():
    """constraints="water" at 2 fs, the groups made of atoms of constrained molecules: the bond lengths are kept as the plain
    run keeps them (TR's bar: four times the plain run's figure plus 8 eps64; SETTLE is analytic)."""
    from torchmd_amd.builders import tip3p_box, water_forcefield
    from torchmd_amd.forces import Forces
    from torchmd_amd.integrator import Integrator, maxwell_boltzmann
    from torchmd_amd.parameters import Parameters

    mol, pos, box = tip3p_box(6, seed=3)
    pos = np.asarray(pos, dtype=np.float64)
    par = Parameters(water_forcefield(mol), mol, WATER_TERMS, precision=torch.float64)
    dev_bond, energy = {}, None
    for name in ("plain", "restrained"):
        gr = None
        if name == "restrained":
            gr, ab = _mixed(pos, box, 1, 4)
            gr = _add_com_distance(gr, ab, par, pos, box, 1)
        torch.manual_seed(9)
        vel0 = maxwell_boltzmann(par.masses, 300.0, 1)
        s = TR._system(mol, pos, box, vel0, "f64", 1)
        f = Forces(par, terms=WATER_TERMS, cutoff=7.0, rfa=True, **({} if gr is None else {"group_restraints": gr}))
        f.compute(s.pos, s.box, s.forces)
        integ = Integrator(s, f, 2.0, _dev(), gamma=1.0, T=300.0, constraints="water")
        for _ in range(10):
            integ.step(20)
        if gr is not None:
            energy = f.group_restraints.energy.copy()
        p = s.pos[0].cpu().double().numpy()
        cs = integ.constraints
        w = np.asarray(cs.waters)
        d = np.stack([np.linalg.norm(p[w[:, 0]] - p[w[:, 1]], axis=1), np.linalg.norm(p[w[:, 0]] - p[w[:, 2]], axis=1),
                      np.linalg.norm(p[w[:, 1]] - p[w[:, 2]], axis=1)], axis=1)
        d0 = np.asarray(cs.water_dist)
        want = np.stack([d0[:, 0], d0[:, 0], d0[:, 1]], axis=1)
        dev_bond[name] = np.abs(d / want - 1.0).max()
    print(f"bond lengths: plain {dev_bond['plain']:.2e}, with group restraints {dev_bond['restrained']:.2e}; energies {energy}")
    assert dev_bond["restrained"] <= 4 * dev_bond["plain"] + 8 * EPS64
    assert np.isfinite(energy).all() and energy.sum() > 0.0


def test_minimize_fire_converges_on_the_total_force():
    from torchmd_amd.minimizers import minimize_fire

    gr = _water291_groups(TR._water291_case("f64", 1), 1)
    s, f, _ = _water291_run(gr)
    e0 = gr.energy_forces(s.pos.cpu().numpy(), np.diagonal(s.box.cpu().numpy(), axis1=1, axis2=2))[0].sum()
    minimize_fire(s, f, fmax=0.5, steps=5000)
    F = torch.zeros_like(s.pos)
    pots = f.compute(s.pos, s.box, F, returnDetails=True)
    fmax = F.norm(dim=2).max().item()
    print(f"FIRE: max|F_total| = {fmax:.3f}, group-restraint energy {e0:.3f} -> {pots[0]['group_restraints']:.3f}")
    assert fmax <= 0.5
    assert pots[0]["group_restraints"] < 0.5 * e0  # the term pulled: a minimiser blind to it would have left its energy


def test_thermostat_ladder_exchange_and_plain_restraints_together():
    """`thermostat=`, `ReplicaExchange` and `restraints=` next to the term: the energies the exchange decides on are compute()'s
    totals, both restraint terms included."""
    from torchmd_amd.exchange import ReplicaExchange
    from torchmd_amd.thermostat import VelocityRescale

    case = TR._water291_case("f64", 2)
    gr = _water291_groups(case, 2)
    rs = TR._water291_mixed(case, 2)
    th, ex = VelocityRescale([300.0, 310.0], tau=0.1, frequency=10, seed=2), ReplicaExchange(frequency=10, seed=2)
    s, f, integ = _water291_run(gr, R=2, fkw=dict(restraints=rs), thermostat=th, exchange=ex)
    integ.step(10)
    pots = f.compute(s.pos, s.box, torch.zeros_like(s.pos), returnDetails=True)
    tot = np.asarray([sum(p.values()) for p in pots])
    eg, er = f.group_restraints.energy.sum(axis=1), f.restraints.energy.sum(axis=1)
    assert list(pots[0])[-2:] == ["restraints", "group_restraints"] and eg.min() > 1.0 and er.min() > 1.0
    assert ex.record is not None and np.allclose(ex.record["U"], tot, rtol=1e-9)
    assert not np.allclose(ex.record["U"], tot - eg, rtol=1e-6)
    from torchmd_amd.barostat import MonteCarloBarostat

    with pytest.raises(ValueError, match="barostat"):
        _water291_run(_water291_groups(TR._water291_case("f64", 1), 1), gamma=1.0, T=300.0,
                      barostat=MonteCarloBarostat(1.0, 300.0, frequency=5, seed=1))
    with pytest.raises(ValueError, match="batch"):
        _water291_run(_water291_groups(TR._water291_case("f64", 1), 1), batch=torch.zeros(291, dtype=torch.long))


def test_alchemical_solute_held_by_a_boresch_set():
    """`alchemical=` plus `GroupRestraints.boresch`: one water decoupled in two replicas and held relative to three oxygens
    of its surroundings; compute()'s total is the sum of its entries, and ten steps run."""
    from torchmd_amd.alchemy import Alchemical
    from torchmd_amd.forces import Forces
    from torchmd_amd.integrator import Integrator

    R = 2
    case = TR._water291_case("f64", R, cutoff=7.3, rfa=True)
    mol, pos, box, par, vel0, _, terms, kw = case
    L = box
    solute = [150, 151, 152]
    ox = np.array([a for a in range(0, len(pos), 3) if a != 150])
    r = np.linalg.norm(min_image(pos[ox] - pos[150], L), axis=1)
    near = ox[np.argsort(r)][:8]
    rng, best = np.random.default_rng(3), None
    for _ in range(500):
        rec = [int(a) for a in rng.permutation(near)[:3]]
        trial = GroupRestraints.boresch(1, rec, solute, 1.0, 1.0, 1.0, 0.0, 0.0, 0.0, 1.0, 1.0, 1.0)
        if M.sines(trial, pos, L).min() > 0.5:
            best = rec
            break
    assert best is not None
    sv = trial.values(pos, L)[0]
    gr = GroupRestraints.boresch(R, best, solute, sv[0] + 0.2, float(np.clip(sv[1] + 0.1, 0.1, 3.0)), float(np.clip(sv[2] - 0.1, 0.1, 3.0)),
                                 sv[3] + 0.1, sv[4] - 0.1, sv[5] + 0.1, 10.0, 10.0, 10.0)
    al = Alchemical(solute, [1.0, 0.5], [1.0, 0.0])
    s = TR._system(mol, pos, box, vel0, "f64", R)
    f = Forces(par, terms=terms, alchemical=al, group_restraints=gr, **kw)
    F = torch.zeros_like(s.pos)
    pots = f.compute(s.pos, s.box, F, returnDetails=True)
    tot = f.compute(s.pos, s.box, s.forces)
    for r_ in range(R):
        assert list(pots[r_])[-2:] == ["alchemical", "group_restraints"] and pots[r_]["group_restraints"] > 0.1
        assert abs(sum(pots[r_].values()) - tot[r_]) <= 1e-9 * abs(tot[r_])
    corr = gr.boresch_standard_state(300.0)
    assert corr.shape == (R,) and np.isfinite(corr).all() and (corr < 0).all()
    torch.manual_seed(1)
    integ = Integrator(s, f, 1.0, _dev(), gamma=1.0, T=300.0)
    ek, ep, _ = integ.step(10)
    assert np.isfinite(np.asarray(ek, dtype=np.float64)).all() and np.isfinite(np.asarray(ep, dtype=np.float64)).all()
    assert np.isfinite(f.group_restraints.energy).all() and torch.isfinite(s.pos).all()


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
np.savez(os.path.join(TMP, "groups.npz"), group_off=np.array([0, 3, 6, 7]), member_atom=np.array([0, 1, 2, 3, 4, 5, 150]),
         kind=np.array([0, 1]), groups=np.array([[0, 1, -1, -1], [0, 2, 1, -1]]), target=np.array([[4.0, 1.0], [4.5, 1.2]]),
         k=np.array([100.0, 50.0]))
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
out["module_after_off"] = "torchmd_amd.group_restraints" in sys.modules
go("log_gr", group_restraints=os.path.join(TMP, "groups.npz"))
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
    assert out["log"]["files"] == files and out["log_gr"]["files"] == files
    assert all(rows[0] == "iter,ns,epot,ekin,etot,T,t" and len(rows) == 3 for rows in out["log"]["rows"])
    energies = []
    for rows in out["log_gr"]["rows"]:
        assert rows[0] == "iter,ns,epot,ekin,etot,T,group_restraints,t" and len(rows) == 3
        vals = np.array([[float(x) for x in r.split(",")] for r in rows[1:]])
        assert np.isfinite(vals).all() and (vals[:, 6] > 0.1).all()
        energies.append(vals[-1, 6])
    assert energies[0] != energies[1]  # a window of its own per replica
