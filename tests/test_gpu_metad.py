"""Well-tempered metadynamics on the device: the kernels of metad.hip against the numpy model
(`Metadynamics.energy_forces`, `deposit_model`), and `Integrator.step` under a bias — which never enters the pair or step
kernels but is applied as an impulse between their launches, and grows by a deposition between two segments — against a loop
made by hand of parts that know nothing of a bias (the helpers of tests/test_gpu_restraints.py, imported).

Bars.  Hills log: the CVs within 1e-12 rad / Å of the model's in fp64 (atan2 and sqrt of the same doubles), 1e-6 in fp32 where
the model reads the rounded positions too (in fact the same bits: metad_math.h's atan2 is made of the four operations alone);
heights as the model's from the same V.  Grid nodes: within 8 eps64 x sum|terms| of the model's own chain (the device's exp is
not glibc's; with a libm atan2 a centre one ulp off would move a far node's term by |Delta| / sigma^2 ulps, and the chain missed
this bar by a factor of ten).  Forces
and velocities: fp32 within 1 ulp of dtype(float64(in) + model), fp64 within 1e-9 max|F_b| (libm ulps x the bounded
conditioning of the dihedral gradient, three decades of margin).  Trajectories: as tests/test_gpu_restraints.py."""

import ctypes as C
import os
import types

import numpy as np
import pytest
import torch

import _metad as M
import test_gpu_restraints as TR
from _golden import PREC, GoldenParameters, load
from torchmd_amd.integrator import BOLTZMAN
from torchmd_amd.metadynamics import Metadynamics

pytestmark = pytest.mark.gpu

NP = {"f32": np.float32, "f64": np.float64}
EPS64 = np.finfo(np.float64).eps
WATER_TERMS = TR.WATER_TERMS
ALL_TERMS = ["bonds", "angles", "dihedrals", "impropers", "1-4", "electrostatics", "lj"]
PHI, PSI = (4, 6, 8, 14), (6, 8, 14, 16)  # alanine dipeptide: C-N-CA-C and N-CA-C-N

_dev, _bits, _tensor, _stream, _ulp = TR._dev, TR._bits, TR._tensor, TR._stream, TR._ulp


def _context(mass, md, prec, R):
    """(Forces, engine) of a context that holds nothing but the bias."""
    from torchmd_amd.forces import Forces

    f = Forces(TR._BarePar(mass, PREC[prec]), terms=[], metadynamics=md)
    eng = f._engine(torch.zeros(R, len(mass), 3, dtype=PREC[prec], device=_dev()))
    md.sync(eng)
    return f, eng


def _boxes(box, R):
    return np.ascontiguousarray(np.broadcast_to(np.asarray(box, dtype=np.float64).reshape(-1, 3), (R, 3)))


def _apply(eng, pos, box, forces=None, vel=None, mass=None, kick=0.0, out=None, check=True):
    from torchmd_amd import _lib as L

    boxes = _boxes(box, pos.shape[0])
    ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p()  # noqa: E731
    rc = eng.lib.tmdhip_metad_apply(eng.ctx, ptr(pos), boxes.ctypes.data_as(C.POINTER(C.c_double)), ptr(forces), ptr(vel), ptr(mass),
                                    float(kick), ptr(out), _stream(pos.device))
    return L.check(rc, "tmdhip_metad_apply") if check else rc


def _state(pos, box, prec):
    """What `Metadynamics.deposit` asks of a system: positions and a [R,3,3] box on the device."""
    R = pos.shape[0]
    b = torch.zeros(R, 3, 3, dtype=PREC[prec])
    b[:, range(3), range(3)] = torch.as_tensor(_boxes(box, R).copy(), dtype=PREC[prec])
    return types.SimpleNamespace(pos=_tensor(pos, prec), box=b.to(_dev()))


def _rounded(a, prec):
    return np.asarray(a).astype(NP[prec]).astype(np.float64)


def _deposit_five(md, pos, box, prec):
    """Five depositions on the device and in the model, at the same (rounded) positions.  Returns the model's grid and rows,
    the device's log, the node sums of the LOGGED hills and the sum of the magnitudes of the model's terms."""
    grid = np.zeros_like(md.grid)
    rows = []
    for k in range(5):
        pk = _rounded(M.moved(pos, k), prec)
        md.deposit(_state(pk, box, prec))
        grid, rk = md.deposit_model(pk, box, grid)
        rows.append(rk)
    log = md.hills()
    fed, mag = np.zeros_like(grid), np.zeros_like(grid)
    for k in range(5):
        for r in range(md.nreplicas):
            g = 0 if md.walkers == "shared" else r
            fed[g] += md.gauss_terms(log[k, r, : md.ncv], log[k, r, md.ncv])
            mag[g] += np.abs(md.gauss_terms(rows[k][r, : md.ncv], rows[k][r, md.ncv]))
    return grid, np.stack(rows), log, fed, mag


def _kernel_against_model(prec, R, second, repeats, walkers="independent", seed=11):
    pos, box, mass, md = M.kernel_case(R=R, second=second, walkers=walkers, seed=seed)
    N = pos.shape[1]
    for r in range(R):
        ang = M.bond_angles(pos[r, 10:15] - box * np.rint((pos[r, 10:15] - pos[r, 12]) / box))
        assert (ang >= 60.0).all() and (ang <= 120.0).all()
    mass = _rounded(mass, prec)
    _, eng = _context(mass, md, prec, R)
    grid, rows, log, fed, mag = _deposit_five(md, pos, box, prec)
    # ---- the hills log and the grid
    ds = np.abs(log[..., : md.ncv] - rows[..., : md.ncv]).max()
    dw = np.abs(log[..., md.ncv] / rows[..., md.ncv] - 1.0).max()
    dev = md.grid
    node = (np.abs(dev - fed) / np.maximum(mag, 1e-300)).max() / EPS64
    chain = (np.abs(dev - grid) / np.maximum(mag, 1e-300)).max() / EPS64
    print(f"{prec} R={R} {second} {walkers}: hills |ds| = {ds:.2e}, |dw/w| = {dw:.2e}; nodes {chain:.2f} eps64 x sum|terms| from the "
          f"model's chain ({node:.2f} from the sums of the logged hills)")
    assert ds <= (1e-12 if prec == "f64" else 1e-6)
    assert dw <= 1e-10 and rows[..., md.ncv].min() < 0.9 * md.height  # (well-tempered: hills on top of a bias are lower)
    assert (np.abs(dev - grid) <= 8 * EPS64 * mag).all() and grid[..., 0].max() > 1.0
    # ---- the bias kernel on that grid
    rng = np.random.default_rng(99)
    p7 = _rounded(M.moved(pos, 7), prec)
    f_in = _rounded(rng.normal(0.0, 20.0, (R, N, 3)), prec)
    v_in = _rounded(rng.normal(0.0, 0.05, (R, N, 3)), prec)
    kick = 0.0123
    E, F, S = md.energy_forces(p7, box, grid)
    touched = np.zeros(N, dtype=bool)
    touched[md.row_atom] = True
    assert touched.sum() == (5 if second == "dihedral" else 6 if second == "distance" else 2)
    p, m = _tensor(p7, prec), _tensor(mass, prec)

    def once(mode):
        f, v = _tensor(f_in, prec), _tensor(v_in, prec)
        o = torch.full((R, 3), -1.0, dtype=torch.float64, device=_dev())
        if mode == "finish":
            _apply(eng, p, box, forces=f, vel=v, mass=m, kick=kick, out=o)
        elif mode == "impulse":
            _apply(eng, p, box, vel=v, mass=m, kick=kick)
        else:
            _apply(eng, p, box, forces=f, out=o)
        return f, v, o

    f, v, o = once("finish")
    got_f, got_v, got_o = f.cpu().double().numpy(), v.cpu().double().numpy(), o.cpu().numpy()
    fb = np.abs(F).max()
    assert fb > 0.5  # (something was added)
    if prec == "f32":
        want_f = _rounded(f_in + F, prec)
        want_v = _rounded(v_in + kick * F / mass[None, :, None], prec)
        df = (np.abs(got_f - want_f) / _ulp(want_f, prec)).max()
        dv = (np.abs(got_v - want_v) / _ulp(want_v, prec)).max()
        print(f"  forces {df:.2f} ulp, velocities {dv:.2f} ulp, max|F_b| = {fb:.3f}")
        assert df <= 1.0 and dv <= 1.0
    else:
        df = np.abs(got_f - (f_in + F)).max() / fb
        dv = np.abs(got_v - (v_in + kick * F / mass[None, :, None])).max() / (kick * fb / mass.min())
        print(f"  forces {df:.2e} max|F_b|, velocities {dv:.2e} of the largest kick, max|F_b| = {fb:.3f}")
        assert df <= 1e-9 and dv <= 1e-9
    assert np.abs(got_o[:, 0] - E).max() <= 1e-10 * np.abs(E).max()
    assert np.abs(got_o[:, 1:1 + md.ncv] - S).max() <= (1e-12 if prec == "f64" else 1e-6)
    # rows of atoms in no CV: never written
    assert torch.equal(_bits(f)[:, ~touched], _bits(_tensor(f_in, prec))[:, ~touched])
    assert torch.equal(_bits(v)[:, ~touched], _bits(_tensor(v_in, prec))[:, ~touched])
    # the impulse writes the velocities only, by the same rule; the evaluation writes no velocity
    fi, vi, _ = once("impulse")
    assert torch.equal(_bits(vi), _bits(v)) and torch.equal(_bits(fi), _bits(_tensor(f_in, prec)))
    fe, ve, oe = once("evaluate")
    assert torch.equal(_bits(fe), _bits(f)) and torch.equal(_bits(ve), _bits(_tensor(v_in, prec))) and torch.equal(oe, o)
    for _ in range(repeats):  # no atomics: the same bits every time
        f2, v2, o2 = once("finish")
        assert torch.equal(_bits(f2), _bits(f)) and torch.equal(_bits(v2), _bits(v)) and torch.equal(o2, o)
    return md, dev


@pytest.mark.parametrize("second", ["dihedral", "distance", None], ids=["phi-psi", "phi-distance", "distance"])
@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_kernel_against_model(prec, second):
    _kernel_against_model(prec, 3, second, repeats=20)


def test_kernel_past_a_chunk_of_sixteen_replicas():
    _kernel_against_model("f32", 17, "distance", repeats=1, seed=12)


@pytest.mark.parametrize("R", [4, 17])
def test_shared_walkers_fill_one_grid_in_replica_order(R):
    """One grid, every node adding the R hills of a deposition in replica order whatever the launch chunking (17 walkers are
    two launches of the height kernel): the model's sums, and the same bits in two runs."""
    md, g1 = _kernel_against_model("f64", R, "distance", repeats=1, walkers="shared")
    assert g1.shape[0] == 1 and md.hills().shape == (5, R, 3)
    md2, g2 = _kernel_against_model("f64", R, "distance", repeats=1, walkers="shared")
    assert np.array_equal(g1.view(np.int64), g2.view(np.int64)) and np.array_equal(md.hills().view(np.int64), md2.hills().view(np.int64))


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_device_heights_on_a_node_follow_the_closed_form(prec):
    md = Metadynamics(("distance", (0, 1)), sigma=0.25, height=1.5, frequency=1, temperature=300.0, bias_factor=5.0, grid_min=1.0,
                      grid_max=5.0, grid_bins=32)
    pos = np.array([[[0.0, 0.0, 0.0], [2.5, 0.0, 0.0], [7.0, 7.0, 7.0]]])  # s0 = node 12 exactly, in either dtype
    _context(np.ones(3), md, prec, 1)
    st = _state(pos, np.zeros(3), prec)
    for _ in range(3):
        md.deposit(st)
    log = md.hills()[:, 0]
    kdt = BOLTZMAN * 4.0 * 300.0
    want = [1.5, 1.5 * np.exp(-1.5 / kdt), 1.5 * np.exp(-(1.5 + 1.5 * np.exp(-1.5 / kdt)) / kdt)]
    print(f"{prec}: heights {log[:, 1]}, closed form {want}, relative deviation {np.abs(log[:, 1] / want - 1).max() / EPS64:.2f} eps64")
    assert (log[:, 0] == 2.5).all()
    assert (np.abs(log[:, 1] - want) <= 4 * EPS64 * np.asarray(want)).all()
    assert md.grid[0, 12, 0] == (log[0, 1] + log[1, 1]) + log[2, 1] and md.grid[0, 12, 1] == 0.0


def test_library_refusals_launch_nothing():
    from torchmd_amd import _lib as L

    pos, box, mass, md = M.kernel_case(R=3, second="distance")
    f, eng = _context(mass, md, "f64", 3)
    lib = eng.lib
    md.deposit(_state(pos, box, "f64"))
    grid0 = md.grid.copy()
    p = _tensor(pos, "f64")
    frc = _tensor(np.zeros_like(pos), "f64")
    before = _bits(frc).clone()

    def refused(change, expect):
        d = md.descriptor()
        change(d)
        assert lib.tmdhip_set_metadynamics(eng.ctx, C.byref(d)) < 0
        assert expect in L.last_error(), (expect, L.last_error())

    def set_(name, value, index=None):
        def change(d):
            if index is None:
                setattr(d, name, value)
            elif isinstance(index, tuple):
                getattr(d, name)[index[0]][index[1]] = value
            else:
                getattr(d, name)[index] = value
        return change

    refused(set_("struct_size", 8), "size mismatch")
    refused(set_("nreplicas", 2), "nreplicas")
    refused(set_("ncv", 3), "more than 2 CVs")
    refused(set_("ncv", 0), "at least one")
    refused(set_("kind", 5, 0), "unknown kind")
    refused(set_("atoms", 200, (0, 3)), "out of range")
    refused(set_("atoms", -1, (1, 0)), "out of range")
    refused(set_("atoms", 10, (0, 2)), "repeated")
    refused(set_("sigma", 0.0, 0), "sigma")
    refused(set_("sigma", float("nan"), 1), "sigma")
    refused(set_("bins", 0, 1), "bins")
    refused(set_("grid_min", 6.0, 1), "grid_min")
    refused(set_("bins", 30, 0), "sigma / 2")
    # the bias in place is the one that was accepted: grid and evaluation are unchanged
    assert np.array_equal(md.grid, grid0)
    o = torch.zeros(3, 3, dtype=torch.float64, device=_dev())
    _apply(eng, p, box, out=o)
    E, _, S = md.energy_forces(pos, box)
    assert np.allclose(o.cpu().numpy()[:, 0], E, rtol=1e-12) and E.min() > 0.5
    # a deposition: height, k_B dT, null pointers
    row = torch.zeros(3, 3, dtype=torch.float64, device=_dev())
    bx = _boxes(box, 3)
    dep = lambda h, kdt, plain, r=row: lib.tmdhip_metad_deposit(eng.ctx, C.c_void_p(p.data_ptr()), bx.ctypes.data_as(C.POINTER(C.c_double)),  # noqa: E731
                                                                h, kdt, plain, C.c_void_p(r.data_ptr()) if r is not None else C.c_void_p(),
                                                                _stream(p.device))
    for h, kdt, plain, expect in ((0.0, 1.0, 0, "height"), (float("inf"), 1.0, 0, "height"), (-1.0, 1.0, 1, "height"),
                                  (1.0, 0.0, 0, "k_B dT"), (1.0, float("nan"), 0, "k_B dT")):
        assert dep(h, kdt, plain) < 0 and expect in L.last_error(), (h, kdt, plain, L.last_error())
    assert dep(1.0, 1.0, 0, None) < 0 and "null" in L.last_error()
    torch.cuda.synchronize()
    assert np.array_equal(md.fetch(), grid0) and (row == 0).all()
    # the grid's host copies: the count must be the grid's
    buf = np.zeros(grid0.size + 1)
    assert lib.tmdhip_metad_get_grid(eng.ctx, buf.ctypes.data_as(C.POINTER(C.c_double)), buf.size) < 0 and "doubles" in L.last_error()
    assert lib.tmdhip_metad_set_grid(eng.ctx, buf.ctypes.data_as(C.POINTER(C.c_double)), buf.size) < 0 and "doubles" in L.last_error()
    # velocities without masses, and a CV atom without mass where masses are first seen
    v = _tensor(np.zeros_like(pos), "f64")
    assert _apply(eng, p, box, vel=v, check=False) < 0 and "masses" in L.last_error()
    m0 = mass.copy()
    m0[12] = 0.0
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
    # a CV atom that is a virtual site of the context
    vd = L.VsiteDesc()
    vd.struct_size = C.sizeof(L.VsiteDesc)
    vd.enable, vd.nsites = 1, 1
    site, parent, weight = np.array([12], np.int32), np.array([[100, 101, -1]], np.int32), np.array([[0.5, 0.5, 0.0]])
    vd.site_host, vd.parent_host, vd.weight_host = (a.ctypes.data_as(C.c_void_p) for a in (site, parent, weight))
    L.check(lib.tmdhip_set_vsites(eng.ctx, C.byref(vd)), "tmdhip_set_vsites")
    refused(lambda d: None, "virtual site")
    vd.enable = 0
    L.check(lib.tmdhip_set_vsites(eng.ctx, C.byref(vd)), "tmdhip_set_vsites")
    # a context with passive atoms (what a brick of the domain decomposition is): a context of its own
    from torchmd_amd.forces import Forces

    f2 = Forces(TR._BarePar(mass, PREC["f64"]), terms=[])
    eng2 = f2._engine(torch.zeros(3, 200, 3, dtype=torch.float64, device=_dev()))
    types_, charges = np.zeros(200, np.int32), np.zeros(200, np.float64)
    L.check(lib.tmdhip_update_atoms(eng2.ctx, 200, types_.ctypes.data_as(C.c_void_p), charges.ctypes.data_as(C.c_void_p), 150),
            "tmdhip_update_atoms")
    dsc = md.descriptor()
    assert lib.tmdhip_set_metadynamics(eng2.ctx, C.byref(dsc)) < 0 and "passive atoms" in L.last_error()
    o2 = torch.full((3, 3), -1.0, dtype=torch.float64, device=_dev())
    _apply(eng2, p, box, forces=frc, out=o2)  # (no bias in place: nothing added, the report zeroed)
    assert torch.equal(_bits(frc), before) and (o2 == 0).all()
    assert dep(1.0, 1.0, 0) == 0  # (the first context still deposits)
    assert lib.tmdhip_metad_deposit(eng2.ctx, C.c_void_p(p.data_ptr()), bx.ctypes.data_as(C.POINTER(C.c_double)), 1.0, 1.0, 0,
                                    C.c_void_p(row.data_ptr()), _stream(p.device)) < 0 and "no metadynamics" in L.last_error()
    # enable = 0 releases everything: nothing is added any more
    dsc = md.descriptor()
    dsc.enable = 0
    assert lib.tmdhip_set_metadynamics(eng.ctx, C.byref(dsc)) == 0
    _apply(eng, p, box, forces=frc, out=o)
    assert torch.equal(_bits(frc), before) and (o == 0).all()


# ----------------------------------------------------------------------------- trajectories
class _Model:
    """What `test_gpu_restraints._by_hand` asks of a restraint model, answered by the bias on a fixed grid."""

    def __init__(self, md, grid):
        self.md, self.grid = md, grid

    def energy_forces(self, pos, box):
        E, F, _ = self.md.energy_forces(pos, box, self.grid)
        return E, F


def _tip3p_bias(pos, box, R, scale=1.0):
    """One O-O distance CV across a face of the 5 184-atom box, frozen, on a grid pre-filled with three hills beside the
    starting distance (every replica with hills of its own)."""
    p = pos[:, :, 0] if pos.ndim == 3 else pos
    Lb = np.asarray(box).reshape(-1)[:3]
    ox = np.arange(0, len(p), 3)
    lo, hi = ox[np.argmin(p[ox, 0])], ox[np.argmax(p[ox, 0])]
    d = p[lo] - p[hi]
    assert np.any(np.rint(d / Lb) != 0)  # across a face
    r = np.sqrt(np.sum((d - Lb * np.rint(d / Lb)) ** 2))
    md = Metadynamics(("distance", (int(lo), int(hi))), sigma=0.3, height=1.0, frequency=1000, temperature=300.0, bias_factor=8.0,
                      grid_min=max(0.5, r - 4.0), grid_max=r + 4.0, grid_bins=64, nreplicas=R)
    grid = np.zeros_like(md.grid)
    for q in range(R):
        for off, w in ((0.3, 30.0), (-0.5, 12.0), (0.9, 8.0)):
            grid[q] += md.gauss_terms(np.array([r + off + 0.05 * q]), scale * w * (1.0 + 0.2 * q))
    md.set_grid(grid)
    md.frozen = True
    return md, grid


def _check_return(prec, out, f, s, md, grid, forces):
    """The potential energy the call returns is compute()'s total at the final positions, and the forces it leaves include F_b."""
    F2 = torch.zeros_like(s.pos)
    pots = f.compute(s.pos, s.box, F2, returnDetails=True)
    tot = [sum(p.values()) for p in pots]
    for r in range(s.pos.shape[0]):
        assert abs(out[1][r] - tot[r]) <= TR.ERTOL[prec] * TR.EFAC * max(1.0, abs(tot[r])), (r, out[1][r], tot[r])
    assert list(pots[0])[-1] == "metadynamics"
    assert np.abs(forces - F2.cpu().double().numpy()).max() <= TR.FTOL[prec] * 10
    hbox = np.diagonal(s.box.cpu().double().numpy(), axis1=1, axis2=2)
    E, Fb, S = md.energy_forces(s.pos.cpu().double().numpy(), hbox, grid)
    assert np.abs(Fb).max() > 10.0 and np.allclose(md.energy, E, rtol=1e-5) and np.allclose(md.cv, S, rtol=1e-5)
    assert np.allclose([p["metadynamics"] for p in pots], E, rtol=1e-5)
    assert np.abs((forces - Fb) - F2.cpu().double().numpy()).max() > 10.0  # (without F_b the forces left are far from the total)


@pytest.mark.parametrize("langevin", [False, True], ids=["nve", "langevin"])
def test_trajectory_fp64_list_path(langevin, monkeypatch):
    monkeypatch.setenv("TMDHIP_VSKIN", "0")
    mol, pos, box, par, vel0 = TR._tip3p("f64", 1)
    md, grid = _tip3p_bias(pos, box, 1)
    case = (mol, pos, box, par, vel0, 1, WATER_TERMS, dict(cutoff=9.0, rfa=True))
    tp, tv = TR._by_hand(case, "f64", _Model(md, grid), TR.CUTS, langevin)
    p, v, frc, out, f, s, integ = TR._under_test(case, "f64", None, TR.CUTS, langevin, metadynamics=md)
    bar_p, bar_v = 64 * EPS64 * 10 * np.abs(tp).max(), 64 * EPS64 * 10 * np.abs(tv).max()
    print(f"fp64 list path, {'Langevin' if langevin else 'NVE'}: |dpos| = {np.abs(p - tp).max():.2e} (bar {bar_p:.2e}), "
          f"|dvel| = {np.abs(v - tv).max():.2e} (bar {bar_v:.2e})")
    assert f.stats(s.pos)["algorithm"] == "celllist" and f.stats(s.pos)["steps_in_pair_launch"] == 0
    assert np.abs(p - tp).max() <= bar_p and np.abs(v - tv).max() <= bar_v
    assert md.nhills == 0 and np.array_equal(md.grid, grid)  # frozen: nothing was deposited
    _check_return("f64", out, f, s, md, grid, frc)


@pytest.mark.parametrize("langevin", [False, True], ids=["nve", "langevin"])
@pytest.mark.parametrize("R", [1, 3], ids=["lone", "batched"])
def test_trajectory_fp32_fused(R, langevin, monkeypatch):
    monkeypatch.setenv("TMDHIP_VSKIN", "0")
    mol, pos, box, par32, vel0 = TR._tip3p("f32", R)
    _, _, _, par64, _ = TR._tip3p("f64", R)
    md, grid = _tip3p_bias(pos, box, R)
    if R == 3:
        assert not np.array_equal(grid[0], grid[1]) and not np.array_equal(grid[1], grid[2])
    kw = dict(cutoff=9.0, rfa=True)
    case64 = (mol, pos, box, par64, vel0, R, WATER_TERMS, kw)
    case32 = (mol, pos, box, par32, vel0, R, WATER_TERMS, kw)
    tp, tv = TR._by_hand(case64, "f64", _Model(md, grid), TR.CUTS, langevin)
    hp, hv = TR._by_hand(case32, "f32", _Model(md, grid), TR.CUTS, langevin)
    p, v, frc, out, f, s, integ = TR._under_test(case32, "f32", None, TR.CUTS, langevin, metadynamics=md)
    noise_p, noise_v = np.abs(hp - tp).max(), np.abs(hv - tv).max()
    dp, dv = np.abs(p - tp).max(), np.abs(v - tv).max()
    print(f"fp32 fused R={R}, {'Langevin' if langevin else 'NVE'}: |dpos| = {dp:.2e} (by hand {noise_p:.2e}), "
          f"|dvel| = {dv:.2e} (by hand {noise_v:.2e})")
    st = [f.stats(s.pos, r) for r in range(R)]
    assert all(x["steps_in_pair_launch"] >= 5 for x in st), st  # the interior steps of 2 + 7 were made by pair launches
    if R == 3:
        assert st[0]["batched_launches"] >= 5
    assert dp <= 2 * noise_p and dv <= 2 * noise_v
    # the control: the same by-hand loop with the model's grid halved misses that bar by more than 10x
    cp, cv = TR._by_hand(case32, "f32", _Model(md, 0.5 * grid), TR.CUTS, langevin)
    assert np.abs(cp - tp).max() > 10 * 2 * noise_p and np.abs(cv - tv).max() > 10 * 2 * noise_v
    _check_return("f32", out, f, s, md, grid, frc)


# ----------------------------------------------------------------------------- alanine dipeptide, phi / psi
# The cell-list path, whose trajectories are the same bits in two runs (all-pairs contexts add forces with atomics, DESIGN
# §11): three cells of cutoff + skin per edge of the 19.6 Å box.
ALA2_KW = dict(cutoff=5.0, switch_dist=4.0, rfa=True, algorithm="celllist", skin=1.0)


def _ala2(prec, R=1, frozen=False, **mdkw):
    from torchmd_amd.forces import Forces
    from torchmd_amd.integrator import Integrator
    from torchmd_amd.systems import System

    g = load("ala2")
    par = GoldenParameters(g, PREC[prec])
    kw = dict(sigma=0.35, height=0.6, frequency=50, temperature=300.0, bias_factor=6.0, grid_bins=[40, 36], nreplicas=R)
    kw.update(mdkw)
    md = Metadynamics([("dihedral", PHI), ("dihedral", PSI)], **kw)
    md.frozen = frozen
    pos = np.asarray(g["pos"], dtype=np.float64).reshape(-1, 3)
    s = System(len(pos), R, PREC[prec], _dev())
    s.set_positions(np.repeat(pos[:, :, None], R, axis=2))
    s.set_box(np.asarray(g["box"], dtype=np.float64).reshape(-1)[:3])
    rng = np.random.default_rng(8)
    s.set_velocities(torch.as_tensor(0.01 * rng.standard_normal((R, len(pos), 3))).to(PREC[prec]))
    f = Forces(par, terms=ALL_TERMS, metadynamics=md, **ALA2_KW)
    f.compute(s.pos, s.box, s.forces)
    assert f.stats(s.pos)["algorithm"] == "celllist"
    torch.manual_seed(3)
    return g, md, s, f, Integrator(s, f, 1.0, _dev())


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_ala2_hills_follow_the_trajectory_whatever_the_cuts(prec, monkeypatch):
    monkeypatch.setenv("TMDHIP_VSKIN", "0")
    g, md, s, f, integ = _ala2(prec)
    box = np.diagonal(s.box.cpu().double().numpy(), axis1=1, axis2=2)  # (the box the device holds)
    grid = np.zeros_like(md.grid)
    for k in range(4):
        integ.step(50)
        assert md.nhills == k + 1
        # the row equals the numpy CVs of the positions of that moment, its height the model's on the model's grid
        grid, rows = md.deposit_model(s.pos.cpu().double().numpy(), box, grid)
        got = md.hills()[k]
        ds, dw = np.abs(got[:, :2] - rows[:, :2]).max(), np.abs(got[:, 2] / rows[:, 2] - 1.0).max()
        print(f"{prec} hill {k}: s = {got[0, :2]}, w = {got[0, 2]:.6f}; |ds| = {ds:.2e}, |dw/w| = {dw:.2e}")
        assert ds <= (1e-6 if prec == "f32" else 1e-12) and dw <= (1e-5 if prec == "f32" else 1e-10)
    assert np.abs(md.grid - grid).max() <= (1e-5 if prec == "f32" else 1e-11) * np.abs(grid).max()
    assert np.allclose(md.cv[0], md.hills()[3, 0, :2], atol=1e-6)  # (the CVs of the last step are those of the last hill)
    log, last = md.hills(), s.pos.clone()
    # one call of 200 steps: the same log and the same trajectory, bit for bit
    g2, md2, s2, f2, integ2 = _ala2(prec)
    integ2.step(200)
    assert md2.nhills == 4 and np.array_equal(md2.hills().view(np.int64), log.view(np.int64))
    assert torch.equal(_bits(s2.pos), _bits(last)) and np.array_equal(md2.grid.view(np.int64), md.grid.view(np.int64))
    assert md2.free_energy().shape == (1, 40, 36) and md2.free_energy().min() < -0.5


def test_ala2_save_load_continues_bit_for_bit(tmp_path, monkeypatch):
    monkeypatch.setenv("TMDHIP_VSKIN", "0")
    g, md, s, f, integ = _ala2("f32")
    integ.step(100)
    md.save(str(tmp_path / "bias.npz"))
    pos, vel, frc = s.pos.clone(), s.vel.clone(), s.forces.clone()
    f.invalidate_lists(s.pos)  # (the Verlet list is no part of a restart: the twin below builds its own at this step too)
    integ.step(100)
    want_log, want_grid, want_pos = md.hills(), md.grid.copy(), s.pos.clone()
    # fresh objects, the state of step 100, the file: the second hundred steps again
    g2, md2, s2, f2, integ2 = _ala2("f32")
    md2.load(str(tmp_path / "bias.npz"))
    assert md2.nhills == 2
    s2.pos.copy_(pos), s2.vel.copy_(vel), s2.forces.copy_(frc)
    f2.invalidate_lists(s2.pos)
    integ2._nstep = 100
    integ2.step(100)
    assert np.array_equal(md2.hills().view(np.int64), want_log.view(np.int64))
    assert np.array_equal(md2.grid.view(np.int64), want_grid.view(np.int64)) and torch.equal(_bits(s2.pos), _bits(want_pos))


def test_ala2_frozen_bias_conserves_energy_like_the_plain_run():
    """NVE, fp64, 200 steps: under a static grid (four hills of an earlier run, `frozen`) the drift of E_kin + E_pot, the bias
    included, is at most twice that of the same run without a bias: the bias is C1 and its force the exact derivative."""
    from torchmd_amd.forces import Forces
    from torchmd_amd.integrator import Integrator

    g, md, s, f, integ = _ala2("f64", height=2.0)
    start = s.pos.clone(), s.vel.clone()
    integ.step(200)
    assert md.nhills == 4
    md.frozen = True
    drift = {}
    for name in ("plain", "biased"):
        s.pos.copy_(start[0]), s.vel.copy_(start[1])
        ff = f if name == "biased" else Forces(f.par, terms=ALL_TERMS, **ALA2_KW)
        ff.compute(s.pos, s.box, s.forces)
        it = Integrator(s, ff, 1.0, _dev())
        e = []
        for _ in range(10):
            ek, ep, _ = it.step(20)
            e.append(float(ek[0]) + ep[0])
        drift[name] = np.abs(np.asarray(e) - e[0]).max()
    print(f"NVE drift over 200 steps: plain {drift['plain']:.3e}, biased (V = {md.energy[0]:.3f}) {drift['biased']:.3e} kcal/mol")
    assert md.nhills == 4 and md.energy[0] > 0.5
    assert drift["biased"] <= 2 * drift["plain"]


def test_independent_and_shared_walkers_in_a_run(monkeypatch):
    monkeypatch.setenv("TMDHIP_VSKIN", "0")
    g, md, s, f, integ = _ala2("f32", R=4, walkers="shared", frequency=10)
    s.vel.mul_(torch.arange(1, 5, device=s.vel.device, dtype=s.vel.dtype).view(4, 1, 1))  # (four walkers that part)
    integ.step(30)
    assert md.grid.shape[0] == 1 and md.hills().shape == (3, 4, 3)
    fed = np.zeros_like(md.grid)
    for row in md.hills():
        for r in range(4):
            fed[0] += md.gauss_terms(row[r, :2], row[r, 2])
    assert np.abs(md.grid - fed).max() <= 1e-12 * np.abs(fed).max()
    g2, md2, s2, f2, integ2 = _ala2("f32", R=4, walkers="shared", frequency=10)
    s2.vel.mul_(torch.arange(1, 5, device=s2.vel.device, dtype=s2.vel.dtype).view(4, 1, 1))
    integ2.step(30)
    assert np.array_equal(md2.grid.view(np.int64), md.grid.view(np.int64)) and torch.equal(_bits(s2.pos), _bits(s.pos))


# ----------------------------------------------------------------------------- what is refused, what composes
def test_integrator_and_compute_refusals():
    from torchmd_amd.barostat import MonteCarloBarostat
    from torchmd_amd.exchange import ReplicaExchange
    from torchmd_amd.forces import Forces
    from torchmd_amd.integrator import Integrator
    from torchmd_amd.thermostat import VelocityRescale

    g, md, s, f, integ = _ala2("f64", R=2)
    with pytest.raises(ValueError, match="barostat"):
        Integrator(s, f, 1.0, _dev(), gamma=1.0, T=300.0, barostat=MonteCarloBarostat(1.0, 300.0, frequency=5, seed=1))
    with pytest.raises(ValueError, match="exchange"):
        Integrator(s, f, 1.0, _dev(), thermostat=VelocityRescale([300.0, 310.0], tau=0.1, frequency=10, seed=2),
                   exchange=ReplicaExchange(frequency=10, seed=2))
    with pytest.raises(ValueError, match="batch"):
        Integrator(s, f, 1.0, _dev(), batch=torch.zeros(688, dtype=torch.long))
    with pytest.raises(ValueError, match="vmap"):
        torch.vmap(lambda x: f.compute(x, s.box, None, toNumpy=False))(s.pos[None])
    one = Metadynamics([("dihedral", PHI), ("dihedral", PSI)], sigma=0.35, height=0.6, frequency=50, temperature=300.0, grid_bins=36)
    f1 = Forces(f.par, terms=ALL_TERMS, metadynamics=one, **ALA2_KW)
    with pytest.raises(ValueError, match="replicas"):
        Integrator(s, f1, 1.0, _dev())
    with pytest.raises(ValueError, match="replicas"):
        f1.compute(s.pos, s.box, s.forces)
    with pytest.raises(ValueError, match="Metadynamics"):
        Forces(f.par, terms=ALL_TERMS, cutoff=9.0, metadynamics="phi")
    # a thermostat's schedule and the bias's compose: the hill of step 20 falls behind the thermostat's application
    th = VelocityRescale([300.0, 310.0], tau=0.1, frequency=10, seed=2)
    md.frequency = 20
    it = Integrator(s, f, 1.0, _dev(), thermostat=th)
    ek, pot, T = it.step(40)
    assert md.nhills == 2 and th.applications == 4 and np.isfinite(pot).all()
    tot = f.compute(s.pos, s.box, torch.zeros_like(s.pos), returnDetails=True)
    assert all(list(p)[-1] == "metadynamics" for p in tot)


def test_rigid_water_with_a_biased_oxygen_pair():
    """constraints="water" at 2 fs with a distance CV between two oxygens: the bond lengths are kept as well as without a bias
    (the bar of tests/test_gpu_restraints.py: four times the plain run's worst bond error plus 8 eps64)."""
    from torchmd_amd.builders import tip3p_box, water_forcefield
    from torchmd_amd.forces import Forces
    from torchmd_amd.integrator import Integrator, maxwell_boltzmann
    from torchmd_amd.parameters import Parameters

    mol, pos, box = tip3p_box(6, seed=3)
    pos = np.asarray(pos, dtype=np.float64)
    par = Parameters(water_forcefield(mol), mol, WATER_TERMS, precision=torch.float64)
    p0 = pos[:, :, 0] if pos.ndim == 3 else pos
    Lb = np.asarray(box, dtype=np.float64).reshape(-1)[:3]
    ox = np.arange(0, len(p0), 3)
    d = p0[ox] - p0[ox[40]]
    r = np.sqrt(((d - Lb * np.rint(d / Lb)) ** 2).sum(axis=1))
    other = int(ox[np.argsort(r)[1]])
    dev_bond = {}
    for name in ("plain", "biased"):
        md = None
        if name == "biased":
            md = Metadynamics(("distance", (int(ox[40]), other)), sigma=0.3, height=1.5, frequency=20, temperature=300.0, bias_factor=8.0,
                              grid_min=1.5, grid_max=9.0, grid_bins=60)
        torch.manual_seed(9)
        vel0 = maxwell_boltzmann(par.masses, 300.0, 1)
        s = TR._system(mol, pos, box, vel0, "f64", 1)
        f = Forces(par, terms=WATER_TERMS, cutoff=7.0, rfa=True, **({} if md is None else {"metadynamics": md}))
        f.compute(s.pos, s.box, s.forces)
        integ = Integrator(s, f, 2.0, _dev(), gamma=1.0, T=300.0, constraints="water")
        integ.step(200)
        p = s.pos[0].cpu().double().numpy()
        cs = integ.constraints
        w = np.asarray(cs.waters)
        dd = np.stack([np.linalg.norm(p[w[:, 0]] - p[w[:, 1]], axis=1), np.linalg.norm(p[w[:, 0]] - p[w[:, 2]], axis=1),
                       np.linalg.norm(p[w[:, 1]] - p[w[:, 2]], axis=1)], axis=1)
        d0 = np.asarray(cs.water_dist)
        dev_bond[name] = np.abs(dd / np.stack([d0[:, 0], d0[:, 0], d0[:, 1]], axis=1) - 1.0).max()
        if md is not None:
            assert md.nhills == 10 and md.grid[0, :, 0].max() > 1.0
    print(f"bond lengths: plain {dev_bond['plain']:.2e}, biased {dev_bond['biased']:.2e}")
    assert dev_bond["biased"] <= 4 * dev_bond["plain"] + 8 * EPS64


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
out["module_after_off"] = "torchmd_amd.metadynamics" in sys.modules
go("log_md", metadynamics={"cvs": [["distance", [0, 30]], ["distance", [3, 60]]], "sigma": 0.4, "height": 1.0, "frequency": 10,
                           "temperature": 300, "bias_factor": 6, "grid_min": 0.5, "grid_max": 12.5, "grid_bins": 60})
h = np.load(os.path.join(TMP, "log_md", "output_hills.npy"))
z = np.load(os.path.join(TMP, "log_md", "output_bias_grid.npz"))
out["hills"] = list(h.shape); out["grid"] = list(z["grid"].shape); out["vmax"] = float(z["grid"][..., 0].max())
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
    assert out["log"]["files"] == files
    assert out["log_md"]["files"] == sorted(files + ["output_hills.npy", "output_bias_grid.npz"])
    assert all(rows[0] == "iter,ns,epot,ekin,etot,T,t" and len(rows) == 3 for rows in out["log"]["rows"])
    for rows in out["log_md"]["rows"]:
        assert rows[0] == "iter,ns,epot,ekin,etot,T,bias,cv0,cv1,t" and len(rows) == 3
        vals = np.array([[float(x) for x in r.split(",")] for r in rows[1:]])
        assert np.isfinite(vals).all() and (vals[:, 6] > 0.0).all() and (vals[:, 7:9] > 0.5).all()
    assert out["hills"] == [4, 2, 3] and out["grid"] == [2, 61, 61, 4] and out["vmax"] > 0.5
