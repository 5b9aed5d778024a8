"""The constrained MD step at its edges (run with `-m gpu` on an MI355X): every unit kind of md_step_cons_kernel — free atom,
rigid three-atom unit of two geometries, clusters of 1 .. 4 hydrogens (cons_cluster<2..5>) — in one context with scrambled
numbering (tests/_constraint_systems.py), all-pairs and cell-list (the CHECK form of the kernel), NVE and Langevin, fp64 and
fp32, against the fp64 host step of tests/_constraints.py; fp32 "hbonds" invariants; tmdhip_md_restore on a cell-list
context; and the failure report of a SHAKE that does not converge / a water too distorted for SETTLE.

fp32 bars.  The kernel reads floats, computes in double and rounds once on store, so the host is fed exactly what the device
read (float positions, velocities, forces, masses, vcoeff, dt and gamma, converted to double; for the second half, which is
a kernel of its own after the force evaluation, the stored float positions and half-step velocities and the device's float
forces after the step) and the result must round to the same float: every position component within one float
ulp of the host's value.  Velocities: one float ulp of the component, plus three terms whose sum is capped at 1e-6 max|v|:
the fp64 bar of the existing one-step test (1e-9 max|v|: host and device arithmetic differ in order, the device SHAKE stops at
1e-10 where the host's goes on to 1e-14, and a component can be much smaller than max|v|); with the thermostat, the
documented 2e-5 difference of the host noise helper's variates times the largest vcoeff; and, for the atoms of a constrained
unit, the half-step velocity between the two kernels of a step, which cannot be read back: the device stores it as floats,
the host rounds its own, and the two values (2.5e-9 apart at the SHAKE tolerance, a third of a float ulp of a typical
component) often round to neighbouring floats.  The velocity constraint is an orthogonal projection in the mass-weighted
norm, so a difference of one ulp in every stored component of a unit U reaches atom i with at most
sqrt(sum_{j in U} 3 m_j ulp(max_k |v_jk|)^2 / m_i) (`_stored_velocity_slack`) — a few ulps; a free atom gets none."""

import copy
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import _constraint_systems as S
import _constraints as H
import _philox as P
from oracle import torchmd_oracle as orc
from test_gpu_constraints import _check_constraints, _golden_system

pytestmark = pytest.mark.gpu

DT = {"f64": torch.float64, "f32": torch.float32}
FAILURE = "a SHAKE cluster did not converge within max_iter sweeps, or a water was too distorted for"


def _dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def _built(size):
    return S.build(size)


def _synthetic(size, prec, langevin=False, seed=0, algorithm="auto"):
    """The synthetic system on the device, on its constraints with Maxwell-Boltzmann velocities projected onto them (host,
    fp64), forces evaluated, and its Integrator (2 fs, "hbonds") past its start-up projection."""
    from torchmd_amd.constraints import find_constraints
    from torchmd_amd.forces import Forces
    from torchmd_amd.integrator import Integrator
    from torchmd_amd.systems import System

    sysm = _built(size)
    dt = DT[prec]
    par = sysm.par(dt)
    m = par.masses.reshape(-1).double().numpy()  # (fp32: the float masses the device reads)
    cs = find_constraints(m, par.bond_params, par.angle_params, "hbonds")
    us = H.units(cs)
    x = H.shake(sysm.pos.copy(), sysm.pos.copy(), m, us)
    v = np.random.default_rng(seed).normal(size=x.shape) * np.sqrt(300.0 * 0.001987191 / m)[:, None]
    v = H.project(x, v, m, us)
    s = System(sysm.natoms, 1, dt, _dev())
    s.set_positions(x[:, :, None])
    s.set_box(sysm.box)
    s.set_velocities(torch.as_tensor(v[None]))
    f = Forces(par, terms=S.TERMS, algorithm=algorithm, **S.FORCE_KW)
    f.compute(s.pos, s.box, s.forces)
    integ = Integrator(s, f, 2.0, _dev(), gamma=5.0 if langevin else None, T=300.0 if langevin else None, constraints="hbonds")
    # the start-up projection of the first step now, not inside it: in fp32 it moves the rounded positions back onto the
    # constraints and evaluates the forces again, and the tests need the state the first kernel reads
    with torch.cuda.device(_dev()):
        integ._project_start()
    return sysm, par, cs, us, m, s, f, integ


def _unit_kinds(cs, m, n):
    """Per atom, the kernel path that steps it: "free atom", "water O" / "water S" (settle_water at two geometries),
    "cluster NA=k" (cons_cluster<k>)."""
    kind = np.full(n, "free atom", dtype=object)
    for w in cs.waters:
        kind[w] = "water O" if m[w[0]] < 20 else "water S"
    for c in cs.clusters():
        kind[c] = f"cluster NA={len(c)}"
    return kind


def _worst_by_kind(kind, ratio):
    """{kind: worst error / bar} of a per-atom ratio array."""
    return {k: float(ratio[kind == k].max()) for k in sorted(set(kind))}


def _noise(integ, step, n, dtype):
    """The device's own variates of global step `step` in the context's precision (tmdhip_normal_fill), held to the host
    Philox of tests/_philox.py at its documented 2e-5."""
    from torchmd_amd import _lib as L

    out = torch.empty(3 * n, dtype=dtype, device=_dev())
    L.check(L.load().tmdhip_normal_fill(L.dtype_code(dtype), 3 * n, out.data_ptr(), C.c_uint64(integ._seed), C.c_uint64(step),
                                        C.c_void_p(torch.cuda.current_stream().cuda_stream)), "tmdhip_normal_fill")
    g = out.cpu().double().numpy().reshape(n, 3)
    h = np.stack(P.normal3(integ._seed, step, np.arange(n, dtype=np.uint64)), axis=1)
    assert np.abs(g - h).max() < 2e-5 * (1 + np.abs(h).max())
    return g


def _state(s):
    return tuple(t[0].cpu().double().numpy() for t in (s.pos, s.vel, s.forces))


def _oracle_forces(par, x, box):
    pairs = orc.candidate_pairs(x, np.asarray(box, dtype=np.float64), S.FORCE_KW["cutoff"] + 2.0, orc.exclusion_pairs(par))
    bt = torch.diag(torch.as_tensor(np.asarray(box, dtype=np.float64)))[None]
    _, F, _ = orc.compute(par, torch.as_tensor(x)[None], bt, S.TERMS, pairs=pairs, **S.FORCE_KW)
    return F[0].double().numpy()


def _thermostat(integ, prec, step, n):
    if not integ.T:
        return {}
    npdt = np.float32 if prec == "f32" else np.float64
    return dict(gamma=float(npdt(integ.gamma)), vcoeff=integ.vcoeff.reshape(-1).cpu().double().numpy(),
                noise=_noise(integ, step, n, DT[prec]))


def _stored_velocity_slack(vh, m, us):
    """[N, 1]: what one float ulp of difference in every stored half-step velocity component of a unit can do to each of its
    atoms after the velocity constraint (module docstring)."""
    e = np.zeros(len(m))
    for at, pairs in us:
        u = np.spacing(np.abs(vh[at]).max(axis=1).astype(np.float32)).astype(np.float64)
        e[at] = np.sqrt(3.0 * np.sum(m[at] * u * u) / m[at])
    return e[:, None]


def _compare(what, prec, kind, xg, vg, x1, v1, integ, slack=0.0):
    """Assert the device's (xg, vg) against the host's (x1, v1); the message names the worst unit kind."""
    vmax = np.abs(v1).max()
    if prec == "f64":
        xbar, vbar = np.full_like(x1, 1e-9), np.full_like(v1, 1e-9 * vmax)
    else:
        xbar = np.spacing(np.abs(x1).astype(np.float32)).astype(np.float64)
        extra = 1e-9 * vmax + slack
        if integ.T:
            extra += 2e-5 * float(integ.vcoeff.max())
        vbar = np.spacing(np.abs(v1).astype(np.float32)).astype(np.float64) + np.minimum(extra, 1e-6 * vmax)
    rx = (np.abs(xg - x1) / xbar).max(axis=1)
    rv = (np.abs(vg - v1) / vbar).max(axis=1)
    wx, wv = _worst_by_kind(kind, rx), _worst_by_kind(kind, rv)
    print(f"{what}: max|dx| = {np.abs(xg - x1).max():.2e} A, max|dv|/max|v| = {np.abs(vg - v1).max() / vmax:.2e}; error / bar by unit kind: "
          f"positions {wx}, velocities {wv}")
    within = (lambda r: r <= 1.0) if prec == "f32" else (lambda r: r < 1.0)
    assert within(rx.max()), (what, "positions, error / bar by unit kind", wx)
    assert within(rv.max()), (what, "velocities, error / bar by unit kind", wv)


# ----------------------------------------------------------------------------- 1. one step, five steps against the host
@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("langevin", [False, True])
@pytest.mark.parametrize("size,algorithm", [("small", "allpairs"), ("large", "celllist")])
def test_step_equals_the_host(size, algorithm, langevin, prec):
    sysm, par, cs, us, m, s, f, integ = _synthetic(size, prec, langevin)
    n = len(m)
    kind = _unit_kinds(cs, m, n)
    assert set(kind) == {"free atom", "water O", "water S"} | {f"cluster NA={k}" for k in (2, 3, 4, 5)}
    dt = float(np.float32(integ.dt)) if prec == "f32" else integ.dt  # (the kernel's arguments are of the context's precision)
    what = f"{size} {algorithm} langevin={langevin} {prec}"

    # one step per call, five times: each against the host step from the state the device started from
    for k in range(5 if prec == "f32" else 1):
        x0, v0, f0 = _state(s)
        integ.step(1)
        if k == 0:
            assert f.stats(s.pos)["algorithm"] == algorithm
        xg, vg, fg = _state(s)
        x1, vh = H.first_half(x0, v0, f0, m, dt, us)
        xs, slack = x1, 0.0
        if prec == "f32":
            # the kernel of the second half reads what the first stored: float positions (the device's own, held to the host's
            # a few lines down) and the float half-step velocity
            xs, vh = xg, vh.astype(np.float32).astype(np.float64)
            slack = _stored_velocity_slack(vh, m, us)
        v1 = H.second_half(xs, vh, fg, m, dt, us, **_thermostat(integ, prec, k, n))
        _compare(f"{what}, step {k}", prec, kind, xg, vg, x1, v1, integ, slack)
    if prec == "f32":
        # (five steps in one call would need the forces between the steps: the oracle's fp64 forces differ from the device's
        # float ones by far more than the bar, so the fused interior kernel is held to the host in fp64 only)
        return

    # five steps in one call (the interior kernel: second kick and first half step fused), oracle forces in between
    sysm, par, cs, us, m, s, f, integ = _synthetic(size, prec, langevin)
    x, v, fx = _state(s)
    integ.step(5)
    for k in range(5):
        x, vh = H.first_half(x, v, fx, m, dt, us)
        fx = _oracle_forces(par, x, sysm.box)
        v = H.second_half(x, vh, fx, m, dt, us, **_thermostat(integ, prec, k, n))
    xg, vg, _ = _state(s)
    _compare(f"{what}, 5 steps in one call", prec, kind, xg, vg, x, v, integ)


# ----------------------------------------------------------------------------- 2. fp32 "hbonds" invariants
@pytest.mark.parametrize("name", ["ala2", "synthetic-large"])
def test_hbonds_invariants_fp32(name):
    if name == "ala2":
        _, _, _, _, cs, m, s, f, integ = _golden_system("ala2", "hbonds", "f32", langevin=True)
    else:
        _, _, cs, _, m, s, f, integ = _synthetic("large", "f32", langevin=True)
    worst = (0.0, 0.0)
    for call in range(10):
        ek, pot, T = integ.step(20)
        w = _check_constraints(s, cs, "f32", f"{name}, call {call}")
        worst = (max(worst[0], w[0]), max(worst[1], w[1]))
        assert np.isfinite(ek).all() and np.isfinite(pot).all(), (name, call)
    if name != "ala2":
        assert f.stats(s.pos)["algorithm"] == "celllist"
    print(f"{name} hbonds fp32, 200 steps at 2 fs: worst bond error {worst[0]:.2e}, velocity along bonds {worst[1]:.2e}, T = {T[0]:.1f} K")


# ----------------------------------------------------------------------------- 3. rewind on a cell-list context
@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_restore_returns_the_entry_state(prec):
    from torchmd_amd import _lib as L

    _, _, cs, _, m, s, f, integ = _synthetic("large", prec, langevin=True)
    integ.step(10)  # (past the start-up projection; the list exists: the next call's first kernel takes the snapshot itself)
    assert f.stats(s.pos)["algorithm"] == "celllist"
    entry = [t.clone() for t in (s.pos, s.vel, s.forces)]
    integ.step(20)
    assert not torch.equal(entry[0], s.pos)
    eng = f._engine(s.pos)
    d = eng._md_cache[3]
    L.check(eng.lib.tmdhip_md_restore(eng.ctx, C.byref(d), C.c_void_p(torch.cuda.current_stream().cuda_stream)), "tmdhip_md_restore")
    torch.cuda.synchronize()
    for what, a, b in zip(("pos", "vel", "forces"), entry, (s.pos, s.vel, s.forces)):
        assert torch.equal(a, b), what  # bit for bit, every unit kind


# ----------------------------------------------------------------------------- 4. the failure report
def _healthy_step(prec):
    _, _, cs, _, _, s, f, integ = _synthetic("small", prec, langevin=False, seed=1, algorithm="allpairs")
    ek, pot, _ = integ.step(1)
    assert np.isfinite(ek).all() and np.isfinite(pot).all()
    _check_constraints(s, cs, prec, "a fresh context after a failure elsewhere")


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_shake_failure_is_reported(prec):
    """max_iter = 1: one sweep of a displaced cluster is never convergence (an error return of the library, no fault)."""
    _, _, cs, _, _, s, f, integ = _synthetic("small", prec, algorithm="allpairs")
    entry = [t.clone() for t in (s.pos, s.vel, s.forces)]
    assert integ.constraints.nclusters > 0
    integ.constraints.max_iter = 1  # (before the first upload: Forces._md_run hands the set to the context once)
    with pytest.raises(RuntimeError, match=FAILURE):
        integ.step(1)
    assert f.stats(s.pos)["algorithm"] == "allpairs"
    assert torch.isfinite(s.pos).all()  # (a sweep short of convergence, not garbage)
    _healthy_step(prec)
    # the same context, its state reset and a set with the production max_iter uploaded: the report was made once
    for t, e in zip((s.pos, s.vel, s.forces), entry):
        t.copy_(e)
    integ.constraints = copy.copy(integ.constraints)
    integ.constraints.max_iter = 200
    ek, pot, _ = integ.step(1)
    assert np.isfinite(ek).all() and np.isfinite(pot).all()
    _check_constraints(s, cs, prec, "the same context after the failure")


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_settle_failure_is_reported(prec):
    """A water whose hydrogens are given opposite velocities of 1 A per step across the molecular plane: the two would end
    2 A apart along the plane's normal, more than d_HH = 1.51 A, and settle_water's sin(psi) = 2.0 / 1.51 has no angle.
    (Opposite velocities in the plane never fail the closed form, it projects any in-plane stretch away; at 0.5 A per step
    across the plane sin(psi) = 0.66 and the water is settled.)"""
    _, _, cs, _, m, s, f, integ = _synthetic("small", prec, algorithm="allpairs")
    integ.step(1)
    assert f.stats(s.pos)["algorithm"] == "allpairs"
    entry = [t.clone() for t in (s.pos, s.vel, s.forces)]
    o, h1, h2 = (int(a) for a in next(w for w in cs.waters if m[w[0]] < 20))  # a TIP3P water
    p = s.pos[0].double()
    u = torch.linalg.cross(p[h1] - p[o], p[h2] - p[o])
    u = (u / u.norm() * (1.0 / integ.dt)).to(s.vel.dtype)
    s.vel[0, h1] += u
    s.vel[0, h2] -= u
    with pytest.raises(RuntimeError, match=FAILURE):
        integ.step(1)
    _healthy_step(prec)
    # the same context and the same uploaded set, positions reset: no stale flag raises again
    for t, e in zip((s.pos, s.vel, s.forces), entry):
        t.copy_(e)
    ek, pot, _ = integ.step(1)
    assert np.isfinite(ek).all() and np.isfinite(pot).all()
    _check_constraints(s, cs, prec, "the same context after the failure")
