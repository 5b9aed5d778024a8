"""The FIRE minimiser on the GPU (run with `-m gpu` on an MI355X): `tmdhip_fire_step` against the numpy model of
tests/_fire.py on harmonic wells (no `Forces` involved), then `minimize_fire` end to end: alanine dipeptide and the 291-atom
water system against the oracle, replicas on the cell-list path, PME, four-site water, and what it is for — a cooler start
of a rigid-water run."""

import ctypes as C

import numpy as np
import pytest
import torch

import _fire as M
import _reduce as RM
from _golden import GoldenParameters, PREC, load

pytestmark = pytest.mark.gpu

# the suite's bars for forces and energies against the oracle (tests/test_gpu_parity.py)
FTOL = {"f64": 1e-8, "f32": 3e-4}
ERTOL = {"f64": 1e-10, "f32": 2e-5}
EFAC = 3
ALL_TERMS = ["bonds", "angles", "dihedrals", "impropers", "1-4", "electrostatics", "lj"]
WATER_TERMS = ["lj", "electrostatics", "bonds", "angles"]


def _dev():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    return torch.device("cuda:0")


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


# ----------------------------------------------------------------------------- 1. the kernels against the model
R_, N_, NITER, K_SPRING = 3, 1000, 300, 10.0
# Positions against the model, relative to the largest coordinate.  The kernel and the model differ in the order in which the
# three dot products are summed and in nothing else (the model sums them exactly, so its figures do not depend on the host).
# POS_OBSERVED: the worst deviation over the 300 iterations on an MI355X; fp32 against the model rounded to float32 at each
# store, where a different sum has to flip a rounding to show at all — it never did.  Asserted: ten times the observed value,
# and in fp64 never looser than 1e-9.
POS_OBSERVED = {"f64": 2.983e-16, "f32": 0.0}
POS_BAR = {k: 10.0 * v for k, v in POS_OBSERVED.items()}
assert POS_BAR["f64"] <= 1e-9


def _harmonic_setup(prec):
    """R = 3 wells of N = 1000 atoms: replica 0 starts converged, replica 1 close (it converges mid-run), replica 2 far."""
    rng = np.random.default_rng(2006)
    np_dt = np.float64 if prec == "f64" else np.float32
    x0 = rng.uniform(-30.0, 30.0, size=(R_, N_, 3))
    amp = np.array([1e-7, 0.05, 3.0])[:, None, None]
    x = x0 + amp * rng.standard_normal((R_, N_, 3))
    mass = np.where(np.arange(N_) % 5 == 4, 0.0, np.where(np.arange(N_) % 2 == 0, 1.008, 15.999))
    vel = np.zeros((R_, N_, 3))
    vel[:, mass == 0] = rng.standard_normal((R_, int((mass == 0).sum()), 3))  # site rows: whatever they hold stays
    prm = M.Params(f_tol=1e-3, dt_start=0.02, dt_max=0.2, max_step=0.1)
    return x0.astype(np_dt), x.astype(np_dt), vel.astype(np_dt), mass.astype(np_dt), prm


def _lib_params(prm):
    from torchmd_amd import _lib as L

    p = L.FireParams()
    p.struct_size = C.sizeof(L.FireParams)
    p.n_min, p.f_tol, p.dt_start, p.dt_max, p.max_step = prm.n_min, prm.f_tol, prm.dt_start, prm.dt_max, prm.max_step
    p.f_inc, p.f_dec, p.alpha_start, p.f_alpha = prm.f_inc, prm.f_dec, prm.alpha_start, prm.f_alpha
    return p


def _run_kernel(prec, niter, per_iteration=None):
    """`niter` iterations on the device; forces -k (x - x0) from torch each iteration.  Returns pos, vel, live state (host)."""
    from torchmd_amd import _lib as L

    lib, dev = L.load(), _dev()
    x0, x, vel, mass, prm = _harmonic_setup(prec)
    p, v, c, m = (torch.as_tensor(a).to(dev).contiguous() for a in (x, vel, x0, mass))
    state = torch.zeros((R_, 2, L.FIRE_STATE_DOUBLES), dtype=torch.float64, device=dev)
    partials = torch.zeros((R_, L.FIRE_MAX_BLOCKS, 4), dtype=torch.float64, device=dev)
    lp = _lib_params(prm)
    L.check(lib.tmdhip_fire_init(R_, state.data_ptr(), C.byref(lp), _stream()), "tmdhip_fire_init")
    code = L.dtype_code(p.dtype)
    for it in range(niter):
        f = (-K_SPRING * (p - c)).contiguous()
        L.check(lib.tmdhip_fire_step(code, R_, N_, p.data_ptr(), v.data_ptr(), f.data_ptr(), m.data_ptr(), state.data_ptr(),
                                     partials.data_ptr(), C.byref(lp), it, _stream()), "tmdhip_fire_step")
        if per_iteration is not None:
            per_iteration(it, p.cpu().numpy(), v.cpu().numpy(), state[:, (it + 1) & 1].cpu().numpy())
    return p.cpu().numpy(), v.cpu().numpy(), state[:, niter & 1].cpu().numpy()


_KERNEL_RUNS = {}


def _checked_run(prec):
    """The 300-iteration run compared with the model at every iteration (made once per precision, shared by the tests)."""
    if prec in _KERNEL_RUNS:
        return _KERNEL_RUNS[prec]
    x0, x, vel, mass, prm = _harmonic_setup(prec)
    store = x.dtype.type
    k = store(K_SPRING)
    mpos, mvel = x.copy(), vel.copy()
    states = [M.init(prm) for _ in range(R_)]
    worst = {"pos": 0.0, "vel": 0.0}
    scale = float(np.abs(x).max())

    def compare(it, gp, gv, gs):
        for r in range(R_):
            M.step(mpos[r], mvel[r], (-k * (mpos[r] - x0[r])).astype(store), mass, states[r], prm, store=store)
            want = states[r].as_row()
            # whole-number state and the branch-only quantities dt, alpha: exactly the model's
            for col in (0, 1, 2, 3, 4, 6):
                assert gs[r, col] == want[col], (it, r, col, gs[r], want)
            assert gs[r, 5] == pytest.approx(want[5], rel=1e-14), (it, r)
        worst["pos"] = max(worst["pos"], float(np.abs(gp.astype(np.float64) - mpos).max()) / scale)
        worst["vel"] = max(worst["vel"], float(np.abs(gv.astype(np.float64) - mvel).max()))

    gp, gv, gs = _run_kernel(prec, NITER, compare)
    print(f"fire kernel {prec}: worst relative position deviation from the model over {NITER} iterations = {worst['pos']:.3e} "
          f"(velocity, absolute: {worst['vel']:.3e}); iterations {gs[:, 4]}, nuphill {gs[:, 6]}, done {gs[:, 3]}")
    _KERNEL_RUNS[prec] = dict(pos=gp, vel=gv, state=gs, worst=worst, start=(x, vel), mass=mass, model=(mpos, mvel))
    return _KERNEL_RUNS[prec]


@pytest.mark.parametrize("prec", ["f64", "f32"])
def test_kernel_against_the_model(prec):
    run = _checked_run(prec)
    st = run["state"]
    assert st[:, 6].max() > 0  # the overshoot of a well: the uphill branch ran
    assert st[0, 3] == 1 and st[0, 4] == 0  # replica 0: done at iteration 0
    assert st[1, 3] == 1 and 0 < st[1, 4] < NITER  # replica 1: converged mid-run
    assert run["worst"]["pos"] <= POS_BAR[prec], run["worst"]


@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("N", RM.SHAPES)
def test_partial_rows_and_state_bit_for_bit(N, prec):
    """The order of the fixed-order sum (tests/_reduce.py): every partial row fire_reduce_kernel writes (the max column and the
    three sums) against the model, addition by addition, and the state's F_max = sqrt of the folded max.  The four wave sums
    meet in sequence here."""
    from torchmd_amd import _lib as L

    lib, dev = L.load(), _dev()
    mass, vel = RM.velocities(2, N, prec, 7)
    frc = RM.forces(2, N, prec, 7)
    on = mass > 0
    p, v, f, m = (torch.as_tensor(a, dtype=PREC[prec]).to(dev).contiguous() for a in (np.zeros_like(vel), vel, frc, mass))
    state = torch.zeros((2, 2, L.FIRE_STATE_DOUBLES), dtype=torch.float64, device=dev)
    partials = torch.full((2, L.FIRE_MAX_BLOCKS, 4), float("nan"), dtype=torch.float64, device=dev)
    lp = _lib_params(M.Params(f_tol=1e-3, dt_start=0.02, dt_max=0.2, max_step=0.1))
    L.check(lib.tmdhip_fire_init(2, state.data_ptr(), C.byref(lp), _stream()), "tmdhip_fire_init")
    L.check(lib.tmdhip_fire_step(L.dtype_code(p.dtype), 2, N, p.data_ptr(), v.data_ptr(), f.data_ptr(), m.data_ptr(), state.data_ptr(),
                                 partials.data_ptr(), C.byref(lp), 0, _stream()), "tmdhip_fire_step")
    rows, new = partials.cpu().numpy(), state[:, 1].cpu().numpy()
    nb = RM.nblocks_of(N)
    for r in range(2):
        cols = RM.fire_columns(vel[r], frc[r])
        want = np.stack([RM.partial_rows(c, on, RM.SEQUENTIAL, op) for c, op in zip(cols, RM.FIRE_OPS)], axis=1)
        differ = int((rows[r, :nb].view(np.int64) != want.view(np.int64)).any(axis=1).sum())
        fmax = np.sqrt(RM.fold(want[:, 0], np.fmax))
        print(f"N = {N} {prec} replica {r}: {differ} of {nb} partial rows differ from the model; F_max {new[r, 5]!r}, model {fmax!r}")
        assert differ == 0 and np.isnan(rows[r, nb:]).all()  # (rows past the grid are never written)
        assert new[r, 5] == fmax == np.sqrt(cols[0][on].max()) and new[r, 4] == 1


@pytest.mark.parametrize("prec", ["f64", "f32"])
def test_massless_rows_and_a_converged_start_are_never_written(prec):
    run = _checked_run(prec)
    x, vel = run["start"]
    site = run["mass"] == 0
    assert site.sum() == N_ // 5
    assert np.array_equal(run["pos"][:, site], x[:, site]) and np.array_equal(run["vel"][:, site], vel[:, site])
    assert np.array_equal(run["pos"][0], x[0]) and np.array_equal(run["vel"][0], vel[0])
    assert not np.array_equal(run["pos"][2][~site], x[2][~site])


@pytest.mark.parametrize("prec", ["f64", "f32"])
def test_repeat_is_bit_identical_and_a_converged_replica_is_frozen(prec):
    run = _checked_run(prec)
    p2, v2, s2 = _run_kernel(prec, NITER)
    assert np.array_equal(p2, run["pos"]) and np.array_equal(v2, run["vel"]) and np.array_equal(s2, run["state"])
    stop = int(run["state"][1, 4])
    p3, v3, s3 = _run_kernel(prec, stop)
    assert s3[1, 3] == 0  # not yet seen to be converged: that takes the next call
    assert np.array_equal(p3[1], run["pos"][1]) and np.array_equal(v3[1], run["vel"][1])


# ----------------------------------------------------------------------------- 2. end to end
def _system(pos, box, R, prec, vel_seed=None):
    from torchmd_amd.systems import System

    pos = np.asarray(pos, dtype=np.float64)
    s = System(pos.shape[-2], R, PREC[prec], _dev())
    s.set_positions(pos[:, :, None] if pos.ndim == 2 else np.ascontiguousarray(pos.transpose(1, 2, 0)))
    s.set_box(np.asarray(box, dtype=np.float64).reshape(-1)[:3])
    if vel_seed is not None:
        s.vel[:] = torch.as_tensor(np.random.default_rng(vel_seed).standard_normal(tuple(s.vel.shape))).to(s.vel)
    return s


def _total(forces, s):
    return np.asarray(forces.compute(s.pos, s.box, s.forces), dtype=np.float64)


@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("which", ["ala2", "water291"])
def test_minimize_against_the_oracle(which, prec):
    from oracle import torchmd_oracle as orc
    from torchmd_amd.forces import Forces
    from torchmd_amd.minimizers import minimize_fire

    g = load(which)
    par = GoldenParameters(g, PREC[prec])
    if which == "ala2":
        terms, kw, R = ALL_TERMS, dict(cutoff=9.0, switch_dist=7.5, rfa=True), 1
    else:
        terms, kw, R = ["lj", "bonds", "angles", "electrostatics"], dict(cutoff=7.3, rfa=True), 2
    s = _system(np.asarray(g["pos"]).reshape(-1, 3), g["box"], R, prec, vel_seed=4)
    f = Forces(par, terms=terms, **kw)
    vel0 = s.vel.clone()
    e0 = _total(f, s)
    res = minimize_fire(s, f, steps=300)
    held = s.forces.clone()  # "system.forces holds the forces of the final positions"
    e1 = _total(f, s)
    print(f"{which} {prec}: E {e0} -> {e1}; iterations {res.iterations}, fmax {res.fmax}, nuphill {res.nuphill}, converged {res.converged}")
    assert np.all(e1 < e0)
    assert torch.equal(s.vel, vel0)
    fresh = s.forces.double().cpu().numpy()
    assert np.abs(held.double().cpu().numpy() - fresh).max() <= FTOL[prec]
    assert np.abs(res.fmax - np.linalg.norm(fresh, axis=2).max(axis=1)).max() <= FTOL[prec]
    assert res.iterations.shape == (R,) and np.all(res.iterations > 0) and np.all(res.iterations <= 300)
    # energies and forces at the returned positions against the oracle, at the suite's bars
    pots = f.compute(s.pos, s.box, s.forces, returnDetails=True)
    po, Fo, _ = orc.compute(par, s.pos.cpu(), s.box.cpu(), terms, **kw)
    err = (s.forces.cpu() - Fo).abs().max().item()
    print(f"  against the oracle at the minimised positions: max|dF| = {err:.2e}")
    assert err <= FTOL[prec], err
    for r in range(R):
        for t in terms:
            if t == "1-4":
                continue
            assert abs(pots[r][t] - po[r][t]) <= ERTOL[prec] * EFAC * max(1.0, abs(po[r][t])), (r, t, pots[r][t], po[r][t])


def _water_box(prec, R, jitter=0.05, seed=3, **kw):
    from torchmd_amd.builders import tip3p_box, water_forcefield
    from torchmd_amd.forces import Forces
    from torchmd_amd.parameters import Parameters

    mol, pos0, box = tip3p_box(12, seed=seed)
    par = Parameters(water_forcefield(mol), mol, WATER_TERMS, precision=PREC[prec])
    rng = np.random.default_rng(5)
    starts = np.stack([pos0 + jitter * r * rng.standard_normal(pos0.shape) for r in range(R)])
    make = lambda: Forces(par, terms=WATER_TERMS, cutoff=9.0, **(kw or dict(rfa=True)))  # noqa: E731
    return par, starts, box, make


def test_celllist_replicas_equal_their_runs_alone(monkeypatch):
    from torchmd_amd.minimizers import minimize_fire

    monkeypatch.setenv("TMDHIP_LPA", "16")  # (a context picks its lanes per atom from the atoms that share a launch: pin it)
    prec, R = "f32", 3
    par, starts, box, make = _water_box(prec, R)
    # a threshold that some replicas reach within the 100 iterations: the smallest force left after 60 iterations of a pilot run
    pilot = _system(starts, box, R, prec)
    fp = make()
    res = minimize_fire(pilot, fp, steps=60, fmax=1e-6)
    assert fp.stats(pilot.pos)["algorithm"] == "celllist" and not res.converged.any()
    tol = float(res.fmax.min()) * 1.001
    s = _system(starts, box, R, prec)
    res = minimize_fire(s, make(), steps=100, fmax=tol)
    print(f"celllist replicas: threshold {tol:.3f}, iterations {res.iterations}, fmax {res.fmax}, converged {res.converged}")
    assert res.converged.any() and len(set(res.iterations.tolist())) >= 2  # the state is per replica
    for r in range(R):
        alone = _system(starts[r], box, 1, prec)
        ra = minimize_fire(alone, make(), steps=100, fmax=tol)
        assert torch.equal(alone.pos[0], s.pos[r]), r
        assert ra.iterations[0] == res.iterations[r] and ra.converged[0] == res.converged[r] and ra.nuphill[0] == res.nuphill[r]


def test_pme_energy_decreases_and_repeats_bit_for_bit():
    from torchmd_amd.minimizers import minimize_fire

    par, starts, box, make = _water_box("f32", 1, pme=True)
    out = []
    for _ in range(2):
        s, f = _system(starts[0], box, 1, "f32"), make()
        e0 = _total(f, s)
        res = minimize_fire(s, f, steps=50)
        e1 = _total(f, s)
        assert f.stats(s.pos)["pme_evaluations"] > 0 and e1[0] < e0[0], (e0, e1)
        out.append((s.pos.clone(), res))
    print(f"PME: E {e0} -> {e1}, fmax {out[0][1].fmax}")
    assert torch.equal(out[0][0], out[1][0]) and np.array_equal(out[0][1].fmax, out[1][1].fmax)


@pytest.mark.parametrize("prec", ["f64", "f32"])
def test_four_site_water(prec):
    from torchmd_amd import _lib as L
    from torchmd_amd.builders import tip4p_box, tip4pew_forcefield
    from torchmd_amd.forces import Forces
    from torchmd_amd.minimizers import minimize_fire
    from torchmd_amd.parameters import Parameters

    mol, pos, box, vs = tip4p_box(6, seed=3)
    par = Parameters(tip4pew_forcefield(mol), mol, WATER_TERMS, precision=PREC[prec])
    f = Forces(par, terms=WATER_TERMS, cutoff=9.0, rfa=True, virtual_sites=vs)
    s = _system(pos, box, 1, prec)
    e0 = _total(f, s)
    res = minimize_fire(s, f, steps=100)
    sites = torch.as_tensor(vs.sites.astype(np.int64), device=_dev())
    assert torch.all(s.forces[0, sites] == 0)  # spread to the parents
    assert torch.any(s.forces[0] != 0)
    e1 = _total(f, s)
    print(f"four-site water {prec}: E {e0} -> {e1}, fmax {res.fmax}, iterations {res.iterations}")
    assert e1[0] < e0[0]
    # the sites sit where their parents put them: placing them again changes no bit
    again = s.pos.clone()
    tabs = [torch.as_tensor(a, device=_dev()) for a in (vs.sites, vs.parents, vs.weights)]
    L.check(L.load().tmdhip_vsite_construct(L.dtype_code(again.dtype), 1, again.shape[1], again.data_ptr(), vs.nsites,
                                            tabs[0].data_ptr(), tabs[1].data_ptr(), tabs[2].data_ptr(), _stream()), "tmdhip_vsite_construct")
    assert torch.equal(again, s.pos)
    assert not torch.equal(s.pos[0, sites].cpu(), torch.as_tensor(pos[vs.sites]).to(PREC[prec]))  # and they moved with them


def test_a_minimised_start_heats_a_rigid_water_run_less():
    """What it is for: 200 unthermostatted rigid-water steps at 2 fs from zero velocities, from the lattice start and from the
    same start after 200 FIRE iterations.  Only the ordering is asserted (both figures: DESIGN §13)."""
    from torchmd_amd.integrator import Integrator
    from torchmd_amd.minimizers import minimize_fire

    par, starts, box, make = _water_box("f32", 1)
    temps = {}
    for label in ("lattice", "minimised"):
        s, f = _system(starts[0], box, 1, "f32"), make()
        if label == "minimised":
            minimize_fire(s, f, steps=200)
        f.compute(s.pos, s.box, s.forces)
        integ = Integrator(s, f, 2.0, _dev(), gamma=None, T=None, constraints="water")
        Ekin, pot, T = integ.step(200)
        temps[label] = float(np.asarray(T).reshape(-1)[0])
    print(f"temperature after 200 rigid-water steps at 2 fs: lattice start {temps['lattice']:.1f} K, minimised {temps['minimised']:.1f} K")
    assert temps["minimised"] < temps["lattice"], temps


def test_refusals():
    from types import SimpleNamespace

    from torchmd_amd.forces import Forces
    from torchmd_amd.minimizers import minimize_fire

    g = load("water291")
    par = GoldenParameters(g, torch.float64)
    s = _system(np.asarray(g["pos"]).reshape(-1, 3), g["box"], 1, "f64")
    f = Forces(par, terms=["lj", "bonds", "angles", "electrostatics"], cutoff=7.3, rfa=True)
    before = s.pos.clone()
    duck = SimpleNamespace(compute=lambda pos, box, forces: [0.0], par=par)
    with pytest.raises(ValueError):
        minimize_fire(s, duck, steps=10)
    assert minimize_fire(s, f, steps=0) is None
    with pytest.raises(ValueError):
        minimize_fire(s, f, fmax=0)
    s.forces = s.forces.float()
    with pytest.raises(ValueError):
        minimize_fire(s, f, steps=10)  # pos and forces of different dtypes
    s.forces = s.forces.double()
    s.pos = s.pos.transpose(1, 2).contiguous().transpose(1, 2)
    with pytest.raises(ValueError):
        minimize_fire(s, f, steps=10)  # not contiguous
    assert torch.equal(s.pos, before)
