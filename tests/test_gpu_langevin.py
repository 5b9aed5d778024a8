"""The Langevin thermostat against a host Philox and the oracle (run with `-m gpu` on an MI355X).

The thermostat's noise is counter based (csrc/rng.h: `normal3(seed, step, row)`), so it can be reproduced exactly:
  - `tmdhip_normal_fill` is compared with the host reference of tests/_philox.py (Philox4x32-10, the fp32 uniforms bit for
    bit, Box-Muller in float64);
  - every path that applies the thermostat is compared with the oracle's `md_step` fed with the device's own noise
    (`tmdhip_normal_fill(seed, step = k, n = 3 R N)` for global step k, row r * N + i): the stepwise
    `tmdhip_langevin_second_vv`, the fused `tmdhip_md_run` kernels, the step blocks of the lean fp32 pair launch, the
    replica-batched cell-list launch, and the domain-decomposition bricks (key seed + 7919 * rank, row =
    brick-local index);
  - the ensemble a free particle reaches is checked statistically (temperature per mass class, Gaussian shape,
    independence of replicas and components, the kinetic-energy fluctuation).
Mixed masses (1.008, 12.011, 15.999 and one atom of 200) and a large friction (gamma = 50/ps, 1 fs steps: gamma dt = 0.05)
put the per-atom coefficients and the order of the kicks far above the tolerances.  fp64 runs are held to 1e-9; fp32 runs
to twice the oracle's own fp32 error on the same inputs (|oracle_f32 - oracle_f64|) plus a floor."""

import ctypes as C

import numpy as np
import pytest
import torch

import _philox as P
from _golden import GoldenParameters, PREC, load
from oracle import torchmd_oracle as orc

pytestmark = pytest.mark.gpu

GAMMA_PS = 50.0
T_BATH = 300.0
MASS_CYCLE = (1.008, 12.011, 15.999)
HEAVY = 200.0
TOL64 = 1e-9  # test_nve_trajectory_vs_reference
ORACLE32_FACTOR = 2.0
# One pair crossing a 9 A cutoff between the fp32 evaluations (no switch: an LJ force step of up to ~2e-3 kcal/mol/A,
# test_gpu_domain.py::_oracle_box) moves the velocity of the lightest atom by dt / m * 2e-3 per step: part of the fp32 floor.
FLIP_FORCE = 2e-3
SEED = 0x9E3779B97F4A7C15  # high 32 bits set
RLIST = 11.0  # the oracle's candidate pairs: every pair within cutoff + 2 A


def _dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _fill(n, seed, step, dtype=torch.float32):
    from torchmd_amd import _lib as L

    out = torch.empty(n, dtype=dtype, device=_dev())
    L.check(L.load().tmdhip_normal_fill(L.dtype_code(dtype), n, out.data_ptr(), C.c_uint64(seed), C.c_uint64(step), _stream()),
            "tmdhip_normal_fill")
    return out.cpu()


def _noise(seed, step, R, N):
    """The noise of global step `step` for R replicas of N atoms, rows r * N + i (fp32 variates, as float64)."""
    return _fill(3 * R * N, seed, step).double().reshape(R, N, 3)


def _masses(n):
    m = np.array([MASS_CYCLE[i % 3] for i in range(n)])
    m[min(7, n - 1)] = HEAVY
    return m


# ----------------------------------------------------------------------------- 2. the noise itself
@pytest.mark.parametrize("n", [1, 2, 4, 3 * 256 + 1, 3 * 10**6])
def test_normal_fill_equals_the_host_philox(n):
    """fp32 variates within 2e-5 of the float64 Box-Muller of the same uniforms (relative to 1 + |g|); fp64 output = the fp32
    output widened, exactly.  Seeds and steps with the high 32 bits set; n % 3 != 0 covers the tail row."""
    worst = 0.0
    for seed, step in ((SEED, 2**32 + 5), (2**64 - 1, 2**63 + 2**32 + 1), (0x0123456789ABCDEF, 7)):
        g32 = _fill(n, seed, step, torch.float32)
        g64 = _fill(n, seed, step, torch.float64)
        assert torch.equal(g64, g32.double()), (n, seed, step)
        ref = P.normal_fill(seed, step, n)
        err = np.abs(g32.double().numpy() - ref) / (1.0 + np.abs(ref))
        worst = max(worst, float(err.max()))
        assert err.max() <= 2e-5, (n, seed, step, err.max(), int(err.argmax()))
    print(f"normal_fill n={n}: max |g_gpu - g_ref| / (1 + |g_ref|) = {worst:.2e}")


# ----------------------------------------------------------------------------- 3. trajectories against the oracle
class Wrapped:
    """Duck-typed forces (not a `Forces`): Integrator.step takes its stepwise loop, tmdhip_langevin_second_vv."""

    def __init__(self, f):
        self.f, self.par = f, f.par

    def compute(self, pos, box, forces):
        return self.f.compute(pos, box, forces)


def _oracle(par, pos, vel, box, masses, terms, calls, seed, dtype, pairs_fn=None, **kw):
    """The oracle's Integrator.step loop fed with the device's noise of global step k; (pos, vel) after every call.
    `pairs_fn(pos)`: candidate pairs, rebuilt at every step's start positions (the drift of one 1 fs step is far below
    RLIST - cutoff); None: all pairs."""
    R, N = pos.shape[:2]
    m = masses.to(dtype).reshape(N, 1)
    dt, gamma, vc = orc.integrator_constants(1.0, GAMMA_PS, T_BATH, m)
    p, v, b = pos.to(dtype).clone(), vel.to(dtype).clone(), box.to(dtype)
    pairs = pairs_fn(p.double()) if pairs_fn else None
    _, f, _ = orc.compute(par, p, b, terms, pairs=pairs, **kw)
    out, k = [], 0
    for c in calls:
        for _ in range(c):
            pairs = pairs_fn(p.double()) if pairs_fn else None
            orc.md_step(par, p, v, f, b, m, dt, terms, gamma=gamma, vcoeff=vc, noise=_noise(seed, k, R, N).to(dtype),
                        pairs=pairs, **kw)
            k += 1
        out.append((p.double().clone(), v.double().clone()))
    return out


def _bounds(ref64, ref32, nsteps, m_min, flip=True):
    """Per call c: (tol_pos, tol_vel).  fp64 (ref32 None): TOL64.  fp32: 2 |oracle_f32 - oracle_f64| + 4 ulp of the largest
    value + the drift that one cutoff flip per step could cause over nsteps[c] steps."""
    dt = 1.0 / orc.TIMEFACTOR
    out = []
    for c, (p64, v64) in enumerate(ref64):
        if ref32 is None:
            out.append((TOL64, TOL64))
            continue
        p32, v32 = ref32[c]
        fv = nsteps[c] * dt / m_min * FLIP_FORCE if flip else 0.0
        tx = ORACLE32_FACTOR * (p32 - p64).abs().max().item() + 4 * np.spacing(np.float32(p64.abs().max().item())) + nsteps[c] * dt * fv
        tv = ORACLE32_FACTOR * (v32 - v64).abs().max().item() + 4 * np.spacing(np.float32(v64.abs().max().item())) + fv
        out.append((float(tx), float(tv)))
    return out


def _compare(what, got, ref64, bounds):
    for c, ((gp, gv), (rp, rv), (tx, tv)) in enumerate(zip(got, ref64, bounds)):
        ex, ev = (gp - rp).abs().max().item(), (gv - rv).abs().max().item()
        print(f"{what} call {c}: max|dx| {ex:.2e} (bound {tx:.1e}), max|dv| {ev:.2e} (bound {tv:.1e})")
        assert ex <= tx and ev <= tv, (what, c, ex, tx, ev, tv)


def _references(par64, par32, pos, vel, box, masses, terms, calls, seed, prec, pairs_fn=None, flip=True, **kw):
    """Oracle trajectories in fp64 (and fp32 for fp32 runs, from the same fp32-rounded start) and their bounds."""
    dt = PREC[prec]
    pos, vel, masses = (t.to(dt).double() for t in (pos, vel, masses))
    ref64 = _oracle(par64, pos, vel, box, masses, terms, calls, seed, torch.float64, pairs_fn=pairs_fn, **kw)
    ref32 = _oracle(par32, pos, vel, box, masses, terms, calls, seed, torch.float32, pairs_fn=pairs_fn, **kw) if prec == "f32" else None
    return ref64, _bounds(ref64, ref32, np.cumsum(calls), float(masses.min()), flip)


def _system(n, R, prec, pos, box, vel, masses):
    from torchmd_amd.systems import System

    s = System(n, R, PREC[prec], _dev())
    s.pos.copy_(pos.to(s.pos))
    s.box.copy_(box.to(s.box))
    s.vel.copy_(vel.to(s.vel))
    s.set_masses(torch.as_tensor(masses))
    return s


def _run(s, forces, calls, seed_torch=9):
    """Integrator.step over `calls`; (pos, vel) after each call, and the integrator."""
    from torchmd_amd.integrator import Integrator

    torch.manual_seed(seed_torch)  # (the noise key is drawn from torch's generator)
    integ = Integrator(s, forces, 1.0, _dev(), gamma=GAMMA_PS, T=T_BATH)
    out = []
    for c in calls:
        integ.step(c)
        out.append((s.pos.cpu().double(), s.vel.cpu().double()))
    return out, integ


def _start(pos0, box3, R, masses, seed, jitter=0.02, vT=T_BATH):
    rng = np.random.default_rng(seed)
    n = len(pos0)
    pos = torch.tensor(np.stack([pos0 + jitter * r * rng.standard_normal(pos0.shape) for r in range(R)]))
    box = torch.zeros(R, 3, 3, dtype=torch.float64)
    for r in range(R):
        box[r].diagonal().copy_(torch.as_tensor(np.asarray(box3, dtype=np.float64)))
    sd = np.sqrt(orc.BOLTZMAN * vT / masses)[None, :, None]
    vel = torch.tensor(rng.standard_normal((R, n, 3)) * sd)
    return pos, box, vel


WATER_TERMS = ["lj", "bonds", "angles", "electrostatics"]
ALL_TERMS = ["bonds", "angles", "dihedrals", "impropers", "1-4", "electrostatics", "lj"]


def _golden_case(name, prec):
    g = load(name)
    if name == "water291":
        return g, GoldenParameters(g, torch.float64), GoldenParameters(g, torch.float32), WATER_TERMS, dict(cutoff=7.3, rfa=True)
    return g, GoldenParameters(g, torch.float64), GoldenParameters(g, torch.float32), ALL_TERMS, \
        dict(cutoff=9.0, switch_dist=7.5, rfa=True)


@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("R", [1, 3])
def test_stepwise_langevin_vs_oracle(R, prec):
    """tmdhip_langevin_second_vv (the Integrator's loop over a duck-typed forces object): water291, calls of 2 and 3 steps."""
    from torchmd_amd.forces import Forces

    g, par64, par32, terms, kw = _golden_case("water291", prec)
    n = len(g["pos"])
    masses = _masses(n)
    pos, box, vel = _start(np.asarray(g["pos"], dtype=np.float64), g["box"], R, masses, seed=R)
    calls = [2, 3]
    s = _system(n, R, prec, pos, box, vel, masses)
    f = Forces(par64 if prec == "f64" else par32, terms=terms, **kw)
    f.compute(s.pos, s.box, s.forces)
    got, integ = _run(s, Wrapped(f), calls)
    ref64, bounds = _references(par64, par32, pos, vel, box, torch.as_tensor(masses), terms, calls, integ._seed, prec, **kw)
    _compare(f"stepwise water291 R={R} {prec}", got, ref64, bounds)


@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("name", ["water291", "ala2"])
def test_fused_md_run_langevin_vs_oracle(name, prec):
    """tmdhip_md_run (the fused MD-step kernels, all-pairs): water291 with R = 2, alanine dipeptide in water (all seven
    terms); calls of 1, 3, 1, 5, 2 steps, so the noise step crosses call boundaries."""
    from torchmd_amd.forces import Forces

    g, par64, par32, terms, kw = _golden_case(name, prec)
    n = len(g["pos"])
    R = 2 if name == "water291" else 1
    masses = _masses(n)
    pos, box, vel = _start(np.asarray(g["pos"], dtype=np.float64), g["box"], R, masses, seed=4)
    calls = [1, 3, 1, 5, 2]
    s = _system(n, R, prec, pos, box, vel, masses)
    f = Forces(par64 if prec == "f64" else par32, terms=terms, algorithm="allpairs", **kw)
    f.compute(s.pos, s.box, s.forces)
    got, integ = _run(s, f, calls)
    assert f.stats(s.pos)["algorithm"] == "allpairs" and integ.replays == 0
    pairs_fn = None
    if name == "ala2":
        ex = orc.exclusion_pairs(par64)
        pairs_fn = lambda p: [orc.candidate_pairs(p[r].numpy(), np.asarray(g["box"], dtype=np.float64), RLIST, ex)  # noqa: E731
                              for r in range(R)]
    ref64, bounds = _references(par64, par32, pos, vel, box, torch.as_tensor(masses), terms, calls, integ._seed, prec,
                                pairs_fn=pairs_fn, **kw)
    _compare(f"fused {name} R={R} {prec}", got, ref64, bounds)


# ----------------------------------------------------------------------------- the ~5k-atom water box on the cell list
_BOX = {}


def _water_box(jitter=0.2):
    from torchmd_amd.builders import tip3p_box, water_forcefield
    from torchmd_amd.parameters import Parameters

    key = jitter
    if key not in _BOX:
        mol, pos, box = tip3p_box(12, seed=3, jitter=jitter)  # 5 184 atoms, L = 37.3 A
        par = {p: Parameters(water_forcefield(mol), mol, WATER_TERMS, precision=PREC[p]) for p in ("f64", "f32")}
        _BOX[key] = (mol, pos, box, par)
    return _BOX[key]


def _box_pairs(box3, par):
    ex = orc.exclusion_pairs(par)
    return lambda p: [orc.candidate_pairs(p[r].numpy(), np.asarray(box3, dtype=np.float64), RLIST, ex) for r in range(p.shape[0])]


def _celllist_case(R, calls, monkeypatch, env=None, skin=0.3, seed=5, prec="f32", jitter=0.2, size_lists_on=None):
    """R replicas of the water box (molecules jittered by `jitter` A) on one cell-list context, Langevin over `calls`, and
    the oracle's trajectories.  `size_lists_on`: build the first lists at these positions (their capacity), then write the
    start through torch (the next call re-plans and rebuilds)."""
    from torchmd_amd.forces import Forces

    for k, v in {"TMDHIP_DEBUG_CHAIN_MIN_ENTRIES": "1", "TMDHIP_LPA": "8", **(env or {})}.items():
        monkeypatch.setenv(k, v)
    mol, pos0, box3, par = _water_box(jitter)
    n = mol.numAtoms
    masses = _masses(n)
    pos, box, vel = _start(pos0, box3, R, masses, seed=seed)
    first = pos if size_lists_on is None else torch.tensor(np.stack([size_lists_on] * R))
    s = _system(n, R, prec, first, box, vel, masses)
    f = Forces(par[prec], terms=WATER_TERMS, cutoff=9.0, rfa=True, algorithm="celllist", skin=skin)
    f.compute(s.pos, s.box, s.forces)
    st0 = [f.stats(s.pos, r) for r in range(R)]
    if size_lists_on is not None:
        s.pos.copy_(pos.to(s.pos))
        fresh = Forces(par[prec], terms=WATER_TERMS, cutoff=9.0, rfa=True, algorithm="celllist")
        fresh.compute(s.pos, s.box, s.forces)  # (the forces of the start, without touching the sized lists)
        fresh.close()
    got, integ = _run(s, f, calls)
    st = [f.stats(s.pos, r) for r in range(R)]
    f.close()
    ref64, bounds = _references(par["f64"], par["f32"], pos, vel, box, torch.as_tensor(masses), WATER_TERMS, calls,
                                integ._seed, prec, pairs_fn=_box_pairs(box3, par["f64"]), cutoff=9.0, rfa=True)
    return got, ref64, bounds, st0, st, integ


def test_step_blocks_of_the_pair_launch_vs_oracle(monkeypatch):
    """The lean fp32 pair launch integrates interior steps in its step blocks; a small skin makes the list rebuild inside
    the window.  Calls of 1, 3, 1, 5, 2 steps; no batch was replayed (a replay after a step-block time-out would have used
    the separate integrator kernel instead)."""
    calls = [1, 3, 1, 5, 2]  # (every rebuild chain in place: chain skipping with this small skin rewinds batches)
    got, ref64, bounds, st0, st, integ = _celllist_case(1, calls, monkeypatch, env={"TMDHIP_CHAIN_SKIP": "0"})
    assert st[0]["algorithm"] == "celllist" and st[0]["overflow"] == 0
    assert integ.replays == 0 and st[0]["fused_step_timeouts"] == 0, (integ.replays, st[0])
    assert st[0]["steps_in_pair_launch"] >= sum(c - 1 for c in calls), st[0]  # (every interior step at least)
    print(f"step blocks: rebuilds {st0[0]['n_rebuilds']} -> {st[0]['n_rebuilds']}")
    assert st[0]["n_rebuilds"] >= st0[0]["n_rebuilds"] + 2, (st0[0], st[0])  # (the first step of the first call may be one)
    _compare("step blocks, water box", got, ref64, bounds)


@pytest.mark.parametrize("R", [2, 3])
def test_replica_batched_celllist_launch_vs_oracle(R, monkeypatch):
    """R replicas of one fp32 cell-list context in one pair + step launch per step: noise rows r * N + i."""
    calls = [3, 4]
    got, ref64, bounds, _, st, integ = _celllist_case(R, calls, monkeypatch, env={"TMDHIP_BATCH_REPLICAS": "1", "TMDHIP_CHAIN_SKIP": "0"},
                                                      seed=10 + R)
    assert st[0]["batched_launches"] > 0, st[0]
    assert integ.replays == 0 and all(x["fused_step_timeouts"] == 0 for x in st), (integ.replays, st)
    _compare(f"batched cell list R={R}", got, ref64, bounds)


@pytest.mark.parametrize("case", ["violation-f32", "overflow-f32", "overflow-f64"])
def test_replayed_batch_vs_oracle(case, monkeypatch):
    """A batch that Integrator.step rewinds (tmdhip_md_restore) and repeats with step0 = nstep - niter must still be the
    oracle's trajectory: same noise steps, velocities restored.
    `violation-f32`: the rewind of test_rebuild_chain_left_out_and_violation_rewound — chain skipping with the "near" report
    disabled and a small skin: the first atom to cross its limit does so in a step without a rebuild chain.
    `overflow-*`: the rewind of test_list_overflow_is_replayed_not_raised — lists sized without slack on the lattice, then
    a start whose molecules are jittered by 0.6 A: the rebuild on the first step overflows and the lists grow.  (Every
    rebuild chain in place: the only rewind is the overflow's.  The start is violent — overlapping molecules fly apart,
    atoms move by more than 1 A in 6 fs — which is why the oracle rebuilds its candidate pairs every step.)"""
    if case == "violation-f32":
        env = {"TMDHIP_CHAIN_SKIP": "1", "TMDHIP_DEBUG_CHAIN_NEAR": "2.0"}
        calls = [4, 6]
        got, ref64, bounds, st0, st, integ = _celllist_case(1, calls, monkeypatch, env=env, seed=7)
    else:
        env = {"TMDHIP_DEBUG_LIST_SLACK": "0", "TMDHIP_CHAIN_SKIP": "0"}
        calls = [6]
        lattice = _water_box(0.0)[1]
        got, ref64, bounds, st0, st, integ = _celllist_case(1, calls, monkeypatch, env=env, prec=case[-3:], jitter=0.6,
                                                            skin=None, seed=21, size_lists_on=lattice)
        assert st[0]["max_neighbours"] > st0[0]["max_neighbours"], (st0[0], st[0])  # the lists grew: it was an overflow
    print(f"{case}: replays {integ.replays}, capacity {st0[0]['max_neighbours']} -> {st[0]['max_neighbours']}, "
          f"rebuilds {st0[0]['n_rebuilds']} -> {st[0]['n_rebuilds']}")
    assert integ.replays >= 1 and st[0]["overflow"] == 0, (integ.replays, st[0])
    _compare(f"replayed batch {case}", got, ref64, bounds)


# ----------------------------------------------------------------------------- domain-decomposition bricks
@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("world", [2, 4])
@pytest.mark.parametrize("mode", ["static", "migrating"])
def test_dd_bricks_langevin_vs_oracle(mode, world, prec):
    """The bricks' native loop (in-process ranks): the noise of brick `rank` is normal3(seed + 7919 rank, k, i) for its
    local row i, mapped to global atoms through `d.ids` as they stand at the kick (read after every single-step call: a
    migration comes before the kick of its step).  LJ + reaction-field mixture, 2 744 atoms.
    `static`: skin 1 A, four single-step calls, then one call of three steps without migration.
    `migrating`: the lattice shifted so that its planes lie on the brick faces, skin 0.3 A and a migration check every
    step: eight single-step calls whose migrations move atoms between bricks and reorder the brick-local rows."""
    from _oracle_sample import mixed_system
    from torchmd_amd.domain import DomainSet, LocalTransport

    dev, dt = _dev(), PREC[prec]
    _, pos0, box3, par64, terms = mixed_system(14, torch.float64)
    par32 = mixed_system(14, torch.float32)[3]
    par = par64 if prec == "f64" else par32
    n = len(pos0)
    masses = _masses(n)
    rng = np.random.default_rng(31)
    vel0 = rng.standard_normal((n, 3)) * np.sqrt(orc.BOLTZMAN * T_BATH / masses)[:, None]
    if mode == "migrating":  # lattice planes (spacing 3.6 A, sites at 1.8 + 3.6 k) onto the faces at multiples of L / 2
        pos0 = np.mod(pos0 + 1.8, np.asarray(box3, dtype=np.float64))
    pos0 = torch.tensor(pos0).to(dt).double().numpy()
    vel0 = torch.tensor(vel0).to(dt).double().numpy()
    m_in = torch.tensor(masses).to(dt).double().numpy()
    A, B = par.get_AB()
    tr = LocalTransport(world, native_threads=True)
    ds = DomainSet(box3, world, dev, dt, terms, 9.0, A=A, B=B, skin=1.0 if mode == "static" else 0.3, transport=tr, rfa=True)
    if mode == "migrating":
        ds.check_every = 1
    ds.scatter(pos0, vel0, par.charges.numpy(), par.mapped_atom_types.numpy(), m_in)
    seed = SEED
    try:
        m0 = ds.migrations
        ds.compute_forces()
        calls, maps = ([1, 1, 1, 1, 3] if mode == "static" else [1] * 8), []
        owners0 = {r: set(d.ids.tolist()) for r, d in ds.domains.items()}
        for c in calls:
            mig = ds.migrations
            before = {r: d.ids.clone() for r, d in ds.domains.items()}
            ds.step(c, timestep_fs=1.0, gamma_ps=GAMMA_PS, T=T_BATH, seed=seed)
            after = {r: (d.rank, d.ids.cpu().clone()) for r, d in ds.domains.items()}
            if c > 1:  # the multi-step call keeps every atom on its brick
                assert ds.migrations == mig and all(torch.equal(before[r], d.ids) for r, d in ds.domains.items())
            maps.append(after)
        moved = sum(len(owners0[r] - set(d.ids.tolist())) for r, d in ds.domains.items())
        print(f"dd bricks {mode} world={world} {prec}: migrations {ds.migrations - m0}, atoms that changed brick {moved}, "
              f"recoveries {ds.recoveries}")
        if mode == "migrating":
            assert ds.migrations > m0 and moved > 0
        got = []
        P_, V_, _ = ds.gather(n)
        got.append((P_.cpu().double(), V_.cpu().double()))
    finally:
        for d in ds.domains.values():
            d.forces_engine.close()
        tr.close()

    def noise_of(k, ranks):
        g = torch.zeros(1, n, 3, dtype=torch.float64)
        for rank, ids in ranks.values():
            g[0, ids.long()] = _fill(3 * len(ids), (seed + 7919 * rank) % 2**64, k).double().reshape(-1, 3)
        return g

    steps = [maps[c] for c, nc in enumerate(calls) for _ in range(nc)]
    box = torch.diag(torch.tensor(np.asarray(box3, dtype=np.float64)))[None]
    pos, vel = torch.tensor(pos0)[None], torch.tensor(vel0)[None]
    mt = torch.tensor(m_in)

    def oracle(p_, dtype):
        m = mt.to(dtype).reshape(n, 1)
        dt_, gamma, vc = orc.integrator_constants(1.0, GAMMA_PS, T_BATH, m)
        p, v, b = pos.to(dtype).clone(), vel.to(dtype).clone(), box.to(dtype)
        pairs = orc.candidate_pairs(pos[0].numpy(), box3, RLIST, None)
        _, f, _ = orc.compute(p_, p, b, terms, pairs=pairs, cutoff=9.0, rfa=True)
        for k, ranks in enumerate(steps):
            orc.md_step(p_, p, v, f, b, m, dt_, terms, gamma=gamma, vcoeff=vc, noise=noise_of(k, ranks).to(dtype), pairs=pairs,
                        cutoff=9.0, rfa=True)
        assert (p.double() - pos.to(dtype).double()).norm(dim=-1).max().item() < 0.5 * (RLIST - 9.0)
        return [(p[0].double(), v[0].double())]

    ref64 = oracle(par64, torch.float64)
    ref32 = oracle(par32, torch.float32) if prec == "f32" else None
    bounds = _bounds(ref64, ref32, [len(steps)], float(mt.min()))
    _compare(f"dd bricks {mode} world={world} {prec}", got, ref64, bounds)


# ----------------------------------------------------------------------------- 4. the ensemble
class ZeroForces:
    def __init__(self, masses):
        self.par = type("P", (), {"masses": masses})()

    def compute(self, pos, box, forces):
        forces.zero_()
        return [0.0] * pos.shape[0]


ENS_MASSES = (1.008, 12.011, 15.999, 200.0)


def _ensemble_masses(n):
    return np.array([ENS_MASSES[i % 4] for i in range(n)])


def _free_gas(prec, fused):
    """Four mass classes, R = 4, 4 fs steps at gamma = 50/ps (gamma dt = 0.2): 200 steps of burn-in, then 40 samples 50 steps
    apart (autocorrelation 0.8^50 = 1.4e-5).  `fused`: a Forces of ε = 0 argon (zero forces) on tmdhip_md_run."""
    from torchmd_amd.integrator import Integrator

    dev, dt = _dev(), PREC[prec]
    R = 4
    if fused:
        from torchmd_amd.builders import Topology, lj_box
        from torchmd_amd.forcefields.ff_yaml import YamlForceField
        from torchmd_amd.forces import Forces
        from torchmd_amd.parameters import Parameters

        mol0, pos0, box3 = lj_box(14, seed=2)  # 2 744 atoms
        n = len(pos0)
        kinds = np.array(["X"] * n, dtype=object)
        ff = {"atomtypes": ["X"], "lj": {"X": {"sigma": 3.4, "epsilon": 0.0}}, "electrostatics": {"X": {"charge": 0.0}},
              "masses": {"X": 40.0}}
        mol = Topology(atomtype=kinds, charge=np.zeros(n, dtype=np.float32), masses=np.full(n, 40.0, dtype=np.float32))
        par = Parameters(YamlForceField(mol, ff), mol, ["lj"], precision=dt)
        forces = Forces(par, terms=["lj"], cutoff=9.0)
    else:
        n = 10_000
        pos0, box3 = np.zeros((n, 3)), np.zeros(3)
        forces = ZeroForces(torch.as_tensor(_ensemble_masses(n)))
    masses = _ensemble_masses(n)
    Tp = T_BATH / (1 - 0.5 * 0.2)
    pos, box, vel = _start(pos0, box3, R, masses, seed=1, jitter=0.0, vT=Tp)
    s = _system(n, R, prec, pos, box, vel, masses)
    if fused:
        forces.compute(s.pos, s.box, s.forces)
    torch.manual_seed(17)
    integ = Integrator(s, forces, 4.0, dev, gamma=GAMMA_PS, T=T_BATH)
    integ.step(200)
    samples = []
    for _ in range(40):
        integ.step(50)
        samples.append(s.vel.cpu().double().numpy())
    if fused:
        assert float(s.forces.abs().max()) == 0.0
        forces.close()
    return np.stack(samples), masses, Tp  # [S, R, N, 3]


@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("path", ["stepwise", "fused"])
def test_free_particle_ensemble(path, prec):
    """v' = (1 - g dt) v + c xi is a Gaussian AR(1) process with stationary variance kT/m / (1 - g dt / 2): per mass class the
    temperature within 4 sigma of T / (1 - g dt / 2), v sqrt(m / kT') Kolmogorov-Smirnov-consistent with N(0, 1), no
    correlation across replicas or components beyond 4 / sqrt(n), and Var(Ekin) / <Ekin>^2 = 2 / (3N) within sampling error."""
    from scipy import stats

    v, masses, Tp = _free_gas(prec, path == "fused")
    S, R, N, _ = v.shape
    kTp = orc.BOLTZMAN * Tp
    z = v * np.sqrt(masses / kTp)[None, None, :, None]  # ~ N(0, 1)
    for c, mc in enumerate(ENS_MASSES):
        zc = z[:, :, c::4, :].reshape(-1)
        ratio = float(np.mean(zc**2))  # T_class / T'
        sig = np.sqrt(2.0 / zc.size)
        p = stats.kstest(zc, "norm").pvalue
        print(f"ensemble {path} {prec} m={mc}: T/T' - 1 = {ratio - 1:+.2e} (4 sigma {4 * sig:.1e}), KS p = {p:.3f}")
        assert abs(ratio - 1) < 4 * sig, (mc, ratio, sig)
        assert p > 1e-3, (mc, p)
    nz = S * N * 3
    lim = 4 / np.sqrt(nz)
    flat = z.transpose(1, 0, 2, 3).reshape(R, -1)  # per replica
    cr = np.corrcoef(flat)
    worst_r = np.abs(cr[np.triu_indices(R, 1)]).max()
    comp = z.transpose(3, 0, 1, 2).reshape(3, -1)
    cc = np.corrcoef(comp)
    worst_c = np.abs(cc[np.triu_indices(3, 1)]).max()
    print(f"ensemble {path} {prec}: max replica correlation {worst_r:.1e}, max component correlation {worst_c:.1e} (bound {lim:.1e})")
    assert worst_r < lim and worst_c < 4 / np.sqrt(comp.shape[1])
    ek = 0.5 * (masses[None, None, :] * (v**2).sum(axis=-1)).sum(axis=-1).reshape(-1)  # S * R values
    rel = ek.var(ddof=1) / ek.mean() ** 2 * (3 * N / 2)
    sig = np.sqrt(2.0 / (ek.size - 1))
    print(f"ensemble {path} {prec}: Var(Ekin) / <Ekin>^2 / (2 / 3N) = {rel:.3f} (4 sigma {4 * sig:.2f})")
    assert abs(rel - 1) < 4 * sig
