"""A context that has lived against a fresh one.

Every other GPU test builds a `Forces`, uses it for one purpose and drops it.  Here one `Forces` lives through a sequence of state
changes — its box walks, its atoms are swapped, its side terms are re-set, a feature is released and set again, callers take
turns on it, a call is refused — and after EVERY change it is compared with a fresh `Forces` built from the final settings and
given the same tensors, by the one rule of tests/_lifecycle.py (`judge`): equal pair counts, each of the two within the parity
bars of the oracle (side terms: their numpy models), and then bit for bit — or, where a docstring names the state that
legitimately differs, within twice the fresh context's own distance from the oracle on that very input (rule 4).

TMDHIP_VSKIN=0 throughout (static skins: a rebuild decision depends on positions only).  What makes bit identity possible:
both lists are built at the positions under test — the change itself forces the rebuild (a new box, an atom swap), or
`invalidate_lists` is called on the lived context before the leg — and forces are stored, not accumulated with atomics, on
the cell-list path.  Energies always go by rule 4 (atomic adds of fp64 partials: tests/_lifecycle.py)."""

import ctypes as C

import numpy as np
import pytest
import torch

import _lifecycle as LC
from _golden import PREC
from test_gpu_parity import EFAC, ERTOL, FTOL

pytestmark = pytest.mark.gpu

WATER_TERMS = ["lj", "electrostatics", "bonds", "angles"]
EPS32, EPS64 = float(np.finfo(np.float32).eps), float(np.finfo(np.float64).eps)


@pytest.fixture(autouse=True)
def _static_skins(monkeypatch):
    monkeypatch.setenv("TMDHIP_VSKIN", "0")


def _dev():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    return torch.device("cuda:0")


def _stream():
    return C.c_void_p(torch.cuda.current_stream(_dev()).cuda_stream)


# ----------------------------------------------------------------------------- systems and references, made once
_WATER, _ORACLE = {}, {}


def _water(nside, prec, seed=8):
    from torchmd_amd.builders import tip3p_box, water_forcefield
    from torchmd_amd.integrator import maxwell_boltzmann
    from torchmd_amd.parameters import Parameters

    key = (nside, prec, seed)
    if key not in _WATER:
        mol, pos, box = tip3p_box(nside, seed=seed)
        par = Parameters(water_forcefield(mol), mol, WATER_TERMS, precision=PREC[prec])
        torch.manual_seed(seed)
        vel = maxwell_boltzmann(Parameters(water_forcefield(mol), mol, WATER_TERMS, precision=torch.float64).masses, 300.0, 3)
        _WATER[key] = (mol, np.asarray(pos, dtype=np.float64), np.asarray(box, dtype=np.float64), par, vel)
    return _WATER[key]


def _box_tensor(edges, prec):
    """[R, 3, 3] device tensor with the diagonals `edges` [R, 3]."""
    e = np.asarray(edges, dtype=np.float64).reshape(-1, 3)
    b = torch.zeros(len(e), 3, 3, dtype=PREC[prec], device=_dev())
    for r in range(len(e)):
        b[r].diagonal().copy_(torch.as_tensor(e[r], dtype=PREC[prec]))
    return b


def _edges(b):
    return torch.diagonal(b.detach(), dim1=-2, dim2=-1).cpu().double().numpy()


def _oracle(par, p, b, terms, okw, side=None, key=None, drop=None, explicit=True):
    """The reference on the tensors the contexts see: the oracle, evaluated in the contexts' precision with a sparse candidate
    list, plus `side(pos [R,N,3] float64, edges [R,3]) -> (energy [R], forces [R,N,3])` of a side term's numpy model (its energy
    under the name "side").  `drop`: atoms whose nonbonded pairs are left out (a solute the engine no longer couples);
    `explicit=False`: the autograd flavour of the forces (-dE/dr).  Results are kept under `key` for the tests that share an input."""
    from oracle import torchmd_oracle as orc

    if key is not None and key in _ORACLE:
        return _ORACLE[key]
    pc, bc = p.detach().cpu(), b.detach().cpu()
    edges = _edges(b)
    excl = orc.exclusion_pairs(par) if getattr(par, "bond_params", None) is not None else None
    pots, Fs, ns = [], [], []
    for r in range(pc.shape[0]):
        pairs = orc.candidate_pairs(pc[r].double().numpy(), edges[r], okw["cutoff"] + 0.6, excl) if okw.get("cutoff") else orc.all_pairs(pc.shape[1], excl)
        if drop is not None:
            gone = np.zeros(pc.shape[1], dtype=bool)
            gone[np.asarray(drop)] = True
            pairs = pairs[~(gone[pairs[:, 0]] | gone[pairs[:, 1]])]
        pr = pc[r : r + 1] if explicit else pc[r : r + 1].clone().requires_grad_(True)
        e, F, n = orc.compute(par, pr, bc[r : r + 1], terms, pairs=pairs, explicit_forces=explicit, **okw)
        F = F.detach()
        pots.append(dict(e[0]))
        Fs.append(F.double())
        ns.append(int(n[0]))
    F = torch.cat(Fs, dim=0)
    if side is not None:
        es, fs = side(pc.double().numpy(), edges)
        F = F + torch.as_tensor(fs)
        for r in range(len(pots)):
            pots[r]["side"] = float(es[r])
    ref = LC.Result(npairs=ns, energies=pots, forces=F)
    if key is not None:
        _ORACLE[key] = ref
    return ref


def _evaluate(f, p, b, side_name=None, count=True):
    """One context on one input, by every evaluation path: `compute(returnDetails=True)` twice (the second call finds a list
    that matches the box: in fp32 the fused evaluation of tmdhip_compute), the forces-only launch of an MD step, the pair count.
    Force buffers are pre-filled with NaN: a row nobody writes shows."""
    F1, F2, F3 = (torch.full_like(p, float("nan")) for _ in range(3))
    pots = f.compute(p, b, F1, returnDetails=True)
    pots2 = f.compute(p, b, F2, returnDetails=True)
    f._evaluate(p, b, F3, False, True)
    n = f.count_pairs(p, b) if count else None
    if side_name is not None:
        for d in pots + pots2:
            d["side"] = d[side_name]
    return LC.Result(npairs=n, energies=pots, forces=F1.cpu(), forces_only=F3.cpu(),
                     extra={"forces_second_compute": F2.cpu()})


def _system(n, R, prec, p, b, vel, forces=None):
    from torchmd_amd.systems import System

    s = System(n, R, PREC[prec], _dev())
    s.box = b
    s.pos.copy_(p)
    s.vel.copy_(vel.to(PREC[prec]).to(_dev()))
    if forces is not None:
        s.forces.copy_(forces)
    return s


def _kinetic(s, masses):
    m = masses.detach().cpu().double().reshape(1, -1, 1)
    return (0.5 * m * s.vel.detach().cpu().double() ** 2).sum(dim=(1, 2)).numpy()


def _check_kinetic(label, out, s, masses, prec):
    """The kinetic energy a step returns is that of the velocities it leaves: a double sum of 3N products on the host against
    the device's, 3N eps64 for the order of the sum and eps32 for the cast of an fp32 run's result."""
    K = _kinetic(s, masses)
    got = np.asarray(out[0], dtype=np.float64)
    bound = K * (3 * s.pos.shape[1] * EPS64 + (EPS32 if prec == "f32" else 0.0))
    print(f"{label}: Ekin returned {got}, of the velocities left {K}")
    assert (np.abs(got - K) <= bound).all(), (label, got, K, bound)


def _step_leg(label, par, terms, okw, fkw, lived, s, integ, n, prec, bitwise=True, side=None, rebuild=True, drop=None):
    """`integ.step(n)` on the lived context against the same call on a fresh context given the state the lived one is in
    (positions, velocities, forces: copies).  `rebuild`: the lived lists are dropped first, so that both contexts build
    theirs at the positions the leg starts from.  Rule 2 holds the forces each run leaves to the reference at its final
    positions.  Returns (the lived call's result, the fresh Forces, the fresh System)."""
    from torchmd_amd.forces import Forces
    from torchmd_amd.integrator import TIMEFACTOR, Integrator

    R, N = s.pos.shape[0], s.pos.shape[1]
    fresh = Forces(par, terms=terms, **okw, **fkw)
    sf = _system(N, R, prec, s.pos, s.box, s.vel, s.forces)
    if rebuild:
        lived.invalidate_lists(s.pos)
    out_l = integ.step(n)
    out_f = Integrator(sf, fresh, integ.dt * TIMEFACTOR, _dev()).step(n)
    ref_l = _oracle(par, s.pos, s.box, terms, okw, side=side, drop=drop)
    same = torch.equal(s.pos, sf.pos)
    ref_f = ref_l if same else _oracle(par, sf.pos, sf.box, terms, okw, side=side, drop=drop)
    dl, df = LC.force_distance(s.forces.cpu(), ref_l.forces), LC.force_distance(sf.forces.cpu(), ref_f.forces)
    diff = {k: LC.force_distance(a.cpu(), b.cpu()) for k, (a, b) in {"pos": (s.pos, sf.pos), "vel": (s.vel, sf.vel), "forces": (s.forces, sf.forces)}.items()}
    print(f"{label} step({n}) [{prec}]: forces left against the reference: lived {dl:.3e}, fresh {df:.3e}; lived - fresh: {diff}; "
          f"Epot {out_l[1]} / {out_f[1]}, Ekin {out_l[0]} / {out_f[0]}")
    assert dl <= FTOL[prec] and df <= FTOL[prec], (label, dl, df)
    for r in range(R):  # the potential energy returned: every term within its parity bar, so the total within their sum
        tot, bar = sum(ref_l.energies[r].values()), ERTOL[prec] * EFAC * sum(max(1.0, abs(v)) for v in ref_l.energies[r].values())
        for name, o in (("lived", out_l), ("fresh", out_f)):
            assert abs(o[1][r] - tot) <= bar, (label, name, o[1][r], tot, bar)
    if bitwise:
        for k, (a, b) in {"pos": (s.pos, sf.pos), "vel": (s.vel, sf.vel), "forces": (s.forces, sf.forces)}.items():
            assert torch.equal(a, b), (label, k, diff[k])
        # (the kinetic energy is a fixed-order sum of the same velocities; the potential is folded with atomic adds: rule 4)
        assert np.array_equal(np.asarray(out_l[0]), np.asarray(out_f[0])), (label, out_l[0], out_f[0])
    else:
        assert diff["forces"] <= 2.0 * df, (label, diff, df)
    for r in range(R):
        tot = sum(ref_l.energies[r].values())
        assert abs(out_l[1][r] - out_f[1][r]) <= 2.0 * abs(out_f[1][r] - tot), (label, out_l[1], out_f[1], tot)
    return out_l, fresh, sf


# ----------------------------------------------------------------------------- 1. box walk, one replica
@pytest.mark.timeout(120)
@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_box_walk_one_replica(prec):
    """2 187-atom water, cutoff 8.5 A (list radius 9.7: cells of 4.85 A, 5.76 per edge at L = 27.95).  Positions and box are
    scaled together: 1.00 -> 1.04 -> 0.97 (IN PLACE: `box.mul_`, the tensor `Forces._box_cache` knows, `_version` bumped) ->
    1.05 (6 cells per edge instead of 5) -> 1.00.  After every stop the lived context answers compute (twice: plain and, in
    fp32, fused), the forces-only launch, count_pairs and Integrator.step(3) like a fresh one, bit for bit: the new box forces
    the re-plan and the rebuild at the positions under test (asserted: n_rebuilds grows), and at 2 187 atoms every context
    takes 64 lanes per atom whatever its list capacity.  For `step` the lived lists are dropped first — found here: a list
    kept from the evaluations (built at the undrifted positions) against the fresh context's (built inside the run, behind
    the first drift) costs one ulp of a position after three steps, both within 2e-13 / 1.1e-4 of the oracle: two valid
    lists, two summation orders.  What legitimately differs and does not show: the list capacity (`lg.maxn`, sized once for
    the first box) and with it the row stride of the list."""
    from torchmd_amd.forces import Forces
    from torchmd_amd.integrator import Integrator

    mol, pos, box, par, vel = _water(9, prec)
    N, cutoff = mol.numAtoms, 8.5
    okw, fkw = dict(cutoff=cutoff, rfa=True), {}
    rlist = cutoff + LC.DEFAULT_SKIN
    lived = Forces(par, terms=WATER_TERMS, **okw)
    b = _box_tensor(box, prec)
    s = integ = None
    seen, rebuilds, fused = [], 0, 0
    for stop, scale in enumerate((1.00, 1.04, 0.97, 1.05, 1.00)):
        if stop == 2:
            b.mul_(0.97 / 1.04)  # in place: the same tensor object, another version
        else:
            b = _box_tensor(box * scale, prec)
        p = torch.as_tensor(pos * scale, dtype=PREC[prec]).to(_dev())[None].contiguous()
        want = LC.planned_cells(_edges(b)[0], rlist, N)
        seen.append(want)
        fresh = Forces(par, terms=WATER_TERMS, **okw)
        ref = _oracle(par, p, b, WATER_TERMS, okw)
        rl, rf = _evaluate(lived, p, b), _evaluate(fresh, p, b)
        for name, f in (("lived", lived), ("fresh", fresh)):
            st = f.stats(p)
            assert st["algorithm"] == "celllist" and st["ncell"] == want and st["overflow"] == 0, (stop, name, st, want)
        assert lived.stats(p)["n_rebuilds"] > rebuilds, (stop, "the new box did not rebuild the list")
        LC.judge(f"box walk, stop {stop} (x{scale})", rl, rf, ref, prec, WATER_TERMS, bitwise=True)
        if s is None:
            s = _system(N, 1, prec, p, b, vel[:1], rl.forces.to(_dev()))
            integ = Integrator(s, lived, 1.0, _dev())
        else:
            s.box = b
            s.pos.copy_(p)
            s.vel.copy_(vel[:1].to(PREC[prec]).to(_dev()))
            s.forces.copy_(rl.forces.to(_dev()))
        # (the lived lists are dropped first: a fresh context builds its list inside the run, behind the first drift, and a list
        # kept from the evaluations above — built at the undrifted positions — is as valid and sums in another order: one ulp)
        out, fr, sf = _step_leg(f"box walk, stop {stop}", par, WATER_TERMS, okw, fkw, lived, s, integ, 3, prec)
        _check_kinetic(f"box walk, stop {stop}", out, s, integ.masses, prec)
        st, stf = lived.stats(s.pos), fr.stats(sf.pos)
        rebuilds = st["n_rebuilds"]
        if prec == "f32":  # the first step builds the list; the second of three is made by the pair launch, on either context
            assert st["steps_in_pair_launch"] >= fused + 1 and stf["steps_in_pair_launch"] >= 1, (stop, st, stf)
        else:
            assert st["steps_in_pair_launch"] == 0
        fused = st["steps_in_pair_launch"]
    assert seen == [(5, 5, 5), (5, 5, 5), (5, 5, 5), (6, 6, 6), (5, 5, 5)], seen


# ----------------------------------------------------------------------------- 2. into and out of the all-pairs fallback
def _oracle_trajectory(par, p, b, vel, forces, masses, dt, n, okw):
    """`n` velocity-Verlet steps of the oracle (integrator.py:115-120) from the given state, in the tensors' precision."""
    from oracle import torchmd_oracle as orc

    pc, vc, fc, bc = p.detach().cpu().clone(), vel.detach().cpu().clone(), forces.detach().cpu().clone(), b.detach().cpu()
    m = masses.detach().cpu().to(pc.dtype).reshape(-1, 1)
    excl = orc.exclusion_pairs(par)
    for _ in range(n):
        orc.first_vv(pc, vc, fc, m, dt)
        pairs = orc.candidate_pairs(pc[0].double().numpy(), _edges(b)[0], okw["cutoff"] + 0.6, excl)
        _, f, _ = orc.compute(par, pc, bc, WATER_TERMS, pairs=pairs, **okw)
        fc.copy_(f)
        orc.second_vv(vc, fc, m, dt)
    return pc, vc, fc


@pytest.mark.timeout(120)
@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_box_walk_into_and_out_of_the_all_pairs_fallback(prec):
    """2 187-atom water, cutoff 9.8 A (list radius 11.0: 5.08 cells of 5.5 A per edge, the fewest the planner takes), AUTO.
    The box shrunk by 3 % holds 4.93: the context switches to the all-pairs kernel and, BY DESIGN, stays there when the box is
    large again (the switch is one-way).  Large: bit for bit.  Small and large again: rule 4 — the all-pairs
    kernel accumulates forces with floating-point atomics, and at the last stop the fresh context is a cell-list one (another
    kernel, another summation order).  Then the same flip inside `Integrator.step`, the box shrinking between two calls: rule 4
    against three steps of the oracle's integrator.  `algorithm="celllist"` forced: the small box raises, and the next call
    with the large box equals a fresh context bit for bit (the list of the large box is still there and still right)."""
    from torchmd_amd.forces import Forces
    from torchmd_amd.integrator import Integrator

    mol, pos, box, par, vel = _water(9, prec)
    N, cutoff = mol.numAtoms, 9.8
    okw = dict(cutoff=cutoff, rfa=True)
    rlist = cutoff + LC.DEFAULT_SKIN
    stops = {}
    for scale in (1.00, 0.97):
        b = _box_tensor(box * scale, prec)
        p = torch.as_tensor(pos * scale, dtype=PREC[prec]).to(_dev())[None].contiguous()
        stops[scale] = (p, b, _oracle(par, p, b, WATER_TERMS, okw))
    assert LC.planned_cells(_edges(stops[1.00][1])[0], rlist, N) == (5, 5, 5)
    assert LC.planned_cells(_edges(stops[0.97][1])[0], rlist, N) is None
    lived = Forces(par, terms=WATER_TERMS, **okw)
    for stop, (scale, algo_l, algo_f) in enumerate(((1.00, "celllist", "celllist"), (0.97, "allpairs", "allpairs"), (1.00, "allpairs", "celllist"))):
        p, b, ref = stops[scale]
        fresh = Forces(par, terms=WATER_TERMS, **okw)
        rl, rf = _evaluate(lived, p, b), _evaluate(fresh, p, b)
        assert lived.stats(p)["algorithm"] == algo_l and fresh.stats(p)["algorithm"] == algo_f, (stop, lived.stats(p), fresh.stats(p))
        if algo_l == "celllist":
            assert lived.stats(p)["ncell"] == (5, 5, 5)
        LC.judge(f"fallback walk, stop {stop} (x{scale})", rl, rf, ref, prec, WATER_TERMS, bitwise=algo_l == "celllist")
    # ---- the flip inside Integrator.step
    lived = Forces(par, terms=WATER_TERMS, **okw)
    p, b, ref = stops[1.00]
    s = _system(N, 1, prec, p, b, vel[:1])
    lived.compute(s.pos, s.box, s.forces)
    integ = Integrator(s, lived, 1.0, _dev())
    _step_leg("fallback in step, large box", par, WATER_TERMS, okw, {}, lived, s, integ, 3, prec)
    assert lived.stats(s.pos)["algorithm"] == "celllist"
    p, b, ref = stops[0.97]
    s.box = b
    s.pos.copy_(p)
    s.vel.copy_(vel[:1].to(PREC[prec]).to(_dev()))
    s.forces.copy_(ref.forces.to(PREC[prec]).to(_dev()))  # (the forces of the shrunk state, from the oracle: no call flips the context yet)
    fresh = Forces(par, terms=WATER_TERMS, **okw)
    sf = _system(N, 1, prec, s.pos, s.box, s.vel, s.forces)
    po, vo, fo = _oracle_trajectory(par, s.pos, s.box, s.vel, s.forces, integ.masses, integ.dt, 3, okw)
    assert lived.stats(s.pos)["algorithm"] == "celllist"
    out_l = integ.step(3)
    out_f = Integrator(sf, fresh, 1.0, _dev()).step(3)
    assert lived.stats(s.pos)["algorithm"] == "allpairs" and fresh.stats(sf.pos)["algorithm"] == "allpairs"
    for k, (a, c, o) in {"pos": (s.pos, sf.pos, po), "vel": (s.vel, sf.vel, vo), "forces": (s.forces, sf.forces, fo)}.items():
        LC.rule4(f"fallback in step, {k}", a.cpu(), c.cpu(), o)
    # (rule 2 for the forces a run leaves: against the oracle at the run's OWN final positions — an ulp of a position moves a
    # bond force by 1e-3 — ; rule 4 above measures the trajectories, forces included, against the oracle's)
    dl = LC.force_distance(s.forces.cpu(), _oracle(par, s.pos, s.box, WATER_TERMS, okw).forces)
    df = LC.force_distance(sf.forces.cpu(), _oracle(par, sf.pos, sf.box, WATER_TERMS, okw).forces)
    print(f"fallback in step [{prec}]: forces left against the oracle at the final positions: lived {dl:.3e}, fresh {df:.3e}")
    assert dl <= FTOL[prec] and df <= FTOL[prec]
    _check_kinetic("fallback in step", out_l, s, integ.masses, prec)
    # ---- the cell list forced
    forced = Forces(par, terms=WATER_TERMS, algorithm="celllist", **okw)
    p, b, ref = stops[1.00]
    _evaluate(forced, p, b)
    with pytest.raises(RuntimeError, match="cell list cannot be used"):
        forced.compute(stops[0.97][0], stops[0.97][1], torch.zeros_like(p))
    fresh = Forces(par, terms=WATER_TERMS, algorithm="celllist", **okw)
    rl, rf = _evaluate(forced, p, b), _evaluate(fresh, p, b)
    assert forced.stats(p)["algorithm"] == "celllist" and forced.stats(p)["ncell"] == (5, 5, 5)
    LC.judge("forced cell list after the refused box", rl, rf, ref, prec, WATER_TERMS, bitwise=True)


# ----------------------------------------------------------------------------- 3. replicas with boxes of their own
def _replica_state(pos, box, scales, jitter, prec):
    p = torch.as_tensor(np.stack([(pos + jitter[r]) * scales[r] for r in range(len(scales))]), dtype=PREC[prec]).to(_dev()).contiguous()
    return p, _box_tensor(np.stack([box * sc for sc in scales]), prec)


@pytest.mark.timeout(180)
@pytest.mark.parametrize("R", [2, 3])
def test_replicas_with_boxes_that_change_independently(R, monkeypatch):
    """fp32, 5 184-atom water, R replicas with coordinates, velocities and boxes of their own in ONE pair + step launch per MD
    step (asserted: batched_launches, steps_in_pair_launch).  Between `step` calls only replica 1's box changes, then the
    boxes of replicas 0 and 1 swap: the cached `batch_host` entries (box constants, list geometry) must be uploaded again
    exactly where they changed.  Every replica equals its own fresh single-replica context bit for bit — the claim of
    test_replicas_of_a_celllist_context_in_one_launch_are_bit_identical, here for a context that has lived.  Lanes per atom
    pinned (TMDHIP_LPA=16) as there: a context picks them from the atoms that share a launch."""
    from torchmd_amd.forces import Forces
    from torchmd_amd.integrator import Integrator

    monkeypatch.setenv("TMDHIP_LPA", "16")
    prec = "f32"
    mol, pos, box, par, vel = _water(12, prec, seed=3)
    N = mol.numAtoms
    okw = dict(cutoff=9.0, rfa=True)
    rng = np.random.default_rng(5)
    jitter = [0.01 * rng.standard_normal(pos.shape) for _ in range(R)]  # (enough to tell the replicas apart; the bonds stay near rest)
    lived = Forces(par, terms=WATER_TERMS, **okw)
    s = integ = None
    batched = fusedsteps = 0
    walks = ([1.0, 1.004, 0.997][:R], [1.0, 1.009, 0.997][:R], [1.009, 1.0, 0.997][:R])
    for stop, scales in enumerate(walks):
        p, b = _replica_state(pos, box, scales, jitter, prec)
        ref = _oracle(par, p, b, WATER_TERMS, okw)
        lived.invalidate_lists(p)
        rl = _evaluate(lived, p, b)
        singles = [Forces(par, terms=WATER_TERMS, **okw) for _ in range(R)]
        rf = LC.stack([_evaluate(singles[r], p[r : r + 1].contiguous(), b[r : r + 1].contiguous()) for r in range(R)])
        for r in range(R):
            st = lived.stats(p, r)
            assert st["algorithm"] == "celllist" and st["ncell"] == LC.planned_cells(_edges(b)[r], 10.2, N) == (7, 7, 7), (stop, r, st)
        LC.judge(f"{R} replicas, stop {stop} {scales}", rl, rf, ref, prec, WATER_TERMS, bitwise=True)
        if s is None:
            s = _system(N, R, prec, p, b, vel[:R], rl.forces.to(_dev()))
            integ = Integrator(s, lived, 1.0, _dev())
        else:
            s.box = b
            s.pos.copy_(p)
            s.vel.copy_(vel[:R].to(PREC[prec]).to(_dev()))
            s.forces.copy_(rl.forces.to(_dev()))
        lived.invalidate_lists(s.pos)
        out = integ.step(4)
        st = lived.stats(s.pos)
        # (of four steps the first builds the lists; the two interior ones behind it are batched launches that make a step)
        assert st["batched_launches"] >= batched + 2 and st["steps_in_pair_launch"] >= fusedsteps + 2, (stop, st)
        batched, fusedsteps = st["batched_launches"], st["steps_in_pair_launch"]
        ends = []
        for r in range(R):
            sr = _system(N, 1, prec, p[r : r + 1], b[r : r + 1].contiguous(), vel[r : r + 1], rl.forces[r : r + 1].to(_dev()))
            fr = Forces(par, terms=WATER_TERMS, **okw)
            Integrator(sr, fr, 1.0, _dev()).step(4)
            assert fr.stats(sr.pos)["steps_in_pair_launch"] >= 2 and fr.stats(sr.pos)["batched_launches"] == 0
            ends.append(sr)
        end_ref = _oracle(par, s.pos, s.box, WATER_TERMS, okw)
        d = LC.force_distance(s.forces.cpu(), end_ref.forces)
        print(f"{R} replicas, stop {stop}: forces left by step(4) against the oracle {d:.3e}")
        assert d <= FTOL[prec]
        for r in range(R):
            for k in ("pos", "vel", "forces"):
                a, c = getattr(s, k)[r : r + 1], getattr(ends[r], k)
                assert torch.equal(a, c), (stop, r, k, LC.force_distance(a.cpu(), c.cpu()))
        _check_kinetic(f"{R} replicas, stop {stop}", out, s, integ.masses, prec)


@pytest.mark.timeout(120)
def test_one_replica_of_two_falls_back_to_all_pairs(monkeypatch):
    """fp32, two replicas of the 2 187-atom water at cutoff 9.8 A in an AUTO context: replica 1 alone gets the box that is too
    small for cells, so `ctx->algorithm` flips in the middle of tmdhip_compute_nonbonded's loop over the replicas — replica 0
    has been evaluated from its list by then, replica 1 and every later call take the all-pairs kernel.  Rule 4 from the flip
    on (force atomics); before it each replica equals its single-replica context bit for bit.  The same flip inside `step`."""
    from torchmd_amd.forces import Forces
    from torchmd_amd.integrator import Integrator

    monkeypatch.setenv("TMDHIP_LPA", "16")
    prec = "f32"
    mol, pos, box, par, vel = _water(9, prec)
    N = mol.numAtoms
    okw = dict(cutoff=9.8, rfa=True)
    rng = np.random.default_rng(6)
    jitter = [0.01 * rng.standard_normal(pos.shape) for _ in range(2)]

    def against_singles(label, f, p, b, bitwise, algos):
        ref = _oracle(par, p, b, WATER_TERMS, okw)
        rl = _evaluate(f, p, b)
        singles = [Forces(par, terms=WATER_TERMS, **okw) for _ in range(2)]
        rf = LC.stack([_evaluate(singles[r], p[r : r + 1].contiguous(), b[r : r + 1].contiguous()) for r in range(2)])
        assert [singles[r].stats(p[r : r + 1])["algorithm"] for r in range(2)] == algos, label
        LC.judge(label, rl, rf, ref, prec, WATER_TERMS, bitwise=bitwise)

    lived = Forces(par, terms=WATER_TERMS, **okw)
    p, b = _replica_state(pos, box, [1.0, 1.002], jitter, prec)
    against_singles("two replicas, both large", lived, p, b, True, ["celllist", "celllist"])
    assert lived.stats(p)["algorithm"] == "celllist"
    p, b = _replica_state(pos, box, [1.0, 0.97], jitter, prec)
    against_singles("two replicas, replica 1 small", lived, p, b, False, ["celllist", "allpairs"])
    assert lived.stats(p)["algorithm"] == "allpairs"
    p, b = _replica_state(pos, box, [1.0, 1.002], jitter, prec)
    against_singles("two replicas, both large again", lived, p, b, False, ["celllist", "celllist"])
    assert lived.stats(p)["algorithm"] == "allpairs"
    # inside step: a context that has stepped both replicas from their lists, then replica 1 shrinks
    lived = Forces(par, terms=WATER_TERMS, **okw)
    s = _system(N, 2, prec, p, b, vel[:2])
    lived.compute(s.pos, s.box, s.forces)
    integ = Integrator(s, lived, 1.0, _dev())
    integ.step(3)
    st = lived.stats(s.pos)
    assert st["algorithm"] == "celllist" and st["batched_launches"] >= 3, st
    p, b = _replica_state(pos, box, [1.0, 0.97], jitter, prec)
    ref = _oracle(par, p, b, WATER_TERMS, okw)
    s.box = b
    s.pos.copy_(p)
    s.vel.copy_(vel[:2].to(PREC[prec]).to(_dev()))
    s.forces.copy_(ref.forces.to(PREC[prec]).to(_dev()))
    out = integ.step(3)
    assert lived.stats(s.pos)["algorithm"] == "allpairs"
    for r in range(2):
        sr = _system(N, 1, prec, p[r : r + 1], b[r : r + 1].contiguous(), vel[r : r + 1], ref.forces[r : r + 1].to(PREC[prec]).to(_dev()))
        fr = Forces(par, terms=WATER_TERMS, **okw)
        integ_r = Integrator(sr, fr, 1.0, _dev())
        integ_r.step(3)
        po, vo, fo = _oracle_trajectory(par, p[r : r + 1], b[r : r + 1], vel[r : r + 1].to(PREC[prec]), ref.forces[r : r + 1].to(PREC[prec]),
                                        integ_r.masses, integ_r.dt, 3, okw)
        for k, o in (("pos", po), ("vel", vo), ("forces", fo)):
            LC.rule4(f"replica {r} of two, flip in step, {k}", getattr(s, k)[r : r + 1].cpu(), getattr(sr, k).cpu(), o)
        own = _oracle(par, s.pos[r : r + 1], s.box[r : r + 1], WATER_TERMS, okw)  # (at the run's own final positions)
        assert LC.force_distance(s.forces[r : r + 1].cpu(), own.forces) <= FTOL[prec]
    _check_kinetic("two replicas, flip in step", out, s, integ.masses, prec)


# ----------------------------------------------------------------------------- 4. atom swaps and back
@pytest.mark.timeout(180)
@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_atom_swaps_and_back(prec):
    """The mixture of tests/_oracle_sample.py (5 832 atoms; two of its three types share their LJ class and differ in charge, so
    the charges are no function of the class) -> 4 000 of its atoms with the charges made one per class and `nactive` = 2 500
    -> the same 4 000 with `nactive=None` -> the 5 832 again, in another order.  The context starts with per-atom skin weights
    (the masses differ); `update_atoms` releases them.  After every swap: a fresh context of the final parameters (for the
    passive stop: a fresh context given the same single swap — there is no other way to make rows passive), bit for bit, the
    force buffer pre-filled with NaN; `charge_by_class` flips 0 -> 1 -> 1 -> 0 in fp32 (the table is an fp32 kernel's).  What
    legitimately differs and does not show: `maxn_keep`, the capacity floor a swap leaves."""
    from _oracle_sample import mixed_system
    from test_gpu_passive_atoms import _local_par
    from test_gpu_passive_atoms import _oracle as passive_oracle
    from torchmd_amd.forces import Forces

    dt = PREC[prec]
    _, pos, box, par, terms = mixed_system(18, dt, seed=9)
    okw = dict(cutoff=9.0, rfa=True)
    n = len(pos)
    rows = (pos - np.floor(pos / box) * box).astype(np.float32 if prec == "f32" else np.float64).astype(np.float64)
    b = _box_tensor(box, prec)
    src = np.arange(n)
    rng = np.random.default_rng(3)

    def tensor(r):
        return torch.as_tensor(r, dtype=dt).to(_dev())[None].contiguous()

    lived = Forces(par, terms=terms, skin_weights="mass", **okw)
    p = tensor(rows)
    ref = _oracle(par, p, b, terms, okw)
    fresh = Forces(par, terms=terms, skin_weights="mass", **okw)
    LC.judge("atom swaps, start (per-atom skins)", _evaluate(lived, p, b), _evaluate(fresh, p, b), ref, prec, terms, bitwise=True)
    st = lived.stats(p)
    uniform = Forces(par, terms=terms, skin_weights=None, **okw)
    uniform.compute(p, b, torch.zeros_like(p))
    # (per-atom skins in place: the heavy atoms' pairs are listed within less than cutoff + skin, so the list is shorter)
    assert st["algorithm"] == "celllist" and st["list_entries"] < uniform.stats(p)["list_entries"], (st, uniform.stats(p))
    assert st["charge_by_class"] == 0
    by_class = 1 if prec == "f32" else 0

    # ---- 4 000 atoms, charges one per class, 2 500 of them active
    order = rng.permutation(n)[:4000]
    lp = _local_par(par, src, order)
    q = lp.charges.clone()
    q[q < 0] = -q[q < 0]  # (A2 carries -0.1 and shares A1's class: now +0.1 like A1)
    lp.charges = q
    k = 2500
    lived.update_atoms(lp, nactive=k)
    fresh = Forces(lp, terms=terms, skin_weights=None, **okw)
    r = rows[order]
    p = tensor(r)
    fresh._engine(p)
    fresh.update_atoms(lp, nactive=k)
    Fo, Eo = passive_oracle(lp, r, box, k, terms, {"rfa": True}, dt)
    full = torch.zeros(1, 4000, 3, dtype=torch.float64)
    full[0, :k] = Fo
    ref = LC.Result(npairs=None, energies=[Eo], forces=full)
    rl, rf = _evaluate(lived, p, b), _evaluate(fresh, p, b)
    LC.judge("atom swaps, 4 000 atoms of which 2 500 active", rl, rf, ref, prec, terms, bitwise=True, rows=slice(0, k), count_ref=False)
    for res in (rl, rf):
        for F in (res.forces, res.forces_only, res.extra["forces_second_compute"]):
            assert torch.equal(F[:, k:], torch.zeros_like(F[:, k:])), "passive rows"
    for name, f in (("lived", lived), ("fresh", fresh)):
        st = f.stats(p)
        assert st["algorithm"] == "celllist" and st["charge_by_class"] == by_class and abs(st["skin"] - 1.2) < 1e-9, (name, st)

    # ---- the same atoms, all active
    lived.update_atoms(lp, nactive=None)
    fresh = Forces(lp, terms=terms, skin_weights=None, **okw)
    ref = _oracle(lp, p, b, terms, okw)
    LC.judge("atom swaps, 4 000 atoms all active", _evaluate(lived, p, b), _evaluate(fresh, p, b), ref, prec, terms, bitwise=True)
    assert lived.stats(p)["charge_by_class"] == by_class and fresh.stats(p)["charge_by_class"] == by_class

    # ---- back to the 5 832, another order
    order = rng.permutation(n)
    lp = _local_par(par, src, order)
    lived.update_atoms(lp, nactive=None)
    fresh = Forces(lp, terms=terms, skin_weights=None, **okw)
    p = tensor(rows[order])
    ref = _oracle(lp, p, b, terms, okw)
    rl, rf = _evaluate(lived, p, b), _evaluate(fresh, p, b)
    LC.judge("atom swaps, back to 5 832 atoms", rl, rf, ref, prec, terms, bitwise=True)
    assert torch.isfinite(rl.forces).all() and torch.isfinite(rl.forces_only).all()
    for name, f in (("lived", lived), ("fresh", fresh)):
        st = f.stats(p)
        assert st["algorithm"] == "celllist" and st["charge_by_class"] == 0 and st["overflow"] == 0, (name, st)


# ----------------------------------------------------------------------------- 5. side terms re-set in place
def _water_restraints(pos, box, R, k=100.0):
    """Two position restraints with references displaced by 1 A and one O-O distance restraint across a face, every replica
    with a distance target of its own (the set of tests/test_gpu_restraints.py)."""
    from torchmd_amd.restraints import Restraints

    ox = np.arange(0, len(pos), 3)
    lo, hi = ox[np.argmin(pos[ox, 0])], ox[np.argmax(pos[ox, 0])]
    d = pos[lo] - pos[hi]
    assert np.any(np.rint(d / box) != 0)  # across a face
    rs = Restraints(R)
    a, c = int(ox[len(ox) // 3]), int(ox[2 * len(ox) // 3])
    rs.add_position([a, c], pos[[a, c]] + np.array([[1.0, 0.0, 0.0], [0.0, -0.6, 0.8]]), k)
    r = np.sqrt(np.sum((d - box * np.rint(d / box)) ** 2))
    rs.add_distance([[int(lo), int(hi)]], np.array([[r + 0.4 * (q + 1)] for q in range(R)]), k)
    return rs


def _restraint_side(rs):
    def side(pos, edges):
        E, F = rs.energy_forces(pos, edges)
        return E.sum(axis=1), F
    return side


@pytest.mark.timeout(180)
@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_restraints_reset_in_place_between_compute_and_step_calls(prec):
    """One `Restraints` object on the 2 187-atom water (cutoff 8.5 A, cell list), changed in place by `set_distance_targets`,
    `set_position_reference` and `set_strengths` — each bumps `version`, and `_Engine.side_seen` keyed on (id, version) makes
    the engine upload again — between `compute` calls and between `step` calls.  The same object is held by a second `Forces`
    (another cutoff, a context of its own): one change is seen by both.  After every change lived equals fresh bit for bit (the
    restraint kernel adds in a fixed order, tests/test_gpu_restraints.py) and both equal oracle + numpy model."""
    from torchmd_amd.forces import Forces
    from torchmd_amd.integrator import Integrator

    mol, pos, box, par, vel = _water(9, prec)
    N = mol.numAtoms
    rs = _water_restraints(pos, box, 1)
    side = _restraint_side(rs)
    okw, okw2 = dict(cutoff=8.5, rfa=True), dict(cutoff=8.0, rfa=True)
    lived, second = Forces(par, terms=WATER_TERMS, restraints=rs, **okw), Forces(par, terms=WATER_TERMS, restraints=rs, **okw2)
    p, b = torch.as_tensor(pos, dtype=PREC[prec]).to(_dev())[None].contiguous(), _box_tensor(box, prec)
    terms = WATER_TERMS + ["side"]

    def both(label):
        for f, kw in ((lived, okw), (second, okw2)):
            fresh = Forces(par, terms=WATER_TERMS, restraints=rs, **kw)
            ref = _oracle(par, p, b, WATER_TERMS, kw, side=side)
            assert ref.energies[0]["side"] > 1.0
            f.invalidate_lists(p)
            LC.judge(f"{label}, cutoff {kw['cutoff']}", _evaluate(f, p, b, "restraints"), _evaluate(fresh, p, b, "restraints"), ref, prec, terms,
                     bitwise=True)
            assert f.stats(p)["algorithm"] == "celllist"

    both("restraints as made")
    e0 = rs.energy_forces(pos[None], box)[0].copy()
    rs.set_distance_targets(rs.dist_r0 + 0.5)
    both("distance target moved")
    rs.set_position_reference(rs.pos_ref + np.array([0.0, 0.7, 0.0]))
    both("position reference moved")
    rs.set_strengths(position_k=40.0, distance_k=250.0)
    both("strengths changed")
    e1 = rs.energy_forces(pos[None], box)[0]
    assert np.abs(e1 - e0).min() > 1.0  # (every change changed the answer by far more than any bar)
    # ---- between step calls
    s = _system(N, 1, prec, p, b, vel[:1])
    lived.compute(s.pos, s.box, s.forces)
    integ = Integrator(s, lived, 1.0, _dev())
    fkw = dict(restraints=rs)
    fused = 0
    for leg, change in enumerate((lambda: None, lambda: rs.set_distance_targets(rs.dist_r0 - 0.3),
                                  lambda: rs.set_position_reference(rs.pos_ref + np.array([0.5, 0.0, 0.0])),
                                  lambda: rs.set_strengths(position_k=90.0, distance_k=60.0))):
        change()
        if leg:  # the forces in `s.forces` hold the restraint force of the old tables: the caller evaluates again, as run.py does
            lived.compute(s.pos, s.box, s.forces)
        out, fr, sf = _step_leg(f"restraints, step leg {leg}", par, WATER_TERMS, okw, fkw, lived, s, integ, 3, prec, side=side)
        _check_kinetic(f"restraints, step leg {leg}", out, s, integ.masses, prec)
        st = lived.stats(s.pos)
        assert st["algorithm"] == "celllist" and (st["steps_in_pair_launch"] >= fused + 1 if prec == "f32" else st["steps_in_pair_launch"] == 0), st
        fused = st["steps_in_pair_launch"]
        Er = rs.energy_forces(s.pos.cpu().double().numpy(), box)[0]
        assert np.allclose(lived._restraint_energy, Er, rtol=1e-5) and np.allclose(fr._restraint_energy, Er, rtol=1e-5)


@pytest.mark.timeout(120)
@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_one_forces_used_with_one_three_and_one_replicas(prec, monkeypatch):
    """A `Forces` keeps one engine per (device, dtype, R, exact).  R = 1, then R = 3, then R = 1 again with other positions and
    another box: the R = 1 engine has lived through the R = 3 use of its owner (`_box_cache`, `_side_potential`, the shared
    `Alchemical` whose `set_lambdas` both engines must `sync`).  Each use equals fresh single-replica contexts bit for bit
    (lanes per atom pinned: a three-replica fp32 context picks them from the atoms that share its launch).  References: at
    the partial coupling (0.6, 0) the oracle without the solute's pairs + the numpy model of tests/_alchemy.py; at (1, 1),
    where the soft-core pair is the plain pair, the plain oracle."""
    from torchmd_amd.alchemy import Alchemical
    from torchmd_amd.forces import Forces

    monkeypatch.setenv("TMDHIP_LPA", "16")
    mol, pos, box, par, vel = _water(9, prec)
    okw = dict(cutoff=8.5, rfa=True)
    solute = np.arange(30, 36)  # two whole waters
    al = Alchemical(solute, 0.6, 0.0)
    lived = Forces(par, terms=WATER_TERMS, alchemical=al, **okw)
    rng = np.random.default_rng(11)
    uses = ((1, [1.0], (1.0, 1.0)), (3, [1.0, 1.003, 0.998], ([1.0, 1.0, 1.0], [1.0, 1.0, 1.0])), (1, [1.002], (1.0, 1.0)))
    for use, (R, scales, lam) in enumerate(uses):
        jitter = [0.02 * rng.standard_normal(pos.shape) for _ in range(R)]
        p, b = _replica_state(pos, box, scales, jitter, prec)
        # first at partial coupling (the engines upload it), then re-set in place to full coupling, where the oracle is the reference
        al.set_lambdas(*(([0.6] * R, [0.0] * R) if R > 1 else (0.6, 0.0)))
        F = torch.full_like(p, float("nan"))
        partial = lived.compute(p, b, F, returnDetails=True)
        refp = _oracle(par, p, b, WATER_TERMS, okw, side=_alchemy_side(par, solute, 0.6, 0.0, okw, prec), drop=solute)
        dp = LC.force_distance(F.cpu(), refp.forces)
        print(f"use {use}: R = {R}, partial coupling [{prec}]: forces against oracle + model {dp:.3e}")
        assert dp <= FTOL[prec]
        for r in range(R):
            want = refp.energies[r]["side"]
            assert abs(partial[r]["alchemical"] - want) <= ERTOL[prec] * EFAC * max(1.0, abs(want)), (r, partial[r]["alchemical"], want)
        al.set_lambdas(*lam)
        ref = _oracle(par, p, b, WATER_TERMS, okw)
        rl = _evaluate(lived, p, b, count=False)
        singles = [Alchemical(solute, 1.0, 1.0) for _ in range(R)]
        rf = LC.stack([_evaluate(Forces(par, terms=WATER_TERMS, alchemical=singles[r], **okw), p[r : r + 1].contiguous(), b[r : r + 1].contiguous(),
                                 count=False) for r in range(R)])
        # the nonbonded energy of the solute's pairs is reported under "alchemical": compare the totals
        for res in (rl, rf):
            for d in res.energies:
                tot = sum(v for k2, v in d.items())
                d.clear()
                d["total"] = tot
        ref_tot = LC.Result(npairs=None, energies=[{"total": sum(e.values())} for e in ref.energies], forces=ref.forces)
        LC.judge(f"use {use}: R = {R}", rl, rf, ref_tot, prec, ["total"], bitwise=True)
        for r in range(R):
            assert abs(partial[r]["alchemical"]) > 1e-3 and lived.stats(p, r)["algorithm"] == "celllist"
        assert (F.cpu() - rl.forces).abs().max().item() > 1e-2  # (the partial coupling was really in force before the re-set)
    assert len(lived._engines) == 2


# ----------------------------------------------------------------------------- 6. features released and set again
@pytest.mark.timeout(180)
@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_restraints_pme_and_constraints_released_and_set_again(prec):
    """Through the C ABI, on the 2 187-atom water: enable -> evaluate and step -> release -> evaluate and step -> enable with
    OTHER parameters.  After the release the context equals one that never had the feature, after the re-enable a fresh one
    with the new parameters, bit for bit.
    * tmdhip_set_restraints (`enable = 0`, what an empty `Restraints` uploads);
    * tmdhip_set_pme (`enable = 0`): the fp32 context gets its fused step back (asserted: steps_in_pair_launch grows again,
      and did not while PME was on); PME on: the reference is tests/_ewald.py's host PME for the electrostatics + the oracle for
      the rest; in fp32 at the bars tests/test_gpu_pme.py holds fp32 PME to (forces 5e-3, energy 2e-5 of the self term);
    * tmdhip_set_constraints (`enable = 0`, what `Integrator(constraints=None)` sends after `constraints="water"`), then
      rigid waters again with every length 1 % longer (another descriptor): the constrained steps are compared lived
      against fresh, their forces against the oracle and their bonds against the bar of tests/test_gpu_constraints.py.
    The other setters with a release have tests of their own below (tmdhip_set_gb, _set_alchemical, _set_metadynamics,
    _set_vsites); tmdhip_set_molecules has no release — a table is only ever replaced — and no leg."""
    import _ewald as E
    from test_gpu_constraints import CONS_TOL
    from torchmd_amd import _lib as L
    from torchmd_amd.forces import Forces
    from torchmd_amd.integrator import Integrator
    from torchmd_amd.restraints import Restraints

    mol, pos, box, par, vel = _water(9, prec)
    N = mol.numAtoms
    p, b = torch.as_tensor(pos, dtype=PREC[prec]).to(_dev())[None].contiguous(), _box_tensor(box, prec)
    okw = dict(cutoff=8.5, rfa=True)

    # ---- restraints
    rs = _water_restraints(pos, box, 1)
    lived = Forces(par, terms=WATER_TERMS, restraints=rs, **okw)
    s = _system(N, 1, prec, p, b, vel[:1])
    lived.compute(s.pos, s.box, s.forces)
    integ = Integrator(s, lived, 1.0, _dev())
    _step_leg("restraints on", par, WATER_TERMS, okw, dict(restraints=rs), lived, s, integ, 3, prec, side=_restraint_side(rs))
    eng = lived._engine(p)
    off = Restraints(1)
    d, keep = off.descriptor()
    assert d.enable == 0
    L.check(eng.lib.tmdhip_set_restraints(eng.ctx, C.byref(d)), "tmdhip_set_restraints")
    eng.side_seen["restraints"] = (id(rs), rs.version)  # (the Python layer keeps believing its tables are in place: the C release alone is under test)
    ref = _oracle(par, p, b, WATER_TERMS, okw)
    never = Forces(par, terms=WATER_TERMS, **okw)
    lived.invalidate_lists(p)
    rl, rf = _evaluate(lived, p, b), _evaluate(never, p, b)
    assert all(d["restraints"] == 0.0 for d in rl.energies)
    for d in rl.energies:
        d.pop("restraints")
    LC.judge("restraints released", rl, rf, ref, prec, WATER_TERMS, bitwise=True)
    lived.compute(s.pos, s.box, s.forces)
    _step_leg("restraints released", par, WATER_TERMS, okw, {}, lived, s, integ, 3, prec)
    rs2 = _water_restraints(pos, box, 1, k=35.0)
    rs2.set_distance_targets(rs2.dist_r0 + 0.8)
    d, keep = rs2.descriptor()
    L.check(eng.lib.tmdhip_set_restraints(eng.ctx, C.byref(d)), "tmdhip_set_restraints")
    fresh = Forces(par, terms=WATER_TERMS, restraints=rs2, **okw)
    ref = _oracle(par, p, b, WATER_TERMS, okw, side=_restraint_side(rs2))
    lived.invalidate_lists(p)
    LC.judge("restraints set again with other tables", _evaluate(lived, p, b, "restraints"), _evaluate(fresh, p, b, "restraints"), ref, prec,
             WATER_TERMS + ["side"], bitwise=True)

    # ---- PME
    def pme_energy(label, rl, rf, eh, beta):
        """The PME total is what is left of parts as large as the self term: tests/test_gpu_pme.py's bound (1e-10 of the total, or
        1e-12 of the self term where the total is below a hundredth of it) for each context, rule 4 between them."""
        eself = abs(E.self_and_background(par.charges.double().cpu().numpy(), box, beta))
        bound = 1e-10 * abs(eh) if abs(eh) > 1e-2 * eself else 1e-12 * eself
        if prec == "f32":  # (test_fp32_against_fp64 there: 2e-5 of the larger of the total and the self term)
            bound = 2e-5 * max(abs(eh), eself)
        el, ef = rl.energies[0]["electrostatics"], rf.energies[0]["electrostatics"]
        print(f"{label}: electrostatics lived {el!r}, fresh {ef!r}, host PME {eh!r} (self term {eself:.3e}, bound {bound:.2e})")
        assert abs(el - eh) <= bound and abs(ef - eh) <= bound and abs(el - ef) <= 2.0 * abs(ef - eh)

    pkw = dict(cutoff=8.5)
    lived = Forces(par, terms=WATER_TERMS, pme=True, pme_grid=(32, 32, 32), **pkw)
    fresh = Forces(par, terms=WATER_TERMS, pme=True, pme_grid=(32, 32, 32), **pkw)
    rl, rf = _evaluate(lived, p, b), _evaluate(fresh, p, b)
    assert lived.stats(p)["pme_evaluations"] > 0 and lived.stats(p)["algorithm"] == "celllist"
    assert torch.equal(rl.forces, rf.forces) and torch.equal(rl.forces_only, rf.forces_only) and rl.npairs == rf.npairs
    # (the host PME of the positions the device holds; fp32: the force bar tests/test_gpu_pme.py holds fp32 PME to)
    pme_ftol = None if prec == "f64" else 5e-3
    hpos = p[0].cpu().double().numpy()
    plain = _oracle(par, p, b, ["lj", "bonds", "angles"], pkw)
    q = par.charges.double().cpu().numpy()
    excl = [tuple(x) for x in par.get_exclusions(("bonds", "angles", "1-4"))]
    eh, fh = E.pme(hpos, q, box, lived.ewald_beta, 8.5, lived.pme_grid, lived.pme_order, excl, pairs="kdtree")
    ref = LC.Result(npairs=None, energies=[dict(plain.energies[0], electrostatics=eh)], forces=plain.forces + torch.as_tensor(fh)[None])
    pme_energy("PME on", rl, rf, eh, lived.ewald_beta)
    LC.judge("PME on", rl, rf, ref, prec, ["lj", "bonds", "angles"], bitwise=True, count_ref=False, ftol=pme_ftol)
    s = _system(N, 1, prec, p, b, vel[:1], rl.forces.to(_dev()))
    integ = Integrator(s, lived, 1.0, _dev())
    integ.step(3)
    assert lived.stats(s.pos)["steps_in_pair_launch"] == 0  # (PME contexts step with the separate kernels)
    eng = lived._engine(p)
    pd = L.PmeDesc()
    pd.struct_size = C.sizeof(L.PmeDesc)
    pd.enable = 0
    L.check(eng.lib.tmdhip_set_pme(eng.ctx, C.byref(pd)), "tmdhip_set_pme")
    never = Forces(par, terms=WATER_TERMS, **pkw)
    ref = _oracle(par, p, b, WATER_TERMS, pkw)
    n_pme = lived.stats(p)["pme_evaluations"]
    lived.invalidate_lists(p)
    LC.judge("PME released", _evaluate(lived, p, b), _evaluate(never, p, b), ref, prec, WATER_TERMS, bitwise=True)
    assert lived.stats(p)["pme_evaluations"] == n_pme
    s.pos.copy_(p)
    s.vel.copy_(vel[:1].to(PREC[prec]).to(_dev()))
    lived.compute(s.pos, s.box, s.forces)
    _step_leg("PME released", par, WATER_TERMS, pkw, {}, lived, s, integ, 3, prec)
    if prec == "f32":
        assert lived.stats(s.pos)["steps_in_pair_launch"] >= 1
    pd.enable, pd.beta, pd.order = 1, lived.ewald_beta * 1.1, 4
    pd.grid[:] = (30, 30, 30)
    L.check(eng.lib.tmdhip_set_pme(eng.ctx, C.byref(pd)), "tmdhip_set_pme")
    fresh = Forces(par, terms=WATER_TERMS, pme=True, pme_grid=(30, 30, 30), pme_order=4, **pkw)
    fresh.ewald_beta = lived.ewald_beta * 1.1
    lived.invalidate_lists(p)
    rl, rf = _evaluate(lived, p, b), _evaluate(fresh, p, b)
    assert torch.equal(rl.forces, rf.forces) and torch.equal(rl.forces_only, rf.forces_only) and rl.npairs == rf.npairs
    eh, fh = E.pme(hpos, q, box, fresh.ewald_beta, 8.5, (30, 30, 30), 4, excl, pairs="kdtree")
    ref = LC.Result(npairs=None, energies=[dict(plain.energies[0], electrostatics=eh)], forces=plain.forces + torch.as_tensor(fh)[None])
    pme_energy("PME set again", rl, rf, eh, fresh.ewald_beta)
    LC.judge("PME set again with another grid, order and beta", rl, rf, ref, prec, ["lj", "bonds", "angles"], bitwise=True, count_ref=False,
             ftol=pme_ftol)

    # ---- constraints
    lived = Forces(par, terms=WATER_TERMS, **okw)
    s = _system(N, 1, prec, p, b, vel[:1])
    lived.compute(s.pos, s.box, s.forces)

    def constrained(scale, label):
        """Rigid waters whose lengths are `scale` x the force field's: the descriptor tmdhip_set_constraints gets is made from
        the integrator's ConstraintSet, lengths included (the start is SHAKEn onto them on the host, as for any rigid start)."""
        integ = Integrator(s, lived, 1.0, _dev(), constraints="water")
        fresh = Forces(par, terms=WATER_TERMS, **okw)
        sf = _system(N, 1, prec, s.pos, s.box, s.vel, s.forces)
        integ_f = Integrator(sf, fresh, 1.0, _dev(), constraints="water")
        for i in (integ, integ_f):
            i.constraints.water_dist = np.ascontiguousarray(i.constraints.water_dist * scale)
        lived.invalidate_lists(s.pos)
        integ.step(3)
        integ_f.step(3)
        ref = _oracle(par, s.pos, s.box, WATER_TERMS, okw)
        dl = LC.force_distance(s.forces.cpu(), ref.forces)
        x = s.pos[0].cpu().double().numpy()
        bp = par.bond_params  # (O-H1, O-H2 and H1-H2 of every water, with the lengths the constraint finder reads)
        idx, r0 = bp["idx"].numpy(), bp["params"][bp["map"][:, 1]][:, 1].double().numpy()
        dev_bond = np.abs(np.linalg.norm(x[idx[:, 0]] - x[idx[:, 1]], axis=1) / (scale * r0) - 1.0).max()
        print(f"{label} [{prec}]: forces left against the oracle {dl:.3e}, worst relative bond-length error {dev_bond:.2e}")
        assert dl <= FTOL[prec]
        assert dev_bond <= CONS_TOL[prec][0]  # (the bond-length bar of tests/test_gpu_constraints.py)
        for k in ("pos", "vel", "forces"):
            assert torch.equal(getattr(s, k), getattr(sf, k)), (label, k)

    constrained(1.0, "constraints: rigid water")
    integ = Integrator(s, lived, 1.0, _dev())  # constraints=None: `_md_run` releases them (tmdhip_set_constraints, enable = 0)
    _step_leg("constraints released", par, WATER_TERMS, okw, {}, lived, s, integ, 3, prec)
    assert lived._engine(s.pos)._constraints is None
    if prec == "f32":
        assert lived.stats(s.pos)["steps_in_pair_launch"] >= 1
    constrained(1.01, "constraints set again: rigid water, every length 1 % longer")


# ----------------------------------------------------------------------------- 7. callers taking turns
@pytest.mark.timeout(180)
@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_callers_take_turns_on_one_forces(prec):
    """The order run.py uses and a few it does not, on one `Forces` and one `System` (2 187-atom water, cutoff 8.5 A):
    minimize_fire -> compute -> step -> pressure() -> step -> compute -> a second Integrator on the same objects -> step after
    the caller overwrote `system.vel` in place (same pointer: `ke_from_run` is pointer-keyed and must not answer for the old
    velocities).  Each leg equals the same call on a fresh context given the state the previous leg left, bit for bit; the
    lived lists are dropped before each leg so that both build theirs where the leg starts."""
    from torchmd_amd.forces import Forces
    from torchmd_amd.integrator import Integrator
    from torchmd_amd.minimizers import minimize_fire

    mol, pos, box, par, vel = _water(9, prec)
    N = mol.numAtoms
    okw = dict(cutoff=8.5, rfa=True)
    p, b = torch.as_tensor(pos, dtype=PREC[prec]).to(_dev())[None].contiguous(), _box_tensor(box, prec)
    lived = Forces(par, terms=WATER_TERMS, **okw)
    s = _system(N, 1, prec, p, b, vel[:1])

    def fresh_copy():
        return Forces(par, terms=WATER_TERMS, **okw), _system(N, 1, prec, s.pos, s.box, s.vel, s.forces)

    # minimize_fire
    fr, sf = fresh_copy()
    res_l, res_f = minimize_fire(s, lived, fmax=0.5, steps=20, check_every=10), minimize_fire(sf, fr, fmax=0.5, steps=20, check_every=10)
    assert res_l.iterations[0] == 20 and res_f.iterations[0] == 20
    ref = _oracle(par, s.pos, s.box, WATER_TERMS, okw)
    dl, df = LC.force_distance(s.forces.cpu(), ref.forces), LC.force_distance(sf.forces.cpu(), ref.forces)
    print(f"minimize_fire [{prec}]: forces left against the oracle: lived {dl:.3e}, fresh {df:.3e}; fmax {res_l.fmax} / {res_f.fmax}")
    assert dl <= FTOL[prec] and df <= FTOL[prec]
    assert torch.equal(s.pos, sf.pos) and torch.equal(s.forces, sf.forces) and np.array_equal(res_l.fmax, res_f.fmax)
    assert (s.pos - p).abs().max().item() > 1e-3  # (it moved)

    def compute_leg(label):
        fr, _ = fresh_copy()
        lived.invalidate_lists(s.pos)
        pp = s.pos.clone()
        LC.judge(label, _evaluate(lived, pp, s.box), _evaluate(fr, pp, s.box), _oracle(par, pp, s.box, WATER_TERMS, okw), prec, WATER_TERMS, bitwise=True)

    compute_leg("compute after minimize_fire")
    lived.compute(s.pos, s.box, s.forces)
    integ = Integrator(s, lived, 1.0, _dev())
    out, _, _ = _step_leg("step after compute", par, WATER_TERMS, okw, {}, lived, s, integ, 4, prec)
    _check_kinetic("step after compute", out, s, integ.masses, prec)
    # pressure(): a fresh context on the same state gives the same number, and the step behind it is the step a fresh context makes
    fr, sf = fresh_copy()
    lived.invalidate_lists(s.pos)
    P_l, P_f = integ.pressure(), Integrator(sf, fr, 1.0, _dev()).pressure()
    print(f"pressure() [{prec}]: lived {P_l}, fresh {P_f}")
    assert np.isfinite(P_l).all() and np.array_equal(P_l, P_f)
    out, _, _ = _step_leg("step after pressure()", par, WATER_TERMS, okw, {}, lived, s, integ, 4, prec, rebuild=True)
    compute_leg("compute after step")
    integ2 = Integrator(s, lived, 1.0, _dev())
    out, _, _ = _step_leg("step of a second Integrator", par, WATER_TERMS, okw, {}, lived, s, integ2, 3, prec)
    _check_kinetic("step of a second Integrator", out, s, integ2.masses, prec)
    K_before = _kinetic(s, integ2.masses)
    ptr = s.vel.data_ptr()
    s.vel.mul_(0.5)  # the caller overwrites the velocities, in place
    assert s.vel.data_ptr() == ptr
    out, _, _ = _step_leg("step after the velocities were overwritten", par, WATER_TERMS, okw, {}, lived, s, integ, 3, prec)
    _check_kinetic("step after the velocities were overwritten", out, s, integ.masses, prec)
    assert out[0][0] < 0.6 * K_before[0]  # (a quarter of the old kinetic energy, plus what three steps add)
    st = lived.stats(s.pos)
    assert st["algorithm"] == "celllist" and st["ncell"] == (5, 5, 5) and st["overflow"] == 0
    # (every leg's first step builds the list: 2 + 2 + 1 + 1 interior steps were made by pair launches)
    assert st["steps_in_pair_launch"] >= 6 if prec == "f32" else st["steps_in_pair_launch"] == 0, st


# ----------------------------------------------------------------------------- 8. a refused call leaves no trace
@pytest.mark.timeout(120)
@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_python_refusals_leave_no_trace(prec):
    """ValueErrors of the Python layer, the kind that launch nothing, each followed by a good call that equals a fresh
    context's: a generalized-Born context given a non-zero box (65-atom cluster of tests/test_gpu_gb.py, reference: its
    model at its bars), `pme=True` with a zero box, a metadynamics bias made for two replicas given one."""
    import test_gpu_gb as GB
    from torchmd_amd.forces import Forces
    from torchmd_amd.metadynamics import Metadynamics

    # generalized Born
    cpos, q, rad, sc = GB._replica_clusters(65, 1, prec)
    lived = Forces(GB._ClusterPar(q, PREC[prec]), terms=[], implicit_solvent=GB._gb(rad, sc))
    p = torch.as_tensor(cpos, dtype=PREC[prec]).to(_dev()).contiguous()
    zero, bad = _box_tensor(np.zeros(3), prec), _box_tensor(np.array([30.0, 30.0, 30.0]), prec)
    F0 = torch.full_like(p, float("nan"))
    d0 = lived.compute(p, zero, F0, returnDetails=True)
    Fbad = torch.full_like(p, 7.0)
    with pytest.raises(ValueError, match="open boundaries"):
        lived.compute(p, bad, Fbad, returnDetails=True)
    assert (Fbad == 7.0).all()
    F1 = torch.full_like(p, float("nan"))
    d1 = lived.compute(p, zero, F1, returnDetails=True)
    GB._check_against_model("GB after a refused box", lived, p, F1, d1, GB._model(65, 1, prec), prec)
    f2, p2, _, F2, d2 = GB._evaluate(65, 1, prec)
    assert torch.equal(F1, F0) and torch.equal(F1, F2) and d1[0]["implicit_solvent"] == d0[0]["implicit_solvent"] == d2[0]["implicit_solvent"]
    assert lived.stats(p)["algorithm"] == "allpairs"

    # PME with a zero box
    mol, pos, box, par, vel = _water(9, prec)
    pw, bw = torch.as_tensor(pos, dtype=PREC[prec]).to(_dev())[None].contiguous(), _box_tensor(box, prec)
    pkw = dict(cutoff=8.5, pme=True, pme_grid=(32, 32, 32))
    lived, fresh = Forces(par, terms=WATER_TERMS, **pkw), Forces(par, terms=WATER_TERMS, **pkw)
    with pytest.raises(ValueError, match="periodic box"):
        lived.compute(pw, _box_tensor(np.zeros(3), prec), torch.zeros_like(pw))
    assert lived.pme_grid == (32, 32, 32)
    rl, rf = _evaluate(lived, pw, bw), _evaluate(fresh, pw, bw)
    assert rl.npairs == rf.npairs and torch.equal(rl.forces, rf.forces) and torch.equal(rl.forces_only, rf.forces_only)
    assert LC.energy_distance(rl.energies, rf.energies, WATER_TERMS) <= 1e-12
    assert lived.stats(pw)["pme_evaluations"] == fresh.stats(pw)["pme_evaluations"] > 0 and lived.stats(pw)["algorithm"] == "celllist"

    # a bias made for two replicas
    okw = dict(cutoff=8.5, rfa=True)

    def bias():
        return Metadynamics(("distance", (0, 3)), sigma=0.2, height=0.3, frequency=5, temperature=300.0, grid_min=1.0, grid_max=12.0, nreplicas=2)

    lived = Forces(par, terms=WATER_TERMS, metadynamics=bias(), **okw)
    with pytest.raises(ValueError, match="2 replicas"):
        lived.compute(pw, bw, torch.zeros_like(pw))
    rng = np.random.default_rng(2)
    p2, b2 = _replica_state(pos, box, [1.0, 1.001], [0.02 * rng.standard_normal(pos.shape) for _ in range(2)], prec)
    fresh = Forces(par, terms=WATER_TERMS, metadynamics=bias(), **okw)
    ref = _oracle(par, p2, b2, WATER_TERMS, okw, side=lambda x, e: (np.zeros(2), np.zeros_like(x)))  # (no hill yet: the bias is zero)
    LC.judge("a two-replica bias after it was offered one replica", _evaluate(lived, p2, b2, "metadynamics"), _evaluate(fresh, p2, b2, "metadynamics"),
             ref, prec, WATER_TERMS + ["side"], bitwise=True)
    assert lived.stats(p2)["algorithm"] == "celllist" and len(lived._engines) == 2


def _md_desc(s, masses, boxes, niter, dt, gamma=0.0, vcoeff=None, energies=None):
    from torchmd_amd import _lib as L

    d = L.MdDesc()
    d.struct_size = C.sizeof(L.MdDesc)
    d.niter, d.pos_dev, d.vel_dev, d.forces_dev = niter, s.pos.data_ptr(), s.vel.data_ptr(), s.forces.data_ptr()
    d.mass_dev, d.box_host, d.dt, d.gamma = masses.data_ptr(), boxes.ctypes.data_as(C.c_void_p), dt, gamma
    d.vcoeff_dev = vcoeff.data_ptr() if vcoeff is not None else None
    d.energies_dev = energies.data_ptr() if energies is not None else None
    return d


@pytest.mark.timeout(120)
@pytest.mark.parametrize("nside", [12, 9], ids=["5184-atoms-kernel-snapshot", "2187-atoms-copied-snapshot"])
@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_restore_after_a_refused_run_is_refused(prec, nside):
    """At the C level: a good tmdhip_md_run of 4 steps (cell-list context: it saves the state at entry), then a tmdhip_md_run
    that a side term refuses before its first kernel (restraints: 1 - gamma dt <= 0), then tmdhip_md_restore.  The restore
    answers for the LAST run, which saved nothing: it must return an error ("no saved state of a matching tmdhip_md_run") and
    leave positions, velocities and forces untouched.  Before the fix in md_loop.hip `snap_bytes` was set before the run and
    never cleared: with 5 184 atoms (16-byte aligned arrays: a kernel of the run takes the snapshot, and the refused run has
    none) the restore returned 0 and wrote the FIRST run's entry state over the current one; with 2 187 atoms (three copies,
    enqueued before the run was looked at) it returned 0 and put back the state the refused run was offered.  After the
    refusal a good run equals the same run on a fresh context."""
    from torchmd_amd import _lib as L
    from torchmd_amd.forces import Forces
    from torchmd_amd.integrator import Integrator

    mol, pos, box, par, vel = _water(nside, prec)
    assert (mol.numAtoms * 3 * (4 if prec == "f32" else 8)) % 16 == (0 if nside == 12 else 4 if prec == "f32" else 8)
    N = mol.numAtoms
    okw = dict(cutoff=8.5, rfa=True)
    rs = _water_restraints(pos, box, 1)
    lived = Forces(par, terms=WATER_TERMS, restraints=rs, **okw)
    p, b = torch.as_tensor(pos, dtype=PREC[prec]).to(_dev())[None].contiguous(), _box_tensor(box, prec)
    s = _system(N, 1, prec, p, b, vel[:1])
    lived.compute(s.pos, s.box, s.forces)
    integ = Integrator(s, lived, 1.0, _dev())
    entry = {k: getattr(s, k).clone() for k in ("pos", "vel", "forces")}
    integ.step(4)
    assert lived.stats(s.pos)["algorithm"] == "celllist"
    torch.cuda.synchronize()
    after = {k: getattr(s, k).clone() for k in ("pos", "vel", "forces")}
    assert (after["pos"] - entry["pos"]).abs().max().item() > 1e-3
    eng = lived._engine(s.pos)
    boxes = np.ascontiguousarray(_edges(s.box))
    d = _md_desc(s, integ.masses, boxes, 2, 0.5, gamma=2.0, vcoeff=integ.masses)
    assert eng.lib.tmdhip_md_run(eng.ctx, C.byref(d), _stream()) < 0 and "1 - gamma dt" in L.last_error()
    rc = eng.lib.tmdhip_md_restore(eng.ctx, C.byref(d), _stream())
    torch.cuda.synchronize()
    for k in after:
        assert torch.equal(getattr(s, k), after[k]), (k, "the restore wrote over the state", rc)
    assert rc < 0 and "no saved state of a matching tmdhip_md_run" in L.last_error(), (rc, L.last_error())
    out, _, _ = _step_leg("good run after the refused one", par, WATER_TERMS, okw, dict(restraints=rs), lived, s, integ, 4, prec, side=_restraint_side(rs))
    _check_kinetic("good run after the refused one", out, s, integ.masses, prec)


@pytest.mark.timeout(120)
@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_restore_after_a_good_run_replays_it_like_a_fresh_context(prec):
    """The other side of the restore: after a good run of 8 steps tmdhip_md_restore (through `_step_body(replay=True)`, as the
    integrator calls it after a list failure) puts the entry state back and the repeated batch ends in the same bits as the
    first pass and as a fresh context's run from the entry state — the restore drops the lists (`rp.box[0] = -1`), so the
    replay builds its list at the restored positions as the fresh context does; a list kept from the end of the first pass
    would be valid and sum in another order.  Asserted: the replay rebuilt (n_rebuilds)."""
    from torchmd_amd.forces import Forces
    from torchmd_amd.integrator import Integrator

    mol, pos, box, par, vel = _water(9, prec)
    N = mol.numAtoms
    okw = dict(cutoff=8.5, rfa=True)
    lived = Forces(par, terms=WATER_TERMS, **okw)
    p, b = torch.as_tensor(pos, dtype=PREC[prec]).to(_dev())[None].contiguous(), _box_tensor(box, prec)
    s = _system(N, 1, prec, p, b, vel[:1])
    lived.compute(s.pos, s.box, s.forces)
    fresh, sf = Forces(par, terms=WATER_TERMS, **okw), _system(N, 1, prec, s.pos, s.box, s.vel, s.forces)
    integ = Integrator(s, lived, 1.0, _dev())
    lived.invalidate_lists(s.pos)
    out1 = integ.step(8)
    first = {k: getattr(s, k).clone() for k in ("pos", "vel", "forces")}
    r0 = lived.stats(s.pos)["n_rebuilds"]
    out2 = integ._step_body(8, replay=True)
    assert lived.stats(s.pos)["n_rebuilds"] > r0, "the replay did not rebuild its list at the restored positions"
    out_f = Integrator(sf, fresh, 1.0, _dev()).step(8)
    ref = _oracle(par, s.pos, s.box, WATER_TERMS, okw)
    dl, df = LC.force_distance(s.forces.cpu(), ref.forces), LC.force_distance(sf.forces.cpu(), ref.forces)
    print(f"replay [{prec}]: forces left against the oracle: replay {dl:.3e}, fresh {df:.3e}; Ekin {out1[0]} / {out2[0]} / {out_f[0]}")
    assert dl <= FTOL[prec] and df <= FTOL[prec]
    for k in first:
        assert torch.equal(getattr(s, k), first[k]), (k, "replay against the first pass")
        assert torch.equal(getattr(s, k), getattr(sf, k)), (k, "replay against a fresh context")
    assert np.array_equal(out1[0], out2[0]) and np.array_equal(out2[0], out_f[0])
    _check_kinetic("replay", out2, s, integ.masses, prec)


# ----------------------------------------------------------------------------- 5 / 6, the other side terms
def _alchemy_side(par, solute, lv, le, okw, prec):
    """`side` of `_oracle` for a solute coupled at (lv, le): the numpy model of tests/_alchemy.py (cross + intra energy, force),
    on top of an oracle that leaves every pair of the solute out (`drop=solute`): what the engine of a `Forces(alchemical=)`
    evaluates."""
    import _alchemy as AM
    from oracle import torchmd_oracle as orc

    A, B = (t.detach().cpu().double().numpy() for t in par.get_AB())
    q = par.charges.detach().cpu().double().numpy().reshape(-1)
    cls = par.mapped_atom_types.detach().cpu().numpy()
    excl = orc.exclusion_pairs(par)

    def side(pos, edges):
        lvs, les = np.broadcast_to(np.atleast_1d(lv), (len(pos),)), np.broadcast_to(np.atleast_1d(le), (len(pos),))
        out = [AM.evaluate(pos[r], edges[r], solute, q, cls, A, B, float(lvs[r]), float(les[r]), alpha=0.5, cutoff=okw["cutoff"],
                           switch_dist=okw.get("switch_dist"), rfa=okw.get("rfa", False), reference_switch=True, excl=excl,
                           dtype=np.float32 if prec == "f32" else np.float64) for r in range(len(pos))]
        return np.array([o["E_lj"] + o["E_el"] + o["E_intra"] for o in out]), np.stack([o["F"] for o in out])

    return side


@pytest.mark.timeout(180)
@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_alchemical_lambdas_between_steps_then_released_and_set_again(prec):
    """Two waters of the 2 187-atom box as the solute.  `Alchemical.set_lambdas` between `step` calls: (0.6, 0) -> (1, 1) ->
    (0.25, 0) -> (0, 0); each leg equals a fresh `Forces` with a fresh `Alchemical` at those couplings bit for bit (the
    alchemical kernels add in a fixed order: tests/test_gpu_alchemy.py), and the forces it leaves equal oracle (without the
    solute's pairs) + the numpy model of tests/_alchemy.py.  Then through the C ABI: tmdhip_set_alchemical with `enable = 0` —
    the context equals one whose engine was never handed the solute (the Python layer keeps its solute in a charge-free class
    of its own either way, so that is the context that never had the feature), reference: the oracle without the solute's
    pairs — and set again with other couplings and another alpha."""
    from torchmd_amd import _lib as L
    from torchmd_amd.alchemy import Alchemical
    from torchmd_amd.forces import Forces
    from torchmd_amd.integrator import Integrator

    mol, pos, box, par, vel = _water(9, prec)
    N = mol.numAtoms
    okw = dict(cutoff=8.5, rfa=True)
    solute = np.arange(30, 36)
    p, b = torch.as_tensor(pos, dtype=PREC[prec]).to(_dev())[None].contiguous(), _box_tensor(box, prec)
    al = Alchemical(solute, 0.6, 0.0)
    lived = Forces(par, terms=WATER_TERMS, alchemical=al, **okw)
    s = _system(N, 1, prec, p, b, vel[:1])
    integ = Integrator(s, lived, 1.0, _dev())
    terms = WATER_TERMS + ["side"]
    fused = 0
    for lv, le in ((0.6, 0.0), (1.0, 1.0), (0.25, 0.0), (0.0, 0.0)):
        al.set_lambdas(lv, le)
        side = _alchemy_side(par, solute, lv, le, okw, prec)
        ref = _oracle(par, s.pos, s.box, WATER_TERMS, okw, side=side, drop=solute)
        fresh = Forces(par, terms=WATER_TERMS, alchemical=Alchemical(solute, lv, le), **okw)
        lived.invalidate_lists(s.pos)
        pp = s.pos.clone()
        rl, rf = _evaluate(lived, pp, s.box, "alchemical", count=False), _evaluate(fresh, pp, s.box, "alchemical", count=False)
        LC.judge(f"lambdas ({lv}, {le}) between compute calls", rl, rf, ref, prec, terms, bitwise=True)
        s.forces.copy_(rl.forces.to(_dev()))  # (the forces of the new couplings: the caller evaluates again, as run.py does)
        out, fr, sf = _step_leg(f"lambdas ({lv}, {le}) between step calls", par, WATER_TERMS, okw, dict(alchemical=Alchemical(solute, lv, le)),
                                lived, s, integ, 3, prec, side=side, drop=solute)
        _check_kinetic(f"lambdas ({lv}, {le})", out, s, integ.masses, prec)
        st = lived.stats(s.pos)
        assert st["algorithm"] == "celllist" and st["steps_in_pair_launch"] - fused == fr.stats(sf.pos)["steps_in_pair_launch"], (st, fr.stats(sf.pos))
        fused = st["steps_in_pair_launch"]
    # ---- released through the C ABI
    eng = lived._engine(s.pos)
    d = L.AlchemicalDesc()
    d.struct_size = C.sizeof(L.AlchemicalDesc)
    d.enable = 0
    L.check(eng.lib.tmdhip_set_alchemical(eng.ctx, C.byref(d)), "tmdhip_set_alchemical")  # (side_seen stays: no upload behind our back)
    never_al = Alchemical(solute, 1.0, 1.0)
    never = Forces(par, terms=WATER_TERMS, alchemical=never_al, **okw)
    never._engine(s.pos).side_seen["alchemical"] = (id(never_al), never_al.version)  # its engine is never handed the solute
    ref = _oracle(par, s.pos, s.box, WATER_TERMS, okw, drop=solute)
    lived.invalidate_lists(s.pos)
    pp = s.pos.clone()
    rl, rf = _evaluate(lived, pp, s.box, count=False), _evaluate(never, pp, s.box, count=False)
    assert all(e["alchemical"] == 0.0 for e in rl.energies + rf.energies)
    LC.judge("alchemical released", rl, rf, ref, prec, WATER_TERMS, bitwise=True)
    s.forces.copy_(rl.forces.to(_dev()))
    sf = _system(N, 1, prec, s.pos, s.box, s.vel, s.forces)
    lived.invalidate_lists(s.pos)
    never.invalidate_lists(sf.pos)  # (it has evaluated above: both build their lists inside the run)
    out_l, out_f = integ.step(3), Integrator(sf, never, 1.0, _dev()).step(3)
    ref = _oracle(par, s.pos, s.box, WATER_TERMS, okw, drop=solute)
    dl = LC.force_distance(s.forces.cpu(), ref.forces)
    print(f"alchemical released, step(3) [{prec}]: forces left against the oracle without the solute's pairs {dl:.3e}")
    assert dl <= FTOL[prec]
    for k in ("pos", "vel", "forces"):
        assert torch.equal(getattr(s, k), getattr(sf, k)), ("alchemical released", k)
    assert np.array_equal(out_l[0], out_f[0])
    if prec == "f32":  # the released context steps inside its pair launch like one that never had the solute
        assert lived.stats(s.pos)["steps_in_pair_launch"] - fused == never.stats(sf.pos)["steps_in_pair_launch"] >= 1
    # ---- set again, other couplings and another alpha
    al2 = Alchemical(solute, 0.4, 0.0, alpha=0.3)
    lived.alchemical = al2
    side2 = _alchemy_side(par, solute, 0.4, 0.0, okw, prec)
    fresh = Forces(par, terms=WATER_TERMS, alchemical=Alchemical(solute, 0.4, 0.0, alpha=0.3), **okw)
    pp = s.pos.clone()
    lived.invalidate_lists(pp)

    def side_alpha(x, e):  # (the model at alpha = 0.3)
        import _alchemy as AM
        from oracle import torchmd_oracle as orc

        A, B = (t.detach().cpu().double().numpy() for t in par.get_AB())
        o = AM.evaluate(x[0], e[0], solute, par.charges.detach().cpu().double().numpy().reshape(-1), par.mapped_atom_types.cpu().numpy(), A, B,
                        0.4, 0.0, alpha=0.3, cutoff=8.5, rfa=True, reference_switch=True, excl=orc.exclusion_pairs(par),
                        dtype=np.float32 if prec == "f32" else np.float64)
        return np.array([o["E_lj"] + o["E_el"] + o["E_intra"]]), o["F"][None]

    ref = _oracle(par, pp, s.box, WATER_TERMS, okw, side=side_alpha, drop=solute)
    rl, rf = _evaluate(lived, pp, s.box, "alchemical", count=False), _evaluate(fresh, pp, s.box, "alchemical", count=False)
    LC.judge("alchemical set again at (0.4, 0), alpha 0.3", rl, rf, ref, prec, terms, bitwise=True)
    assert abs(ref.energies[0]["side"] - _oracle(par, pp, s.box, WATER_TERMS, okw, side=side2, drop=solute).energies[0]["side"]) > 1e-3  # (alpha shows)


@pytest.mark.timeout(180)
@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_metadynamics_hills_travel_between_the_explicit_and_the_autograd_engine(prec):
    """A `Forces` with an LJ switch keeps two engines, one per force flavour of the switch (the `exact` key); the bias grid lives
    in whichever of them `Metadynamics._eng` names, and `_host_dirty` / `_dev_dirty` say which copy is newer.  A hill is
    deposited through the explicit engine, the next evaluation runs through the autograd engine and must see it; a second hill,
    `grid` read back after each `deposit`, both flavours again; then `set_grid`.  References: the oracle in the matching flavour +
    the numpy model of the bias (`Metadynamics.energy_forces` / `deposit_model` on a model-side grid, the bars of
    tests/test_gpu_metad.py: nodes within 8 eps64 x the sum of the terms' magnitudes); fresh: a `Forces` whose bias is given
    the lived grid with `set_grid`.  Then tmdhip_set_metadynamics with `enable = 0` (the context equals one that never had a
    bias) and a bias on another pair with another width set in its place."""
    import types

    from torchmd_amd import _lib as L
    from torchmd_amd.forces import Forces
    from torchmd_amd.integrator import Integrator
    from torchmd_amd.metadynamics import Metadynamics

    mol, pos, box, par, vel = _water(9, prec)
    N = mol.numAtoms
    okw = dict(cutoff=8.5, rfa=True, switch_dist=7.0)
    b = _box_tensor(box, prec)
    terms = WATER_TERMS + ["side"]

    def bias(pair=(0, 3), sigma=0.2):
        return Metadynamics(("distance", pair), sigma=sigma, height=1.5, frequency=5, temperature=300.0, grid_min=1.0, grid_max=12.0)

    def at(k):  # atom 0 walks: the CV moves by a fraction of sigma per stop
        q = pos.copy()
        q[0] += k * np.array([0.11, -0.05, 0.07])
        return torch.as_tensor(q, dtype=PREC[prec]).to(_dev())[None].contiguous()

    def evaluate(f, p, exact, name="metadynamics"):
        F = torch.full_like(p, float("nan"))
        if exact:
            pots = f.compute(p.clone().requires_grad_(True), b, F, returnDetails=True, explicit_forces=False)
        else:
            pots = f.compute(p, b, F, returnDetails=True)
        for d in pots:
            d["side"] = d[name] if name else 0.0
        return LC.Result(npairs=None, energies=pots, forces=F.cpu())

    md, mm = bias(), bias()  # (the lived bias, and a bias that is only ever used as the numpy model)
    lived = Forces(par, terms=WATER_TERMS, metadynamics=md, **okw)
    grid, mag = np.zeros_like(mm.grid), np.zeros_like(mm.grid)

    def check(label, p, exact, g):
        side = lambda x, e: mm.energy_forces(x, e, g)[:2]  # noqa: E731
        ref = _oracle(par, p, b, WATER_TERMS, okw, side=side, explicit=not exact)
        eng = lived._engine(p, exact)  # (the engine of this flavour drops its list: both contexts build theirs at `p`)
        L.check(eng.lib.tmdhip_invalidate_list(eng.ctx, 0), "tmdhip_invalidate_list")
        rl = evaluate(lived, p, exact)
        mf = bias()
        mf.set_grid(md.grid)
        rf = evaluate(Forces(par, terms=WATER_TERMS, metadynamics=mf, **okw), p, exact)
        LC.judge(label, rl, rf, ref, prec, terms, bitwise=True)
        return ref.energies[0]["side"]

    def deposit(p, k):
        nonlocal grid, mag
        md.deposit(types.SimpleNamespace(pos=p, box=b))
        grid, rows = mm.deposit_model(p.cpu().double().numpy(), box, grid)
        mag += np.abs(mm.gauss_terms(rows[0, :1], rows[0, 1]))[None]
        return rows

    def read_back(k, rows):
        dev = md.grid
        log = md.hills()
        assert log.shape[0] == k + 1 and abs(log[k, 0, 0] - rows[0, 0]) <= (1e-12 if prec == "f64" else 1e-6)
        assert abs(log[k, 0, 1] / 1.5 - 1.0) <= 1e-10  # (plain metadynamics: every hill has the height)
        worst = (np.abs(dev - grid) / np.maximum(mag, 1e-300)).max() / EPS64
        print(f"hill {k} [{prec}]: s = {log[k, 0, 0]:.6f}, nodes {worst:.2f} eps64 x sum|terms| from the model's chain")
        assert (np.abs(dev - grid) <= 8 * EPS64 * mag).all() and dev[..., 0].max() > 1.0

    assert check("no hill yet, explicit engine", at(0), False, grid) == 0.0
    rows = deposit(at(0), 0)  # through the explicit engine (`deposit` takes the engine of the default flavour)
    assert md._dev_dirty  # (nobody has read the grid back: the autograd engine's sync has to fetch it from the other engine)
    v = check("one hill, autograd engine", at(1), True, grid)
    assert 0.5 < v < 1.51, v
    read_back(0, rows)
    rows = deposit(at(1), 1)  # the grid goes back to the explicit engine first
    read_back(1, rows)  # `deposit` followed by `grid`: read back from the engine that deposited
    check("two hills, explicit engine", at(2), False, grid)
    check("two hills, autograd engine", at(2), True, grid)
    half = 0.5 * md.grid
    md.set_grid(half)
    check("set_grid, autograd engine", at(2), True, half)
    check("set_grid, explicit engine", at(3), False, half)
    assert len(lived._engines) == 2 and lived.stats(at(0))["algorithm"] == "celllist"
    # ---- a run that deposits (frequency 5), against a fresh Forces whose bias starts from the lived grid
    p = at(3)
    s = _system(N, 1, prec, p, b, vel[:1])
    lived.compute(s.pos, s.box, s.forces)
    mf = bias()
    mf.set_grid(md.grid)
    fresh, sf = Forces(par, terms=WATER_TERMS, metadynamics=mf, **okw), _system(N, 1, prec, s.pos, s.box, s.vel, s.forces)
    lived.invalidate_lists(s.pos)
    nh = md.nhills
    out_l, out_f = Integrator(s, lived, 1.0, _dev()).step(5), Integrator(sf, fresh, 1.0, _dev()).step(5)
    assert md.nhills == nh + 1 and mf.nhills == 1
    for k in ("pos", "vel", "forces"):
        assert torch.equal(getattr(s, k), getattr(sf, k)), ("a run that deposits", k)
    assert np.array_equal(md.grid, mf.grid) and np.array_equal(out_l[0], out_f[0])
    g5 = md.grid.copy()
    ref = _oracle(par, s.pos, s.box, WATER_TERMS, okw, side=lambda x, e: mm.energy_forces(x, e, half)[:2])
    dl = LC.force_distance(s.forces.cpu(), ref.forces)  # (the forces a run leaves are those before its deposition)
    print(f"a run that deposits [{prec}]: forces left against oracle + model {dl:.3e}")
    assert dl <= FTOL[prec]
    # ---- released through the C ABI, then another bias in its place
    eng = lived._engine(s.pos)
    d = md.descriptor()
    d.enable = 0
    L.check(eng.lib.tmdhip_set_metadynamics(eng.ctx, C.byref(d)), "tmdhip_set_metadynamics")
    never = Forces(par, terms=WATER_TERMS, **okw)
    pp = s.pos.clone()
    ref = _oracle(par, pp, b, WATER_TERMS, okw)
    lived.metadynamics = None  # (the Python layer follows the release: nothing of the bias is synced or applied any more)
    lived.invalidate_lists(pp)
    LC.judge("bias released", evaluate(lived, pp, False, None), evaluate(never, pp, False, None), ref, prec, WATER_TERMS, bitwise=True)
    integ = Integrator(s, lived, 1.0, _dev())
    lived.compute(s.pos, s.box, s.forces)
    r0 = lived.stats(s.pos)["steps_in_pair_launch"]
    _step_leg("bias released", par, WATER_TERMS, okw, {}, lived, s, integ, 3, prec)
    if prec == "f32":
        assert lived.stats(s.pos)["steps_in_pair_launch"] >= r0 + 1
    md2, mm2 = bias((0, 6), 0.3), bias((0, 6), 0.3)
    g2 = np.zeros_like(mm2.grid)
    g2, rows = mm2.deposit_model(s.pos.cpu().double().numpy(), box, g2)
    md2.set_grid(g2)
    md2._forces = lived
    lived.metadynamics = md2
    pp = s.pos.clone()
    pp[0, 0, 2] += 0.2  # (atom 6 is two lattice sites up the z axis: the CV moves by about that much)
    mf2 = bias((0, 6), 0.3)
    mf2.set_grid(g2)
    ref = _oracle(par, pp, b, WATER_TERMS, okw, side=lambda x, e: mm2.energy_forces(x, e, g2)[:2])
    lived.invalidate_lists(pp)
    LC.judge("another bias set in its place", evaluate(lived, pp, False), evaluate(Forces(par, terms=WATER_TERMS, metadynamics=mf2, **okw), pp, False),
             ref, prec, terms, bitwise=True)
    assert ref.energies[0]["side"] > 0.3 and g5[..., 0].max() > 1.0


@pytest.mark.timeout(120)
@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_generalized_born_released_and_set_again(prec):
    """The 130-atom bonded cluster of tests/test_gpu_gb.py (bonds + Coulomb within 6 A on the cell-list path, open boundaries)
    with OBC2 + surface area: evaluate and step -> tmdhip_set_gb with `enable = 0` -> evaluate and step like a context that
    never had the model, bit for bit -> the model set again with another solvent dielectric and surface tension, like a fresh
    context with those.  Reference: oracle + the numpy model of tests/_gb.py, the force bar the parity bar plus the model's own
    rounding bound per atom (tests/test_gpu_gb.py: C_REAL eps + M eps64 times the sum of the addends' magnitudes)."""
    import _gb as GM
    import test_gpu_gb as GB
    from torchmd_amd import _lib as L
    from torchmd_amd.forces import Forces
    from torchmd_amd.integrator import Integrator

    cpos, par, rad, sc, vel0 = GB._bonded_cluster(prec)
    fkw = GB.PATHS["celllist"]
    okw = dict(cutoff=fkw["cutoff"])
    q = par.charges.double().numpy()
    n = len(cpos)
    p = torch.as_tensor(cpos, dtype=PREC[prec]).to(_dev())[None].contiguous()
    zero = _box_tensor(np.zeros(3), prec)
    npf = np.float32 if prec == "f32" else np.float64

    def reference(x, **gbkw):
        """(forces [1, n, 3], per-atom bar [n], GB + SA energy and its bar) at positions `x` [1, n, 3] (device tensor)."""
        ref = _oracle(par, x, zero, GB.TERMS, okw)
        F = ref.forces.clone()
        bar = np.full(n, FTOL[prec])
        e = ebar = 0.0
        if gbkw is not None and gbkw.get("on", True):
            kw = {k: v for k, v in gbkw.items() if k != "on"}
            o = GM.evaluate(x[0].cpu().double().numpy(), q, rad, sc, dtype=npf, bounds=True, **kw)
            u = GB.C_REAL * GB.EPS[prec] + o["M"] * EPS64
            F = F + torch.as_tensor(o["F"])[None]
            bar = bar + u * o["S_F"]
            e, ebar = o["E_gb"] + o["E_sa"], u * (o["S_Egb"] + o["S_Esa"])
        return F, bar, e, ebar

    def held(label, F, x, **gbkw):
        Fr, bar, _, _ = reference(x, **gbkw)
        err = (F.cpu().double() - Fr)[0].abs().max(dim=1).values.numpy()
        print(f"{label} [{prec}]: worst force error / bar = {(err / bar).max():.3f}")
        assert (err <= bar).all(), (label, (err / bar).max())

    def evaluate_both(label, lived, other, x, **gbkw):
        out = []
        for f in (lived, other):
            F1, F2 = torch.full_like(x, float("nan")), torch.full_like(x, float("nan"))
            pots = f.compute(x, zero, F1, returnDetails=True)
            f._evaluate(x, zero, F2, False, True)
            held(label, F1, x, **gbkw)
            out.append((pots, F1, F2))
        (pl, a1, a2), (pf, b1, b2) = out
        assert torch.equal(a1, b1) and torch.equal(a2, b2), (label, "lived and fresh differ")
        _, _, e, ebar = reference(x, **gbkw)
        if gbkw.get("on", True):
            for pots in (pl, pf):
                assert abs(pots[0]["implicit_solvent"] - e) <= ebar, (label, pots[0]["implicit_solvent"], e, ebar)
            assert abs(pl[0]["implicit_solvent"] - pf[0]["implicit_solvent"]) <= 2.0 * abs(pf[0]["implicit_solvent"] - e)
        return a1

    def step_both(label, lived, integ, s, other, **gbkw):
        sf = _system(n, 1, prec, s.pos, s.box, s.vel, s.forces)
        lived.invalidate_lists(s.pos)
        out_l, out_f = integ.step(3), Integrator(sf, other, 1.0, _dev()).step(3)
        held(label + ", step(3)", s.forces, s.pos, **gbkw)
        for k in ("pos", "vel", "forces"):
            assert torch.equal(getattr(s, k), getattr(sf, k)), (label, k)
        assert np.array_equal(out_l[0], out_f[0])
        assert lived.stats(s.pos)["algorithm"] == "celllist" == other.stats(sf.pos)["algorithm"]

    gb = GB._gb(rad, sc)
    lived = Forces(par, terms=GB.TERMS, implicit_solvent=gb, **fkw)
    F = evaluate_both("GB on", lived, Forces(par, terms=GB.TERMS, implicit_solvent=GB._gb(rad, sc), **fkw), p)
    s = _system(n, 1, prec, p, zero, vel0, F)
    integ = Integrator(s, lived, 1.0, _dev())
    step_both("GB on", lived, integ, s, Forces(par, terms=GB.TERMS, implicit_solvent=GB._gb(rad, sc), **fkw))
    # ---- released
    eng = lived._engine(s.pos)
    d = L.GbDesc()
    d.struct_size = C.sizeof(L.GbDesc)
    d.enable = 0
    L.check(eng.lib.tmdhip_set_gb(eng.ctx, C.byref(d)), "tmdhip_set_gb")  # (side_seen stays: no upload behind our back)
    x = s.pos.clone()
    lived.invalidate_lists(x)
    F = evaluate_both("GB released", lived, Forces(par, terms=GB.TERMS, **fkw), x, on=False)
    assert lived.compute(x, zero, torch.zeros_like(x), returnDetails=True)[0]["implicit_solvent"] == 0.0
    s.forces.copy_(F)
    step_both("GB released", lived, integ, s, Forces(par, terms=GB.TERMS, **fkw), on=False)
    # ---- set again with other parameters
    new = dict(solvent_dielectric=40.0, surface_tension=0.009)
    r64, s64 = np.array(rad, dtype=np.float64), np.array(sc, dtype=np.float64)
    d.enable, d.radii_host, d.scale_host = 1, r64.ctypes.data_as(C.c_void_p), s64.ctypes.data_as(C.c_void_p)
    d.solute_dielectric, d.solvent_dielectric, d.surface_tension, d.probe_radius = 1.0, 40.0, 0.009, 1.4
    L.check(eng.lib.tmdhip_set_gb(eng.ctx, C.byref(d)), "tmdhip_set_gb")
    x = s.pos.clone()
    lived.invalidate_lists(x)
    F = evaluate_both("GB set again", lived, Forces(par, terms=GB.TERMS, implicit_solvent=GB._gb(rad, sc, **new), **fkw), x, **new)
    s.forces.copy_(F)
    step_both("GB set again", lived, integ, s, Forces(par, terms=GB.TERMS, implicit_solvent=GB._gb(rad, sc, **new), **fkw), **new)


@pytest.mark.timeout(120)
@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_virtual_sites_set_released_and_set_again(prec):
    """tmdhip_set_vsites on the 2 187-atom water context (a site on an ordinary atom's row, as the refusal tests of
    tests/test_gpu_restraints.py make one): with sites and no constraints tmdhip_md_run refuses the call before its first kernel
    and nothing moves; evaluations do not look at the table.  `enable = 0`: evaluate and step like a context that never had
    sites, bit for bit.  Another table: refused again, state untouched, and released again."""
    from torchmd_amd import _lib as L
    from torchmd_amd.forces import Forces
    from torchmd_amd.integrator import Integrator

    mol, pos, box, par, vel = _water(9, prec)
    N = mol.numAtoms
    okw = dict(cutoff=8.5, rfa=True)
    p, b = torch.as_tensor(pos, dtype=PREC[prec]).to(_dev())[None].contiguous(), _box_tensor(box, prec)
    lived = Forces(par, terms=WATER_TERMS, **okw)
    s = _system(N, 1, prec, p, b, vel[:1])
    lived.compute(s.pos, s.box, s.forces)
    integ = Integrator(s, lived, 1.0, _dev())
    _step_leg("before any site", par, WATER_TERMS, okw, {}, lived, s, integ, 3, prec)
    eng = lived._engine(s.pos)
    ref = _oracle(par, p, b, WATER_TERMS, okw)

    def sites(site, parents, enable=1):
        vd = L.VsiteDesc()
        vd.struct_size = C.sizeof(L.VsiteDesc)
        vd.enable, vd.nsites = enable, 1
        keep = (np.array([site], np.int32), np.array([parents + [-1]], np.int32), np.array([[0.5, 0.5, 0.0]]))
        vd.site_host, vd.parent_host, vd.weight_host = (a.ctypes.data_as(C.c_void_p) for a in keep)
        L.check(eng.lib.tmdhip_set_vsites(eng.ctx, C.byref(vd)), "tmdhip_set_vsites")

    for site, parents in ((7, [1, 2]), (100, [40, 41])):
        sites(site, parents)
        before = {k: getattr(s, k).clone() for k in ("pos", "vel", "forces")}
        with pytest.raises(RuntimeError, match="virtual sites"):
            integ.step(3)
        torch.cuda.synchronize()
        for k in before:
            assert torch.equal(getattr(s, k), before[k]), (site, k)
        fresh = Forces(par, terms=WATER_TERMS, **okw)
        lived.invalidate_lists(p)
        LC.judge(f"site {site} set: evaluations", _evaluate(lived, p, b), _evaluate(fresh, p, b), ref, prec, WATER_TERMS, bitwise=True)
        sites(site, parents, enable=0)
        out, fr, sf = _step_leg(f"site {site} released", par, WATER_TERMS, okw, {}, lived, s, integ, 3, prec)
        _check_kinetic(f"site {site} released", out, s, integ.masses, prec)
        if prec == "f32":
            assert fr.stats(sf.pos)["steps_in_pair_launch"] >= 1
    assert lived.stats(s.pos)["algorithm"] == "celllist" and (lived.stats(s.pos)["steps_in_pair_launch"] >= 3 if prec == "f32" else True)
