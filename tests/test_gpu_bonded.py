"""Every bonded-term evaluator against the oracle at its edges (run with `-m gpu` on an MI355X).

The synthetic topologies of tests/_bonded_systems.py reach what the golden molecules never do: records in slots 4-7 of
the light scheme and torsion / 1-4 records on it, a third 64-entry pass of the wave kernel and of the all-pairs ride rows,
harmonic torsion tables with their +-pi wrap, bonds dropped by the cutoff to the ulp, angles at and near linear, bonds
across periodic images with a box per replica, and molecules spread over many 64-atom step blocks.  Each case is compared
with oracle/torchmd_oracle.py: forces on all atoms and the per-term energies; fp32 runs against the fp64 oracle on the
same fp32-rounded inputs and parameters."""

import numpy as np
import pytest
import torch

from oracle import torchmd_oracle as orc

import _bonded_systems as B

pytestmark = pytest.mark.gpu

PREC = {"f64": torch.float64, "f32": torch.float32}
FTOL = {"f64": 1e-8, "f32": 1e-4}  # max |dF| / (1 + |F|)
ETOL = {"f64": 1e-10, "f32": 6e-5}  # per-term energies, relative (to max(1, |E|))
# fp32 floor: twice what the oracle's own fp32 arithmetic misses by on the same inputs — coordinates a box length or two
# outside the box (up to ~230 A) leave fp32 differences ~1e-5 A off, which the stiff bonds turn into ~5e-4 of force
ORACLE32_FACTOR = 2.0
# MD: ten fp32 steps amplify those differences further along the trajectory; the same rule with a factor 3
MD_ORACLE32_FACTOR = 3.0
CUTOFF = 9.0
_CACHE = {}


def _dev():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    return torch.device("cuda:0")


def _system(name, size, prec):
    key = (name, size, prec if name == "edges" else None)
    if key not in _CACHE:
        _CACHE[key] = B.build(name, size, PREC[prec])
    return _CACHE[key]


def _oracle(s, terms, pos, box, dtype=torch.float64, **kw):
    """Oracle energies [R] dicts and forces [R, N, 3] (float64) for positions pos [R, N, 3] (float64 values)."""
    par = s.par(dtype)
    nb = any(t in orc.NONBONDED for t in terms)
    pots, F = [], []
    for r in range(pos.shape[0]):
        pairs = None
        if nb:
            pairs = orc.candidate_pairs(pos[r].numpy(), box[r].diagonal().numpy(), (kw.get("cutoff") or CUTOFF) + 0.5,
                                        orc.exclusion_pairs(par))
        p, f, _ = orc.compute(par, pos[r:r + 1].to(dtype), box[r:r + 1].to(dtype), terms, pairs=pairs, **kw)
        pots.append(p[0])
        F.append(f[0].double())
    return pots, torch.stack(F)


def _reference(s, terms, prec, R=1, seed=0, **kw):
    """(fp32-rounded) inputs, the fp64 oracle on them, and for fp32 the force / energy floors of ORACLE32_FACTOR."""
    dt = PREC[prec]
    sr = s.rounded(dt)
    pos, box = B.positions_for(sr, R, dt, seed=seed)
    pos64, box64 = pos.double(), box.double()
    pots, F = _oracle(sr, terms, pos64, box64, **kw)
    ftol, etol = FTOL[prec], ETOL[prec]
    if prec == "f32":
        _, F32 = _oracle(sr, terms, pos64, box64, dtype=torch.float32, **kw)
        ftol = max(ftol, ORACLE32_FACTOR * _ferr(F32, F, _mask(s)))
    return sr, pos, box, pots, F, ftol, etol


def _mask(s):
    """Atoms whose fp32 force is compared: all but those of the near-linear angles of `edges`, where sin(theta) =
    sqrt(1 - cos^2) keeps ~2 significant digits in fp32 (cos within 5e-7 of -1) — any fp32 evaluation, the oracle's too,
    is off there by percents; they are held to the fp64 bound in the fp64 runs."""
    m = np.ones(s.natoms, bool)
    if "near_linear_angles" in s.meta:
        m[s.g["par_angle_idx"][s.meta["near_linear_angles"]].reshape(-1)] = False
    return torch.tensor(m)


def _ferr(F, Fo, mask=None):
    e = ((F.double().cpu() - Fo).abs() / (1.0 + Fo.abs())).amax(dim=-1)
    if mask is not None:
        e = e[..., mask]
    return e.max().item()


def _compare(pots, F, opots, oF, terms, ftol, etol, mask=None, what=""):
    err = _ferr(F, oF, mask)
    assert err <= ftol, (what, "forces", err, ftol)
    worst = 0.0
    for r in range(len(opots)):
        for t in terms:
            if t == "1-4":  # (the reference reports 1-4 pairs under lj / electrostatics)
                assert pots[r][t] == 0.0 and opots[r][t] == 0.0
                continue
            rel = abs(pots[r][t] - opots[r][t]) / max(1.0, abs(opots[r][t]))
            worst = max(worst, rel)
            assert rel <= etol, (what, r, t, pots[r][t], opots[r][t])
    print(f"{what}: max|dF|/(1+|F|) = {err:.2e} (bound {ftol:.1e}), energies {worst:.2e}")
    return err


def _gpu(s, terms, prec, pos, box, **kw):
    from torchmd_amd.forces import Forces

    dev = _dev()
    f = Forces(s.par(PREC[prec]), terms=terms, **kw)
    p, b = pos.to(dev), box.to(dev)
    F = torch.full_like(p, 7.0)  # (must be overwritten)
    pots = f.compute(p, b, F, returnDetails=True)
    st = f.stats(p)
    f.close()
    return pots, F.cpu(), st


# ----------------------------------------------------------------------------- bonded terms alone
ALONE_CASES = [(n, R) for n in ("light-full", "light-plus-one", "hub", "harmonic", "harmonic-dihedrals") for R in (1, 3)] + [("edges", 1)]


@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("name,R", ALONE_CASES, ids=[f"{n}-R{r}" for n, r in ALONE_CASES])
def test_bonded_terms_alone(name, R, prec):
    """The five bonded terms with no nonbonded engine: light-full / harmonic / edges on bonded_atom_kernel (light records,
    slots 4-7 in the second pass of each lane), light-plus-one and hub on bonded_wave_kernel (hub: three passes of 64).
    R = 3: one launch for three replicas, each with its own box (scaled 1.00 / 1.01 / 1.02, positions with it) and
    displaced positions — bonds across the faces take the right replica's image.  (`edges` runs with one replica: its
    exactly linear and near-cutoff geometry is built for one box.)"""
    s = _system(name, B.SMALL, prec)
    sr, pos, box, opots, oF, ftol, etol = _reference(s, B.BONDED, prec, R=R, seed=R)
    heavy = B.records_per_atom(sr.par(), B.BONDED).max() > B.ATOM_CENTRIC_LIMIT
    assert heavy == (name in ("light-plus-one", "hub"))
    pots, F, _ = _gpu(sr, B.BONDED, prec, pos, box)
    _compare(pots, F, opots, oF, B.BONDED, ftol, etol, _mask(s) if prec == "f32" else None, f"{name} {prec} R={R}")


# ----------------------------------------------------------------------------- with the nonbonded engine
NB_CASES = [("light-full", B.SMALL, "allpairs"), ("light-full", B.LARGE, "celllist"),
            ("light-plus-one", B.SMALL, "allpairs"), ("light-plus-one", B.LARGE, "celllist"),
            ("hub", B.SMALL, "allpairs"), ("hub", B.LARGE, "celllist"),
            ("harmonic", B.SMALL, "allpairs"), ("harmonic-dihedrals", B.LARGE, "celllist"),
            ("edges", B.SMALL, "allpairs"), ("edges", B.LARGE, "celllist")]


@pytest.mark.parametrize("switch", [None, 7.5], ids=["noswitch", "switch7.5"])
@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("name,size,algorithm", NB_CASES, ids=[f"{n}-{z}-{a}" for n, z, a in NB_CASES])
def test_bonded_terms_with_lj_and_reaction_field(name, size, algorithm, prec, switch, monkeypatch):
    """All seven terms through Forces.compute, cutoff 9 A, reaction field.  all-pairs at <= 2048 atoms (the bonded
    kernels beside the tiled pair kernel); cell list at 4-8k atoms: light topologies in the evaluation-only step blocks of
    the lean fp32 launch (FINAL == 2) — bit-identical to the separate kernels (TMDHIP_FUSED_EVAL=0) —, heavy ones through
    bonded_wave_kernel.  Bonds longer than the cutoff and those a few ulps beyond it are dropped like the reference's
    `dist <= cutoff`."""
    s = _system(name, size, prec)
    if name == "edges" and prec == "f32":
        # bonds within ulps of the cutoff are kept or dropped by fp32 arithmetic, which the fp64 oracle does not share:
        # test_bond_cutoff_keeps_exactly_the_bonds_the_reference_keeps holds them against the oracle in fp32
        keep = np.ones(len(s.g["par_bond_idx"]), bool)
        keep[s.meta["near_cutoff_bonds"]] = False
        s = s.with_tables(bond=keep)
    kw = dict(cutoff=CUTOFF, rfa=True, switch_dist=switch)
    sr, pos, box, opots, oF, ftol, etol = _reference(s, B.ALL_TERMS, prec, **kw)
    runs = {}
    for fused in (("1", "0") if algorithm == "celllist" else ("1",)):
        monkeypatch.setenv("TMDHIP_FUSED_EVAL", fused)
        runs[fused] = _gpu(sr, B.ALL_TERMS, prec, pos, box, algorithm=algorithm, **kw)
    pots, F, st = runs["1"]
    assert st["algorithm"] == algorithm
    if algorithm == "allpairs":
        assert s.natoms <= 2048
    _compare(pots, F, opots, oF, B.ALL_TERMS, ftol, etol, _mask(s) if prec == "f32" else None,
             f"{name}-{size} {algorithm} {prec} switch={switch}")
    if "0" in runs:
        p0, F0, _ = runs["0"]
        assert torch.equal(F, F0)
        for t in B.ALL_TERMS:
            assert abs(pots[0][t] - p0[0][t]) <= 1e-12 * max(1.0, abs(p0[0][t])), t


@pytest.mark.parametrize("prec", ["f64", "f32"])
def test_bond_cutoff_keeps_exactly_the_bonds_the_reference_keeps(prec):
    """Bonds of length cutoff + k ulps (k = -2..2) and bonds well beyond the cutoff, alone in the table: a bond is kept
    iff the oracle's dist <= cutoff on the same inputs, in the same precision (the reference's decision in fp32 is an
    fp32 one).  Each kept bond adds k0 x^2 (x ~ 1 A) to the bonds energy and a force to its two atoms (which have no
    other term); a dropped one neither."""
    s = _system("edges", B.SMALL, prec)
    rows = np.concatenate([s.meta["near_cutoff_bonds"], s.meta["long_bonds"]])
    keep = np.zeros(len(s.g["par_bond_idx"]), bool)
    keep[rows] = True
    t = s.with_tables(bond=keep, angle=None, dihedral=None, improper=None, nonbonded_14=None)
    sr = t.rounded(PREC[prec])
    pos, box = B.positions_for(sr, 1, PREC[prec])
    opots, oF = _oracle(sr, ["bonds"], pos.double(), box.double(), dtype=PREC[prec], cutoff=CUTOFF)
    ftol, etol = FTOL[prec], ETOL[prec]
    pots, F, _ = _gpu(sr, ["bonds"], prec, pos, box, cutoff=CUTOFF)
    idx = torch.tensor(sr.g["par_bond_idx"])
    d = orc.pair_geometry(pos[0], idx, box[0].diagonal())[0]
    kept_oracle = (d <= CUTOFF).numpy()
    kept_gpu = (F[0][idx[:, 0]].abs().amax(dim=1) > 0).numpy()
    assert np.array_equal(kept_gpu, kept_oracle), (kept_gpu, kept_oracle, s.meta["near_cutoff_offsets"])
    near = np.isin(np.sort(rows), s.meta["near_cutoff_bonds"])  # (with_tables keeps the table order: long bonds first)
    assert kept_oracle[near].tolist() == (s.meta["near_cutoff_offsets"] <= 0).tolist()
    assert not kept_oracle[~near].any()
    prm = sr.g["par_bond_params"][sr.g["par_bond_map"][:, 1]]
    x = d.double().numpy() - prm[:, 1]
    smallest = (prm[:, 0] * x * x)[kept_oracle].min()
    assert smallest > 100 * etol * max(1.0, abs(opots[0]["bonds"]))  # one bond more or less shows in the energy
    assert abs(pots[0]["bonds"] - opots[0]["bonds"]) <= etol * max(1.0, abs(opots[0]["bonds"])), (pots[0], opots[0])
    assert _ferr(F, oF) <= ftol


# ----------------------------------------------------------------------------- MD
def _oracle_md(sr, pos, vel, box, terms, niter, dtype=torch.float64, **kw):
    """The oracle's Integrator.step loop (NVE) on every replica: final positions, velocities, forces, energies."""
    par = sr.par(dtype)
    dt = 1.0 / orc.TIMEFACTOR
    out = []
    for r in range(pos.shape[0]):
        p, v = pos[r:r + 1].to(dtype).clone(), vel[r:r + 1].to(dtype).clone()
        b = box[r:r + 1].to(dtype)
        pairs = orc.candidate_pairs(p[0].double().numpy(), b[0].diagonal().double().numpy(), CUTOFF + 1.5, orc.exclusion_pairs(par))
        _, f, _ = orc.compute(par, p, b, terms, pairs=pairs, **kw)
        m = par.masses.to(dtype)
        for _ in range(niter):
            pots, _ = orc.md_step(par, p, v, f, b, m, dt, terms, pairs=pairs, **kw)
        ek = orc.kinetic_energy(m, v.double())
        out.append((p[0].double(), v[0].double(), f[0].double(), sum(pots[0].values()), ek.item()))
    return out


def _md(name, size, R, algorithm, prec, monkeypatch, env=None):
    from torchmd_amd.forces import Forces
    from torchmd_amd.integrator import Integrator
    from torchmd_amd.systems import System

    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)
    dev, dt = _dev(), PREC[prec]
    s = _system(name, size, prec)
    sr = s.rounded(dt)
    pos, box = B.positions_for(sr, R, dt, seed=7)
    rng = np.random.default_rng(8)
    m = sr.g["par_masses"]
    vel = torch.tensor(np.stack([rng.standard_normal(sr.pos.shape) * np.sqrt(orc.BOLTZMAN * 300.0 / m) for _ in range(R)])).to(dt)
    kw = dict(cutoff=CUTOFF, rfa=True)
    key = ("md", name, size, R, prec)
    if key not in _CACHE:
        ref = _oracle_md(sr, pos.double(), vel.double(), box.double(), B.ALL_TERMS, 10, **kw)
        ref32 = _oracle_md(sr, pos.double(), vel.double(), box.double(), B.ALL_TERMS, 10, dtype=torch.float32, **kw) if prec == "f32" else None
        _CACHE[key] = (ref, ref32)
    ref, ref32 = _CACHE[key]
    system = System(sr.natoms, R, dt, dev)
    system.pos.copy_(pos.to(dev))
    system.box.copy_(box.to(dev))
    system.vel.copy_(vel.to(dev))
    f = Forces(sr.par(dt), terms=B.ALL_TERMS, algorithm=algorithm, **kw)
    f.compute(system.pos, system.box, system.forces)
    integ = Integrator(system, f, 1.0, dev)
    ek, ep, _ = integ.step(niter=10)
    st = [f.stats(system.pos, r) for r in range(R)]
    got = (system.pos.cpu().double(), system.vel.cpu().double(), system.forces.cpu().double())
    f.close()
    for r in range(R):
        what = f"md {name}-{size} {algorithm} {prec} R={R} {env or ''} replica {r}"
        for k, (label, x) in enumerate(zip(("pos", "vel", "forces"), got)):
            tol = FTOL[prec]
            if ref32 is not None:
                tol = max(tol, MD_ORACLE32_FACTOR * _ferr(ref32[r][k], ref[r][k]))
            err = _ferr(x[r], ref[r][k])
            print(f"{what}: {label} {err:.2e} (bound {tol:.1e})")
            assert err <= tol, (what, label, err, tol)
        etol = ETOL[prec]
        if ref32 is not None:
            etol = max(etol, MD_ORACLE32_FACTOR * abs(ref32[r][3] - ref[r][3]) / max(1.0, abs(ref[r][3])))
        assert abs(ep[r] - ref[r][3]) <= etol * max(1.0, abs(ref[r][3])), (what, ep[r], ref[r][3])
        assert abs(ek[r] - ref[r][4]) <= max(ETOL[prec], 2e-6) * max(1.0, abs(ref[r][4])), (what, ek[r], ref[r][4])
    return st


@pytest.mark.parametrize("env", [{}, {"TMDHIP_FUSED_STEP": "0"}, {"TMDHIP_FUSED_FINAL": "0"}], ids=["default", "no-fused-step", "no-fused-final"])
def test_md_nve_on_the_cell_list_against_the_oracle(env, monkeypatch):
    """Ten NVE steps of light-full (cell list, fp32) against the oracle's Integrator.step loop: by default the interior
    steps are made by the pair launch's step blocks and the last one by its FINAL step blocks — molecules spread over
    many 64-atom step blocks, so a block reading a partner another block has already moved would show; then with the
    separate integrator (TMDHIP_FUSED_STEP=0) and the separate final kernels (TMDHIP_FUSED_FINAL=0)."""
    st = _md("light-full", B.LARGE, 1, "celllist", "f32", monkeypatch, env)[0]
    assert st["algorithm"] == "celllist"
    if env.get("TMDHIP_FUSED_STEP") == "0":
        assert st["steps_in_pair_launch"] == 0
    else:
        assert st["steps_in_pair_launch"] > 0
    if env:
        assert st["final_steps_in_pair_launch"] == 0 or env.get("TMDHIP_FUSED_STEP") == "0"
    else:
        assert st["final_steps_in_pair_launch"] > 0


@pytest.mark.parametrize("prec", ["f64", "f32"])
def test_md_nve_all_pairs_light_topology(prec, monkeypatch):
    """The interior steps of an all-pairs light system: md_step_bonded_kernel evaluates the records inline (wave w takes
    slots w, w + 4)."""
    st = _md("light-full", B.SMALL, 1, "allpairs", prec, monkeypatch)[0]
    assert st["algorithm"] == "allpairs"


@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("name", ["hub", "light-plus-one"])
def test_md_nve_all_pairs_heavy_topology(name, prec, monkeypatch):
    """The MD loop of a heavy topology of <= 2048 atoms: its bonded terms ride on the all-pairs launch (rows of one wave
    per atom behind the pair blocks, pair_generic.hip) — the hub centres in three passes of 64 entries."""
    st = _md(name, B.SMALL, 1, "allpairs", prec, monkeypatch)[0]
    assert st["algorithm"] == "allpairs"


@pytest.mark.parametrize("batch", ["1", "0"])
def test_md_nve_three_replicas_with_their_own_boxes(batch, monkeypatch):
    """R = 3 replicas of light-full (boxes 1.00 / 1.01 / 1.02, displaced positions) in one context: batched into one
    pair + step launch (batched_launches > 0), and replica by replica (TMDHIP_BATCH_REPLICAS=0); each against the oracle."""
    st = _md("light-full", B.LARGE, 3, "celllist", "f32", monkeypatch, {"TMDHIP_BATCH_REPLICAS": batch})
    if batch == "1":
        assert st[0]["batched_launches"] > 0 and st[0]["steps_in_pair_launch"] > 0
    else:
        assert st[0]["batched_launches"] == 0
