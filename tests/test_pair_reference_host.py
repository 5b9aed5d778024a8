"""The dimer system and the long-double pair reference of tests/_pair_reference.py checked on the host: the dimers are
isolated, the reference agrees with the CPU oracle, its exact-mode force is the derivative of its energy, the inputs are
well conditioned (a plain evaluation in the engine's precision stays under 16 eps x S), and the edge dimers carry the
labels their exact distances give them.  tests/test_gpu_pair_resolved.py holds the kernels to this reference."""

import numpy as np
import pytest
import torch

import _pair_reference as pr
from _golden import PREC, GoldenParameters, box_tensor
from _pair_reference import LD

EPS = {"f32": float(np.finfo(np.float32).eps), "f64": float(np.finfo(np.float64).eps)}
BOXES = {"pbc": np.full(3, pr.BOX), "box0": np.zeros(3)}


def _tables(system, prec):
    par = GoldenParameters(system.golden(), PREC[prec])
    A, B = par.get_AB()
    return par, A.numpy(), B.numpy(), par.charges.numpy()


def test_long_double_is_wider_than_double():
    assert np.finfo(LD).eps <= 2.0**-63, "the reference needs an extended long double"


@pytest.mark.parametrize("prec", ["f32", "f64"])
@pytest.mark.parametrize("classes", [3, 40])
def test_dimers_are_isolated(prec, classes):
    """Every atom has exactly one other atom within cutoff + 1.5 A, in the scan configuration and in every band
    configuration where its dimer is closed; an opened dimer's atoms have nobody."""
    from scipy.spatial import cKDTree

    s = pr.dimer_system(pr.NP_DTYPE[prec], classes)
    assert s.natoms == 1152 and s.npairs == 576
    assert np.abs(s.pairs[:, 0] - s.pairs[:, 1]).min() > 1  # not neighbours in memory
    for band in [None] + list(range(pr.N_BANDS)):
        pos = np.asarray(s.positions(band), dtype=np.float64)
        assert pos.min() >= 0 and pos.max() < pr.BOX
        tree = cKDTree(pos, boxsize=pr.BOX)
        nb = tree.query_ball_point(pos, pr.ISOLATION)
        closed = np.ones(s.npairs, dtype=bool) if band is None else s.band == band
        for a, lst in enumerate(nb):
            others = [b for b in lst if b != a]
            p = s.pair_of[a]
            if closed[p]:
                mate = s.pairs[p, 1] if s.pairs[p, 0] == a else s.pairs[p, 0]
                assert others == [mate], (band, a, others)
            else:
                assert others == [], (band, a, others)


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_system_layout(prec):
    s = pr.dimer_system(pr.NP_DTYPE[prec], 3)
    pos = s.positions()
    d = pr.stored_delta(pos, s.pairs, s.box).astype(LD)
    r = np.sqrt((d * d).sum(axis=1))
    scan = ~s.is_edge
    assert scan.sum() == 512 and s.is_edge.sum() == 64
    assert np.abs(r[scan] - pr.CUTOFF).min() >= 1e-4  # the decision at the cutoff is the edge dimers'
    assert np.abs(r[scan] - s.dist[scan]).max() < 1e-4
    assert r[scan].min() < 0.81 and r[scan].max() > 9.17
    assert (np.abs(r[scan] - pr.SWITCH_DIST) <= 1.1e-3).sum() >= 32 and (np.abs(r[scan] - pr.CUTOFF) <= 1.1e-3).sum() >= 32
    assert s.on_face.sum() == 128
    # the dimers on a face interact through the minimum image: the raw difference is a box edge off
    raw = pos[s.pairs[:, 0]].astype(np.float64) - pos[s.pairs[:, 1]].astype(np.float64)
    straddle = (np.abs(raw) > 0.5 * pr.BOX).any(axis=1)
    assert (straddle & scan).sum() >= 64 and (straddle & s.is_edge).sum() == 32
    for b in range(pr.N_SCAN_BANDS):  # a band spans at most a factor 1.4 of r
        rb = r[s.band == b]
        assert len(rb) > 20 and rb.max() / rb.min() <= 1.4
    if s.classes == 3:  # all six class pairs, each over the whole range of r
        ti, tj = s.types[s.pairs[:, 0]], s.types[s.pairs[:, 1]]
        key = np.minimum(ti, tj) * 3 + np.maximum(ti, tj)
        for k in (0, 1, 2, 4, 5, 8):
            rk = r[scan & (key == k)]
            assert len(rk) > 60 and rk.min() < 0.9 and rk.max() > 8.9


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_edge_dimer_labels(prec):
    """Axis-aligned, on multiples of 2^-10 A up to the one stepped coordinate: the engine's d is exact, and in / out
    follows from |d| <= cutoff on the exact |d| — computed here in exact rational arithmetic."""
    from fractions import Fraction

    dt = pr.NP_DTYPE[prec]
    s = pr.dimer_system(dt, 3)
    pos = s.positions()
    A = np.ones((3, 3))
    ref = pr.reference(s, pos, s.box, A, A, s.charges, ("repulsion",))
    seen = set()
    nthreshold = 0
    for e, (ax, a, b, moved, ulps, perp) in enumerate(pr._edge_specs()):
        p = pr.N_SCAN + e
        if perp is not None:  # r2 == r2max: in by the reference's rounded decision, although |d| > 9
            r2 = pr.engine_norm2(pr.stored_delta(pos, s.pairs[p:p + 1], s.box))[0]
            assert r2 == np.nextafter(dt(81.0), dt(np.inf)) and np.sqrt(r2) == dt(9.0) and np.sqrt(np.nextafter(r2, dt(np.inf))) > dt(9.0)
            assert ref.included[p] and ref.r[p] > 9 and ref.S_F[p] > 0
            assert abs(float(ref.d[p, ax])) == 9.0 and float(ref.d[p, perp]) == pr.threshold_offset(dt)
            nthreshold += 1
            continue
        xi, xj = pos[s.pairs[p, 0]], pos[s.pairs[p, 1]]
        others = [k for k in range(3) if k != ax]
        assert all(xi[k] == xj[k] for k in others)
        d = Fraction(float(xi[ax])) - Fraction(float(xj[ax]))
        d -= 180 * round(d / 180)
        assert Fraction(float(ref.d[p, ax])) == d and ref.d[p, others[0]] == 0 and ref.d[p, others[1]] == 0
        assert Fraction(float(ref.r[p])) == abs(d)
        assert bool(ref.included[p]) == (abs(d) <= 9)
        through_face = abs(float(xi[ax]) - float(xj[ax])) > 90
        nominal = 9.0 if abs(abs(d) - 9) < 1e-3 else 7.5
        step = np.spacing(dt(173.0 if through_face else nominal))
        assert abs(d) - Fraction(nominal) in (0, Fraction(float(step)), -Fraction(float(step)))
        seen.add((ax, through_face, nominal, (abs(d) > nominal) - (abs(d) < nominal)))
        if not ref.included[p]:
            assert ref.S_F[p] == 0 and np.all(ref.F[s.pairs[p]] == 0) and ref.E["repulsion"][p] == 0
    assert nthreshold == 4
    for ax in range(3):
        for face in (False, True):
            assert {(ax, face, 9.0, 0), (ax, face, 9.0, 1), (ax, face, 7.5, -1), (ax, face, 7.5, 0), (ax, face, 7.5, 1)} <= seen
    # interior: the successor of 9.0 itself
    assert any(float(ref.r[pr.N_SCAN + e]) == float(np.nextafter(dt(9.0), dt(np.inf))) for e in range(pr.N_EDGE))


def _oracle_pairs(s):
    pairs = np.sort(s.pairs, axis=1)
    return pairs[np.lexsort((pairs[:, 1], pairs[:, 0]))]


@pytest.mark.parametrize("boxname", ["pbc", "box0"])
@pytest.mark.parametrize("classes", [3, 40])
@pytest.mark.parametrize("tid,terms,kw", pr.TERM_SETS, ids=[t[0] for t in pr.TERM_SETS])
def test_reference_agrees_with_oracle(tid, terms, kw, classes, boxname):
    """float64: the oracle (the reference implementation's own torch expressions) against the long-double closed forms,
    per atom and per term, within 16 eps64 x S."""
    from oracle import torchmd_oracle as orc

    s = pr.dimer_system(np.float64, classes)
    box = BOXES[boxname]
    par, A, B, q = _tables(s, "f64")
    pos = s.positions()
    ref = pr.reference(s, pos, box, A, B, q, terms, **kw)
    okw = dict(cutoff=pr.CUTOFF, rfa=kw.get("rfa", False), switch_dist=kw.get("switch_dist"))
    exact = kw.get("switch_mode") == "exact"
    tpos = torch.tensor(np.array(pos))[None]
    if exact:
        tpos.requires_grad_(True)
    pots, F, npairs = orc.compute(par, tpos, box_tensor(box, 1, torch.float64), list(terms), pairs=_oracle_pairs(s),
                                  explicit_forces=not exact, **okw)
    assert npairs[0] == int(ref.included.sum())
    bar = 16 * EPS["f64"]
    errF = np.abs(F[0].detach().numpy().astype(LD) - ref.F).max(axis=1)
    S_atom = ref.S_F[s.pair_of]
    assert np.all(errF <= bar * S_atom), float((errF / np.where(S_atom > 0, S_atom, 1)).max() / EPS["f64"])
    # per term and per pair, from the oracle's pair functions
    idx = torch.as_tensor(s.pairs)
    boxdiag = torch.tensor(box)
    dist, _, _ = orc.pair_geometry(tpos[0].detach(), idx, boxdiag)
    types = torch.as_tensor(s.types)
    tA, tB = par.get_AB()
    for t in terms:
        if t == "lj":
            E, _ = orc.lj(dist, idx, types, tA, tB, okw["switch_dist"], pr.CUTOFF)
        elif t == "electrostatics":
            E, _ = orc.electrostatics(dist, idx, par.charges, 1, pr.CUTOFF, okw["rfa"], pr.DIELECTRIC)
        elif t == "repulsion":
            E, _ = orc.repulsion(dist, idx, types, tA)
        else:
            E, _ = orc.repulsion_cg(dist, idx, types, tB)
        E = np.where((dist <= pr.CUTOFF).numpy(), E.numpy(), 0.0)
        assert np.all(np.abs(E.astype(LD) - ref.E[t]) <= bar * ref.S_E[t]), (t,)
        assert abs(LD(pots[0][t]) - ref.E[t].sum()) <= bar * ref.S_E[t].sum()


@pytest.mark.parametrize("classes", [3, 40])
def test_exact_mode_force_is_the_energy_derivative(classes):
    """The test's own formulas: a central difference of the long-double energy in r equals the long-double exact-mode
    dE/dr.  h = 1e-5 r: truncation h^2/6 E''' ~ 1e-10 (13 14 15 / 6) relative to the r^-13 term, rounding 1e-19 / 1e-5."""
    s = pr.dimer_system(np.float64, classes)
    par, A, B, q = _tables(s, "f64")
    for tid, terms, kw in pr.TERM_SETS:
        if kw.get("switch_mode") == "reference":
            continue
        ref = pr.reference(s, s.positions(), s.box, A, B, q, terms, **kw)
        ti, tj = s.types[s.pairs[:, 0]], s.types[s.pairs[:, 1]]
        Ap, Bp = A[ti, tj].astype(LD), B[ti, tj].astype(LD)
        qq = LD(pr.ELEC_FACTOR) * q[s.pairs[:, 0]].astype(LD) * q[s.pairs[:, 1]].astype(LD)
        h = ref.r * LD(1e-5)

        def energy(r):
            ep = pr.pair_partials(r, Ap, Bp, qq, terms, **kw)[0]
            return sum(sum(v) for v in ep.values())

        fd = (energy(ref.r + h) - energy(ref.r - h)) / (2 * h)
        m = ref.included & (np.abs(ref.r - pr.SWITCH_DIST) > 2 * h) & (ref.r + h < pr.CUTOFF)
        assert m.sum() > 400
        assert np.all(np.abs(fd[m] - ref.dEdr[m]) <= 1e-7 * ref.S_F[m]), tid


@pytest.mark.parametrize("prec", ["f32", "f64"])
@pytest.mark.parametrize("classes", [3, 40])
def test_inputs_are_well_conditioned(prec, classes):
    """On exactly the inputs the GPU test uses (every configuration, term set and box), the plain evaluation in the
    engine's precision stays under 16 eps x S in force and energy: what a kernel may lose to the conditioning of the
    inputs is a quarter of the GPU test's 64 eps."""
    s = pr.dimer_system(pr.NP_DTYPE[prec], classes)
    par, A, B, q = _tables(s, prec)
    worstF = worstE = 0.0
    for tid, terms, kw in pr.TERM_SETS:
        for boxname, box in BOXES.items():
            for band in [None] + list(range(pr.N_BANDS)):
                pos = s.positions(band)
                ref = pr.reference(s, pos, box, A, B, q, terms, **kw)
                got = pr.naive(s, pos, box, A, B, q, terms, **kw)
                assert np.array_equal(got.included, ref.included)
                S_atom = ref.S_F[s.pair_of]
                errF = np.abs(got.F.astype(LD) - ref.F).max(axis=1)
                ok = S_atom > 0
                assert np.all(errF[~ok] == 0)
                worstF = max(worstF, float((errF[ok] / S_atom[ok]).max()) / EPS[prec])
                for t in terms:
                    errE = np.abs(got.E[t].astype(LD) - ref.E[t])
                    okE = ref.S_E[t] > 0
                    assert np.all(errE[~okE] == 0)
                    worstE = max(worstE, float((errE[okE] / ref.S_E[t][okE]).max()) / EPS[prec])
    print(f"plain evaluation {prec}, {classes} classes: force {worstF:.1f} eps x S_F, energy {worstE:.1f} eps x S_E")
    assert worstF <= 16 and worstE <= 16


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_why_the_switch_is_scaled_monomial_by_monomial(prec):
    """With |S| and |S'| taken at their VALUES, the scale of a switched force vanishes like (r_c - r)^2 towards the cutoff while
    its sensitivity to r vanishes like (r_c - r) only (the term E S''): the exact closed form, evaluated at a distance that
    carries half an ulp of the engine's precision — less than any kernel's r can carry — already misses 64 eps x that
    scale more than tenfold for every one of the dimers packed at the cutoff.  Scaled monomial by monomial (S_F as returned) the same
    perturbation stays under 16 eps over the whole range."""
    s = pr.dimer_system(pr.NP_DTYPE[prec], 3)
    par, A, B, q = _tables(s, prec)
    eps = EPS[prec]
    for mode in ("reference", "exact"):
        kw = dict(switch_dist=pr.SWITCH_DIST, switch_mode=mode)
        ref = pr.reference(s, s.positions(), s.box, A, B, q, ("lj",), **kw)
        ti, tj = s.types[s.pairs[:, 0]], s.types[s.pairs[:, 1]]
        m = ref.included
        _, fpart, _, _ = pr.pair_partials(ref.r[m] * (1 + LD(eps) / 2), A[ti, tj].astype(LD)[m], B[ti, tj].astype(LD)[m],
                                          np.zeros(m.sum(), dtype=LD), ("lj",), **kw)
        err = np.abs(sum(fpart) - ref.dEdr[m])
        near = (np.abs(ref.r[m] - pr.CUTOFF) < 1.1e-3) & ~s.is_edge[m]
        assert near.sum() >= 16
        assert float((err[near] / ref.S_F_literal[m][near]).min()) > 10 * 64 * eps
        assert float((err[~s.is_edge[m]] / ref.S_F[m][~s.is_edge[m]]).max()) < 16 * eps
