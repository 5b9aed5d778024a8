"""The nonbonded pair VALUE arithmetic, one pair at a time, in every kernel that holds a copy of it (run with `-m gpu`).

The system is tests/_pair_reference.py's: 576 isolated dimers (1 152 atoms), so the force on an atom is ONE pair's force,
and the reference is the long-double closed form on the distance the engine itself sees.  Every test of these kernels
elsewhere compares sums over 90 - 440 partners per atom with absolute tolerances; this one resolves r — the last 1.5 A of
the switch, r2 == r2max, r == switch_dist, the r^-12 end — and tells a wrong force from a wrong energy.

Kernel paths (the second parameter of a case id), and why a case reaches the kernel it names — the selection rule of
launch_list_pair (pair_generic.hip):

    only_lj_el = the terms are LJ and / or electrostatics, nothing else
    lean       = only_lj_el, no pair count wanted, at most kEntryTypes = 32 LJ classes, no PME
    lean                              -> list_pair_fast_f32_kernel (fp32: body pair_fast_body) / list_pair_lean_f64_kernel (fp64)
    otherwise                         -> list_pair_kernel<FAST>, FAST = 1 iff only_lj_el with BOTH terms, no switch,
                                         no energies wanted, no PME  (body pair_fast_lj_rf); FAST = 0: pair_terms

  allpairs  algorithm="allpairs": allpairs_kernel, pair_terms, every term set.
  lean      algorithm="celllist", 3 classes: the lean kernel of the precision, for the LJ / electrostatics sets (a repulsion
            term is not only_lj_el: those two sets run pair_terms on the other paths only).  TMDHIP_LPA = 4, 8, 64 lanes
            per atom.  fp32: the first launch after a list build runs its tail in the checked loop (cutoff by select) and
            writes the row padding; the second runs every group unchecked (cutoff as the factor clamp((r2max' - r2) 2^100)):
            both meet the bar and are identical to the bit.
  generic   algorithm="celllist", 40 classes (> kEntryTypes): list_pair_kernel.  FAST = 1 for the `lj_rf` set evaluated
            for forces only; FAST = 0 for every other set and for every evaluation with energies.  The two
            electrostatics-only sets carry no LJ table (one class, whatever the topology holds) and would run the lean
            kernel: they are evaluated together with the pair count, which the lean kernels do not keep — and the count
            must be the number of included dimers.

Bar: |F_got - F_truth|_inf <= 64 eps S_F per atom of an included pair, exactly 0 for an excluded one, no atom left out
(the buffer is pre-filled with NaN); |F_i + F_j|_inf <= 64 eps S_F; per term and distance band |E_got - sum E_truth| <=
64 eps sum S_E.  Why 64: in the lean fp32 body r2 from the stored coordinates carries ~2 eps, v_rsq_f32 1 ulp, so 1/r is good
to ~2 eps and r^-13 to ~25 eps, plus a handful of roundings of the fused expressions: ~2.5 x headroom, and 4 x the 16 eps the
plain evaluation is held to on the host (test_pair_reference_host.py: it reaches 11.6).  The same multiple in fp64, whose
fast_rsqrt claims full precision.  The observed worst values are printed by every case and recorded in DESIGN.md §15.

Energies are resolved by distance band: compute() returns totals, so nine calls on the same context each keep the dimers
of one band (a factor <= 1.4 of r; the edge dimers are a band of their own) and open all others to 11.7 A, where they
contribute exactly 0 — which also drives the list rebuild.  (Nine, not eight: 0.8 .. 9.18 A is a factor 11.5 > 1.4^7.)
"""

import numpy as np
import pytest
import torch

import _pair_reference as pr
from _golden import PREC, GoldenParameters, box_tensor
from _pair_reference import LD

pytestmark = pytest.mark.gpu

BAR = 64
EPS = {"f32": float(np.finfo(np.float32).eps), "f64": float(np.finfo(np.float64).eps)}
BOXES = {"pbc": np.full(3, pr.BOX), "box0": np.zeros(3)}
SETS = {t[0]: t for t in pr.TERM_SETS}
LEAN_SETS = [t[0] for t in pr.TERM_SETS if not t[0].startswith("repulsion")]
CASES = (
    [("allpairs", t[0], b) for t in pr.TERM_SETS for b in ("pbc", "box0")]
    + [("lean", t, b) for t in LEAN_SETS for b in ("pbc", "box0")]
    + [("generic", t[0], "pbc") for t in pr.TERM_SETS]
)
FD_H = 1e-3  # exact mode: step of the central difference in r (A)

_truth_cache = {}


def _setup(prec, classes):
    s = pr.dimer_system(pr.NP_DTYPE[prec], classes)
    par = GoldenParameters(s.golden(), PREC[prec])
    A, B = par.get_AB()
    return s, par, A.numpy(), B.numpy(), par.charges.numpy()


def _truth(prec, classes, tid, boxname, band):
    """Long-double reference of one configuration, computed once and shared by the paths that use it."""
    key = (prec, classes, tid, boxname, band)
    if key not in _truth_cache:
        s, par, A, B, q = _setup(prec, classes)
        _, terms, kw = SETS[tid]
        _truth_cache[key] = pr.reference(s, s.positions(band), BOXES[boxname], A, B, q, terms, **kw)
    return _truth_cache[key]


def _check_forces(tag, F, ref, s, eps):
    """-> (worst force error, worst third-law residual) in eps x S_F, pairs antisymmetric to the bit, r of the worst."""
    got = F[0].cpu().numpy()
    assert np.isfinite(got).all(), f"{tag}: an atom was left out (NaN pre-fill survives)"
    got = got.astype(LD)
    inc = ref.included[s.pair_of]
    assert np.all(got[~inc] == 0), f"{tag}: a pair beyond the cutoff got a force"
    S = ref.S_F[s.pair_of]
    err = np.abs(got - ref.F).max(axis=1)
    live = inc & (S > 0)
    assert np.all(err[inc & ~live] == 0), tag  # (a neutral atom in an electrostatics-only set)
    ratio = np.zeros(len(S))
    ratio[live] = (err[live] / S[live]).astype(np.float64) / eps
    a = int(np.argmax(ratio))
    Fi, Fj = got[s.pairs[:, 0]], got[s.pairs[:, 1]]
    res = np.abs(Fi + Fj).max(axis=1)
    plive = ref.included & (ref.S_F > 0)
    third = float((res[plive] / ref.S_F[plive]).max()) / eps if plive.any() else 0.0
    nbit = int(np.all(Fi == -Fj, axis=1)[ref.included].sum())
    line = (f"{tag}: force {ratio[a]:.1f} eps x S_F at r = {float(ref.r[s.pair_of[a]]):.6f} (pair {s.pair_of[a]}), "
            f"third law {third:.1f}, antisymmetric to the bit {nbit}/{int(ref.included.sum())}")
    print(line)
    assert ratio[a] <= BAR, line
    assert np.all(res[~plive] == 0) and third <= BAR, line
    return ratio[a], third


def _check_energies(tag, pots, ref, terms, eps):
    worst = 0.0
    for t in terms:
        want, scale = ref.E[t].sum(), ref.S_E[t].sum()
        err = abs(LD(pots[t]) - want)
        if scale == 0:
            assert err == 0, (tag, t)
            continue
        ratio = float(err / scale) / eps
        worst = max(worst, ratio)
        assert ratio <= BAR, f"{tag}: {t} energy {pots[t]!r} vs {float(want)!r}: {ratio:.1f} eps x sum S_E"
    return worst


def _exact_mode_difference(tag, f, s, ref, pos, b, F, prec, A, B, q, terms, kw, dev):
    """The engine against itself: central difference of the band energy in r of one dimer (its atom i moved by -+ h along
    the axis) against the computed force, -F_i . u = dE/dr.  h = 1e-3 A.  The difference's own error is the truncation
    h^2 / 6 max|E'''| over [r - h, r + h] — E''' from the long-double energy by differences (step 1e-3, relative error
    ~1e-6), times 1.1 — plus what the bars above allow the three quantities: 64 eps sum S_E / h for the two energies and
    64 eps S_F for the force."""
    eps = EPS[prec]
    h = FD_H
    band_pairs = np.nonzero((s.band == 7) & ref.included & ~s.is_edge)[0]
    chosen = [band_pairs[np.argmin(np.abs(ref.r[band_pairs].astype(np.float64) - r0))] for r0 in (7.8, 8.3, 8.8)]
    sumSE = float(sum(ref.S_E[t].sum() for t in terms))
    for p in chosen:
        i, j = s.pairs[p]
        r = ref.r[p]
        u = (ref.d[p] / r).astype(np.float64)
        e = []
        for sgn in (+1, -1):
            q_pos = np.array(pos)
            q_pos[i] += sgn * h * u
            pt = torch.tensor(q_pos, device=dev)[None]
            e.append(f.compute(pt, b, None, calculateForces=False)[0])
        fd = (e[0] - e[1]) / (2 * h)
        force = -float(np.dot(F[0, i].cpu().numpy(), u))
        qq = pr.ELEC_FACTOR * q[i] * q[j]
        Aij, Bij = A[s.types[i], s.types[j]], B[s.types[i], s.types[j]]
        k = LD(1e-3)
        rs = r + np.linspace(-h, h, 5).astype(LD)
        E = lambda x: pr.pair_energy_of_r(x, Aij, Bij, qq, terms, **kw)  # noqa: E731
        d3 = (E(rs + 2 * k) - 2 * E(rs + k) + 2 * E(rs - k) - E(rs - 2 * k)) / (2 * k**3)
        tol = 1.1 * h * h / 6 * float(np.abs(d3).max()) + BAR * eps * sumSE / h + BAR * eps * float(ref.S_F[p])
        print(f"{tag}: exact mode at r = {float(r):.4f}: dE/dr by difference {fd:.10e}, from the force {force:.10e}, "
              f"|diff| {abs(fd - force):.2e} (bound {tol:.2e})")
        assert abs(fd - force) <= tol, (tag, float(r), fd, force, tol)


@pytest.mark.parametrize("path,tid,boxname", CASES, ids=[f"{p}-{t}-{b}" for p, t, b in CASES])
@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_pair_resolved(prec, path, tid, boxname, monkeypatch):
    from torchmd_amd import _lib as L
    from torchmd_amd.forces import Forces

    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    dev = torch.device("cuda:0")
    classes = 40 if path == "generic" else 3
    s, par, A, B, q = _setup(prec, classes)
    _, terms, kw = SETS[tid]
    eps = EPS[prec]
    b = box_tensor(BOXES[boxname], 1, PREC[prec], dev)
    algorithm = "allpairs" if path == "allpairs" else "celllist"
    count = path == "generic" and "lj" not in terms and not any(t.startswith("repulsion") for t in terms)
    worstF = worst3 = worstE = 0.0
    for lpa in (4, 8, 64) if path == "lean" else (None,):
        if lpa is not None:
            monkeypatch.setenv("TMDHIP_LPA", str(lpa))
        tag = f"pair-resolved {prec} {path} {tid} {boxname}" + (f" lpa={lpa}" if lpa else "")
        f = Forces(par, terms=list(terms), cutoff=pr.CUTOFF, algorithm=algorithm, **kw)
        # ---- forces only, twice on the same positions
        ref = _truth(prec, classes, tid, boxname, None)
        p = torch.tensor(np.array(s.positions()), device=dev)[None]
        launches = []
        for k in range(2):
            F = torch.full_like(p, float("nan"))
            f._evaluate(p, b, F, False, True, count_pairs=count)
            wF, w3 = _check_forces(f"{tag} launch {k + 1}", F, ref, s, eps)
            worstF, worst3 = max(worstF, wF), max(worst3, w3)
            launches.append(F)
        assert f.stats(p)["algorithm"] == algorithm
        if count:
            assert f.stats(p)["pairs_in_cutoff"] == int(ref.included.sum())
        if path == "lean":
            assert torch.equal(launches[0], launches[1]), f"{tag}: checked and unchecked launch differ"
        if lpa not in (None, 8):
            f.close()
            continue
        # ---- with energies: every dimer, then band by band
        for band in [None] + list(range(pr.N_BANDS)):
            refb = _truth(prec, classes, tid, boxname, band)
            pos = s.positions(band)
            pb = torch.tensor(np.array(pos), device=dev)[None]
            F = torch.full_like(pb, float("nan"))
            if count:
                ebuf = f._evaluate(pb, b, F, True, True, count_pairs=True).cpu().numpy()
                pots = {t: float(ebuf[0, L.ENERGY_SLOT[t]]) for t in terms}
                assert f.stats(pb)["pairs_in_cutoff"] == int(refb.included.sum())
            else:
                pots = f.compute(pb, b, F, returnDetails=True)[0]
            btag = f"{tag} band {band}"
            wF, w3 = _check_forces(btag, F, refb, s, eps)
            wE = _check_energies(btag, pots, refb, terms, eps)
            print(f"{btag}: energy {wE:.1f} eps x sum S_E")
            worstF, worst3, worstE = max(worstF, wF), max(worst3, w3), max(worstE, wE)
            if band == 7 and kw.get("switch_mode") == "exact" and prec == "f64":
                _exact_mode_difference(btag, f, s, refb, pos, b, F, prec, A, B, q, terms, kw, dev)
        f.close()
    print(f"pair-resolved {prec} {path} {tid} {boxname} WORST: force {worstF:.1f} third-law {worst3:.1f} energy {worstE:.1f} (eps x S)")
