"""Isolated dimers and a long-double reference of the nonbonded pair arithmetic, one pair at a time (numpy only).

The system (`dimer_system`): 576 dimers = 1 152 atoms near the sites of a 9 x 9 x 9 lattice (spacing 20 A, periodic box
180 A), built for cutoff 9, switch distance 7.5 and the default skin.  No atom has more than ONE other atom within
cutoff + 1.5 A, in the scan configuration and in every band configuration (below), so the force on an atom is the force
of one pair, and an energy is a sum over the few dozen pairs of a band.

  * 512 scan dimers, random orientations, centres jittered by up to 2 A around their site: 448 with distances log-spaced
    over [0.8, 9.18] A (1.02 x cutoff: the last ones are out), 32 packed within 1e-3 A of the switch distance, 32 within
    1e-3 A of the cutoff.  None lies within 1e-4 A of the cutoff: the in/out decision is the edge dimers' business.
    A quarter sit on sites of a box face (centre within 1 A of it); their atoms are wrapped into [0, box) and interact
    through the minimum image with k = +-1.
  * 64 edge dimers, axis-aligned on coordinates that are multiples of 2^-10 A, one of them then moved by one ulp of its
    coordinate: fl(x_i - x_j) and |d| are exact in fp32 and in fp64.  |d| = 9 exactly (in), its successor (out), 7.5 and
    its two neighbours; each of these again across a periodic face (there one ulp of the coordinate near 173 is 16 ulp of 9:
    |d| = 9 -+ ulp(173)); each on every axis.  Four more have |d|^2 == r2max as the engine rounds it (the successor of 81:
    9.0 along one axis, a tiny exact offset along another): the one value at which the lean fp32 kernel's arithmetic cutoff
    needs its `+ 1`.
  * classes = 3: three LJ classes (one neutral, two of opposite charge), all six class pairs at every distance;
    classes = 40: more LJ classes than a list entry's type field holds.
  * the atom indices are shuffled: the two atoms of a dimer are not neighbours in memory.

Band configurations (`DimerSystem.positions(band)`): only the dimers of one band keep their distance, all others are
opened to 11.7 A (1.3 x cutoff) along their axis and contribute exactly 0.  Scan bands 0..7 each span a factor
(9.18 / 0.8)^(1/8) = 1.357 of r; the edge dimers are band 8.

The reference (`reference`): the closed forms of the reference implementation's pair potentials (forces.py:390-491) in
np.longdouble.  The DISTANCE is the engine's: coordinates as stored in the engine's precision, d = fl(x_i - x_j), for a
straddling pair d = fl(d - k box), all in that precision (pair_math.h: min_image), and only then long double.  The
parameters are taken as given (the A / B tables and the charges of the Parameters object), unrounded.

Errors are measured against condition scales, not against the value: S_F = sum of the absolute values of the partial
force terms |sw f12| + |sw f6| + |e12 dsw| + |e6 dsw| + |f_coul| + |f_rf|, S_E likewise from the partial energies.  The
plain relative error is useless where the LJ force changes sign.  `naive` is the same arithmetic written plainly in the
engine's precision: it says how well conditioned the inputs are (tests/test_pair_reference_host.py).
"""

from types import SimpleNamespace

import numpy as np

LD = np.longdouble
ELEC_FACTOR = 332.06371307417066  # the reference's 1/(4 pi eps0) in kcal A / (mol e^2)
CUTOFF, SWITCH_DIST, BOX, SPACING = 9.0, 7.5, 180.0, 20.0
OPEN_DIST = 1.3 * CUTOFF  # 11.7 A
ISOLATION = CUTOFF + 1.5
DIELECTRIC = 78.5
R_MIN, R_MAX = 0.8, 1.02 * CUTOFF
N_LOG, N_PACKED, N_EDGE = 448, 32, 64
N_SCAN = N_LOG + 2 * N_PACKED
N_SCAN_BANDS, EDGE_BAND = 8, 8
N_BANDS = N_SCAN_BANDS + 1
NP_DTYPE = {"f32": np.float32, "f64": np.float64}
ENERGY_TERMS = ("lj", "electrostatics", "repulsion", "repulsioncg")
_CLASS_PAIRS3 = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))


def _edge_specs():
    """(axis, a, b, moved, ulps): the first atom at coordinate a of the axis, the second at b, then atom `moved` (0 / 1)
    stepped by `ulps` representable numbers.  The moved atom's binade is the binade of |d| where the pair is interior
    (one ulp of the coordinate = one ulp of |d|); across a face the atom near 173 moves."""
    per_axis = []
    for a, b, moved in ((1.0, 10.0, 1), (11.5, 2.5, 0)):  # |d| = 9
        per_axis += [(a, b, moved, 0), (a, b, moved, +1)]
    for a, b, moved in ((0.25, 7.75, 1), (7.625, 0.125, 0)):  # |d| = 7.5
        per_axis += [(a, b, moved, 0), (a, b, moved, -1), (a, b, moved, +1)]
    for a, b, moved in ((2.0, 173.0, 1), (177.5, 6.5, 0)):  # |d| = 9 through the face: stepping towards the face shortens
        per_axis += [(a, b, moved, 0), (a, b, moved, -1)]
    for a, b, moved in ((1.5, 174.0, 1), (175.25, 2.75, 0)):  # |d| = 7.5 through the face
        per_axis += [(a, b, moved, 0), (a, b, moved, -1), (a, b, moved, +1)]
    specs = [(ax,) + s + (None,) for ax in range(3) for s in per_axis]
    # r2 == r2max: 9.0 along one axis and a small offset dy along another, (dx, dy, 0) exact in the engine's precision, with
    # dy^2 within half an ulp of ulp(81): the engine's |d|^2 rounds to the successor of 81, the largest value whose
    # correctly rounded square root is still 9.0 — included by the reference's `norm(d) <= cutoff`, although |d| > 9
    specs += [(0, 1.0, 10.0, 1, 0, 1), (1, 10.0, 1.0, 0, 0, 2), (2, 2.0, 173.0, 1, 0, 0), (0, 177.5, 6.5, 0, 0, 2)]
    assert len(specs) == N_EDGE
    return specs


def threshold_offset(dtype):
    """dy of the r2 == r2max dimers: dy^2 = 1.125 ulp32(81) in fp32 (3 x 2^-10 A), exactly ulp64(81) in fp64 (2^-23 A)."""
    return 3 * 2.0**-10 if np.dtype(dtype) == np.float32 else 2.0**-23


def engine_norm2(d):
    """|d|^2 as pair_math.h's norm2 rounds it: fp32 fma(dz, dz, fma(dy, dy, dx dx)) — products and sums formed in long
    double, which holds them exactly for the operands used here, and rounded once —, fp64 (dx dx + dy dy) + dz dz."""
    if d.dtype == np.float32:
        x, y, z = (d[:, k].astype(LD) for k in range(3))
        s = (x * x).astype(np.float32)
        s = (y * y + s.astype(LD)).astype(np.float32)
        return (z * z + s.astype(LD)).astype(np.float32)
    return (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]


def engine_includes(d, cutoff):
    """The reference's decision `norm(d) <= cutoff` in the precision of d (a correctly rounded square root)."""
    return np.sqrt(engine_norm2(d)) <= d.dtype.type(cutoff)


def _min_image_np(d, box):
    return d - box * np.rint(d / box)


class DimerSystem:
    def __init__(self, dtype, classes, seed):
        assert classes in (3, 40)
        self.dtype = np.dtype(dtype).type
        self.classes = classes
        self.box = np.full(3, BOX)
        rng = np.random.default_rng(seed)
        npairs = N_SCAN + N_EDGE
        centre = np.zeros((npairs, 3))
        unit = np.zeros((npairs, 3))
        dist = np.zeros(npairs)
        explicit = {}  # edge dimers: their two positions, exact in self.dtype
        placed = np.empty((4 * npairs, 3))  # the four points of every placed dimer (ends at its distance and opened)
        nplaced = 0

        def points(c, u, r):
            return np.stack([c + 0.5 * r * u, c - 0.5 * r * u, c + 0.5 * OPEN_DIST * u, c - 0.5 * OPEN_DIST * u])

        def clear_of(pts, others):
            d = _min_image_np(pts[:, None, :] - others[None, :, :], BOX)
            return len(others) == 0 or (d * d).sum(-1).min() > ISOLATION**2

        def clear_of_all(pts):
            return clear_of(pts, placed[:nplaced])

        # ---- edge dimers: near the low face of their axis, one lattice column each
        count = [0, 0, 0]
        for e, (ax, a, b, moved, ulps, perp) in enumerate(_edge_specs()):
            p = N_SCAN + e
            k = count[ax]
            count[ax] += 1
            col = (2 + k % 6, 2 + k // 6)
            off = ((k % 5) - 2) * 0.3125, ((k % 3) - 1) * 0.4375
            xi, xj = np.zeros(3), np.zeros(3)
            for o, other in enumerate([x for x in range(3) if x != ax]):
                xi[other] = xj[other] = SPACING * col[o] + off[o]
            xi[ax], xj[ax] = a, b
            assert np.all(xi * 1024 == np.rint(xi * 1024)) and np.all(xj * 1024 == np.rint(xj * 1024))
            if perp is not None:
                xi[perp] += threshold_offset(self.dtype)
            xi, xj = xi.astype(self.dtype), xj.astype(self.dtype)
            tgt = xi if moved == 0 else xj
            if ulps:
                tgt[ax] = np.nextafter(tgt[ax], self.dtype(np.inf if ulps > 0 else -np.inf))
            explicit[p] = (xi, xj)
            d = _min_image_np(xi.astype(np.float64) - xj.astype(np.float64), BOX)
            dist[p] = np.sqrt((d * d).sum())
            unit[p] = d / dist[p]
            centre[p] = xj.astype(np.float64) + 0.5 * d
            pts = points(centre[p], unit[p], dist[p])
            assert clear_of_all(pts), "edge dimers are isolated by construction"
            placed[nplaced:nplaced + 4] = pts
            nplaced += 4

        # ---- scan dimers
        r = np.empty(N_SCAN)
        r[:N_LOG] = R_MIN * (R_MAX / R_MIN) ** (np.arange(N_LOG) / (N_LOG - 1))
        near = np.abs(r[:N_LOG] - CUTOFF) < 3e-4
        r[:N_LOG][near] = CUTOFF - 3e-4
        r[N_LOG:N_LOG + N_PACKED] = SWITCH_DIST + rng.uniform(-1e-3, 1e-3, N_PACKED)
        r[N_LOG + N_PACKED:] = CUTOFF + rng.choice([-1.0, 1.0], N_PACKED) * rng.uniform(3e-4, 1e-3, N_PACKED)
        dist[:N_SCAN] = r
        on_face = np.zeros(N_SCAN, dtype=bool)
        on_face[rng.permutation(N_SCAN)[: N_SCAN // 4]] = True
        sites = np.stack(np.meshgrid(*[np.arange(9)] * 3, indexing="ij"), -1).reshape(-1, 3)
        sites = sites[rng.permutation(len(sites))]
        free = np.ones(len(sites), dtype=bool)
        site_on_face = (sites == 0).any(axis=1)
        for p in range(N_SCAN):
            done = False
            for s in np.nonzero(free & (site_on_face == on_face[p]))[0]:
                # (only points within jitter + half an opened dimer + the isolation distance of the site can matter)
                ds = _min_image_np(placed[:nplaced] - SPACING * sites[s], BOX)
                nearby = placed[:nplaced][(ds * ds).sum(-1) < (2 * 3**0.5 + 0.5 * OPEN_DIST + ISOLATION + 0.1) ** 2]
                for _ in range(8):
                    u = rng.normal(size=3)
                    u /= np.linalg.norm(u)
                    jitter = rng.uniform(-1.0, 1.0, 3) * np.where(sites[s] == 0, 1.0, 2.0)
                    c = SPACING * sites[s] + jitter
                    pts = points(c, u, r[p])
                    if clear_of(pts, nearby):
                        done = True
                        break
                if done:
                    break
            assert done, "no isolated place left for a scan dimer"
            free[s] = False
            centre[p], unit[p] = c, u
            placed[nplaced:nplaced + 4] = pts
            nplaced += 4

        self.npairs = npairs
        self.natoms = 2 * npairs
        self.centre, self.unit, self.dist = centre, unit, dist
        self.explicit = explicit
        self.is_edge = np.arange(npairs) >= N_SCAN
        self.on_face = np.concatenate([on_face, np.zeros(N_EDGE, dtype=bool)])
        band = np.floor(N_SCAN_BANDS * np.log(dist / R_MIN) / np.log(R_MAX / R_MIN)).astype(np.int64)
        self.band = np.where(self.is_edge, EDGE_BAND, np.clip(band, 0, N_SCAN_BANDS - 1))
        perm = rng.permutation(self.natoms)
        while np.abs(perm[0::2] - perm[1::2]).min() <= 1:  # the two atoms of a dimer are no neighbours in memory
            perm = rng.permutation(self.natoms)
        self.pairs = np.stack([perm[0::2], perm[1::2]], axis=1).astype(np.int64)  # (i, j) of every dimer
        self.pair_of = np.empty(self.natoms, dtype=np.int64)
        self.pair_of[self.pairs[:, 0]] = self.pair_of[self.pairs[:, 1]] = np.arange(npairs)

        # ---- classes and charges
        types = np.zeros(self.natoms, dtype=np.int64)
        k = np.arange(npairs)
        if classes == 3:
            cp = np.array(_CLASS_PAIRS3)[k % 6]
            ti, tj = cp[:, 0], cp[:, 1]
            sigma = np.array([3.40, 3.15, 4.05])
            epsilon = np.array([0.238, 0.152, 0.070])
            qclass = np.array([0.0, 0.834, -0.834])
        else:
            ti, tj = (7 * k + 1) % classes, (11 * k + 3) % classes
            c = np.arange(classes)
            sigma = 2.6 + 1.5 * ((c * 17) % classes) / classes
            epsilon = 0.05 + 0.25 * ((c * 23) % classes) / classes
            qclass = np.array([0.0, 0.834, -0.834])[c % 3]
        swap = rng.random(npairs) < 0.5  # which atom of the dimer carries which class
        types[self.pairs[:, 0]] = np.where(swap, tj, ti)
        types[self.pairs[:, 1]] = np.where(swap, ti, tj)
        self.types = types
        self.nonbonded_params = np.stack([sigma, epsilon], axis=1)
        self.charges = qclass[types]
        self.masses = np.full(self.natoms, 39.95)
        self._pos = {}

    def positions(self, band=None):
        """[natoms, 3] in the system's precision, wrapped into [0, box).  band = None: every dimer at its distance;
        band = b: the dimers of band b at their distance, every other dimer opened to OPEN_DIST along its axis."""
        if band not in self._pos:
            keep = np.ones(self.npairs, dtype=bool) if band is None else self.band == band
            r = np.where(keep, self.dist, OPEN_DIST)[:, None]
            xi = self.centre + 0.5 * r * self.unit
            xj = self.centre - 0.5 * r * self.unit
            pos = np.empty((self.natoms, 3), dtype=self.dtype)
            for x, col in ((xi, 0), (xj, 1)):
                w = x - np.floor(x / BOX) * BOX
                w = w.astype(self.dtype)
                w[w >= self.dtype(BOX)] = 0  # (a coordinate just below 0 can round up to the box edge)
                pos[self.pairs[:, col]] = w
            for p, (ei, ej) in self.explicit.items():
                if keep[p]:
                    pos[self.pairs[p, 0]], pos[self.pairs[p, 1]] = ei, ej
            pos.setflags(write=False)
            self._pos[band] = pos
        return self._pos[band]

    def golden(self):
        """The arrays `_golden.GoldenParameters` is built from."""
        return {"par_charges": self.charges, "par_masses": self.masses, "par_types": self.types,
                "par_nonbonded_params": self.nonbonded_params}


_SYSTEMS = {}


def dimer_system(dtype, classes=3, seed=11):
    key = (np.dtype(dtype).name, classes, seed)
    if key not in _SYSTEMS:
        _SYSTEMS[key] = DimerSystem(dtype, classes, seed)
    return _SYSTEMS[key]


def stored_delta(pos, pairs, box):
    """d = x_i - x_j of every pair as the engine forms it, in the precision of `pos`: one rounding for the difference,
    then (periodic edges only) d - box * round(d / box) with the product and the difference rounded separately."""
    dt = pos.dtype.type
    d = pos[pairs[:, 0]] - pos[pairs[:, 1]]
    assert d.dtype == pos.dtype
    for k in range(3):
        if box[k] != 0:
            b = dt(box[k])
            kk = np.rint(d[:, k] / b)
            d[:, k] = d[:, k] - b * kk
    return d


def _rf_constants(cutoff, real):
    denom = real(2 * DIELECTRIC + 1)
    return real(1) / real(cutoff) ** 3 * real(DIELECTRIC - 1) / denom, real(1) / real(cutoff) * real(3 * DIELECTRIC) / denom


def pair_partials(r, A, B, qq, terms, rfa=False, switch_dist=None, switch_mode="reference", cutoff=CUTOFF):
    """The partial energy and dE/dr terms of pairs at distance r (any real type; closed forms of forces.py:390-491).
    Returns ({term: [partial energies]}, [partial dE/dr terms], {term: [energy scales]}, [force scales]); an energy / the
    force coefficient is the sum of its partials, a condition scale S the sum of the scales.  A scale is the absolute
    value of its partial term, with the switching polynomials taken monomial by monomial as the reference writes them:
    |S| -> 1 + 10 t^3 + 15 t^4 + 6 t^5, |S'| -> (30 t^2 + 60 t^3 + 30 t^4) / (r_c - r_s)  (see the module docstring)."""
    real = r.dtype.type
    one = real(1)
    rinv = one / r
    rinv6 = rinv**6
    rinv12 = rinv6 * rinv6
    epart = {t: [] for t in terms}
    escale = {t: [] for t in terms}
    fpart, fscale = [], []
    if "lj" in terms:
        e12, e6 = A * rinv12, -B * rinv6
        f12, f6 = real(-12) * A * rinv12 * rinv, real(6) * B * rinv6 * rinv
        sw = sw_abs = np.ones_like(r)
        if switch_dist is not None:
            m = r > real(switch_dist)
            width = real(cutoff) - real(switch_dist)
            t = np.where(m, (r - real(switch_dist)) / width, real(0))
            sw = one + t * t * t * (real(-10) + t * (real(15) - t * real(6)))
            dsw = t * t * (real(-30) + t * (real(60) - t * real(30))) / width
            sw_abs = one + t * t * t * (real(10) + t * (real(15) + t * real(6)))
            dsw_abs = t * t * (real(30) + t * (real(60) + t * real(30))) / width
            if switch_mode == "reference":  # upstream's explicit force divides the switching term by r once more
                dsw, dsw_abs = dsw * rinv, dsw_abs * rinv
            else:
                assert switch_mode == "exact"
            fpart += [sw * f12, sw * f6, e12 * dsw, e6 * dsw]
            fscale += [sw_abs * np.abs(f12), sw_abs * np.abs(f6), np.abs(e12) * dsw_abs, np.abs(e6) * dsw_abs]
        else:
            fpart += [f12, f6]
            fscale += [np.abs(f12), np.abs(f6)]
        epart["lj"] = [sw * e12, sw * e6]
        escale["lj"] = [sw_abs * np.abs(e12), sw_abs * np.abs(e6)]
    if "electrostatics" in terms:
        if rfa:
            krf, crf = _rf_constants(cutoff, real)
            epart["electrostatics"] = [qq * rinv, qq * krf * r * r, -qq * crf]
            f_el = [-qq * rinv * rinv, real(2) * krf * qq * r]
        else:
            epart["electrostatics"] = [qq * rinv]
            f_el = [-qq * rinv * rinv]
        escale["electrostatics"] = [np.abs(x) for x in epart["electrostatics"]]
        fpart += f_el
        fscale += [np.abs(x) for x in f_el]
    if "repulsion" in terms:
        epart["repulsion"] = [A * rinv12]
        escale["repulsion"] = [np.abs(A * rinv12)]
        fpart += [real(-12) * A * rinv12 * rinv]
        fscale += [np.abs(fpart[-1])]
    if "repulsioncg" in terms:
        epart["repulsioncg"] = [B * rinv6]
        escale["repulsioncg"] = [np.abs(B * rinv6)]
        fpart += [real(-6) * B * rinv6 * rinv]
        fscale += [np.abs(fpart[-1])]
    return epart, fpart, escale, fscale


def _evaluate(real, system, pos, box, A, B, charges, terms, cutoff, **opts):
    pairs = system.pairs
    d = stored_delta(pos, pairs, np.asarray(box, dtype=np.float64)).astype(real)
    if real is LD:
        r = np.sqrt((d * d).sum(axis=1))
    else:  # the plain evaluation: every operation rounded in the engine's precision
        r = np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2])
    ti, tj = system.types[pairs[:, 0]], system.types[pairs[:, 1]]
    Ap, Bp = np.asarray(A)[ti, tj].astype(real), np.asarray(B)[ti, tj].astype(real)
    q = np.asarray(charges).astype(real)
    qq = real(ELEC_FACTOR) * q[pairs[:, 0]] * q[pairs[:, 1]]
    epart, fpart, escale, fscale = pair_partials(r, Ap, Bp, qq, terms, cutoff=cutoff, **opts)
    # in or out is the engine's documented decision (it differs from |d| <= cutoff for the r2 == r2max dimers only)
    included = engine_includes(stored_delta(pos, pairs, np.asarray(box, dtype=np.float64)), cutoff)
    zero = np.zeros_like(r)
    E = {t: np.where(included, sum(epart[t], zero), zero) for t in terms}
    S_E = {t: np.where(included, sum(escale[t], zero), zero) for t in terms}
    dEdr = np.where(included, sum(fpart, zero), zero)
    S_F = np.where(included, sum(fscale, zero), zero)
    S_F_literal = np.where(included, sum((np.abs(x) for x in fpart), zero), zero)
    fv = -(dEdr / r)[:, None] * d  # force on atom i; atom j gets the opposite
    F = np.zeros((system.natoms, 3), dtype=real)
    F[pairs[:, 0]] = fv
    F[pairs[:, 1]] = -fv
    return SimpleNamespace(F=F, E=E, S_F=S_F, S_E=S_E, S_F_literal=S_F_literal, included=included, r=r, d=d, dEdr=dEdr)


def reference(system, pos, box, A, B, charges, terms, rfa=False, switch_dist=None, switch_mode="reference", cutoff=CUTOFF):
    """Long-double truth for the dimers of `system` at the stored positions `pos` (the engine's precision) in `box`
    (three edges; 0 = open).  Returns F [natoms, 3] (the force on every atom: its one pair's), E {term: [npairs]},
    S_F [npairs], S_E {term: [npairs]}, included [npairs] (r <= cutoff), r, d, dEdr; an excluded pair has zeros."""
    return _evaluate(LD, system, pos, box, A, B, charges, terms, cutoff, rfa=rfa, switch_dist=switch_dist, switch_mode=switch_mode)


def naive(system, pos, box, A, B, charges, terms, rfa=False, switch_dist=None, switch_mode="reference", cutoff=CUTOFF):
    """The same closed forms evaluated plainly in the precision of `pos` (sqrt, divisions, powers by multiplication)."""
    return _evaluate(pos.dtype.type, system, pos, box, A, B, charges, terms, cutoff, rfa=rfa, switch_dist=switch_dist,
                     switch_mode=switch_mode)


def pair_energy_of_r(r, A, B, qq, terms, **opts):
    """Total long-double energy of one pair as a function of r alone (for derivatives by differences)."""
    epart = pair_partials(np.asarray(r, dtype=LD).reshape(-1), LD(A), LD(B), LD(qq), terms, **opts)[0]
    return sum(sum(v) for v in epart.values())


# the term sets every kernel path is tested with: (id, terms, Forces keywords)
TERM_SETS = (
    ("lj", ("lj",), dict()),
    ("lj_sw_ref", ("lj",), dict(switch_dist=SWITCH_DIST, switch_mode="reference")),
    ("lj_sw_exact", ("lj",), dict(switch_dist=SWITCH_DIST, switch_mode="exact")),
    ("coul", ("electrostatics",), dict()),
    ("rf", ("electrostatics",), dict(rfa=True)),
    ("lj_rf", ("lj", "electrostatics"), dict(rfa=True)),
    ("lj_rf_sw", ("lj", "electrostatics"), dict(rfa=True, switch_dist=SWITCH_DIST, switch_mode="reference")),
    ("repulsion", ("repulsion",), dict()),
    ("repulsioncg", ("repulsioncg",), dict()),
)
