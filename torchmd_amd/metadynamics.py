"""Well-tempered metadynamics on one or two collective variables.

    md = Metadynamics([("dihedral", (4, 6, 8, 14)), ("dihedral", (6, 8, 14, 16))], sigma=0.35, height=0.3, frequency=500,
                      temperature=300.0, bias_factor=8.0, grid_bins=64, nreplicas=R)
    forces = Forces(..., metadynamics=md)
    Integrator(systems, forces, ...).step(n)      # deposits a hill every `frequency` steps

A CV is `("distance", (i, j))` (Å, not periodic: needs `grid_min` / `grid_max`) or `("dihedral", (i, j, k, l))` (radians,
periodic on [-pi, pi)).  The bias lives on a grid whose nodes hold the analytic sum of the deposited Gaussians and its
derivatives; the bias IS the cubic / bicubic Hermite interpolant of those nodes, and its force the exact derivative of that.
`walkers="independent"` keeps one grid per replica, `"shared"` one grid that every replica deposits into (multiple walkers).
The grid lives on the device of the `Forces` that holds the object; `grid` reads it back.  `energy_forces` and `deposit_model`
are the numpy models of the bias kernel and of the deposit chain (the tests' reference); the module-level functions are the
expressions of csrc/metad_math.h.

CVs of groups of atoms (csrc/cv_math.h and metad_group.hip):

    ("group_distance", (A, B))   ("group_angle", (A, B, C))   ("group_dihedral", (A, B, C, D))
    ("coordination", (A, B), {"r0": 3.5, "n": 6, "d0": 0.0, "d_max": 9.0})

A group is a sequence of atom indices or `{"atoms": [...], "weights": [...]}`; weights default to the masses the `Forces` hands
over.  The first three act on the centres X_g = x_a0 + sum_a w_a mi(x_a - x_a0) (every member within half a box edge of the
first: `check_extent`), the angle in [0, pi] and not periodic, the dihedral periodic.  The coordination number is
s = sum_{i in A} sum_{j in B, j != i} f(r_ij) with x = (r - d0) / r0, phi = 1 for x <= 0 and 1 / (1 + x^n) otherwise, and, with
`d_max`, f = (phi - phi_max) / (1 - phi_max) below d_max and 0 from there on; in a periodic box `d_max` is required and at most
half the shortest edge (`check_box`).  A "distance" or "dihedral" beside a new kind is served as single-atom groups of weight 1;
a bias of the two old kinds alone is untouched by all this (`grouped` is False)."""

from __future__ import annotations

import ctypes as C
import math

import numpy as np

from . import _lib as L
from .controls import Control, whole_frequency

KINDS = {"distance": 0, "dihedral": 1}
# CVs of groups of atoms (csrc/cv_math.h, tmdhip_set_metadynamics_groups); a bias that names one of them is "grouped", and a
# distance / dihedral beside it is served as single-atom groups of weight 1
GROUP_KINDS = {"group_distance": 2, "group_angle": 3, "group_dihedral": 4, "coordination": 5}
GROUP_ARITY = {2: 2, 3: 3, 4: 4, 5: 2}
PERIODIC_KINDS = ("dihedral", "group_dihedral")
TWO_PI = 2.0 * np.pi


def min_image(d, box):
    d = np.array(d, dtype=np.float64)
    box = np.asarray(box, dtype=np.float64).reshape(3)
    for c in range(3):
        if box[c] != 0.0:
            d[..., c] = d[..., c] - box[c] * np.rint(d[..., c] / box[c])
    return d


def _dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def _cross(a, b):
    return np.array([a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]])


_ATAN_EIGHTHS = (0.0, 0.12435499454676144, 0.24497866312686414, 0.35877067027057225, 0.4636476090008061, 0.5585993153435624,
                 0.6435011087932844, 0.7188299996216245, 0.7853981633974483)


def atan_unit(x):
    """atan on [0, 1] by the four operations alone (metad_math.h: the same operations in the same order, so the same bits)."""
    x = float(x)
    k = int(8.0 * x + 0.5)
    c = 0.125 * k
    z = (x - c) / (1.0 + x * c)
    q = z * z
    p = 1.0 / 17.0
    for n in (15.0, 13.0, 11.0, 9.0, 7.0, 5.0, 3.0):
        p = 1.0 / n - q * p
    p = 1.0 - q * p
    return _ATAN_EIGHTHS[k] + z * p


def atan2_portable(y, x):
    """atan2(y, x) in [-pi, pi] as metad_math.h computes it; (0, 0) gives 0."""
    y, x = float(y), float(x)
    ax, ay = abs(x), abs(y)
    if ax != ax or ay != ay or ax == np.inf or ay == np.inf:
        return float("nan")
    a = 0.0
    if ay <= ax:
        if ax > 0.0:
            a = atan_unit(ay / ax)
    else:
        a = 0.5 * np.pi - atan_unit(ax / ay)
    if x < 0.0:
        a = np.pi - a
    return -a if y < 0.0 else a


def cv_distance(x, box):
    """r = |minimum image of x[0] - x[1]| and its gradients [4,3] (rows 2, 3 zero)."""
    d = min_image(x[0] - x[1], box)
    r = np.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])
    g = np.zeros((4, 3))
    if r > 0.0:
        g[0] = d / r
        g[1] = -g[0]
    return r, g


def cv_dihedral(x, box):
    """The torsion of x[0..3] with the sign of the bonded term, and its gradients [4,3] in the form without 1 / sin phi."""
    b1, b2, b3 = min_image(x[1] - x[0], box), min_image(x[2] - x[1], box), min_image(x[3] - x[2], box)
    A, B = _cross(b1, b2), _cross(b2, b3)
    n2 = _dot(b2, b2)
    nb = np.sqrt(n2)
    A2, B2 = _dot(A, A), _dot(B, B)
    phi = atan2_portable(nb * _dot(b1, B), _dot(A, B))
    g = np.zeros((4, 3))
    if A2 > 0.0 and B2 > 0.0:
        gi, gl = (-nb / A2) * A, (nb / B2) * B
        p, q = _dot(b1, b2) / n2, _dot(b3, b2) / n2
        g[0], g[3] = gi, gl
        g[1] = (-gi - p * gi) + q * gl
        g[2] = (-gl - q * gl) + p * gi
    return phi, g


def hermite_basis(t, h):
    """(val [2,2], der [2,2]): val[a] = (weight of node a's value, of its slope, h included); der = d/ds of those."""
    u = 1.0 - t
    val = np.array([[(1.0 + 2.0 * t) * (u * u), h * (t * (u * u))], [(t * t) * (3.0 - 2.0 * t), h * ((t * t) * (t - 1.0))]])
    der = np.array([[(6.0 * t * (t - 1.0)) / h, u * (1.0 - 3.0 * t)], [(6.0 * t * u) / h, t * (3.0 * t - 2.0)]])
    return val, der


def locate(lo, h, nodes, periodic, s):
    """(k0, k1, t, live): the cell of s on an axis; live = 0 outside a non-periodic grid, where s is clamped."""
    x = (s - lo) / h
    if periodic:
        if not x == x:
            x = 0.0
        fl = np.floor(x)
        k0 = int(fl) % nodes
        return k0, (k0 + 1) % nodes, x - fl, 1.0
    bins, live = nodes - 1, 1.0
    if not x >= 0.0:
        x, live = 0.0, 0.0
    elif x > bins:
        x, live = float(bins), 0.0
    fl = min(np.floor(x), float(bins - 1))
    return int(fl), int(fl) + 1, x - fl, live


def coord_phi(x, n):
    """(phi, d phi / dx) of cv_math.h for an array x: 1 and 0 for x <= 0, else q = x^(n-1) by repeated multiplication,
    1 / (1 + q x) and -(n q) / (1 + q x)^2."""
    x = np.asarray(x, dtype=np.float64)
    on = x > 0.0
    xs = np.where(on, x, 1.0)
    with np.errstate(over="ignore", invalid="ignore"):  # (an infinite distance: phi = 0, the slope is not a number)
        q = np.ones_like(xs)
        for _ in range(1, int(n)):
            q = q * xs
        den = 1.0 + q * xs
        return np.where(on, 1.0 / den, 1.0), np.where(on, -(float(n) * q) / (den * den), 0.0)


def coord_switch(r, r0, n, d0=0.0, d_max=None):
    """(f, df/dr) of the coordination switch for an array of distances (cv_math.h's coord_switch)."""
    r = np.asarray(r, dtype=np.float64)
    phi, dphi = coord_phi((r - d0) / r0, n)
    if d_max is None:
        return phi, dphi / r0
    phimax = coord_phi((d_max - d0) / r0, n)[0]
    scale = 1.0 / (1.0 - phimax)
    inside = r < d_max
    return np.where(inside, (phi - phimax) * scale, 0.0), np.where(inside, (dphi / r0) * scale, 0.0)


def coordination_pairs(pos, box, A, B, r0, n, d0=0.0, d_max=None):
    """Every pair of a coordination CV seen from the atoms of A: (f [nA,nB], gd [nA,nB,3]) with gd = (df/dr / r) mi(x_i - x_j);
    an atom of both sets has zeros against itself.  s = f.sum(), ds/dx_i += gd.sum(1) for i in A, ds/dx_j -= gd.sum(0) for j in B."""
    A, B = np.asarray(A), np.asarray(B)
    d = min_image(pos[A][:, None, :] - pos[B][None, :, :], box)
    r = np.sqrt((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2])
    f, df = coord_switch(r, r0, n, d0, d_max)
    other = A[:, None] != B[None, :]
    f = np.where(other, f, 0.0)
    on = other & (df != 0.0)
    g = np.where(on, df / np.where(on, r, 1.0), 0.0)
    return f, g[..., None] * d


def cv_of_centres(kind, X, box):
    """A CV of centres X [arity,3] (cv_math.h's cv_of_centres, operation by operation): (s, ds/dX [4,3])."""
    g = np.zeros((4, 3))
    if kind == GROUP_KINDS["group_distance"]:
        d = min_image(X[0] - X[1], box)
        r = np.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])
        if r > 0.0:
            g[0] = d / r
            g[1] = -g[0]
        return r, g
    if kind == GROUP_KINDS["group_angle"]:
        u, v = min_image(X[0] - X[1], box), min_image(X[2] - X[1], box)
        nu, nv = np.sqrt(_dot(u, u)), np.sqrt(_dot(v, v))
        co = 1.0
        if nu > 0.0 and nv > 0.0:
            co = _dot(u, v) / (nu * nv)
        co = 1.0 if co > 1.0 else (-1.0 if co < -1.0 else co)
        theta = float(np.arccos(co))
        si = np.sqrt(1.0 - co * co)
        if nu > 0.0 and nv > 0.0 and si > 0.0:
            fa, fc = 1.0 / (nu * si), 1.0 / (nv * si)
            uh, vh = u / nu, v / nv
            g[0] = -(fa * (vh - co * uh))
            g[2] = -(fc * (uh - co * vh))
            g[1] = -g[0] - g[2]
        return theta, g
    return cv_dihedral(X, box)


class Metadynamics(L.SideTerm, Control):
    rank = 3  # (the deposition, as a scheduled control: after the thermostat's application where both fall on one step)
    side_name, side_width = "metadynamics", 3  # (V, s_0, s_1)
    side_potential = slice(0, 1)
    side_apply, side_energy = "tmdhip_metad_apply", "tmdhip_metad_energy"
    refusals = {
        "vmap": "compute() with metadynamics cannot run under torch.vmap (its grids are per replica of the context)",
        "batch": "metadynamics does not support atom groups (batch=): its grids are per replica",
        "barostat": "metadynamics cannot run under barostat=",
        "exchange": "metadynamics cannot run under exchange=: the bias would have to travel with the rung",
        "domain": "metadynamics cannot be domain-decomposed (a CV's atoms would straddle bricks, and atom indices change "
                  "at every migration)",
    }

    def __init__(self, cvs, sigma, height, frequency, temperature, bias_factor=None, grid_min=None, grid_max=None, grid_bins=None,
                 nreplicas=1, walkers="independent"):
        if isinstance(cvs, tuple) and len(cvs) in (2, 3) and isinstance(cvs[0], str):
            cvs = [cvs]
        cvs = list(cvs)
        if not 1 <= len(cvs) <= 2:
            raise ValueError("Metadynamics: one or two CVs (more than 2 CVs are not supported)")
        self.ncv = len(cvs)
        self.kinds, self.atoms = [], np.full((2, 4), -1, dtype=np.int32)
        self.grouped = any(isinstance(cv, (tuple, list)) and len(cv) >= 1 and cv[0] in GROUP_KINDS for cv in cvs)
        self.group_atoms, self.group_weights = [], []  # per group: int32 [n] in the order given; float64 [n] > 0 or None = the masses
        self.cv_kind, self.cv_groups, self.coord = [], [], [None, None]  # the library's kind, the CV's groups, the switch
        self.masses = None  # what a Forces hands over (check): the default weights
        for c, cv in enumerate(cvs):
            if self.grouped:
                self._add_group_cv(c, cv)
                continue
            try:
                kind, at = cv
            except (TypeError, ValueError):
                raise ValueError('Metadynamics: a CV is ("distance", (i, j)) or ("dihedral", (i, j, k, l))') from None
            if kind not in KINDS:
                raise ValueError(f"Metadynamics: unknown CV kind {kind!r} (distance, dihedral)")
            at = np.asarray(at)
            want = 2 if kind == "distance" else 4
            if at.shape != (want,) or not np.issubdtype(at.dtype, np.integer) or np.any(at < 0):
                raise ValueError(f"Metadynamics: a {kind} needs {want} non-negative atom indices")
            if len(np.unique(at)) != want:
                raise ValueError(f"Metadynamics: CV {c} repeats an atom")
            self.kinds.append(kind)
            self.atoms[c, :want] = at
        if int(nreplicas) != nreplicas or nreplicas < 1:
            raise ValueError("Metadynamics: nreplicas must be a positive whole number")
        self.nreplicas = int(nreplicas)
        if walkers not in ("independent", "shared"):
            raise ValueError('Metadynamics: walkers is "independent" or "shared"')
        self.walkers = walkers
        self.sigma = self._per_cv(sigma, "sigma")
        if not np.all(np.isfinite(self.sigma)) or np.any(self.sigma <= 0):
            raise ValueError("Metadynamics: sigma must be finite and positive")
        if not np.isfinite(height) or height <= 0:
            raise ValueError("Metadynamics: height must be finite and positive")
        self.height = float(height)
        self.frequency = whole_frequency(frequency, "Metadynamics: frequency must be a positive whole number of steps")
        if not np.isfinite(temperature) or temperature <= 0:
            raise ValueError("Metadynamics: temperature must be finite and positive")
        self.temperature = float(temperature)
        if bias_factor is not None and (not np.isfinite(bias_factor) or bias_factor <= 1):
            raise ValueError("Metadynamics: bias_factor must be finite and above 1 (None: plain metadynamics)")
        self.bias_factor = None if bias_factor is None else float(bias_factor)
        lo = self._per_cv(grid_min, "grid_min", allow_none=True)
        hi = self._per_cv(grid_max, "grid_max", allow_none=True)
        self.lo, self.h, self.nodes, self.periodic = np.zeros(2), np.ones(2), np.ones(2, dtype=np.int64), [False, False]
        self.grid_min, self.grid_max = np.zeros(2), np.zeros(2)
        bins_in = [None] * self.ncv if grid_bins is None else list(np.atleast_1d(grid_bins))
        if len(bins_in) == 1:
            bins_in = bins_in * self.ncv
        if len(bins_in) != self.ncv:
            raise ValueError("Metadynamics: grid_bins must be a whole number or one per CV")
        self.bins = np.ones(2, dtype=np.int32)
        for c, kind in enumerate(self.kinds):
            if kind in PERIODIC_KINDS:
                a, b = -np.pi, np.pi
            else:
                a, b = lo[c], hi[c]
                if not (np.isfinite(a) and np.isfinite(b)) or not a < b:
                    raise ValueError(f"Metadynamics: CV {c} ({kind}) needs finite grid_min < grid_max")
            nb = bins_in[c]
            if nb is None:
                nb = int(np.ceil((b - a) / (0.5 * self.sigma[c])))
            if int(nb) != nb or nb < 1:
                raise ValueError("Metadynamics: grid_bins must be positive whole numbers")
            h = (b - a) / float(nb)
            if h > 0.5 * self.sigma[c] * (1.0 + 1e-12):
                raise ValueError(f"Metadynamics: CV {c}: the grid spacing {h:.6g} must not exceed sigma / 2 = {0.5 * self.sigma[c]:.6g} "
                                 "(the Hermite interpolant's force error is not small enough to integrate under beyond that)")
            self.bins[c], self.lo[c], self.h[c] = int(nb), a, h
            self.grid_min[c], self.grid_max[c] = a, b
            self.periodic[c] = kind in PERIODIC_KINDS
            self.nodes[c] = int(nb) if self.periodic[c] else int(nb) + 1
        self.ngrids = 1 if walkers == "shared" else self.nreplicas
        self.width = 2 if self.ncv == 1 else 4
        shape = (self.ngrids,) + tuple(int(n) for n in self.nodes[: self.ncv]) + (self.width,)
        self._grid = np.zeros(shape)
        self._eng = None          # the forces._Engine whose context holds the grid
        self._forces = None
        self._host_dirty = False  # the host copy was set and the device has not seen it
        self._dev_dirty = False   # the device has deposited since the host copy was read
        self._log = None          # torch double [capacity, R, ncv + 1] on the device
        self._log_host = np.zeros((0, self.nreplicas, self.ncv + 1))  # hills loaded or deposited before a device log exists
        self.nhills = 0
        self.frozen = False
        self.cv = None      # [R, ncv] of the last evaluation
        self.energy = None  # [R] V(s(x)) of the last evaluation
        if self.grouped:
            self.row_atom = np.unique(np.concatenate(self.group_atoms)).astype(np.int64)
            self.row_role = None
            return
        all_atoms = sorted({int(a) for a in self.atoms.reshape(-1) if a >= 0})
        self.row_atom = np.asarray(all_atoms, dtype=np.int64)
        self.row_role = np.full((len(all_atoms), 2), -1, dtype=np.int64)
        for t, a in enumerate(all_atoms):
            for c in range(self.ncv):
                hit = np.nonzero(self.atoms[c] == a)[0]
                if len(hit):
                    self.row_role[t, c] = hit[0]

    # ------------------------------------------------------------------ CVs of groups
    def _group(self, c, spec, weight_one=False):
        """Add a group: a sequence of indices, or {"atoms": [...], "weights": [...]}; returns its index."""
        weights = None
        if isinstance(spec, dict):
            unknown = sorted(set(spec) - {"atoms", "weights"})
            if unknown or "atoms" not in spec:
                raise ValueError(f'Metadynamics: CV {c}: a group is a list of indices or {{"atoms": [...], "weights": [...]}}')
            spec, weights = spec["atoms"], spec.get("weights")
        atoms = np.atleast_1d(np.asarray(spec))
        if atoms.ndim != 1 or len(atoms) == 0:
            raise ValueError(f"Metadynamics: CV {c}: an empty group (a group is a non-empty list of atom indices)")
        if not np.issubdtype(atoms.dtype, np.integer) or np.any(atoms < 0):
            raise ValueError(f"Metadynamics: CV {c}: a group needs non-negative whole atom indices")
        if len(np.unique(atoms)) != len(atoms):
            raise ValueError(f"Metadynamics: CV {c}: a group repeats an atom")
        if weight_one:
            weights = np.ones(len(atoms))
        if weights is not None:
            weights = np.array(weights, dtype=np.float64)
            if weights.shape != atoms.shape or not np.all(np.isfinite(weights)) or np.any(~(weights > 0)):
                raise ValueError(f"Metadynamics: CV {c}: weights must be [{len(atoms)}], finite and > 0")
        for g, (at, w) in enumerate(zip(self.group_atoms, self.group_weights)):  # (the same group named again: one centre)
            if np.array_equal(at, atoms) and ((w is None and weights is None) or (w is not None and weights is not None and np.array_equal(w, weights))):
                return g
        self.group_atoms.append(atoms.astype(np.int32))
        self.group_weights.append(weights)
        return len(self.group_atoms) - 1

    def _add_group_cv(self, c, cv):
        form = ('Metadynamics: a CV is (kind, groups) with kind group_distance, group_angle or group_dihedral, ("coordination", (A, B), '
                '{"r0": ..., "n": 6, "d0": 0.0, "d_max": ...}), ("distance", (i, j)) or ("dihedral", (i, j, k, l))')
        if not isinstance(cv, (tuple, list)) or len(cv) not in (2, 3) or not isinstance(cv[0], str):
            raise ValueError(form)
        kind = cv[0]
        if kind not in KINDS and kind not in GROUP_KINDS:
            raise ValueError(f"Metadynamics: unknown CV kind {kind!r} ({', '.join(list(KINDS) + list(GROUP_KINDS))})")
        if kind == "coordination" and (len(cv) != 3 or not isinstance(cv[2], dict)):
            raise ValueError('Metadynamics: a coordination CV takes {"r0": ..., "n": 6, "d0": 0.0, "d_max": ...}')
        if len(cv) == 3 and kind != "coordination":
            raise ValueError(form)
        if kind in KINDS:  # served as single-atom groups of weight 1
            at = np.asarray(cv[1])
            want = 2 if kind == "distance" else 4
            if at.shape != (want,) or not np.issubdtype(at.dtype, np.integer) or np.any(at < 0):
                raise ValueError(f"Metadynamics: a {kind} needs {want} non-negative atom indices")
            if len(np.unique(at)) != want:
                raise ValueError(f"Metadynamics: CV {c} repeats an atom")
            code, groups = (2 if kind == "distance" else 4), [self._group(c, [int(a)], weight_one=True) for a in at]
        else:
            code = GROUP_KINDS[kind]
            try:
                specs = list(cv[1])
            except TypeError:
                raise ValueError(form) from None
            if len(specs) != GROUP_ARITY[code]:
                raise ValueError(f"Metadynamics: a {kind} needs {GROUP_ARITY[code]} groups")
            groups = [self._group(c, sp) for sp in specs]
            if code != 5 and len(set(groups)) != len(groups):
                raise ValueError(f"Metadynamics: CV {c}: a group is named twice")
        if code == 5:
            par = dict(cv[2]) if isinstance(cv[2], dict) else None
            if par is None or "r0" not in par or set(par) - {"r0", "n", "d0", "d_max"}:
                raise ValueError('Metadynamics: a coordination CV takes {"r0": ..., "n": 6, "d0": 0.0, "d_max": ...}')
            r0, n, d0, d_max = par["r0"], par.get("n", 6), par.get("d0", 0.0), par.get("d_max")
            if not np.isfinite(r0) or not r0 > 0:
                raise ValueError(f"Metadynamics: CV {c}: r0 must be finite and positive")
            if int(n) != n or not 2 <= n <= 24:
                raise ValueError(f"Metadynamics: CV {c}: n must be a whole number in [2, 24]")
            if not np.isfinite(d0) or d0 < 0:
                raise ValueError(f"Metadynamics: CV {c}: d0 must be finite and >= 0")
            if d_max is not None and (not np.isfinite(d_max) or not d0 < d_max):
                raise ValueError(f"Metadynamics: CV {c}: d_max must lie above d0")
            if len(self.group_atoms[groups[0]]) * len(self.group_atoms[groups[1]]) >= 2**31:
                raise ValueError(f"Metadynamics: CV {c}: |A| |B| must stay below 2^31")
            self.coord[c] = {"r0": float(r0), "n": int(n), "d0": float(d0), "d_max": None if d_max is None else float(d_max)}
        self.kinds.append(kind)
        self.cv_kind.append(code)
        self.cv_groups.append(groups)

    def raw_weights(self, g):
        """The raw weights of group g: the explicit ones, or the masses a `Forces` handed over (`masses` may be set by hand)."""
        if self.group_weights[g] is not None:
            return self.group_weights[g]
        if self.masses is None:
            raise ValueError("Metadynamics: a group without explicit weights needs masses (pass the object to Forces, or set .masses)")
        return np.asarray(self.masses, dtype=np.float64)[self.group_atoms[g]]

    def _table_weights(self, g):
        """What the library's table takes for group g: its raw weights; ones for a set of a coordination CV alone (not read)."""
        centre = any(g in self.cv_groups[c] for c in range(self.ncv) if self.cv_kind[c] != 5)
        if not centre and self.group_weights[g] is None and self.masses is None:
            return np.ones(len(self.group_atoms[g]))
        return self.raw_weights(g)

    def weights(self, g):
        """The normalised weights of group g, the sum taken in member order (as the library normalises)."""
        W = self.raw_weights(g)
        total = 0.0
        for x in W:
            total += float(x)
        return W / total

    def centres(self, pos, box):
        """[G,3] of one replica: X_g = x_a0 + sum_a w_a mi(x_a - x_a0), the sum in the centre block's order (reduce.h)."""
        from .group_restraints import fixed_order_sum

        X = np.zeros((len(self.group_atoms), 3))
        used = {g for c in range(self.ncv) if self.cv_kind[c] != 5 for g in self.cv_groups[c]}
        for g, at in enumerate(self.group_atoms):
            if g not in used:  # (the sets of a coordination CV: no centre is read)
                continue
            x0 = pos[at[0]]
            X[g] = x0 + fixed_order_sum(self.weights(g)[:, None] * min_image(pos[at] - x0, box))
        return X

    def check_extent(self, pos, box):
        """Whether the centres' precondition holds for `pos` [R,N,3] or [N,3] in `box`: every atom of a group of a centre CV
        lies within half a box edge of the group's first atom along every periodic axis."""
        if not self.grouped:
            return True
        pos = np.asarray(pos, dtype=np.float64)
        if pos.ndim == 2:
            pos = pos[None]
        box = self._boxes(box, pos.shape[0])
        used = {g for c in range(self.ncv) if self.cv_kind[c] != 5 for g in self.cv_groups[c]}
        for g in sorted(used):
            at = self.group_atoms[g]
            for r in range(pos.shape[0]):
                d, per = np.abs(min_image(pos[r, at] - pos[r, at[0]], box[r])), box[r] != 0  # (as GroupRestraints.check_extent)
                if np.any(d[:, per] >= 0.5 * box[r][per] * (1.0 - 1e-12)):
                    return False
        return True

    def check_box(self, box, R=None):
        """What the library refuses of a coordination CV in a box (ValueError): with any non-zero edge `d_max` is required
        and must not exceed half the shortest non-zero edge."""
        if not self.grouped:
            return
        for b in self._boxes(box, self.nreplicas if R is None else R):
            edges = b[b != 0]
            for c in range(self.ncv):
                if self.cv_kind[c] != 5 or not len(edges):
                    continue
                d_max = self.coord[c]["d_max"]
                if d_max is None:
                    raise ValueError(f"Metadynamics: CV {c}: a coordination CV in a periodic box needs d_max")
                if d_max > 0.5 * edges.min():
                    raise ValueError(f"Metadynamics: CV {c}: d_max must not exceed half the shortest non-zero box edge")

    def _per_cv(self, v, what, allow_none=False):
        if v is None:
            if allow_none:
                return np.full(self.ncv, np.nan)
            raise ValueError(f"Metadynamics: {what} is needed")
        a = np.asarray([np.nan if x is None else x for x in np.atleast_1d(v)], dtype=np.float64)
        if a.shape == (1,):
            a = np.repeat(a, self.ncv)
        if a.shape != (self.ncv,):
            raise ValueError(f"Metadynamics: {what} must be a scalar or one value per CV")
        return a

    # ------------------------------------------------------------------ refusals of a Forces
    def check(self, natoms, masses=None, virtual_sites=None):
        at = self.row_atom
        if at[-1] >= natoms:
            raise ValueError(f"Metadynamics: atom {at[-1]} is beyond the system's {natoms} atoms")
        if masses is not None:
            m = np.array(masses, dtype=np.float64).reshape(-1)
            if np.any(~(m[at] > 0)):
                raise ValueError(f"Metadynamics: atom {at[~(m[at] > 0)][0]} belongs to a CV and has no mass")
            if self.grouped and (self.masses is None or not np.array_equal(self.masses, m)):
                # the default weights: a context that holds older ones is set again, from the grid as it stands on the device
                if self._eng is not None and self._eng.ctx:
                    self._pull()
                self.masses, self._eng, self._dev_dirty = m, None, False
        if virtual_sites is not None and getattr(virtual_sites, "nsites", 0):
            hit = np.intersect1d(at, np.asarray(virtual_sites.sites))
            if len(hit):
                raise ValueError(f"Metadynamics: atom {hit[0]} is a virtual site (use its parents)")

    @property
    def kdt(self):
        """k_B (bias_factor - 1) T, or None for plain metadynamics."""
        from .integrator import BOLTZMAN

        return None if self.bias_factor is None else BOLTZMAN * (self.bias_factor - 1.0) * self.temperature

    # ------------------------------------------------------------------ the model
    def _grid_of(self, grid, r):
        return grid[0 if self.walkers == "shared" else r]

    def cv_values(self, pos, box):
        """(s [ncv], gradients [ncv,4,3]) of one replica: `pos` [N,3], `box` edge lengths [3]."""
        if self.grouped:
            return self.group_cv_values(pos, box)
        s, g = np.zeros(self.ncv), np.zeros((self.ncv, 4, 3))
        for c, kind in enumerate(self.kinds):
            if kind == "distance":
                s[c], g[c] = cv_distance(pos[self.atoms[c, :2]], box)
            else:
                s[c], g[c] = cv_dihedral(pos[self.atoms[c]], box)
        return s, g

    def group_cv_values(self, pos, box):
        """(s [ncv], ds/dx as a list of [N,3] per CV) of one replica for a grouped bias, after cv_math.h and the scatter kernel
        of metad_group.hip: a centre CV adds w_a ds/dX_g over its groups in ascending group order, a coordination CV what an
        atom gathers as a member of A, then of B."""
        pos = np.asarray(pos, dtype=np.float64)
        box = np.asarray(box, dtype=np.float64).reshape(3)
        s, grads = np.zeros(self.ncv), []
        X = None
        for c in range(self.ncv):
            ds = np.zeros_like(pos)
            if self.cv_kind[c] == 5:
                A, B = (self.group_atoms[g] for g in self.cv_groups[c])
                f, gd = coordination_pairs(pos, box, A, B, **self.coord[c])
                # (the addends are the kernel's to the bit; their sums are taken exactly and rounded once, so that a comparison
                #  carries the rounding of the device's order of summation alone)
                s[c] = math.fsum(f.ravel())
                ds[A] += np.array([[math.fsum(gd[i, :, k]) for k in range(3)] for i in range(len(A))]).reshape(len(A), 3)
                ds[B] += -np.array([[math.fsum(gd[:, j, k]) for k in range(3)] for j in range(len(B))]).reshape(len(B), 3)
            else:
                X = self.centres(pos, box) if X is None else X
                s[c], gC = cv_of_centres(self.cv_kind[c], X[self.cv_groups[c]], box)
                for g, role in sorted((g, role) for role, g in enumerate(self.cv_groups[c])):
                    ds[self.group_atoms[g]] += self.weights(g)[:, None] * gC[role]
            grads.append(ds)
        return s, grads

    def interp(self, grid, s):
        """(V, dV [ncv]) of the Hermite interpolant on one grid ([n0,2] or [n0,n1,4]) at CV values s [ncv]."""
        k0a, k0b, t0, live0 = locate(self.lo[0], self.h[0], int(self.nodes[0]), self.periodic[0], s[0])
        v0, d0 = hermite_basis(t0, self.h[0])
        if self.ncv == 1:
            V = dv = 0.0
            for a, k in enumerate((k0a, k0b)):
                nd = grid[k]
                V += v0[a, 0] * nd[0] + v0[a, 1] * nd[1]
                dv += d0[a, 0] * nd[0] + d0[a, 1] * nd[1]
            return V, np.array([live0 * dv])
        k1a, k1b, t1, live1 = locate(self.lo[1], self.h[1], int(self.nodes[1]), self.periodic[1], s[1])
        v1, d1 = hermite_basis(t1, self.h[1])
        V = da = db = 0.0
        for a, ka in enumerate((k0a, k0b)):
            for b, kb in enumerate((k1a, k1b)):
                nd = grid[ka, kb]
                V += (v0[a, 0] * v1[b, 0] * nd[0] + v0[a, 1] * v1[b, 0] * nd[1]) + (v0[a, 0] * v1[b, 1] * nd[2] + v0[a, 1] * v1[b, 1] * nd[3])
                da += (d0[a, 0] * v1[b, 0] * nd[0] + d0[a, 1] * v1[b, 0] * nd[1]) + (d0[a, 0] * v1[b, 1] * nd[2] + d0[a, 1] * v1[b, 1] * nd[3])
                db += (v0[a, 0] * d1[b, 0] * nd[0] + v0[a, 1] * d1[b, 0] * nd[1]) + (v0[a, 0] * d1[b, 1] * nd[2] + v0[a, 1] * d1[b, 1] * nd[3])
        return V, np.array([live0 * da, live1 * db])

    def _boxes(self, box, R):
        box = np.asarray(box, dtype=np.float64)
        if box.ndim == 3:
            box = np.stack([np.diag(b) for b in box])
        return np.broadcast_to(box.reshape(-1, 3), (R, 3))

    def _positions(self, pos):
        pos = np.asarray(pos, dtype=np.float64)
        if pos.ndim == 2:
            pos = pos[None]
        if pos.shape[0] != self.nreplicas:
            raise ValueError(f"Metadynamics: {pos.shape[0]} replicas of positions for {self.nreplicas} replicas of bias")
        return pos

    def energy_forces(self, pos, box, grid=None):
        """The numpy model of the bias kernel: `pos` [R,N,3] (or [N,3] with one replica), `box` [3], [R,3] or a diagonal
        [R,3,3]; `grid`: as `self.grid` (the default).  Returns (V [R], forces [R,N,3], CVs [R,ncv]) in double."""
        pos = self._positions(pos)
        R = pos.shape[0]
        box = self._boxes(box, R)
        grid = self.grid if grid is None else grid
        E, F, S = np.zeros(R), np.zeros_like(pos), np.zeros((R, self.ncv))
        for r in range(R):
            s, g = self.cv_values(pos[r], box[r])
            V, dV = self.interp(self._grid_of(grid, r), s)
            E[r], S[r] = V, s
            if self.grouped:
                f = np.zeros_like(pos[r])
                for c in range(self.ncv):  # (CV order)
                    f += -dV[c] * g[c]
                F[r, self.row_atom] = f[self.row_atom]
                continue
            for t, a in enumerate(self.row_atom):
                f = np.zeros(3)
                for c in range(self.ncv):  # (CV order: the order in which the kernel's thread adds)
                    if self.row_role[t, c] >= 0:
                        f += -dV[c] * g[c, self.row_role[t, c]]
                F[r, a] = f
        return E, F, S

    def gauss_terms(self, s0, w):
        """What a hill of height w at s0 adds to every node of one grid: [n0,2] or [n0,n1,4]."""
        dl = []
        for c in range(self.ncv):
            d = (self.lo[c] + np.arange(int(self.nodes[c]), dtype=np.float64) * self.h[c]) - s0[c]
            if self.periodic[c]:
                d = d - TWO_PI * np.rint(d / TWO_PI)
            dl.append(d)
        sg = self.sigma
        if self.ncv == 1:
            e = w * np.exp(-((dl[0] * dl[0]) / (2.0 * (sg[0] * sg[0]))))
            return np.stack([e, (-dl[0] / (sg[0] * sg[0])) * e], axis=-1)
        d0, d1 = dl[0][:, None], dl[1][None, :]
        e = w * np.exp(-((d0 * d0) / (2.0 * (sg[0] * sg[0])) + (d1 * d1) / (2.0 * (sg[1] * sg[1]))))
        return np.stack([e, (-d0 / (sg[0] * sg[0])) * e, (-d1 / (sg[1] * sg[1])) * e,
                         ((d0 / (sg[0] * sg[0])) * (d1 / (sg[1] * sg[1]))) * e], axis=-1)

    def hill_height(self, V):
        return self.height if self.bias_factor is None else self.height * np.exp(-V / self.kdt)

    def deposit_model(self, pos, box, grid=None):
        """The numpy model of the deposit chain: the rows (s0..., w) [R, ncv + 1] with every height read from `grid` as it
        is, and the grid after every node has added its hills (a shared grid: all R, in replica order).  `grid` is not changed."""
        pos = self._positions(pos)
        R = pos.shape[0]
        box = self._boxes(box, R)
        grid = np.array(self.grid if grid is None else grid, dtype=np.float64)
        rows = np.zeros((R, self.ncv + 1))
        for r in range(R):
            s, _ = self.cv_values(pos[r], box[r])
            V, _ = self.interp(self._grid_of(grid, r), s)
            rows[r, : self.ncv], rows[r, self.ncv] = s, self.hill_height(V)
        for r in range(R):
            g = self._grid_of(grid, r)
            g += self.gauss_terms(rows[r, : self.ncv], rows[r, self.ncv])
        return grid, rows

    def bias(self, s, replica=0):
        """V of the interpolant at CV values `s` ([ncv] or [M, ncv]) on the grid of `replica` (a shared grid: the one)."""
        s = np.asarray(s, dtype=np.float64)
        g = self._grid_of(self.grid, replica)
        if s.ndim <= 1 and s.size == self.ncv:
            return self.interp(g, s.reshape(self.ncv))[0]
        return np.array([self.interp(g, x)[0] for x in s.reshape(-1, self.ncv)])

    def free_energy(self):
        """-gamma / (gamma - 1) V on the nodes (-V for plain metadynamics): [grids, n0(, n1)]."""
        V = self.grid[..., 0]
        return -V if self.bias_factor is None else -(self.bias_factor / (self.bias_factor - 1.0)) * V

    def node_coordinates(self):
        return [self.lo[c] + np.arange(int(self.nodes[c])) * self.h[c] for c in range(self.ncv)]

    # ------------------------------------------------------------------ the device side
    def group_descriptor(self):
        """(tmdhip_metad_group_desc, the arrays it points at) of a grouped bias."""
        d = L.MetadGroupDesc()
        d.struct_size = C.sizeof(L.MetadGroupDesc)
        d.enable, d.nreplicas, d.ncv, d.ngroups = 1, self.nreplicas, self.ncv, len(self.group_atoms)
        d.shared = 1 if self.walkers == "shared" else 0
        for c in range(2):
            for a in range(4):
                d.groups[c][a] = -1
        for c in range(self.ncv):
            d.kind[c] = self.cv_kind[c]
            for a, g in enumerate(self.cv_groups[c]):
                d.groups[c][a] = g
            d.bins[c] = int(self.bins[c])
            d.grid_min[c], d.grid_max[c], d.sigma[c] = self.grid_min[c], self.grid_max[c], self.sigma[c]
            if self.coord[c] is not None:
                p = self.coord[c]
                d.coord_n[c], d.coord_r0[c], d.coord_d0[c] = p["n"], p["r0"], p["d0"]
                d.coord_dmax[c] = 0.0 if p["d_max"] is None else p["d_max"]
        off = np.concatenate([[0], np.cumsum([len(a) for a in self.group_atoms])]).astype(np.int32)
        keep = [np.ascontiguousarray(off), np.ascontiguousarray(np.concatenate(self.group_atoms).astype(np.int32)),
                np.ascontiguousarray(np.concatenate([self._table_weights(g) for g in range(len(self.group_atoms))]).astype(np.float64))]
        d.group_off_host, d.member_atom_host, d.member_weight_host = (a.ctypes.data_as(C.c_void_p) for a in keep)
        return d, keep

    def descriptor(self):
        d = L.MetadDesc()
        d.struct_size = C.sizeof(L.MetadDesc)
        d.enable, d.nreplicas, d.ncv = 1, self.nreplicas, self.ncv
        d.shared = 1 if self.walkers == "shared" else 0
        for c in range(self.ncv):
            d.kind[c] = KINDS[self.kinds[c]]
            for a in range(4):
                d.atoms[c][a] = int(self.atoms[c, a])
            d.bins[c] = int(self.bins[c])
            d.grid_min[c], d.grid_max[c], d.sigma[c] = self.grid_min[c], self.grid_max[c], self.sigma[c]
        return d

    def _pull(self):
        if self._dev_dirty and self._eng is not None:
            out = np.empty(self._grid.shape)
            L.check(self._eng.lib.tmdhip_metad_get_grid(self._eng.ctx, out.ctypes.data_as(C.POINTER(C.c_double)), out.size),
                    "tmdhip_metad_get_grid")
            self._grid = out
        self._dev_dirty = False

    @property
    def grid(self):
        """The node values [grids, n0, 2] or [grids, n0, n1, 4] (a host copy: read back after a deposition)."""
        self._pull()
        return self._grid

    def fetch(self):
        """Read the grid back from the device whatever this object believes about it (after direct calls of the library)."""
        self._dev_dirty = self._eng is not None
        return self.grid

    def set_grid(self, grid):
        grid = np.ascontiguousarray(grid, dtype=np.float64)
        if grid.shape != self._grid.shape:
            raise ValueError(f"Metadynamics.set_grid: the grid is {self._grid.shape}, got {grid.shape}")
        self._grid, self._dev_dirty, self._host_dirty = grid.copy(), False, True

    def sync(self, eng, owner=None):
        """Make the context of `eng` hold this bias (tmdhip_set_metadynamics on first sight, the grid when the host's is newer)."""
        if self._eng is not eng:
            self._pull()
            if eng.nreplicas != self.nreplicas:
                raise ValueError(f"the metadynamics bias was made for {self.nreplicas} replicas, the positions have {eng.nreplicas}")
            if self.grouped:
                d, keep = self.group_descriptor()
                L.check(eng.lib.tmdhip_set_metadynamics_groups(eng.ctx, C.byref(d)), "tmdhip_set_metadynamics_groups")
                del keep
            else:
                d = self.descriptor()
                L.check(eng.lib.tmdhip_set_metadynamics(eng.ctx, C.byref(d)), "tmdhip_set_metadynamics")
            self._eng, self._host_dirty = eng, True
        if self._host_dirty:
            g = np.ascontiguousarray(self._grid)
            L.check(eng.lib.tmdhip_metad_set_grid(eng.ctx, g.ctypes.data_as(C.POINTER(C.c_double)), g.size), "tmdhip_metad_set_grid")
            self._host_dirty = False

    def detach(self):
        """Read the grid back and forget the context that held it (before that context is destroyed)."""
        if self._eng is not None and self._eng.ctx:
            self._pull()
        self._eng, self._dev_dirty = None, False

    def deposit(self, systems):
        """One deposition at the CV values of `systems.pos`, enqueued on the current stream (tmdhip_metad_deposit): a row of
        the hills log on the device and one read-modify-write per node; nothing is read back."""
        import torch

        if self._forces is None:
            raise RuntimeError("Metadynamics.deposit: give the object to a Forces(metadynamics=) first")
        pos = systems.pos
        eng = self._forces._engine(pos.detach())
        boxes = self._forces._replica_boxes(systems.box, pos.shape[0])
        if self.grouped:
            self.check_box(boxes.reshape(-1, 3))
        with torch.cuda.device(pos.device):
            self.sync(eng)
            if self._log is None or self._log.device != pos.device:
                self._log = torch.zeros((64, self.nreplicas, self.ncv + 1), dtype=torch.float64, device=pos.device)
                nh = len(self._log_host)
                if nh:
                    while self._log.shape[0] < nh + 1:
                        self._log = torch.cat([self._log, torch.zeros_like(self._log)])
                    self._log[:nh] = torch.as_tensor(self._log_host, device=pos.device)
            if self.nhills >= self._log.shape[0]:
                self._log = torch.cat([self._log, torch.zeros_like(self._log)])
            row = self._log[self.nhills]
            plain = self.bias_factor is None
            L.check(eng.lib.tmdhip_metad_deposit(eng.ctx, C.c_void_p(pos.data_ptr()), boxes.ctypes.data_as(C.POINTER(C.c_double)),
                                                 self.height, 0.0 if plain else self.kdt, 1 if plain else 0, C.c_void_p(row.data_ptr()),
                                                 C.c_void_p(torch.cuda.current_stream(pos.device).cuda_stream)), "tmdhip_metad_deposit")
        self.nhills += 1
        self._dev_dirty = True

    def after_segment(self, integrator, out):
        """A frozen bias still cuts the call and deposits nothing.  The potential energy returned contains V(s(x)) as of
        before the deposition, and `systems.forces` stay as they are: a Gaussian is flat at its own centre."""
        if not self.frozen:
            self.deposit(integrator.systems)
        return out

    def report(self, out):
        """Take (V, s_0, s_1) [R,3] of an evaluation: `energy` [R] and `cv` [R, ncv]."""
        out = np.asarray(out, dtype=np.float64).reshape(self.nreplicas, 3)
        self.energy, self.cv = out[:, 0].copy(), out[:, 1 : 1 + self.ncv].copy()

    store = report  # (the side-term protocol's name for it)

    def monitor_columns(self):
        return ("bias",) + tuple(f"cv{c}" for c in range(self.ncv))

    def monitor_row(self, k):
        """The bias energy inside `epot` and the CVs of replica k."""
        return {"bias": float(self.energy[k]), **{f"cv{c}": float(self.cv[k, c]) for c in range(self.ncv)}}

    def hills(self):
        """The hills log [n, R, ncv + 1]: (s0..., w) of every deposition."""
        if self._log is None:
            return self._log_host[: self.nhills].copy()
        return self._log[: self.nhills].cpu().numpy()

    @classmethod
    def from_config(cls, conf, nreplicas):
        """The `metadynamics:` mapping of run.py: the constructor's arguments, `cvs` as [[kind, [atoms]], ...]."""
        conf = dict(conf)
        known = ("cvs", "sigma", "height", "frequency", "temperature", "bias_factor", "grid_min", "grid_max", "grid_bins", "walkers")
        unknown = sorted(set(conf) - set(known))
        if unknown:
            raise ValueError(f"metadynamics: unknown keys {unknown} (known: {', '.join(known)})")
        missing = [k for k in known[:5] if k not in conf]
        if missing:
            raise ValueError(f"metadynamics: missing keys {missing}")
        def atom_list(v):  # a list of indices, or the name of a .npy file of indices
            if isinstance(v, str):
                v = np.load(v)
            return [int(a) for a in np.asarray(v).reshape(-1)]

        try:
            cvs = []
            for entry in conf.pop("cvs"):
                kind = str(entry[0])
                if kind in GROUP_KINDS:
                    groups = tuple(atom_list(g) for g in entry[1])
                    cvs.append((kind, groups, dict(entry[2])) if kind == "coordination" else (kind, groups))
                else:
                    kind, atoms = entry
                    cvs.append((kind, tuple(int(a) for a in atoms)))
        except (TypeError, ValueError, IndexError, KeyError):
            raise ValueError('metadynamics: cvs is a list of [kind, [atoms]] entries, e.g. [["dihedral", [4, 6, 8, 14]]], '
                             '["group_distance", [[...], [...]]] or ["coordination", [[...], [...]], {r0: 3.5, n: 6, d_max: 9.0}]') from None
        return cls(cvs, nreplicas=nreplicas, **conf)

    # ------------------------------------------------------------------ restart
    def save(self, path):
        np.savez(path, grid=self.grid, hills=self.hills(), lo=self.lo, h=self.h, nodes=self.nodes, sigma=self.sigma,
                 shared=np.array(self.walkers == "shared"))

    def load(self, path):
        z = np.load(path if str(path).endswith(".npz") else str(path) + ".npz")
        if z["grid"].shape != self._grid.shape or not np.array_equal(z["lo"], self.lo) or not np.array_equal(z["h"], self.h):
            raise ValueError("Metadynamics.load: the file was written for another grid")
        hills = np.asarray(z["hills"], dtype=np.float64)
        if hills.ndim != 3 or hills.shape[1:] != (self.nreplicas, self.ncv + 1):
            raise ValueError("Metadynamics.load: the hills log was written for other replicas or CVs")
        self.set_grid(z["grid"])
        self._log, self._log_host, self.nhills = None, hills.copy(), len(hills)
