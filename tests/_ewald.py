"""NumPy fp64 host references for Ewald electrostatics in an orthorhombic periodic box.

* `ewald`        classic Ewald sum: real space over lattice images, reciprocal space over |n| <= kmax, self, excluded-pair
                 and neutralising-background terms.  Converged, it is exact and does not depend on beta.
* `pme`          smooth PME (Essmann et al. 1995) with the library's conventions (torchmd_amd/csrc/pme.hip): atom i with
                 u = K (s - floor(s)), s = x / L, contributes M_p(w + j) to grid point floor(u) - j; B-spline moduli with
                 the neighbour mean where a modulus is below 1e-7; real space within the cutoff under the minimum image.

Both return (energy, forces) in kcal/mol and kcal/mol/A with charges in e.  Excluded pairs (i, j) lose their minimum-image
Coulomb interaction: real space leaves them out and the correction -k q_i q_j erf(beta r)/r removes their share of the
reciprocal sum.
"""

import math

import numpy as np
from scipy.special import erf, erfc

KE = 332.06371307417066
NACL_MADELUNG = 1.747564594633


def ewald_beta(cutoff, tolerance):
    return math.sqrt(-math.log(2.0 * tolerance)) / cutoff


def _excl_pairs(excl):
    if excl is None or len(excl) == 0:
        return np.zeros((0, 2), dtype=np.int64)
    e = np.sort(np.asarray(excl, dtype=np.int64).reshape(-1, 2), axis=1)
    e = e[e[:, 0] != e[:, 1]]
    return np.unique(e, axis=0)


def _min_image(d, box):
    return d - box * np.round(d / box)


def excluded_correction(pos, q, box, beta, excl):
    """-k q_i q_j erf(beta r)/r over the excluded pairs (minimum image), and its forces."""
    pos = np.asarray(pos, np.float64)
    F = np.zeros_like(pos)
    e = _excl_pairs(excl)
    if len(e) == 0:
        return 0.0, F
    i, j = e[:, 0], e[:, 1]
    d = _min_image(pos[i] - pos[j], box)
    r = np.linalg.norm(d, axis=1)
    qq = KE * q[i] * q[j]
    E = -np.sum(qq * erf(beta * r) / r)
    # dE/dr = -qq (2 beta/sqrt(pi) e^{-b^2 r^2} / r - erf(beta r)/r^2)
    dEdr = -qq * (2 * beta / math.sqrt(math.pi) * np.exp(-(beta * r) ** 2) / r - erf(beta * r) / r**2)
    f = -(dEdr / r)[:, None] * d
    np.add.at(F, i, f)
    np.add.at(F, j, -f)
    return E, F


def self_and_background(q, box, beta):
    V = float(np.prod(box))
    return -KE * beta / math.sqrt(math.pi) * np.sum(q * q) - KE * math.pi * np.sum(q) ** 2 / (2 * V * beta * beta)


def ewald(pos, q, box, beta, excl=None, nimg=2, kmax=12):
    """Classic Ewald sum (energy, forces)."""
    pos = np.asarray(pos, np.float64)
    q = np.asarray(q, np.float64)
    box = np.asarray(box, np.float64)
    n = len(q)
    F = np.zeros_like(pos)
    E = 0.0
    ex = _excl_pairs(excl)
    exmask = np.zeros((n, n), dtype=bool)
    exmask[ex[:, 0], ex[:, 1]] = exmask[ex[:, 1], ex[:, 0]] = True
    d0 = _min_image(pos[:, None, :] - pos[None, :, :], box)  # [n, n, 3]
    qq = KE * q[:, None] * q[None, :]
    rng = range(-nimg, nimg + 1)
    for a in rng:
        for b in rng:
            for c in rng:
                shift = np.array([a, b, c], np.float64) * box
                d = d0 + shift
                r = np.linalg.norm(d, axis=2)
                keep = r > 0
                if a == 0 and b == 0 and c == 0:
                    keep &= ~exmask
                rr = np.where(keep, r, 1.0)
                e = np.where(keep, qq * erfc(beta * rr) / rr, 0.0)
                E += 0.5 * e.sum()
                dEdr = -(e / rr + np.where(keep, qq * 2 * beta / math.sqrt(math.pi) * np.exp(-(beta * rr) ** 2) / rr, 0.0))
                F += -np.sum((dEdr / rr)[:, :, None] * d, axis=1)
    # reciprocal space
    V = float(np.prod(box))
    k = np.arange(-kmax, kmax + 1)
    mx, my, mz = np.meshgrid(k, k, k, indexing="ij")
    m = np.stack([mx.ravel(), my.ravel(), mz.ravel()], 1).astype(np.float64)
    m = m[np.any(m != 0, axis=1)] / box
    m2 = np.sum(m * m, axis=1)
    f = np.exp(-math.pi**2 * m2 / beta**2) / m2
    keepk = f > 1e-300
    m, m2, f = m[keepk], m2[keepk], f[keepk]
    for s in range(0, len(m), 4096):
        mm, ff = m[s : s + 4096], f[s : s + 4096]
        th = 2 * math.pi * pos @ mm.T  # [n, k]
        cs, sn = np.cos(th), np.sin(th)
        C, S = q @ cs, q @ sn
        E += KE / (2 * math.pi * V) * np.sum(ff * (C * C + S * S))
        # F_i = -(k/(2 pi V)) sum f 4 pi m q_i (S cos - C sin)
        g = (S[None, :] * cs - C[None, :] * sn) * ff[None, :]  # [n, k]
        F += -KE * 2.0 / V * q[:, None] * (g @ mm)
    Ex, Fx = excluded_correction(pos, q, box, beta, excl)
    return E + Ex + self_and_background(q, box, beta), F + Fx


def bspline(w, p):
    """M_p(w + j), j = 0 .. p-1, and the derivatives, for every w (same recursion as pme.hip)."""
    w = np.asarray(w, np.float64)
    a = np.zeros((len(w), p))
    a[:, 0] = w
    a[:, 1] = 1 - w
    dth = None
    for n in range(3, p + 1):
        if n == p:
            dth = a - np.concatenate([np.zeros((len(w), 1)), a[:, :-1]], axis=1)
        b = np.zeros_like(a)
        for j in range(p):
            x = w + j
            hi = a[:, j] if j < n - 1 else 0.0
            lo = a[:, j - 1] if j > 0 else 0.0
            b[:, j] = (x * hi + (n - x) * lo) / (n - 1)
        a = b
    return a, dth


def bspline_moduli(K, p):
    a, _ = bspline(np.zeros(1), p)
    a = a[0]
    mod = np.zeros(K)
    for m in range(K):
        arg = 2 * math.pi * m * np.arange(p - 1) / K
        re, im = np.sum(a[1:p] * np.cos(arg)), np.sum(a[1:p] * np.sin(arg))
        mod[m] = re * re + im * im
    for m in range(K):
        if mod[m] < 1e-7:
            mod[m] = 0.5 * (mod[(m - 1) % K] + mod[(m + 1) % K])
    return 1.0 / mod


def pme_reciprocal(pos, q, box, beta, grid, order):
    pos = np.asarray(pos, np.float64)
    qs = np.asarray(q, np.float64) * math.sqrt(KE)
    box = np.asarray(box, np.float64)
    K = np.asarray(grid, dtype=np.int64)
    s = pos / box
    s = s - np.floor(s)
    u = s * K
    b = np.floor(u).astype(np.int64)
    w = u - b
    b = np.where(b >= K, b - K, b)
    th, dth = zip(*[bspline(w[:, d], order) for d in range(3)])
    Q = np.zeros(tuple(K))
    idx = [(b[:, d][:, None] - np.arange(order)[None, :]) % K[d] for d in range(3)]  # [n, p]
    for jx in range(order):
        for jy in range(order):
            for jz in range(order):
                np.add.at(Q, (idx[0][:, jx], idx[1][:, jy], idx[2][:, jz]), qs * th[0][:, jx] * th[1][:, jy] * th[2][:, jz])
    S = np.fft.fftn(Q)
    f = [np.fft.fftfreq(K[d]) * K[d] / box[d] for d in range(3)]
    m2 = f[0][:, None, None] ** 2 + f[1][None, :, None] ** 2 + f[2][None, None, :] ** 2
    B = [bspline_moduli(int(K[d]), order) for d in range(3)]
    V = float(np.prod(box))
    with np.errstate(divide="ignore", invalid="ignore"):
        G = B[0][:, None, None] * B[1][None, :, None] * B[2][None, None, :] * np.exp(-math.pi**2 * m2 / beta**2) / (math.pi * V * m2)
    G[0, 0, 0] = 0.0
    E = 0.5 * np.sum(G * np.abs(S) ** 2)
    phi = np.fft.ifftn(G * S).real * float(np.prod(K))
    g = np.zeros_like(pos)
    for jx in range(order):
        for jy in range(order):
            for jz in range(order):
                v = phi[idx[0][:, jx], idx[1][:, jy], idx[2][:, jz]]
                g[:, 0] += dth[0][:, jx] * th[1][:, jy] * th[2][:, jz] * v
                g[:, 1] += th[0][:, jx] * dth[1][:, jy] * th[2][:, jz] * v
                g[:, 2] += th[0][:, jx] * th[1][:, jy] * dth[2][:, jz] * v
    F = -qs[:, None] * g * (K / box)[None, :]
    return E, F


def _real_space_kdtree(pos, q, box, beta, cutoff, exkeys):
    """real_space over the pairs a periodic k-d tree finds (O(N) memory; for systems of 10^5 atoms)."""
    from scipy.spatial import cKDTree

    n = len(q)
    wrapped = pos - box * np.floor(pos / box)
    wrapped[wrapped >= box] = 0.0  # (x - L floor(x / L) may round up to L)
    # a slightly wider search, then the dense path's own test r^2 <= cutoff^2 on the minimum-image difference
    pairs = cKDTree(wrapped, boxsize=box).query_pairs(cutoff * (1 + 1e-9), output_type="ndarray")
    gi, gj = np.minimum(pairs[:, 0], pairs[:, 1]), np.maximum(pairs[:, 0], pairs[:, 1])
    dd = _min_image(pos[gi] - pos[gj], box)
    r2 = np.sum(dd * dd, axis=1)
    keep = r2 <= cutoff * cutoff
    if len(exkeys):
        keep &= ~np.isin(gi * n + gj, exkeys)
    gi, gj, dd, r2 = gi[keep], gj[keep], dd[keep], r2[keep]
    r = np.sqrt(r2)
    qq = KE * q[gi] * q[gj]
    e = qq * erfc(beta * r) / r
    dEdr = -(e / r + qq * 2 * beta / math.sqrt(math.pi) * np.exp(-(beta * r) ** 2) / r)
    f = -(dEdr / r)[:, None] * dd
    F = np.stack([np.bincount(gi, f[:, d], n) - np.bincount(gj, f[:, d], n) for d in range(3)], axis=1)
    return float(e.sum()), F


def real_space(pos, q, box, beta, cutoff, excl=None, chunk=1024, pairs="dense"):
    """erfc(beta r)/r over the non-excluded pairs within the cutoff (minimum image).  pairs="dense": every pair, in
    chunks of rows; pairs="kdtree": the pairs of a periodic k-d tree (scipy.spatial.cKDTree), same result to rounding."""
    pos = np.asarray(pos, np.float64)
    q = np.asarray(q, np.float64)
    n = len(q)
    ex = _excl_pairs(excl)
    exkeys = np.sort(ex[:, 0] * n + ex[:, 1])
    if pairs == "kdtree":
        return _real_space_kdtree(pos, q, np.asarray(box, np.float64), beta, cutoff, exkeys)
    assert pairs == "dense", pairs
    E = 0.0
    F = np.zeros_like(pos)
    for s in range(0, n, chunk):
        i = np.arange(s, min(n, s + chunk))
        d = _min_image(pos[i][:, None, :] - pos[None, :, :], box)
        r2 = np.sum(d * d, axis=2)
        ii, jj = np.nonzero((r2 <= cutoff * cutoff) & (np.arange(n)[None, :] > i[:, None]))
        gi, gj = i[ii], jj
        keys = gi * n + gj
        keep = ~np.isin(keys, exkeys) if len(exkeys) else np.ones(len(keys), bool)
        ii, gi, gj = ii[keep], gi[keep], gj[keep]
        dd = d[ii, gj]
        r = np.sqrt(r2[ii, gj])
        qq = KE * q[gi] * q[gj]
        e = qq * erfc(beta * r) / r
        E += e.sum()
        dEdr = -(e / r + qq * 2 * beta / math.sqrt(math.pi) * np.exp(-(beta * r) ** 2) / r)
        f = -(dEdr / r)[:, None] * dd
        np.add.at(F, gi, f)
        np.add.at(F, gj, -f)
    return E, F


def pme(pos, q, box, beta, cutoff, grid, order, excl=None, pairs="dense"):
    """Smooth PME total: real space + reciprocal + excluded-pair correction + self + background."""
    box = np.asarray(box, np.float64)
    q = np.asarray(q, np.float64)
    Er, Fr = real_space(pos, q, box, beta, cutoff, excl, pairs=pairs)
    Ek, Fk = pme_reciprocal(pos, q, box, beta, grid, order)
    Ex, Fx = excluded_correction(pos, q, box, beta, excl)
    return Er + Ek + Ex + self_and_background(q, box, beta), Fr + Fk + Fx


def nacl_lattice(r0, cells=2):
    """Rock salt: `cells`^3 conventional cells of edge 2 r0 (r0 = nearest-neighbour distance); (pos, q, box)."""
    pts, qs = [], []
    n = 2 * cells
    for a in range(n):
        for b in range(n):
            for c in range(n):
                pts.append((a * r0, b * r0, c * r0))
                qs.append(1.0 if (a + b + c) % 2 == 0 else -1.0)
    return np.array(pts), np.array(qs), np.full(3, n * r0)


def random_ions(n, box, seed=0, min_dist=2.0, net=0):
    """n ions of charge +-1 (net charge `net`) at random positions at least `min_dist` apart (minimum image)."""
    rng = np.random.default_rng(seed)
    box = np.asarray(box, np.float64)
    pos = []
    while len(pos) < n:
        p = rng.uniform(0, 1, 3) * box
        if all(np.linalg.norm(_min_image(p - o, box)) >= min_dist for o in pos):
            pos.append(p)
    q = np.array([1.0] * ((n + net) // 2) + [-1.0] * ((n - net) // 2))
    rng.shuffle(q)
    return np.array(pos), q
