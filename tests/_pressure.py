"""A numpy model of the pressure observable: the molecular virial of the nonbonded force field, the kinetic term
of the molecules' centres and the energy whose volume derivative the virial is.

    W_aa = sum_{i<j} f_ij,a (d_ij,a - delta_i,a + delta_j,a)          f_ij = -(dE/dr) d_ij / r, the force on i

(the two visits of a pair, from i and from j, of the kernels' 1/2 sum_i sum_j d f - sum_i delta_i F_i added up).  The pair set:
dense O(N^2) in chunks of rows minus the exclusions, or, for the one large box, candidates from a periodic k-d tree with a
margin (the decision is the model's own in both cases).  Closed forms: `_pair_reference.pair_partials`.

Precision modes.  "f64": everything in float64.  "f32": the positions are taken as stored in float32 and d is formed with numpy
float32 operations in the engine's order — x_i - x_j, d * invbox, rint, box * k, d - p, each one IEEE rounding (pair_math.h:
min_image) — and the cutoff decision is the engine's (`engine_includes`); everything after that runs in float64.  The model thus
has the engine's distance, as the truth of tests/_pair_reference.py does.

The scale S_a = sum_{i<j} S_F / r (d_a^2 + (|delta_i,a| + |delta_j,a|) |d_a|), S_F the monomial-wise force scale of
`pair_partials`: what one relative rounding error of the pair force moves W_aa by at most.
"""

from types import SimpleNamespace

import numpy as np

from _pair_reference import ELEC_FACTOR, engine_includes, pair_partials

NP_DTYPE = {"f32": np.float32, "f64": np.float64}


def molecule_centres(pos, mass, off, mem, mol_of):
    """R_I [nmol, 3] (mass weighted, float64) and delta_i = r_i - R_I(i) [N, 3]."""
    M = np.add.reduceat(mass[mem], off[:-1])
    R = np.stack([np.add.reduceat((mass[:, None] * pos)[mem, k], off[:-1]) for k in range(3)], axis=1) / M[:, None]
    return R, pos - R[mol_of], M


def kinetic_model(vel, mass, off, mem):
    """sum_I M_I V_I,a^2 [3] with V_I = sum m v / M_I."""
    M = np.add.reduceat(mass[mem], off[:-1])
    P = np.stack([np.add.reduceat((mass[:, None] * vel)[mem, k], off[:-1]) for k in range(3)], axis=1)
    return (P * P / M[:, None]).sum(axis=0)


def engine_delta(p, i, j, box):
    """d = x_i - x_j of the pairs as the engine forms it, in the precision of `p`."""
    dt = p.dtype.type
    d = p[i] - p[j]
    for k in range(3):
        if box[k] != 0:
            b = dt(box[k])
            inv = dt(1) / b
            kk = np.rint(d[:, k] * inv)
            prod = b * kk
            d[:, k] = d[:, k] - prod
    assert d.dtype == p.dtype
    return d


def _exclusion_keys(excl_csr, n):
    off, idx = excl_csr
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(off))
    return np.unique(rows * n + np.asarray(idx, dtype=np.int64))


def dense_pairs(n, chunk=512):
    """Chunks (i, j) of all pairs i < j."""
    for i0 in range(0, n, chunk):
        i1 = min(n, i0 + chunk)
        ii, jj = np.meshgrid(np.arange(i0, i1), np.arange(i0 + 1, n), indexing="ij")
        keep = jj > ii
        yield ii[keep], jj[keep]


def tree_pairs(pos, box, radius, chunk=2_000_000):
    """Chunks (i, j), i < j, of the pairs within `radius` under the periodic minimum image (a superset of any cutoff below it)."""
    from scipy.spatial import cKDTree

    w = pos - np.floor(pos / box) * box
    w[w >= box] = 0.0
    pairs = cKDTree(w, boxsize=box).query_pairs(radius, output_type="ndarray")
    for k in range(0, len(pairs), chunk):
        yield pairs[k:k + chunk, 0], pairs[k:k + chunk, 1]


def nonbonded_model(pos, box, sys, terms, cutoff, prec="f64", rfa=False, switch_dist=None, switch_mode="reference", ewald_beta=None,
                    pairs=None):
    """pos [N, 3], box [3]; `sys`: types, A, B (tables), charges, mass, off / mem / mol_of, excl (CSR).  Returns W [3], S [3], the
    energy U, the number of pairs within the cutoff and the number of addends of W."""
    dt = NP_DTYPE[prec]
    p = np.ascontiguousarray(pos, dtype=np.float64).astype(dt)
    box = np.asarray(box, dtype=np.float64).reshape(3)
    p64 = p.astype(np.float64)
    _, delta, _ = molecule_centres(p64, sys.mass, sys.off, sys.mem, sys.mol_of)
    n = len(p)
    W, S, U, npairs = np.zeros(3), np.zeros(3), 0.0, 0
    q = np.asarray(sys.charges, dtype=np.float64)
    keys = _exclusion_keys(sys.excl, n)
    for i, j in (pairs if pairs is not None else dense_pairs(n)):
        keep = ~np.isin(i.astype(np.int64) * n + j, keys) if len(keys) else np.ones(len(i), dtype=bool)
        i, j = i[keep], j[keep]
        d = engine_delta(p, i, j, box)
        inc = engine_includes(d, cutoff) if cutoff is not None else np.ones(len(i), dtype=bool)
        i, j, d = i[inc], j[inc], d[inc].astype(np.float64)
        if len(i) == 0:
            continue
        r = np.sqrt((d * d).sum(axis=1))
        ti, tj = sys.types[i], sys.types[j]
        qq = ELEC_FACTOR * q[i] * q[j]
        lr_terms = tuple(t for t in terms if not (t == "electrostatics" and ewald_beta is not None))
        epart, fpart, _, fscale = pair_partials(r, sys.A[ti, tj], sys.B[ti, tj], qq, lr_terms, rfa=rfa, switch_dist=switch_dist,
                                                switch_mode=switch_mode, cutoff=cutoff if cutoff is not None else 1.0)
        dEdr = sum(fpart, np.zeros_like(r))
        SF = sum(fscale, np.zeros_like(r))
        E = sum((sum(v, np.zeros_like(r)) for v in epart.values()), np.zeros_like(r))
        if ewald_beta is not None and "electrostatics" in terms:  # the real-space Ewald branch of pair_terms
            from scipy.special import erfc

            br = ewald_beta * r
            e_el = qq * erfc(br) / r
            g = qq * (2.0 / np.sqrt(np.pi)) * ewald_beta * np.exp(-br * br)
            dEdr = dEdr - (e_el + g) / r
            SF = SF + (np.abs(e_el) + np.abs(g)) / r
            E = E + e_el
        f = -(dEdr / r)[:, None] * d  # force on i
        W += (f * (d - delta[i] + delta[j])).sum(axis=0)
        S += ((SF / r)[:, None] * (d * d + (np.abs(delta[i]) + np.abs(delta[j])) * np.abs(d))).sum(axis=0)
        U += float(E.sum())
        npairs += len(i)
    return SimpleNamespace(W=W, S=S, U=U, npairs=npairs, addends=2 * npairs)


def reciprocal_model(pos, box, sys, beta, grid, order):
    """The reciprocal-space part of the PME virial, written on `_ewald.pme_reciprocal`'s transcription of the library's
    conventions (its energy and forces are that function's; the grid, S(m) and G(m) are rebuilt here the same way):
        W_aa = sum_m e(m) [1 - 2 (1 + pi^2 m^2 / beta^2) m_a^2 / m^2] - sum_i delta_i,a F^rec_i,a + E_background
    with e(m) = G(m) |S(m)|^2 / 2 over the full complex grid.  Returns W [3], its three parts, the scales sum |e(m) factor|
    and sum |delta_i,a| (what an energy-like and a force-like error bound multiply) and the energy E_rec + E_background."""
    import math

    import _ewald as E

    pos = np.asarray(pos, np.float64)
    box = np.asarray(box, np.float64)
    q = np.asarray(sys.charges, np.float64)
    Erec, F = E.pme_reciprocal(pos, q, box, beta, grid, order)
    qs = q * math.sqrt(E.KE)
    K = np.asarray(grid, dtype=np.int64)
    sfr = pos / box
    sfr = sfr - np.floor(sfr)
    u = sfr * K
    b = np.floor(u).astype(np.int64)
    w = u - b
    b = np.where(b >= K, b - K, b)
    th = [E.bspline(w[:, d], order)[0] for d in range(3)]
    Q = np.zeros(tuple(K))
    idx = [(b[:, d][:, None] - np.arange(order)[None, :]) % K[d] for d in range(3)]
    for jx in range(order):
        for jy in range(order):
            for jz in range(order):
                np.add.at(Q, (idx[0][:, jx], idx[1][:, jy], idx[2][:, jz]), qs * th[0][:, jx] * th[1][:, jy] * th[2][:, jz])
    S = np.fft.fftn(Q)
    f = [np.fft.fftfreq(K[d]) * K[d] / box[d] for d in range(3)]
    fa2 = [f[0][:, None, None] ** 2 + 0 * f[1][None, :, None] + 0 * f[2][None, None, :],
           0 * f[0][:, None, None] + f[1][None, :, None] ** 2 + 0 * f[2][None, None, :],
           0 * f[0][:, None, None] + 0 * f[1][None, :, None] + f[2][None, None, :] ** 2]
    m2 = fa2[0] + fa2[1] + fa2[2]
    B = [E.bspline_moduli(int(K[d]), order) for d in range(3)]
    V = float(np.prod(box))
    with np.errstate(divide="ignore", invalid="ignore"):
        G = B[0][:, None, None] * B[1][None, :, None] * B[2][None, None, :] * np.exp(-math.pi**2 * m2 / beta**2) / (math.pi * V * m2)
    G[0, 0, 0] = 0.0
    e = 0.5 * G * np.abs(S) ** 2
    assert abs(e.sum() - Erec) <= 1e-12 * abs(Erec)
    m2s = np.where(m2 > 0, m2, 1.0)
    modes, scale = np.zeros(3), np.zeros(3)
    for a in range(3):
        t = e * (1.0 - 2.0 * (1.0 + math.pi**2 * m2 / beta**2) * fa2[a] / m2s)
        modes[a], scale[a] = t.sum(), np.abs(t).sum()
    _, delta, _ = molecule_centres(pos, sys.mass, sys.off, sys.mem, sys.mol_of)
    corr = -(delta * F).sum(axis=0)
    bg = -E.KE * math.pi * q.sum() ** 2 / (2 * V * beta * beta)
    return SimpleNamespace(W=modes + corr + bg, modes=modes, correction=corr, background=bg, S_modes=scale,
                           S_delta=np.abs(delta).sum(axis=0), S_dF=(np.abs(delta) * np.abs(F)).sum(axis=0), U=Erec + bg, Erec=Erec)


def scale_molecules(pos, box, sys, s):
    """Rigid molecular scaling about the mass-weighted centres: box edges and centres times s [3] (float64), offsets kept."""
    s = np.broadcast_to(np.asarray(s, dtype=np.float64), (3,))
    R, delta, _ = molecule_centres(pos, sys.mass, sys.off, sys.mem, sys.mol_of)
    return (R * s)[sys.mol_of] + delta, np.asarray(box, dtype=np.float64) * s


def system_of(par, terms, excl_csr, virtual_sites=None):
    """The arrays the model needs from a Parameters-shaped object (and the molecule table the package makes from its bonds)."""
    from torchmd_amd.pressure import molecule_table

    n = len(par.masses)
    bp = getattr(par, "bond_params", None)
    bonds = bp["idx"].detach().cpu().numpy() if bp is not None and len(bp["idx"]) else None
    off, mem, mol_of = molecule_table(n, bonds, virtual_sites)
    if any(t in terms for t in ("lj", "repulsion", "repulsioncg")):
        A, B = par.get_AB()
        A, B = A.detach().cpu().double().numpy(), B.detach().cpu().double().numpy()
    else:
        A = B = np.zeros((1, 1))
    types = par.mapped_atom_types.detach().cpu().numpy().astype(np.int64) if A.shape[0] > 1 else np.zeros(n, dtype=np.int64)
    return SimpleNamespace(types=types, A=A, B=B, charges=par.charges.detach().cpu().double().numpy().reshape(-1),
                           mass=par.masses.detach().cpu().double().numpy().reshape(-1), off=off, mem=mem, mol_of=mol_of, excl=excl_csr)
