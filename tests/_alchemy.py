"""A float64 numpy model of the alchemical decoupling of DESIGN §22, written from the formulas, and the small systems its tests
share.  Nothing here imports the package.

Cross pairs (i in S, j in E) inside the cutoff, A, B from the class table, sigma^6 = A / B:
    s = r^6 + alpha sigma^6 (1 - lv);  U_lj = lv (A / s^2 - B / s) sw(r);  U_el = le qq g(r)
    dU/dlv = (A / s^2 - B / s) sw - lv (-2 A / s^3 + B / s^2) alpha sigma^6 sw;  dU/dle = qq g(r)
with sw the quintic switch between switch_dist and the cutoff and g = 1/r or 1/r + k_rf r^2 - c_rf.  Intra: the non-excluded
S-S pairs with the plain 12-6 + electrostatics formula under the same cutoff, switch and g, and the 1-4 Coulomb term
qq / (scee r).  The pair vector and the decision r <= cutoff can be formed in float32 (`dtype`), as an fp32 context forms them;
everything behind them is float64."""

import numpy as np

KE = 332.06371307417066


def r2max(cutoff, dtype):
    """The largest |d|^2 of `dtype` whose correctly rounded square root is <= cutoff (the engine's decision threshold)."""
    if cutoff is None:
        return np.inf
    t = np.dtype(dtype).type
    c = t(cutoff)
    r2 = t(c * c)
    while np.sqrt(r2) <= c:
        r2 = np.nextafter(r2, t(np.inf))
    while np.sqrt(r2) > c:
        r2 = np.nextafter(r2, t(0))
    return r2


def pair_vectors(xi, xj, box, dtype=np.float64):
    """d = minimum image of x_i - x_j and |d|^2 in `dtype`, in the engine's order of operations; returned as float64."""
    t = np.dtype(dtype).type
    d = (np.asarray(xi, dtype=dtype) - np.asarray(xj, dtype=dtype)).astype(dtype)
    b = np.asarray(box, dtype=dtype)
    if np.any(b != 0):
        inv = np.where(b != 0, t(1) / np.where(b != 0, b, t(1)), t(0)).astype(dtype)
        k = np.rint((d * inv).astype(dtype)).astype(dtype)
        d = (d - (b * k).astype(dtype)).astype(dtype)
    if dtype == np.float32:  # fma(dz, dz, fma(dy, dy, dx * dx)): the products are exact in float64
        d64 = d.astype(np.float64)
        a = (d64[..., 0] * d64[..., 0]).astype(np.float32).astype(np.float64)
        a = (d64[..., 1] * d64[..., 1] + a).astype(np.float32).astype(np.float64)
        r2 = (d64[..., 2] * d64[..., 2] + a).astype(np.float32).astype(np.float64)
        return d64, r2
    return d, (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def switch(r, cutoff, switch_dist):
    """(sw, dsw/dr) of the quintic switching function."""
    sw, dsw = np.ones_like(r), np.zeros_like(r)
    if cutoff is None or switch_dist is None:
        return sw, dsw
    m = r > switch_dist
    t = (r[m] - switch_dist) / (cutoff - switch_dist)
    sw[m] = 1 + t * t * t * (-10 + t * (15 - t * 6))
    dsw[m] = t * t * (-30 + t * (60 - t * 30)) / (cutoff - switch_dist)
    return sw, dsw


def rf_consts(cutoff, eps=78.5):
    return (1 / cutoff**3) * (eps - 1) / (2 * eps + 1), (1 / cutoff) * (3 * eps) / (2 * eps + 1)


def pair(r2, qq, A, B, lv, le, alpha, cutoff=None, switch_dist=None, rfa=False, eps=78.5, reference_switch=False, lj=True, el=True):
    """One array of pairs at squared distances r2 (already inside the cutoff).  Returns a dict: ulj, uel (at le), gel, dv, fs
    (force on i = -d fs) and `addends`, the absolute values of the addends of fs, ulj and dv (for the rounding bars)."""
    r2 = np.asarray(r2, dtype=np.float64)
    qq, A, B = (np.broadcast_to(np.asarray(v, dtype=np.float64), r2.shape) for v in (qq, A, B))
    r = np.sqrt(r2)
    with np.errstate(divide="ignore", invalid="ignore"):
        rinv = np.where(r > 0, 1 / r, 0.0)
        sig6 = np.where(A != 0, A / np.where(B != 0, B, 1.0), 0.0)
    a6 = alpha * sig6
    s = r2**3 + a6 * (1 - lv)
    on = (A != 0) & lj
    with np.errstate(divide="ignore", invalid="ignore"):
        sinv = np.where(on, 1 / np.where(on, s, 1.0), 0.0)
    u = (A * sinv - B) * sinv
    du = (-2 * A * sinv + B) * sinv * sinv
    sw, dsw = switch(r, cutoff, switch_dist)
    if reference_switch:
        dsw = dsw * rinv
    # the sums of the absolute addends of the two polynomials
    S_sw, S_dsw = np.ones_like(r), np.zeros_like(r)
    if cutoff is not None and switch_dist is not None:
        t = np.where(r > switch_dist, (r - switch_dist) / (cutoff - switch_dist), 0.0)
        S_sw = 1 + 10 * t**3 + 15 * t**4 + 6 * t**5
        S_dsw = (30 * t**2 + 60 * t**3 + 30 * t**4) / (cutoff - switch_dist) * (rinv if reference_switch else 1.0)
    u, du = np.where(on, u, 0.0), np.where(on, du, 0.0)
    ulj = lv * u * sw
    dv = u * sw - lv * du * a6 * sw
    f1, f2 = lv * du * 6 * r2 * r2 * sw, lv * u * dsw * rinv
    gel, f3 = np.zeros_like(r2), np.zeros_like(r2)
    if el:
        krf, crf = rf_consts(cutoff, eps) if rfa else (0.0, 0.0)
        gel = np.where(r > 0, qq * (rinv + krf * r2 - crf), 0.0)
        f3 = np.where(r > 0, le * qq * (2 * krf * r - rinv * rinv) * rinv, 0.0)
    # the largest addends on the way to each result (A/s^2 and B/s separately)
    a_u = (np.abs(A * sinv * sinv) + np.abs(B * sinv)) * np.where(on, 1.0, 0.0)
    a_du = (np.abs(2 * A * sinv**3) + np.abs(B * sinv * sinv)) * np.where(on, 1.0, 0.0)
    krf_, crf_ = rf_consts(cutoff, eps) if (rfa and el) else (0.0, 0.0)
    a_g = np.abs(qq) * (rinv + abs(krf_) * r2 + abs(crf_)) * (1.0 if el else 0.0) * (r > 0)
    return dict(ulj=ulj, uel=le * gel, gel=gel, dv=dv, fs=f1 + f2 + f3,
                a_ulj=lv * a_u * S_sw, a_gel=a_g, a_dv=(a_u + lv * a_du * a6) * S_sw,
                a_fs=lv * a_du * 6 * r2 * r2 * S_sw + lv * a_u * S_dsw * rinv
                + le * np.abs(qq) * (2 * abs(krf_) * r + rinv * rinv) * rinv * (1.0 if el else 0.0) * (r > 0))


def evaluate(pos, box, atoms, q, cls, A, B, lv, le, alpha=0.5, cutoff=None, switch_dist=None, rfa=False, eps=78.5,
             reference_switch=False, excl=(), pairs14=(), scee=(), dtype=np.float64, lj=True, el=True):
    """One replica.  pos [N, 3], box [3] (zeros: open), atoms: the solute, q [N] true charges (e), cls [N] true classes,
    A, B [T, T].  Returns E_lj, E_el, E_intra, dv, de, F [N, 3], the per-atom sum of absolute force addends `S_F` [N], the sums
    of absolute energy addends `S_E` (5) and `near` [N]: atoms with a solute atom inside the cutoff (and the solute itself)."""
    pos = np.asarray(pos, dtype=np.float64)
    N = len(pos)
    S = np.asarray(atoms, dtype=np.int64)
    mask = np.zeros(N, dtype=bool)
    mask[S] = True
    E = np.nonzero(~mask)[0]
    q, cls = np.asarray(q, dtype=np.float64), np.asarray(cls, dtype=np.int64)
    kw = dict(cutoff=cutoff, switch_dist=switch_dist, rfa=rfa, eps=eps, reference_switch=reference_switch, lj=lj, el=el)
    F, SF = np.zeros((N, 3)), np.zeros(N)
    near = mask.copy()
    out = dict(E_lj=0.0, E_el=0.0, E_intra=0.0, dv=0.0, de=0.0)
    SE = np.zeros(5)
    lim = r2max(cutoff, dtype)
    if len(E):
        ii, jj = np.meshgrid(S, E, indexing="ij")
        ii, jj = ii.reshape(-1), jj.reshape(-1)
        d, r2 = pair_vectors(pos[ii], pos[jj], box, dtype)
        m = r2 <= lim
        ii, jj, d, r2 = ii[m], jj[m], d[m], r2[m]
        p = pair(r2, KE * q[ii] * q[jj], A[cls[ii], cls[jj]], B[cls[ii], cls[jj]], lv, le, alpha, **kw)
        out.update(E_lj=p["ulj"].sum(), E_el=p["uel"].sum(), dv=p["dv"].sum(), de=p["gel"].sum())
        SE[[0, 1, 3, 4]] = p["a_ulj"].sum(), le * p["a_gel"].sum(), p["a_dv"].sum(), p["a_gel"].sum()
        f = -d * p["fs"][:, None]
        np.add.at(F, ii, f)
        np.add.at(F, jj, -f)
        af = np.abs(d).max(axis=1) * p["a_fs"] if len(d) else np.zeros(0)
        np.add.at(SF, ii, af)
        np.add.at(SF, jj, af)
        near[jj] = True
    ex = {(min(a, b), max(a, b)) for a, b in np.asarray(excl, dtype=np.int64).reshape(-1, 2)}
    prs = [(a, b) for k, a in enumerate(S) for b in S[k + 1:] if (a, b) not in ex]
    if prs:
        ii, jj = np.array(prs).T
        d, r2 = pair_vectors(pos[ii], pos[jj], box, dtype)
        m = r2 <= lim
        ii, jj, d, r2 = ii[m], jj[m], d[m], r2[m]
        p = pair(r2, KE * q[ii] * q[jj], A[cls[ii], cls[jj]], B[cls[ii], cls[jj]], 1.0, 1.0, alpha, **kw)
        out["E_intra"] += (p["ulj"] + p["uel"]).sum()
        SE[2] += (p["a_ulj"] + p["a_gel"]).sum()
        f = -d * p["fs"][:, None]
        np.add.at(F, ii, f)
        np.add.at(F, jj, -f)
        af = np.abs(d).max(axis=1) * p["a_fs"] if len(d) else np.zeros(0)
        np.add.at(SF, ii, af)
        np.add.at(SF, jj, af)
    p14 = np.asarray(pairs14, dtype=np.int64).reshape(-1, 2)
    if len(p14) and el:
        ii, jj = p14.T
        d, r2 = pair_vectors(pos[ii], pos[jj], box, dtype)
        r = np.sqrt(r2)
        ee = KE * q[ii] * q[jj] / r / np.asarray(scee, dtype=np.float64)
        out["E_intra"] += ee.sum()
        SE[2] += np.abs(ee).sum()
        f = d * (ee / r2)[:, None]
        np.add.at(F, ii, f)
        np.add.at(F, jj, -f)
        af = np.abs(d).max(axis=1) * np.abs(ee) / r2
        np.add.at(SF, ii, af)
        np.add.at(SF, jj, af)
    out.update(F=F, S_F=SF, S_E=SE, near=near)
    return out


def total_energy(pos, lv, le, **kw):
    o = evaluate(pos, lv=lv, le=le, **kw)
    return o["E_lj"] + o["E_el"] + o["E_intra"]


# ---------------------------------------------------------------------------------------------- small systems
def chain_system(n, nenv, seed=0, edge=14.0, periodic=True):
    """A bonded chain of n solute atoms (two LJ classes, charges summing to zero, bonds / angles / 1-4 exclusions) in a cavity
    of nenv monatomic environment atoms of two further classes (one of them all-zero with a charge, like TIP3P hydrogen).
    Returns a dict of model inputs."""
    rng = np.random.default_rng(seed)
    # the chain: a random walk of 1.5 A steps near the box centre, folded back to stay inside a 6 A ball
    x = np.zeros((n, 3))
    ball = max(5.0, 2.3 * n ** (1.0 / 3.0))
    for k in range(1, n):
        for _ in range(2000):
            step = rng.normal(size=3)
            cand = x[k - 1] + 1.5 * step / np.linalg.norm(step)
            if np.linalg.norm(cand) < ball and (k < 2 or np.min(np.linalg.norm(x[: k - 1] - cand, axis=1)) > 2.0):
                break
        x[k] = cand
    x += edge / 2
    env = []
    while len(env) < nenv:
        c = rng.uniform(0, edge, size=3)
        if not env:  # the first one within reach of the chain, whatever the box
            u = rng.normal(size=3)
            c = x[0] + rng.uniform(3.2, 6.0) * u / np.linalg.norm(u)
        d = np.concatenate([x, np.array(env).reshape(-1, 3)]) - c
        if periodic:
            d -= edge * np.rint(d / edge)
        if np.min(np.linalg.norm(d, axis=1)) > 3.0:
            env.append(c)
    pos = np.concatenate([x, np.array(env).reshape(-1, 3)])
    N = n + nenv
    cls = np.concatenate([np.arange(n) % 2, 2 + (np.arange(nenv) % 2)])
    qs = 0.3 * np.where(np.arange(n) % 2 == 0, 1.0, -1.0)
    if n % 2:
        qs[-1] = 0.0
    qe = np.where(np.arange(nenv) % 2 == 0, -0.8, 0.4)
    sig = np.array([1.7, 1.5, 3.15, 0.0])  # (the chain's non-bonded neighbours come as close as 2 A)
    epsv = np.array([0.10, 0.08, 0.152, 0.0])
    s = 0.5 * (sig[:, None] + sig[None, :])
    e4 = 4 * np.sqrt(epsv[:, None] * epsv[None, :])
    A, B = e4 * s**12, e4 * s**6
    bonds = np.array([(k, k + 1) for k in range(n - 1)], dtype=np.int64).reshape(-1, 2)
    angles = np.array([(k, k + 1, k + 2) for k in range(n - 2)], dtype=np.int64).reshape(-1, 3)
    p14 = np.array([(k, k + 3) for k in range(n - 3)], dtype=np.int64).reshape(-1, 2)
    excl = np.concatenate([bonds, angles[:, [0, 2]], p14]).reshape(-1, 2)
    return dict(pos=pos, box=np.full(3, edge) if periodic else np.zeros(3), atoms=np.arange(n), q=np.concatenate([qs, qe]), cls=cls,
                A=A, B=B, excl=excl, pairs14=p14, scee=np.full(len(p14), 1.2), bonds=bonds, angles=angles, N=N)
