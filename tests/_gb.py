"""Float64 numpy model of the OBC2 generalized-Born / surface-area implicit solvent, written from the formulas
and not from csrc/gb_math.h, in row chunks so that a few thousand atoms fit in memory.

    rho_i = r_i - 0.09, sigma_j = s_j rho_j; every ordered pair i != j, no cutoff, no image, no exclusions
    I_i   = 1/2 sum_j t(r_ij; rho_i, sigma_j)          psi = rho I, T = tanh(psi - 0.8 psi^2 + 4.85 psi^3)
    B_i   = 1 / (1/rho_i - T/r_i)                      c_i = rho (1 - 1.6 psi + 14.55 psi^2)(1 - T^2) / r_i
    E_GB  = 1/2 sum_ij p q_i q_j / f_ij (i = j too)    f^2 = r^2 + B_i B_j exp(-D), D = r^2 / (4 B_i B_j)
    E_SA  = sum_i 4 pi gamma (r_i + r_probe)^2 (r_i / B_i)^6

`evaluate(..., dtype=np.float32)` forms the pair vector d = x_j - x_i with float32 operations, as an fp32 engine does, and
computes everything else in float64.  With `bounds=True` it also returns, for every quantity, S: the sum of the absolute values
of its addends with the sums of the quantities it depends on carried through to first order (see `evaluate`), the number the
rounding bars of the GPU tests multiply by (c eps_R + M eps64)."""

import numpy as np

KE = 332.06371307417066  # the engine's Coulomb constant, kcal/mol A / e^2
OFFSET = 0.09
CHUNK = 256

RADII = {"H": 1.2, "HN": 1.3, "C": 1.7, "N": 1.55, "O": 1.5, "F": 1.5, "P": 1.85, "S": 1.8, "Cl": 1.7}
SCALES = {"H": 0.85, "HN": 0.85, "C": 0.72, "N": 0.79, "O": 0.85, "F": 0.88, "P": 0.86, "S": 0.96, "Cl": 0.8}


def _pairs(pos, lo, hi, dtype, work=np.float64):
    """d = x_j - x_i [m, N, 3] formed in `dtype`, then float64; r [m, N] (1 on the diagonal); the off-diagonal mask."""
    p = np.asarray(pos).astype(dtype)
    d = (p[None, :, :] - p[lo:hi, None, :]).astype(work)
    r = np.sqrt((d[..., 0] ** 2 + d[..., 1] ** 2) + d[..., 2] ** 2)
    off = np.ones(r.shape, dtype=bool)
    off[np.arange(hi - lo), np.arange(lo, hi)] = False
    return d, np.where(off, r, 1.0), off


def pair_t(r, rho_i, sig_j):
    """The addends of t(i <- j) as a list of arrays (their sum is t) and the regime of every pair:
    0 none (rho_i >= r + sigma_j), 1 separate, 2 overlapping, 3 engulfed."""
    r, rho_i, sig_j = np.broadcast_arrays(np.asarray(r), np.asarray(rho_i), np.asarray(sig_j))
    on = rho_i < r + sig_j
    a = np.abs(r - sig_j)
    l = 1.0 / np.maximum(rho_i, a)
    u = 1.0 / (r + sig_j)
    eng = on & (rho_i < sig_j - r)
    terms = [l, -u, 0.25 * r * (u * u - l * l), np.log(u / l) / (2.0 * r), sig_j * sig_j / (4.0 * r) * (l * l - u * u),
             np.where(eng, 2.0 / rho_i, 0.0), np.where(eng, -2.0 * l, 0.0)]
    regime = np.where(~on, 0, np.where(eng, 3, np.where(a >= rho_i, 1, 2)))
    return [np.where(on, t, 0.0) for t in terms], regime


def pair_t3(r, rho_i, sig_j):
    """The two addends of t3(i <- j) = -(dt/dr)/2."""
    r, rho_i, sig_j = np.broadcast_arrays(np.asarray(r), np.asarray(rho_i), np.asarray(sig_j))
    on = rho_i < r + sig_j
    l = 1.0 / np.maximum(rho_i, np.abs(r - sig_j))
    u = 1.0 / (r + sig_j)
    terms = [0.125 * (1.0 + sig_j * sig_j / (r * r)) * (l * l - u * u), 0.25 * np.log(u / l) / (r * r)]
    return [np.where(on, t, 0.0) for t in terms]


def born_close(I, radii):
    rho = radii - OFFSET
    psi = rho * I
    T = np.tanh(psi - 0.8 * psi ** 2 + 4.85 * psi ** 3)
    B = 1.0 / (1.0 / rho - T / radii)
    c = rho * (1.0 - 1.6 * psi + 14.55 * psi ** 2) * (1.0 - T * T) / radii
    return B, c, T


def evaluate(pos, charges, radii, scale, solute_dielectric=1.0, solvent_dielectric=78.5, surface_tension=0.0054, probe_radius=1.4,
             dtype=np.float64, bounds=False, forces=True, work=np.float64, born_only=False):
    """One structure: pos [N, 3], charges / radii / scale [N].  Returns a dict: I, B, c, E_gb, E_sa, F [N, 3], regimes (counts of
    the regimes 0..3 over ordered pairs), and with `bounds` S_I, S_B [N], S_Egb, S_Esa, S_F [N], M (addends per atom).

    The bounds to first order, per unit relative rounding error of one operation:
      S_I  = 1/2 sum_j sum |addends of t|                           S_B = B^2 (c S_I + 1/rho + |T|/r)   (the close's own addends)
      with e_i = S_B,i / B_i:
      S_Egb = 1/2 sum_ij |G_ij| (1 + w_ij (e_i + e_j)),   w = |dlnG/dlnB| = B_i B_j e^-D (1 + D) / (2 f^2) <= 1/2
      S_Esa = sum_i E_SA,i (1 + 6 e_i)
      direct force addend g_ij d:  |g_ij| |d| (1 + 2 (e_i + e_j))        (|dln g / dln B| <= 1/2 + 1 + 0.13 < 2)
      chain addend h_ij B_j:       |h_ij B_j| (1 + (3.5 + D)(e_i + e_j))  (|dln(h B_j)/dln B| <= 1/2 + D + 1 + 1 + 1)
      S_b  = B^2 c (sum of those + 6 E_SA/B (1 + 7 e)) + |b| (2 e + S_c / c),  S_c = |dc/dI| S_I
      third-pass addend:  S_b,i |t3_ij| + |b_i| sum |addends of t3_ij|, and the same with i and j exchanged."""
    pos = np.asarray(pos, dtype=np.float64)
    q = np.asarray(charges, dtype=np.float64)
    radii = np.asarray(radii, dtype=np.float64)
    scale = np.asarray(scale, dtype=np.float64)
    N = len(pos)
    rho = radii - OFFSET
    sig = scale * rho
    p = -KE * (1.0 / solute_dielectric - 1.0 / solvent_dielectric)
    I = np.zeros(N, dtype=work)
    S_I = np.zeros(N)
    regimes = np.zeros(4, dtype=np.int64)
    for lo in range(0, N, CHUNK):
        hi = min(N, lo + CHUNK)
        _, r, off = _pairs(pos, lo, hi, dtype, work)
        terms, reg = pair_t(r, rho[lo:hi, None], sig[None, :])
        t = sum(terms)
        I[lo:hi] = 0.5 * np.where(off, t, 0.0).sum(axis=1)
        S_I[lo:hi] = 0.5 * np.where(off, sum(np.abs(x) for x in terms), 0.0).sum(axis=1)
        regimes += np.bincount(reg[off], minlength=4)
    B, c, T = born_close(I, radii)
    sa = 4.0 * np.pi * surface_tension * (radii + probe_radius) ** 2
    esa = sa * (radii / B) ** 6
    out = {"I": I, "B": B, "c": c, "regimes": regimes, "E_sa": esa.sum() if work is not np.float64 else float(esa.sum()), "E_sa_atoms": esa}
    S_B = B * B * (c * S_I + 1.0 / rho + np.abs(T) / radii)
    if born_only:
        out.update(S_I=S_I, S_B=S_B)
        return out
    e = S_B / B
    E = work(0.0)
    S_E = 0.0
    b = np.zeros(N, dtype=work)
    S_b = np.zeros(N)
    F = np.zeros((N, 3), dtype=work)
    S_F = np.zeros(N)
    for lo in range(0, N, CHUNK):
        hi = min(N, lo + CHUNK)
        d, r, off = _pairs(pos, lo, hi, dtype, work)
        r2 = np.where(off, r * r, 0.0)
        BB = B[lo:hi, None] * B[None, :]
        D = r2 / (4.0 * BB)
        ex = np.exp(-D)
        f2 = r2 + BB * ex
        G = p * q[lo:hi, None] * q[None, :] / np.sqrt(f2)
        E += 0.5 * G.sum()
        g = -G * (1.0 - 0.25 * ex) / f2
        h = -0.5 * G * ex * (1.0 + D) / f2 * B[None, :]
        b[lo:hi] = h.sum(axis=1)
        F[lo:hi] += (g[..., None] * d).sum(axis=1)
        if bounds:
            ee = e[lo:hi, None] + e[None, :]
            w = BB * ex * (1.0 + D) / (2.0 * f2)
            S_E += 0.5 * (np.abs(G) * (1.0 + w * ee)).sum()
            S_b[lo:hi] = (np.abs(h) * (1.0 + (3.5 + D) * ee)).sum(axis=1)
            S_F[lo:hi] += (np.abs(g) * np.where(off, r, 0.0) * (1.0 + 2.0 * ee)).sum(axis=1)
    out["E_gb"] = E if work is not np.float64 else float(E)
    b_raw = b - 6.0 * esa / B
    bt = b_raw * B * B * c
    out["b"] = bt
    if bounds:
        psi = rho * I
        dc_dI = rho * rho / radii * ((-1.6 + 29.1 * psi) * (1.0 - T * T)
                                     - (1.0 - 1.6 * psi + 14.55 * psi ** 2) * 2.0 * T * (1.0 - T * T) * (1.0 - 1.6 * psi + 14.55 * psi ** 2))
        S_c = np.abs(dc_dI) * S_I + np.abs(c)
        S_bt = B * B * np.abs(c) * (S_b + 6.0 * esa / B * (1.0 + 7.0 * e)) + np.abs(b_raw) * B * B * (2.0 * e * np.abs(c) + S_c)
    if forces:
        for lo in range(0, N, CHUNK):
            hi = min(N, lo + CHUNK)
            d, r, off = _pairs(pos, lo, hi, dtype, work)
            a_ij = pair_t3(r, rho[lo:hi, None], sig[None, :])  # t3(i <- j)
            a_ji = pair_t3(r, rho[None, :], sig[lo:hi, None])  # t3(j <- i)
            s = np.where(off, bt[lo:hi, None] * sum(a_ij) + bt[None, :] * sum(a_ji), 0.0)
            F[lo:hi] += (-(s / r)[..., None] * d).sum(axis=1)  # (x_i - x_j) / r = -d / r
            if bounds:
                ab_ij, ab_ji = sum(np.abs(x) for x in a_ij), sum(np.abs(x) for x in a_ji)
                S_F[lo:hi] += np.where(off, S_bt[lo:hi, None] * np.abs(sum(a_ij)) + np.abs(bt[lo:hi, None]) * ab_ij
                                       + S_bt[None, :] * np.abs(sum(a_ji)) + np.abs(bt[None, :]) * ab_ji, 0.0).sum(axis=1)
        out["F"] = F
    if bounds:
        out.update(S_I=S_I, S_B=S_B, S_Egb=float(S_E), S_Esa=float((esa * (1.0 + 6.0 * e)).sum()), S_F=S_F, M=7 * (N - 1) + 8)
    return out


def energy(pos, charges, radii, scale, **kw):
    o = evaluate(pos, charges, radii, scale, forces=False, **kw)
    return o["E_gb"] + o["E_sa"]


def cluster(n, seed, edge=None):
    """A random cluster at a density that produces overlapping and engulfed pairs: n atoms uniform in a cube (7 A for 40 atoms,
    the same density otherwise), no two closer than 0.25 A, charges in +-0.8, radii and scales drawn from the default tables."""
    rng = np.random.default_rng(seed)
    edge = edge if edge is not None else 7.0 * (n / 40.0) ** (1.0 / 3.0)
    pos = np.zeros((0, 3))
    while len(pos) < n:
        x = rng.uniform(0.0, edge, size=3)
        if len(pos) == 0 or np.sqrt(((pos - x) ** 2).sum(axis=1)).min() > 0.25:
            pos = np.vstack([pos, x])
    names = list(RADII)
    kind = rng.integers(0, len(names), size=n)
    radii = np.array([RADII[names[k]] for k in kind])
    scale = np.array([SCALES[names[k]] for k in kind])
    q = rng.uniform(-0.8, 0.8, size=n)
    return pos, q, radii, scale


THROMBIN_GOLDEN = "thrombin_gb"  # tests/golden/thrombin_gb.npz: this model on the thrombin golden, recorded (12 s of numpy)


def thrombin_inputs():
    """(pos [N, 3] float64, charges, default radii and scales) of tests/golden/thrombin.npz."""
    import torch

    import _golden as G
    from torchmd_amd.implicit import GeneralizedBorn

    g = G.load("thrombin")
    par = G.GoldenParameters(g, torch.float64)
    gb = GeneralizedBorn.from_parameters(par)
    return np.asarray(g["pos"], dtype=np.float64).reshape(-1, 3), par.charges.numpy().astype(np.float64), gb.radii, gb.scale


def thrombin_reference():
    """What the golden file holds: the model with default parameters at the float32-rounded positions of the thrombin golden, d
    formed in float32 (`f32_*`) and in float64 (`f64_*`), and the bounds S of the float64 evaluation (the two differ by 1e-7 of
    their values)."""
    pos, q, rad, sc = thrombin_inputs()
    p32 = pos.astype(np.float32).astype(np.float64)
    out = {}
    for tag, dt in (("f64", np.float64), ("f32", np.float32)):
        o = evaluate(p32, q, rad, sc, dtype=dt, bounds=tag == "f64")
        out.update({f"{tag}_B": o["B"], f"{tag}_F": o["F"], f"{tag}_E": np.array([o["E_gb"], o["E_sa"]])})
        if tag == "f64":
            out.update(S_B=o["S_B"], S_F=o["S_F"], S_E=np.array([o["S_Egb"], o["S_Esa"]]), M=np.array(o["M"]), regimes=o["regimes"])
    return out


if __name__ == "__main__":
    import os

    np.savez(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", THROMBIN_GOLDEN + ".npz"), **thrombin_reference())
