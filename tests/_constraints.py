"""Host reference of the constrained MD step, fp64 numpy, one unit at a time (independent of torchmd_amd/constraints.py's
vectorised projection and of the device's analytic SETTLE): iterated SHAKE to 1e-14, the exact velocity projection (the
unit's k x k system by np.linalg.solve), and one constrained velocity-Verlet step in the order of the HIP kernel
(thermostat, second half kick, velocity constraint | first half kick, drift, position constraint, v += dx / dt)."""

import numpy as np


def units(cs):
    """[(atoms, [(a, b, d), ...] local pairs)] of a ConstraintSet."""
    out = []
    for (o, h1, h2), (doh, dhh) in zip(cs.waters, cs.water_dist):
        out.append((np.array([o, h1, h2]), [(0, 1, doh), (0, 2, doh), (1, 2, dhh)]))
    for c in range(cs.nclusters):
        s, e = cs.offsets[c], cs.offsets[c + 1]
        out.append((np.array(cs.atoms[s:e]), [(0, k, cs.dist[s + k]) for k in range(1, e - s)]))
    return out


def shake(x, ref, m, us, tol=1e-14, max_iter=100000):
    """x [N, 3] in place: every constraint |s| = d to relative tol, displacements along the bonds of `ref`.  A unit is iterated
    in coordinates relative to its first atom's reference position (the constraints do not see a translation): at a
    coordinate of 60 A one ulp is 7e-15 A, and |s|^2 taken from absolute positions cannot be told from d^2 to 1e-14."""
    for at, pairs in us:
        o = ref[at[0]].copy()
        xl, rl = x[at] - o, ref[at] - o
        for _ in range(max_iter):
            done = True
            for a, b, d in pairs:
                s = xl[a] - xl[b]
                diff = d * d - s @ s
                if abs(diff) > 2 * tol * d * d:
                    done = False
                r = rl[a] - rl[b]
                g = diff / (2.0 * (r @ s) * (1 / m[at[a]] + 1 / m[at[b]]))
                xl[a] += g * r / m[at[a]]
                xl[b] -= g * r / m[at[b]]
            if done:
                break
        else:
            raise AssertionError("host SHAKE did not converge")
        x[at] = xl + o
    return x


def project(x, v, m, us):
    """v [N, 3] in place: r_c . (v_a - v_b) = 0 for every constraint, exactly."""
    for at, pairs in us:
        k = len(pairs)
        r = [x[at[a]] - x[at[b]] for a, b, _ in pairs]
        A = np.zeros((k, k))
        rhs = np.array([-(r[c] @ (v[at[a]] - v[at[b]])) for c, (a, b, _) in enumerate(pairs)])
        for c, (ac, bc, _) in enumerate(pairs):
            for e, (ae, be, _) in enumerate(pairs):
                sa = (ac == ae) - (ac == be)
                sb = (bc == ae) - (bc == be)
                A[c, e] = (r[c] @ r[e]) * (sa / m[at[ac]] - sb / m[at[bc]])
        mu = np.linalg.solve(A, rhs)
        for c, (a, b, _) in enumerate(pairs):
            v[at[a]] += mu[c] * r[c] / m[at[a]]
            v[at[b]] -= mu[c] * r[c] / m[at[b]]
    return v


def first_half(x, v, f, m, dt, us):
    """Kick + drift + SHAKE + velocity correction: (x', v(t + dt/2))."""
    a = f / m[:, None]
    xn = x + (v * dt + 0.5 * a * dt * dt)
    u = xn.copy()
    vh = v + 0.5 * dt * a
    shake(xn, x, m, us)
    return xn, vh + (xn - u) / dt


def second_half(x, v, f, m, dt, us, gamma=None, vcoeff=None, noise=None):
    """Thermostat + kick + velocity constraint at positions x."""
    v = v.copy()
    if noise is not None:
        v += -gamma * v * dt + noise * vcoeff[:, None]
    v += 0.5 * dt * f / m[:, None]
    return project(x, v, m, us)


def residuals(x, v, pairs, d):
    """max relative bond-length error, max |relative velocity along the bond| / rms relative speed."""
    s = x[pairs[:, 0]] - x[pairs[:, 1]]
    ln = np.linalg.norm(s, axis=1)
    dv = v[pairs[:, 0]] - v[pairs[:, 1]]
    along = np.abs(np.einsum("ij,ij->i", s, dv)) / ln
    return float(np.max(np.abs(ln - d) / d)), float(along.max() / np.sqrt(np.mean(np.einsum("ij,ij->i", dv, dv))))
