"""Cases shared by tests/test_group_restraints_host.py and tests/test_gpu_group_restraints.py."""

import numpy as np

from torchmd_amd.group_restraints import ANGLE, DIHEDRAL, DISTANCE, GroupRestraints, restraint_terms
from torchmd_amd.restraints import min_image

SIZES = (1, 2, 63, 64, 65, 256, 257)  # on the wave and block boundaries of the centre kernel


def _ball(rng, n, radius):
    """n points uniform in a ball."""
    v = rng.normal(size=(n, 3))
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    return v * (radius * rng.uniform(0.0, 1.0, (n, 1)) ** (1.0 / 3.0))


def sines(gr, pos, box):
    """The sine of every angle between consecutive arms of the angle and dihedral restraints (replica-wise minimum)."""
    X = gr.centres(pos, box)
    boxes = gr._boxes(box, X.shape[0])
    out = []
    for m in range(gr.nrestraints):
        n = int(gr.kind[m]) + 2
        g = gr.groups[m, :n]
        for a in range(n - 2):
            worst = 1.0
            for r in range(X.shape[0]):
                u, v = min_image(X[r, g[a]] - X[r, g[a + 1]], boxes[r]), min_image(X[r, g[a + 2]] - X[r, g[a + 1]], boxes[r])
                c = np.dot(u, v) / np.linalg.norm(u) / np.linalg.norm(v)
                worst = min(worst, np.sqrt(max(0.0, 1.0 - c * c)))
            out.append(worst)
    return np.asarray(out)


def kernel_case(R=3, N=600, seed=11, L=30.0):
    """(pos [R,N,3] wrapped into the box, box [3], mass [N], GroupRestraints): groups of SIZES atoms, each inside a sphere of
    8 A (radius 4), centres at least 2 A apart, the group of 256 wrapped across a face, one atom in three groups; five distance,
    four angle and four dihedral restraints with per-replica targets, k and flat, some k = 0, one distance across a face."""
    assert N >= 600
    rng = np.random.default_rng(seed)
    box = np.array([L, L, L])
    base = rng.uniform(0.0, L, (N, 3))
    c6, c5, c2 = np.array([8.0, 8.0, 8.0]), np.array([L - 0.5, 20.0, 15.0]), np.array([20.0, 8.0, 22.0])
    a6, a5, a2 = np.arange(0, 257), np.arange(257, 513), np.arange(513, 578)
    off6, off5 = _ball(rng, 257, 4.0), _ball(rng, 256, 4.0)
    base[a6], base[a5], base[a2] = c6 + off6, c5 + off5, c2 + _ball(rng, 65, 4.0)
    g4 = a6[np.argsort(off6[:, 0])[-64:]]  # the cap of the 257 with the largest x
    g3 = a5[np.argsort(off5[:, 1])[-63:]]  # the cap of the 256 with the largest y
    t = int(g4[np.argmax(base[g4, 1])])  # in the 257, its cap of 64 and the pair
    base[578] = base[t] + np.array([0.0, 3.0, 1.0])
    base[580] = np.array([0.7, 25.0, 5.0])
    pos = base[None] + rng.normal(0.0, 0.1, (R, N, 3))
    pos = pos - L * np.floor(pos / L)
    mass = rng.uniform(1.0, 16.0, N)
    gr = GroupRestraints(R)
    p5 = rng.permutation(a5)
    first = int(np.argmax(off5[p5 - 257, 0] < 0.0))  # its anchor on the high side of the face: the centre lies near x = L - 0.5
    p5[[0, first]] = p5[[first, 0]]
    members = [np.array([580]), np.array([578, t]), rng.permutation(g3), rng.permutation(g4), a2, p5, a6]
    assert tuple(len(m) for m in members) == SIZES
    for i, m in enumerate(members):
        gr.add_group(m, weights=rng.uniform(0.5, 2.0, len(m)) if i in (2, 5) else None)
    gr.masses = mass.copy()
    X = gr.centres(pos, box)
    gap = min(np.linalg.norm(min_image(X[r, i] - X[r, j], box)) for r in range(R) for i in range(7) for j in range(i))
    assert gap >= 2.0, gap
    dist = [(0, 5), (6, 2), (1, 4), (3, 0), (2, 5)]  # (0, 5): atom 580 at x = 0.7 and the group around x = L - 0.5
    ang = [(6, 2, 5), (0, 4, 2), (1, 6, 3), (5, 0, 4)]
    dih = [(6, 2, 5, 0), (4, 0, 2, 3), (1, 6, 2, 5), (3, 6, 0, 2)]
    for g in dist:
        gr.add_distance(g, 1.0, 1.0)
    for g in ang:
        gr.add_angle(g, 1.0, 1.0)
    for g in dih:
        gr.add_dihedral(g, 1.0, 1.0)
    assert sines(gr, pos, box).min() > 0.3, sines(gr, pos, box)
    s = gr.values(pos, box)
    d0 = min_image(X[0, 0] - X[0, 5], box)
    assert np.any(np.abs((X[0, 0] - X[0, 5]) - d0) > 0)  # across a face
    M = gr.nrestraints
    target = s + rng.uniform(-0.6, 0.6, (R, M))
    target[:, gr.kind == ANGLE] = np.clip(target[:, gr.kind == ANGLE], 0.05, np.pi - 0.05)
    target[:, gr.kind == DISTANCE] = np.abs(target[:, gr.kind == DISTANCE])
    k = rng.uniform(20.0, 120.0, (R, M))
    k[R // 2, 1] = k[0, 6] = k[R - 1, 10] = 0.0
    flat = np.where(rng.uniform(size=(R, M)) < 0.5, 0.0, 0.2)
    gr.set_targets(target)
    gr.set_strengths(k)
    gr.set_flat(flat)
    return pos, box, mass, gr


def big_case(N=70001, nbig=30000, seed=3, L=60.0):
    """One group of `nbig` atoms inside a sphere of 8 A, one of a single atom, a distance between them; one replica."""
    rng = np.random.default_rng(seed)
    box = np.array([L, L, L])
    pos = rng.uniform(0.0, L, (1, N, 3))
    big = rng.permutation(N)[:nbig]
    pos[0, big] = np.array([L - 1.0, 30.0, 30.0]) + _ball(rng, nbig, 4.0)
    pos = pos - L * np.floor(pos / L)
    lone = int(np.setdiff1d(np.arange(N), big)[-1])
    pos[0, lone] = np.array([6.0, 33.0, 28.0])
    mass = rng.uniform(1.0, 16.0, N)
    gr = GroupRestraints(1)
    a, b = gr.add_group(big), gr.add_group([lone])
    gr.masses = mass.copy()
    gr.add_distance((a, b), 5.0, 300.0)
    return pos, box, mass, gr


__all__ = ["ANGLE", "DIHEDRAL", "DISTANCE", "GroupRestraints", "restraint_terms", "kernel_case", "big_case", "sines", "SIZES"]
