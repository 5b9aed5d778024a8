"""Shared pieces of the tests of metadynamics on CVs of groups of atoms: the jittered lattice and its groups,
the cases of the kernel tests, a grid pre-filled beside the CVs of a configuration, the sums of the absolute addends and the
number of additions an addend passes through on the device (the c of the bars)."""

import numpy as np

from torchmd_amd.metadynamics import Metadynamics, coordination_pairs, min_image

EPS64 = np.finfo(np.float64).eps
THREADS, SPLIT_PAIRS, SPLIT_BLOCKS = 256, 64, 1024  # kCvThreads, kCvSplitPairs, kCvSplitBlocks of csrc/cv_math.h
L = 30.0
SWITCH = {"r0": 3.5, "n": 6, "d_max": 9.0}


def lattice(R=3, nside=12, edge=L, seed=5, jitter=0.4):
    """R replicas of nside^3 atoms on a cubic lattice in a box of `edge`, every atom displaced by up to `jitter` Å per
    component (replicas differently), wrapped into the box; masses in {1.008, 15.999}."""
    rng = np.random.default_rng(seed)
    a = edge / nside
    g = (np.stack(np.meshgrid(*[np.arange(nside)] * 3, indexing="ij"), axis=-1).reshape(-1, 3) + 0.5) * a
    pos = np.mod(g[None] + rng.uniform(-jitter, jitter, (R, len(g), 3)), edge)
    mass = np.where(rng.random(len(g)) < 0.6, 1.008, 15.999)
    return pos, mass


def nearest(pos0, centre, n, box, skip=()):
    """The n atoms of pos0 [N,3] nearest to `centre` in the minimum image, nearest first, without those in `skip`."""
    d = min_image(pos0 - np.asarray(centre, dtype=np.float64), box)
    order = [int(i) for i in np.argsort((d * d).sum(axis=1), kind="stable") if int(i) not in set(skip)]
    return order[:n]


def nsplit(nlane, nstream):
    nblocks = (nlane + THREADS - 1) // THREADS
    return max(1, min((nstream + SPLIT_PAIRS - 1) // SPLIT_PAIRS, max(1, SPLIT_BLOCKS // nblocks)))


def value_depth(nA, nB):
    """The additions one addend of a coordination CV's value passes through on the device: the lane's own chunk, the butterfly
    (6), the meet of four waves (2), the folding lane's rows, the butterfly (6)."""
    nlane, nstream = (nA, nB) if nA >= nB else (nB, nA)
    S = nsplit(nlane, nstream)
    chunk = (nstream + S - 1) // S
    rows = (nlane + THREADS - 1) // THREADS * S
    return chunk + 6 + 2 + (rows + 63) // 64 + 6


def gradient_depth(nA, nB):
    """... of an atom's gradient: the chunk of a lane, its splits, and one more addition for an atom of both sets."""
    worst = 0
    for nlane, nstream in ((nA, nB), (nB, nA)):
        S = nsplit(nlane, nstream)
        worst = max(worst, (nstream + S - 1) // S + S)
    return worst + 1


def coordination_magnitudes(md, c, pos, box):
    """(sum |f|, sum over the pairs of |gd| per atom [N,3]) of coordination CV c of one replica."""
    A, B = (md.group_atoms[g] for g in md.cv_groups[c])
    f, gd = coordination_pairs(pos, box, A, B, **md.coord[c])
    mag = np.zeros_like(pos)
    np.add.at(mag, A, np.abs(gd).sum(axis=1))
    np.add.at(mag, B, np.abs(gd).sum(axis=0))
    return float(np.abs(f).sum()), mag


def cv_bars(md, pos, box):
    """The bar of every CV of one replica against the model, c eps64 sum|addends| with c counted from the operation sequence.
    Coordination: the addends are the model's to the bit (the same IEEE operations on the same doubles), the model's sum is
    exact and rounded once (1 half-ulp), the device's passes every addend through `value_depth` additions of at most half an
    ulp of sum|addends| each: c = (depth + 1) / 2.  Centres: the model takes the centre sums in the kernel's order and the CV by
    the same operations; only acos (an angle) is a libm call on either side, 1 ulp each: 4 eps64 |s| covers it, the rounding of
    the centre itself (x_a0 + sum, an ulp of a coordinate of up to L against a distance of a few Å) included."""
    s, _ = md.group_cv_values(pos, box)
    out = np.zeros(md.ncv)
    for c in range(md.ncv):
        if md.cv_kind[c] == 5:
            nA, nB = (len(md.group_atoms[g]) for g in md.cv_groups[c])
            out[c] = 0.5 * (value_depth(nA, nB) + 1) * EPS64 * coordination_magnitudes(md, c, pos, box)[0]
        else:
            out[c] = 4 * EPS64 * max(abs(s[c]), 1.0)
    return out


def prefill(md, pos, box, offsets=((0.3, 30.0), (-0.5, 12.0), (0.9, 8.0)), scale=1.0):
    """A grid with hills beside the CVs of `pos` [R,N,3]: per replica, centres at s + off sigma (off per hill, the second CV
    with the sign turned), heights w (1 + 0.2 r); every grid of a shared bias gets all of them."""
    pos = np.asarray(pos, dtype=np.float64)
    box = md._boxes(box, pos.shape[0])
    grid = np.zeros_like(md.grid)
    for r in range(pos.shape[0]):
        s, _ = md.cv_values(pos[r], box[r])
        for off, w in offsets:
            s0 = np.array([s[c] + (off if c == 0 else -off) * md.sigma[c] for c in range(md.ncv)])
            grid[0 if md.walkers == "shared" else r] += md.gauss_terms(s0, scale * w * (1.0 + 0.2 * r))
    return grid


def _range(md_kw, c, lo, hi, sigma, bins):
    md_kw["grid_min"][c], md_kw["grid_max"][c], md_kw["sigma"][c], md_kw["grid_bins"][c] = lo, hi, sigma, bins


def kernel_case(name, R=3, walkers="independent", seed=5):
    """(pos [R,N,3], box [3], mass [N], Metadynamics) of the kernel tests on the 1 728-atom lattice.  Every centre group is the
    n atoms nearest to a point, nearest first (so every member lies within half an edge of the first)."""
    pos, mass = lattice(R=R, seed=seed)
    box = np.full(3, L)
    p0 = pos[0]
    near = lambda centre, n, skip=(): nearest(p0, centre, n, box, skip)  # noqa: E731
    kw = dict(sigma=[0.0, 0.0], height=1.2, frequency=1, temperature=300.0, bias_factor=6.0, grid_min=[None, None],
              grid_max=[None, None], grid_bins=[1, 1], nreplicas=R, walkers=walkers)
    if name == "centres":
        # a single atom against 600 atoms around a corner of the box (across three faces); the angle of 2, 255 and 256 atoms
        g600 = near([0.5, 0.5, 29.5], 600)
        g1 = near([9.0, 8.0, 10.0], 1, skip=g600)
        cvs = [("group_distance", (g1, g600)), ("group_angle", (near([6.0, 20.0, 9.0], 2), near([15.0, 15.0, 15.0], 255),
                                                                near([24.0, 9.0, 22.0], 256)))]
        _range(kw, 0, 5.0, 25.0, 0.4, 120)
        _range(kw, 1, 0.0, np.pi, 0.1, 80)
    elif name == "shared atom":
        # a dihedral of 257, 2, 1 and 256 atoms and a distance whose first group shares atoms with the dihedral's first: those
        # atoms are in two groups and in both CVs; explicit weights on one group
        a = near([5.0, 5.0, 5.0], 257)
        b, c_, d = near([14.0, 6.0, 8.0], 2), near([16.0, 15.0, 9.0], 1), near([24.0, 17.0, 20.0], 256)
        e = {"atoms": a[:40] + near([8.0, 22.0, 24.0], 20, skip=a), "weights": list(np.linspace(0.5, 3.0, 60))}
        cvs = [("group_dihedral", (a, b, c_, d)), ("group_distance", (e, near([22.0, 24.0, 6.0], 30)))]
        kw["sigma"][0], kw["grid_bins"][0] = 0.3, 48
        _range(kw, 1, 5.0, 25.0, 0.4, 120)
    elif name == "coordination 63x1000, 130=130":
        A = near([10.0, 10.0, 10.0], 63)
        S = near([20.0, 20.0, 20.0], 130)
        cvs = [("coordination", (A, near([12.0, 12.0, 12.0], 1000)), SWITCH), ("coordination", (S, S), dict(SWITCH, d0=0.5, n=4))]
        _range(kw, 0, 0.0, 2000.0, 20.0, 250)
        _range(kw, 1, 0.0, 3000.0, 20.0, 300)
    elif name == "coordination 1x257, 65x64 overlapping":
        A = near([3.0, 28.0, 15.0], 65)  # (by a face)
        B = A[50:] + near([6.0, 2.0, 15.0], 49, skip=A)
        cvs = [("coordination", (near([15.0, 15.0, 15.0], 1), near([15.0, 15.0, 15.0], 257)), SWITCH), ("coordination", (A, B), SWITCH)]
        _range(kw, 0, 0.0, 60.0, 1.0, 150)
        _range(kw, 1, 0.0, 400.0, 8.0, 120)
    elif name == "coordination 64x65, 130x1":
        cvs = [("coordination", (near([10.0, 20.0, 10.0], 64), near([12.0, 21.0, 11.0], 65)), dict(SWITCH, n=12)),
               ("coordination", (near([21.0, 8.0, 16.0], 130), near([21.0, 8.0, 16.0], 1)), SWITCH),]
        _range(kw, 0, 0.0, 600.0, 8.0, 160)
        _range(kw, 1, 0.0, 60.0, 1.0, 150)
    elif name == "zero box":
        box = np.zeros(3)
        near = lambda centre, n, skip=(): nearest(p0, centre, n, box, skip)  # noqa: E731
        cvs = [("coordination", (near([10.0, 10.0, 10.0], 64), near([12.0, 12.0, 12.0], 1000)), {"r0": 3.5, "n": 6}),
               ("group_distance", (near([5.0, 5.0, 5.0], 255), near([25.0, 25.0, 25.0], 2)))]
        _range(kw, 0, 0.0, 2000.0, 20.0, 250)
        _range(kw, 1, 20.0, 50.0, 0.4, 200)
    elif name == "one open axis":
        box = np.array([L, 0.0, L])
        near = lambda centre, n, skip=(): nearest(p0, centre, n, box, skip)  # noqa: E731
        cvs = [("coordination", (near([1.0, 10.0, 29.0], 65), near([29.0, 12.0, 1.0], 257)), SWITCH),
               ("group_angle", (near([1.0, 3.0, 15.0], 40), near([29.0, 15.0, 15.0], 600), near([15.0, 27.0, 1.0], 40)))]
        _range(kw, 0, 0.0, 1000.0, 10.0, 250)
        _range(kw, 1, 0.0, np.pi, 0.1, 80)
    else:
        raise KeyError(name)
    md = Metadynamics(cvs, **kw)
    md.masses = mass.copy()
    return pos, box, mass, md


KERNEL_CASES = ("centres", "shared atom", "coordination 63x1000, 130=130", "coordination 1x257, 65x64 overlapping",
                "coordination 64x65, 130x1", "zero box", "one open axis")


def moved(pos, k, box, seed=3, amp=0.05):
    """The positions of deposition k: every atom displaced by up to `amp` Å per component, wrapped along the periodic axes."""
    rng = np.random.default_rng(seed + 1000 * k)
    p = pos + rng.uniform(-amp, amp, pos.shape)
    for c in range(3):
        if box[c] != 0.0:
            p[..., c] = np.mod(p[..., c], box[c])
    return p
