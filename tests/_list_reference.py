"""A reference for the SIZE of the Verlet lists (stats()["list_entries"]): numpy, fp64, no GPU."""

import numpy as np

FP32_EPS = 2.0 ** -23  # spacing of fp32 numbers in [1, 2)
BUILD_MARGIN_F64 = 2.0e-4  # engine.h: kBuildMarginF64


def fp32_ulp(x):
    """Spacing of the fp32 numbers at |x|"""
    return float(np.spacing(np.float32(abs(x))))


def bracket_margins(box, fp64_context):
    """(eps_lo, eps_hi) of `listing_bracket` for a list built in a periodic box with edges `box` (see there)."""
    eps_lo = 8.0 * fp32_ulp(np.max(box))
    return eps_lo, eps_lo + (BUILD_MARGIN_F64 if fp64_context else 0.0)


def min_image_distance(pos, box, i, j):
    d = pos[i] - pos[j]
    if np.any(box != 0):
        d = d - box * np.round(d / box)
    return np.sqrt((d * d).sum(axis=1))


def listing_bracket(pos, box, excl, cutoff, half_skin, eps_lo, eps_hi, max_width=1e-3):
    """(lower, upper): the numbers of ordered pairs i != j, not excluded, whose fp64 minimum-image distance d satisfies
    d <= cutoff + s_i + s_j - eps_lo (lower) and d <= cutoff + s_i + s_j + eps_hi (upper).  The list rows of all atoms together
    (every pair is held by both of its atoms) must hold at least `lower` and at most `upper` entries.

    Where the margins come from (bracket_margins) — derived, not measured.  The build (list_build.hip) lists j for i when
    |x_i - x_j'|^2 <= (cutoff + s_i + s_j [+ kBuildMarginF64])^2 in fp32, x the coordinates folded into [0, L) and x_j' the
    image of j next to i's cell.  With u = one fp32 spacing at the largest box edge L (every folded coordinate is below L, an
    image below 2L), per coordinate:
      - the fold x - floor(x / L) L: the product is exact for the few box lengths an atom strays, the difference rounds once,
        <= 0.5 u — twice, for i and j; an fp64 context folds in fp64 and rounds to fp32 once, the same bound;
      - the image shift x_j +- L: a result below 2L, <= 1 u;
      - the difference x_i - x_j': <= 0.5 u.
    That is <= 2.5 u per coordinate and <= sqrt(3) x 2.5 u = 4.4 u on the distance.  The square, the three-term sum and the
    squared radius carry relative roundings of 2^-24 each, ~3 x 2^-24 on d^2, so 1.5 x 2^-24 x d on d: at d <= 10.2 A and
    L >= 25 A below 0.4 u; the half skins, rounded to fp32, add 2^-24 x 0.6 A each.  Sum < 5 u; eps_lo = 8 u leaves room for the
    compiler's contractions.  An fp64 context adds kBuildMarginF64 to every radius, on purpose (engine.h): eps_hi = eps_lo +
    2e-4 there, and eps_lo alone in fp32.  The exact filter below is fp64 on the same inputs the context received.

    The bracket must be narrow or it would hide a missing stencil row: asserted here, upper - lower <= 1e-3 lower (max_width=None:
    not asserted — for the comparison of this function itself with a brute force on a few hundred atoms).
    """
    from scipy.spatial import cKDTree

    pos = np.asarray(pos, dtype=np.float64)
    box = np.asarray(box, dtype=np.float64).reshape(3)
    s = np.asarray(half_skin, dtype=np.float64)
    n = len(pos)
    assert s.shape == (n,) and eps_lo >= 0 and eps_hi >= 0
    rmax = cutoff + 2.0 * s.max() + eps_hi
    if np.all(box == 0):
        tree = cKDTree(pos)
    else:
        assert (box > 2.0 * rmax).all(), "a pair would be within reach through two images"
        w = pos - np.floor(pos / box) * box
        w = np.where(w >= box, w - box, w)
        tree = cKDTree(w, boxsize=box)
    pairs = tree.query_pairs(rmax * (1 + 1e-12) + 1e-9, output_type="ndarray").astype(np.int64)
    i, j = pairs.min(axis=1), pairs.max(axis=1)
    if excl is not None and len(excl):
        e = np.asarray(excl, dtype=np.int64).reshape(-1, 2)
        ekey = np.minimum(e[:, 0], e[:, 1]) * n + np.maximum(e[:, 0], e[:, 1])
        keep = ~np.isin(i * n + j, ekey)
        i, j = i[keep], j[keep]
    d = min_image_distance(pos, box, i, j)
    r = cutoff + s[i] + s[j]
    lower = 2 * int((d <= r - eps_lo).sum())
    upper = 2 * int((d <= r + eps_hi).sum())
    assert max_width is None or upper - lower <= max_width * lower, (lower, upper)
    return lower, upper


def pairs_within(pos, box, excl, cutoff):
    """Unordered non-excluded pairs (i < j) with fp64 minimum-image distance <= cutoff, as an [P, 2] array sorted by (i, j)."""
    from oracle import torchmd_oracle as orc

    p = orc.candidate_pairs(pos, box, cutoff + 1e-6, excl)
    d = min_image_distance(np.asarray(pos, dtype=np.float64), np.asarray(box, dtype=np.float64), p[:, 0], p[:, 1])
    return p[d <= cutoff]
