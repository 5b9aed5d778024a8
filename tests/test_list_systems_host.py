"""The list-build tests' own tools, checked without a GPU: the reference for the size of the lists (_list_reference.py)
against an O(N^2) brute force, and every system of _list_systems.py against the preconditions its GPU test
(test_gpu_list_build.py) relies on — so that none of those tests can pass vacuously."""

import numpy as np
import pytest

import _list_systems as ls
from _list_reference import bracket_margins, listing_bracket, pairs_within
from torchmd_amd.forces import build_exclusion_csr


def _brute(pos, box, excl, cutoff, s, eps_lo, eps_hi):
    n = len(pos)
    d = pos[:, None, :] - pos[None, :, :]
    if np.any(box != 0):
        d -= box * np.round(d / box)
    dist = np.sqrt((d * d).sum(-1))
    allowed = ~np.eye(n, dtype=bool)
    for a, b in excl:
        allowed[a, b] = allowed[b, a] = False
    r = cutoff + s[:, None] + s[None, :]
    return int(((dist <= r - eps_lo) & allowed).sum()), int(((dist <= r + eps_hi) & allowed).sum())


@pytest.mark.parametrize("periodic", [True, False])
def test_bracket_equals_brute_force(periodic):
    rng = np.random.default_rng(5)
    n = 300
    box = np.array([9.0, 11.5, 14.2]) if periodic else np.zeros(3)
    pos = rng.uniform(-3.0, 17.0, size=(n, 3))  # (periodic: atoms up to two box lengths outside)
    excl = rng.integers(0, n, size=(200, 2))
    excl = excl[excl[:, 0] != excl[:, 1]]
    s = rng.uniform(0.05, 0.5, size=n)
    # (margins wide enough that lower and upper differ on 300 atoms; the width condition is about real systems, checked below)
    for eps_lo, eps_hi in ((0.0, 0.0), (1e-3, 2e-3)):
        want = _brute(pos, box, excl, 3.0, s, eps_lo, eps_hi)
        assert listing_bracket(pos, box, excl, 3.0, s, eps_lo, eps_hi, max_width=None) == want and want[0] > 1000
    assert _brute(pos, box, excl, 3.0, s, 1e-3, 2e-3)[1] > _brute(pos, box, excl, 3.0, s, 1e-3, 2e-3)[0]


def test_bracket_refuses_a_wide_margin():
    s = ls.water_box(4, 4, 7, seed=1)
    hs = np.full(s.natoms, 0.3)
    listing_bracket(s.pos, s.box * 3, s.exclusions(), 3.0, hs, 0.0, 0.0)
    with pytest.raises(AssertionError):
        listing_bracket(s.pos, s.box * 3, s.exclusions(), 3.0, hs, 0.05, 0.05)


def _systems():
    from _bonded_systems import LARGE, hub

    sd = ls.SEEDS
    out = {"m2": ls.water_box(*ls.BOX_M2, seed=sd["m2"]), "m3": ls.water_box(*ls.BOX_M3, seed=sd["m3"]),
           "all": ls.water_box(*ls.BOX_ALL, seed=sd["all"]), "slab": ls.water_slab(*ls.BOX_M2, seed=sd["slab"]),
           "permuted": ls.water_box(*ls.BOX_M2, seed=sd["permuted"], permute=True)}
    for k in (1, 2):
        nxyz = tuple(np.roll(ls.BOX_M2, k))
        out[f"m2-roll{k}"] = ls.water_box(*nxyz, seed=sd["m2"])
    h = hub(LARGE)
    from oracle import torchmd_oracle as orc

    out["hub"] = ls.ListSystem("hub", None, h.pos, h.box, "bonded", {"excl": orc.exclusion_pairs(h.par()), "par": h.par})
    return out


@pytest.fixture(scope="module")
def systems():
    return _systems()


def _excl(s):
    return s.meta["excl"] if s.kind == "bonded" else s.exclusions()


def test_planned_cells(systems):
    """The cell counts the GPU tests assert, from the planner's floor(L / (rlist / m)): three different values, the smallest 2m + 1."""
    assert ls.expected_cells(systems["m2"].box, 2) == (5, 7, 12)
    assert ls.expected_cells(systems["m2-roll1"].box, 2) == (12, 5, 7)
    assert ls.expected_cells(systems["m2-roll2"].box, 2) == (7, 12, 5)
    assert ls.expected_cells(systems["m3"].box, 3) == (7, 10, 13)
    assert [ls.expected_cells(systems["all"].box, m) for m in (1, 2, 3)] == [(3, 3, 4), (6, 7, 9), (9, 11, 13)]
    assert systems["m2"].natoms == 6480 and max(s.natoms for s in systems.values()) <= 7200
    for s in systems.values():  # no edge is a multiple of another
        if s.kind == "water":
            q = s.box[:, None] / s.box[None, :]
            assert (np.abs(q - np.round(q))[~np.eye(3, dtype=bool)] > 0.02).all(), s.name
    # m = 1 on water: every cell holds more than the 64 atoms of a member array and of one pass of the build's atom loop
    s = systems["all"]
    nc = np.array([3, 3, 4])
    c = np.floor((s.pos % s.box) / (s.box / nc)).astype(int)
    counts = np.bincount((c[:, 0] * nc[1] + c[:, 1]) * nc[2] + c[:, 2], minlength=nc.prod())
    assert counts.min() > 128 and counts.max() < 192


@pytest.mark.parametrize("f32", [True, False])
def test_bracket_width_on_every_periodic_system(systems, f32):
    for name, s in systems.items():
        w = ls.skin_weights(s.natoms, seed=3)
        hs = ls.half_skins(w, f32)
        lo, hi = listing_bracket(ls.round_to(s.pos, f32), s.box, _excl(s), ls.CUTOFF, hs, *bracket_margins(s.box, not f32))
        print(name, "f32" if f32 else "f64", lo, hi, (hi - lo) / lo)
        assert lo > 0 and hi - lo <= 1e-3 * lo  # (asserted by the helper too)
        # ... also at the displaced positions the aged-list tests use
        moved = ls.displaced(ls.round_to(s.pos, f32), hs, seed=4)
        listing_bracket(ls.round_to(moved, f32), s.box, _excl(s), ls.CUTOFF, hs, *bracket_margins(s.box, not f32))


def test_the_oracle_resolves_the_energy_bar_in_fp32(systems):
    """The GPU tests hold each energy term to ERTOL x EFAC x max(1, |E|) against the oracle evaluated in the context's precision.
    The electrostatic energy of randomly oriented waters is a small remainder of large pair terms, so the fp32 oracle itself
    carries an error (against fp64 on the same fp32 values) that does not shrink with |E|: it may use at most half of the bar,
    or a case would test the cancellation of the sum, not the list.  (_list_systems.SEEDS: seed 12 on the m = 3 box does not.)"""
    import torch

    from _golden import box_tensor, pos_tensor
    from oracle import torchmd_oracle as orc
    from test_gpu_parity import EFAC, ERTOL

    terms = ["lj", "electrostatics"]
    for name, s in systems.items():
        ref = ls.round_to(s.pos, True)
        par = s.meta["par"] if s.kind == "bonded" else s.par
        pairs = orc.candidate_pairs(ref, s.box, ls.CUTOFF + 0.6, orc.exclusion_pairs(par(torch.float64)))
        e = {}
        for dt in (torch.float32, torch.float64):
            e[dt] = orc.compute(par(dt), pos_tensor(ref, 1, dt), box_tensor(s.box, 1, dt), terms, pairs=pairs, cutoff=ls.CUTOFF, rfa=True)[0][0]
        for t in terms:
            own, bar = abs(e[torch.float32][t] - e[torch.float64][t]), ERTOL["f32"] * EFAC * max(1.0, abs(e[torch.float64][t]))
            print(name, t, e[torch.float64][t], "fp32 oracle off by", own, "bar", bar)
            assert own <= 0.5 * bar, (name, t, own, bar)


def test_permuted_box_aliases_in_the_exclusion_bitmap(systems):
    """The build's bitmap is keyed by original index mod 2048: the permuted box has in-cutoff, non-excluded pairs whose key equals
    the atom's own, and pairs whose key equals that of one of the atom's first two excluded partners."""
    s, twin = systems["permuted"], systems["m2"]
    assert s.natoms >= 4097
    perm = s.meta["perm"]
    assert np.allclose(s.pos[perm], twin.pos) and sorted(perm) == list(range(s.natoms))
    p = pairs_within(s.pos, s.box, s.exclusions(), ls.CUTOFF)
    pt = pairs_within(twin.pos, twin.box, twin.exclusions(), ls.CUTOFF)
    assert len(p) == len(pt) > 900_000
    both = np.concatenate([p, p[:, ::-1]])  # ordered (i, j)
    own = ((both[:, 0] - both[:, 1]) % 2048 == 0).sum()
    off, idx = build_exclusion_csr(s.natoms, s.exclusions())
    assert (np.diff(off) == 2).all()  # water: the two other atoms of the molecule
    first_two = idx.reshape(-1, 2)
    partner = ((both[:, 1, None] - first_two[both[:, 0]]) % 2048 == 0).any(axis=1).sum()
    print("aliased pairs: own key", own, "partner's key", partner)
    assert own >= 100 and partner >= 100
    # the molecule-ordered twin has none of the first kind within reach of a partner: its aliases are 2 048 atoms = 683 molecules apart
    assert (((pt[:, 0] - pt[:, 1]) % 2048 == 0).sum()) < own


def test_slab_differs_from_the_full_box(systems):
    slab, full = systems["slab"], systems["m2"]
    assert 0.45 * full.natoms < slab.natoms < 0.55 * full.natoms and slab.natoms % 3 == 0
    ns, nf = len(pairs_within(slab.pos, slab.box, slab.exclusions(), ls.CUTOFF)), len(pairs_within(full.pos, full.box, full.exclusions(), ls.CUTOFF))
    assert ns != nf and ns < 0.5 * nf
    # the upper half holds no oxygen: at m = 2, whole layers of cells hold no atom at all
    nc = np.array(ls.expected_cells(slab.box, 2))
    cz = np.floor((slab.pos[:, 2] % slab.box[2]) / (slab.box[2] / nc[2])).astype(int)
    assert len(np.unique(cz)) <= nc[2] // 2 + 2


def test_clusters_need_the_axis_clamp_and_the_looped_build():
    s = ls.two_clusters(**ls.CLUSTERS)
    assert s.natoms == 2 * ls.CLUSTERS["n_each"] <= 7000 and (s.box == 0).all()
    lo, hi = s.pos.min(axis=0) - 1e-3, s.pos.max(axis=0) + 1e-3  # (context.hip: replan)
    ext = hi - lo
    # the two inequalities, with the half-width-2 cells of rlist / 2 ...
    fine = np.floor(ext / (ls.RLIST / 2))
    assert fine[0] > 1024 and 1024 * fine[1] * fine[2] > 16384
    # ... and with the cells the planner takes here: at 0.0003 atoms per cell it steps down to m = 1 (grid_plan.h)
    coarse = np.floor(ext / ls.RLIST)
    assert s.natoms / (1024 * fine[1] * fine[2]) < 4.0
    assert coarse[0] > 1024 and 1024 * coarse[1] * coarse[2] > 16384
    assert ls.expected_cells(ext, 1) == (1024, 5, 5)
    # no atom of one droplet is within reach of the other, each droplet is one liquid blob
    half = ls.CLUSTERS["n_each"]
    assert s.pos[:half, 0].max() + 1000 < s.pos[half:, 0].min()
    p = pairs_within(s.pos, s.box, None, ls.CUTOFF)
    assert len(p) > 20 * s.natoms and ((p[:, 0] < half) == (p[:, 1] < half)).all()
    # fp32 spacing at these coordinates against the slack of the aged-list leg (0.02 half skins >= 3.6e-3 A)
    assert np.sqrt(3) * 0.5 * np.spacing(np.float32(np.abs(s.pos).max())) < 0.25 * 3.6e-3


@pytest.mark.parametrize("f32", [True, False])
def test_displacements_stay_inside_the_skin_and_change_the_pair_set(systems, f32):
    every = dict(systems, clusters=ls.two_clusters(**ls.CLUSTERS))
    for name, s in every.items():
        ref = ls.round_to(s.pos, f32)
        w = ls.skin_weights(s.natoms, seed=3)
        assert w.max() == 1.0 and w.min() == 0.3 and (w == w.min()).sum() == 1
        hs = ls.half_skins(w, f32)
        moved = ls.round_to(ls.displaced(ref, hs, seed=4), f32)
        step = np.linalg.norm(moved - ref, axis=1)
        assert (step < hs).all() and (step > 0.95 * hs).all(), name
        weakest = int(np.argmin(w))
        beyond = ls.round_to(ls.one_atom_beyond(ref, moved, hs, weakest, seed=5), f32)
        step2 = np.linalg.norm(beyond - ref, axis=1)
        assert step2[weakest] > hs[weakest] and (np.delete(step2, weakest) < np.delete(hs, weakest)).all(), name
        excl = None if s.kind == "argon" else _excl(s)
        key = lambda p: set((p[:, 0] * s.natoms + p[:, 1]).tolist())
        a, b = key(pairs_within(ref, s.box, excl, ls.CUTOFF)), key(pairs_within(moved, s.box, excl, ls.CUTOFF))
        print(name, "pairs", len(a), "entering", len(b - a), "leaving", len(a - b))
        assert len(b - a) >= 1000 and len(a - b) >= 1000, name
