"""The Verlet-list build (csrc/list_build.hip, planned by grid_plan.h and chain_plan.h) off the cubic, molecule-ordered lattices of
the rest of the suite: anisotropic boxes in all three placements, every stencil half-width, every blocks-per-cell split, a slab
with empty cells, scrambled atom numbers that alias in the exclusion bitmap, two droplets 10 000 A apart (the 1 024-cell clamp
and the looped build) and replicas with different grids in one batched chain.

Every case compares forces, per-term energies and the in-cutoff pair count with the CPU oracle on the same tensors (the bars of
test_gpu_parity.py), asserts the grid it claims to exercise (stats: ncell, n_rebuilds), and — periodic boxes — holds
stats()["list_entries"] inside the bracket of _list_reference.listing_bracket.  Aged lists: every atom is moved by 0.98 of its
half skin (no rebuild allowed: the list must still hold every pair inside the cutoff), then one atom to 1.02 (exactly one
rebuild).  The systems' preconditions are asserted without a GPU in test_list_systems_host.py.

TMDHIP_VSKIN=0 throughout: half skins are exactly 0.5 skin w_i, with explicit weights from [0.3, 1]."""

import numpy as np
import pytest
import torch

import _list_systems as ls
from _golden import PREC, box_tensor, pos_tensor
from _list_reference import bracket_margins, listing_bracket
from test_gpu_parity import EFAC, ERTOL, FTOL

pytestmark = pytest.mark.gpu

TERMS = ["lj", "electrostatics"]
KW = dict(cutoff=ls.CUTOFF, rfa=True)
REL = {"f32": 1e-4, "f64": 1e-10}  # displaced configurations: |dF| / (1 + |F|), as test_water_box_celllist_vs_oracle
ENV = ["TMDHIP_STENCIL", "TMDHIP_BUILD_SPLIT", "TMDHIP_PREP_SMALL", "TMDHIP_BIN2", "TMDHIP_BATCH_REPLICAS", "TMDHIP_LPA"]

_cache = {}


def _cached(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def _system(name):
    def make():
        if name == "hub":
            from _bonded_systems import LARGE, hub

            return hub(LARGE)
        if name == "clusters":
            return ls.two_clusters(**ls.CLUSTERS)
        kind, _, roll = name.partition("/")
        n = tuple(int(v) for v in np.roll({"m2": ls.BOX_M2, "slab": ls.BOX_M2, "permuted": ls.BOX_M2, "m3": ls.BOX_M3, "all": ls.BOX_ALL}[kind],
                                          int(roll or 0)))
        seed = ls.SEEDS[kind]
        return ls.water_slab(*n, seed=seed) if kind == "slab" else ls.water_box(*n, seed=seed, permute=kind == "permuted")

    return _cached(("system", name), make)


def _par(name, prec):
    s = _system(name)
    return _cached(("par", name, prec), lambda: s.par(PREC[prec]))


def _excl(name):
    from oracle import torchmd_oracle as orc

    return _cached(("excl", name), lambda: orc.exclusion_pairs(_par(name, "f64")))


def _weights(name):
    return _cached(("w", name), lambda: ls.skin_weights(_system(name).natoms, seed=3))


def _oracle(name, prec, tag, pos64):
    """(energies, forces, pairs in the cutoff) of the oracle for `pos64` (already rounded to the context's type), once per `tag`"""
    from oracle import torchmd_oracle as orc

    def make():
        s = _system(name)
        pairs = orc.candidate_pairs(pos64, s.box, ls.CUTOFF + 0.6, _excl(name))
        e, F, npairs = orc.compute(_par(name, prec), pos_tensor(pos64, 1, PREC[prec]), box_tensor(s.box, 1, PREC[prec]), TERMS, pairs=pairs, **KW)
        return e[0], F[0], npairs[0]

    return _cached(("oracle", name, prec, tag), make)


def _env(monkeypatch, **env):
    for var in ENV:
        monkeypatch.delenv(var, raising=False)
    monkeypatch.setenv("TMDHIP_VSKIN", "0")  # before any Forces object exists: half skins are exactly 0.5 skin w_i
    for var, val in env.items():
        monkeypatch.setenv("TMDHIP_" + var, str(val))


def _forces(name, prec, w=None):
    from torchmd_amd.forces import Forces

    return Forces(_par(name, prec), terms=TERMS, algorithm="celllist", skin_weights=_weights(name) if w is None else w, **KW)


def _evaluate(f, name, prec, pos64):
    """One evaluation at pos64: (energies, forces on the host, pair count, stats, device positions)"""
    dev = torch.device("cuda:0")
    s = _system(name)
    p, b = pos_tensor(pos64, 1, PREC[prec], dev), box_tensor(s.box, 1, PREC[prec], dev)
    F = torch.full_like(p, 7.0)
    e = f.compute(p, b, F, returnDetails=True)
    npairs = f.count_pairs(p, b)[0]
    return e[0], F[0].cpu(), npairs, f.stats(p), p


def _compare(name, prec, tag, pos64, e, F, npairs, relative=False):
    oe, oF, on = _oracle(name, prec, tag, pos64)
    assert npairs == on, (name, tag, npairs, on)
    if relative:
        err = ((F - oF).abs() / (1.0 + oF.abs())).max().item()
        print(name, prec, tag, "max |dF| / (1 + |F|):", err)
        assert err < REL[prec], (name, tag, err)
    else:
        err = (F - oF).abs().max().item()
        print(name, prec, tag, "max |dF|:", err)
        assert err <= FTOL[prec], (name, tag, err)
        for t in TERMS:
            assert abs(e[t] - oe[t]) <= ERTOL[prec] * EFAC * max(1.0, abs(oe[t])), (name, tag, t, e[t], oe[t])


def _in_bracket(name, prec, pos64, st, w=None):
    s = _system(name)
    hs = ls.half_skins(_weights(name) if w is None else w, prec == "f32")
    lo, hi = _cached(("bracket", name, prec, hash(pos64.tobytes()), hash(hs.tobytes())),
                     lambda: listing_bracket(pos64, s.box, _excl(name), ls.CUTOFF, hs, *bracket_margins(s.box, prec == "f64")))
    print(name, prec, "list_entries", st["list_entries"], "bracket", lo, hi)
    assert lo <= st["list_entries"] <= hi, (name, st["list_entries"], lo, hi)


def _static(name, prec, cells=None, w=None):
    """Fresh context, one evaluation at the builder's positions against the oracle and the bracket -> (context, result)"""
    s = _system(name)
    ref = ls.round_to(s.pos, prec == "f32")
    f = _forces(name, prec, w)
    e, F, npairs, st, p = _evaluate(f, name, prec, ref)
    assert st["algorithm"] == "celllist" and st["skin"] == ls.SKIN and st["overflow"] == 0
    if cells is not None:
        assert st["ncell"] == cells, (name, st["ncell"], cells)
    _compare(name, prec, "static", ref, e, F, npairs)
    if s.box.any():
        _in_bracket(name, prec, ref, st, w)
    return f, (e, F, npairs, st)


def _aged_leg(f, name, prec, bracket=True):
    """After one evaluation at the builder's positions: all atoms to 0.98 half skins (the aged list must serve), then one atom to 1.02."""
    s = _system(name)
    f32 = prec == "f32"
    ref = ls.round_to(s.pos, f32)
    w = _weights(name)
    hs = ls.half_skins(w, f32)
    # 0.98: the 0.02 s >= 0.02 x 0.5 x 1.2 x 0.3 = 3.6e-3 A of slack cover the fp32 rounding of positions below 64 A (spacing
    # 3.8e-6 A; the droplets at 10 500 A: 9.8e-4 A, test_list_systems_host.py) and of the squared displacement test
    moved = ls.round_to(ls.displaced(ref, hs, seed=4), f32)
    r0 = f.stats(pos_tensor(ref, 1, PREC[prec], "cuda:0"))["n_rebuilds"]
    e, F, npairs, st, _ = _evaluate(f, name, prec, moved)
    assert st["n_rebuilds"] == r0, (name, "the list was rebuilt inside the skin", st["n_rebuilds"], r0)
    _compare(name, prec, "moved", moved, e, F, npairs, relative=True)
    weakest = int(np.argmin(w))
    beyond = ls.round_to(ls.one_atom_beyond(ref, moved, hs, weakest, seed=5), f32)
    e, F, npairs, st, _ = _evaluate(f, name, prec, beyond)
    assert st["n_rebuilds"] == r0 + 1, (name, "one atom beyond its half skin: one rebuild", st["n_rebuilds"], r0)
    _compare(name, prec, "beyond", beyond, e, F, npairs, relative=True)
    if bracket and s.box.any():
        _in_bracket(name, prec, beyond, st)


# ---------------------------------------------------------------------------------------------------------------- (a)
@pytest.mark.parametrize("prec", ["f32", "f64"])
@pytest.mark.parametrize("roll,cells", [(0, (5, 7, 12)), (1, (12, 5, 7)), (2, (7, 12, 5))])
def test_anisotropic_box_in_every_axis_placement(roll, cells, prec, monkeypatch):
    """9 x 12 x 20 molecules: three different cell counts, the smallest exactly 2m + 1 = 5, the short axis on x, y and z."""
    _env(monkeypatch)
    assert len(set(cells)) == 3 and min(cells) == 5
    f, _ = _static(f"m2/{roll}", prec, cells)
    f.close()


# ---------------------------------------------------------------------------------------------------------------- (b)
@pytest.mark.parametrize("prec", ["f32", "f64"])
@pytest.mark.parametrize("m,name,cells", [(1, "all", (3, 3, 4)), (2, "m2", (5, 7, 12)), (3, "m3", (7, 10, 13))])
def test_every_stencil_half_width_at_its_smallest_grid(m, name, cells, prec, monkeypatch):
    """TMDHIP_STENCIL = m on a box whose shortest axis plans exactly 2m + 1 cells: every stencil row wraps onto the whole axis."""
    _env(monkeypatch, STENCIL=m)
    assert min(cells) == 2 * m + 1
    f, _ = _static(name, prec, cells)
    f.close()


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_the_three_stencils_list_the_same_pairs(prec, monkeypatch, record_property):
    """One box that admits m = 1, 2 and 3 (10 x 12 x 15 molecules): every list_entries inside the bracket, equal pair counts."""
    got = {}
    for m, cells in ((1, (3, 3, 4)), (2, (6, 7, 9)), (3, (9, 11, 13))):
        _env(monkeypatch, STENCIL=m)
        f, (e, F, npairs, st) = _static("all", prec, cells)
        got[m] = (npairs, st["list_entries"], F)
        f.close()
    print("list_entries at m = 1, 2, 3 (", prec, "):", [got[m][1] for m in (1, 2, 3)])
    record_property("list_entries_m123", [got[m][1] for m in (1, 2, 3)])
    assert got[1][0] == got[2][0] == got[3][0]


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_water_at_half_width_one_overflows_the_member_arrays(prec, monkeypatch):
    """m = 1 on water: ~150 atoms per cell (test_list_systems_host.py: every cell > 128) — three passes of the build's 64-atom
    loop, and more than the 64 members a cell of the two-launch binning holds.  With the one-launch binning switched off
    (TMDHIP_PREP_SMALL=0; it would take a system this small) the first build raises F_CELLCAP and the replica falls back to
    the four launches.  The library reports the binning through no accessor; what shows is the thrown-away build: one more
    rebuild than the same context counts when it starts with the four launches (TMDHIP_BIN2=0), and the same forces bit for
    bit — while the oracle comparison of `_static` would miss the atoms beyond the 64th of every cell without the fallback."""
    out = {}
    for bin2 in ("1", "0"):
        _env(monkeypatch, STENCIL=1, PREP_SMALL=0, BIN2=bin2)
        f, (e, F, npairs, st) = _static("all", prec, (3, 3, 4))
        out[bin2] = (F, npairs, st["n_rebuilds"], st["list_entries"])
        f.close()
    assert out["1"][2] == out["0"][2] + 1, ("the two-launch binning did not overflow", out["1"][2], out["0"][2])
    assert out["1"][1] == out["0"][1] and out["1"][3] == out["0"][3]
    if prec == "f32":
        assert torch.equal(out["1"][0], out["0"][0])
    else:
        assert ((out["1"][0] - out["0"][0]).abs() <= 1e-12 * (1.0 + out["0"][0].abs())).all()


# ---------------------------------------------------------------------------------------------------------------- (c)
@pytest.mark.parametrize("prec", ["f32", "f64"])
@pytest.mark.parametrize("name,env", [("m2/1", {}), ("all", {"STENCIL": 1}), ("all", {"STENCIL": 2}), ("all", {"STENCIL": 3}), ("slab", {}),
                                      ("permuted", {}), ("hub", {})],
                         ids=["anisotropic", "m1", "m2", "m3", "slab", "permuted", "hub"])
def test_aged_lists_serve_until_an_atom_leaves_its_skin(name, env, prec, monkeypatch):
    _env(monkeypatch, **env)
    f, _ = _static(name, prec)
    _aged_leg(f, name, prec)
    f.close()


# ---------------------------------------------------------------------------------------------------------------- (d)
@pytest.mark.parametrize("prec", ["f32", "f64"])
@pytest.mark.parametrize("name,env", [("slab", {}), ("all", {"STENCIL": 1})], ids=["slab", "m1"])
def test_blocks_per_cell_do_not_change_a_row(name, env, prec, monkeypatch):
    """TMDHIP_BUILD_SPLIT 1, 2, 3, 5, 8: shares of a cell's atoms that are no multiples of four, empty shares (the slab's thin
    cells at 8), cells of more than 64 atoms (m = 1).  chain_plan.h: which block builds an atom's row does not change the row."""
    out = {}
    for split in (1, 2, 3, 5, 8):
        _env(monkeypatch, BUILD_SPLIT=split, **env)  # (a fresh context per setting: the chain is planned with it)
        f, (e, F, npairs, st) = _static(name, prec)
        out[split] = (F, npairs, st["list_entries"])
        f.close()
    for split in (2, 3, 5, 8):
        assert out[split][1] == out[1][1] and out[split][2] == out[1][2], split
        if prec == "f32":
            assert torch.equal(out[split][0], out[1][0]), split
        else:
            assert ((out[split][0] - out[1][0]).abs() <= 1e-12 * (1.0 + out[1][0].abs())).all(), split


# ---------------------------------------------------------------------------------------------------------------- (e)
@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_scrambled_numbering_lists_what_molecule_order_lists(prec, monkeypatch):
    """6 480 atoms numbered by a random permutation: in-cutoff neighbours whose bitmap key (index mod 2048) equals the atom's own
    or an excluded partner's (hundreds of each, test_list_systems_host.py).  Same geometry as the molecule-ordered twin: equal
    pair count and list size, forces equal atom for atom within the fp32 bar."""
    _env(monkeypatch)
    perm = _system("permuted").meta["perm"]
    w_twin = _weights("m2")
    w_perm = np.empty_like(w_twin)
    w_perm[perm] = w_twin  # the same weight on the same physical atom
    f, (e, F, npairs, st) = _static("permuted", prec, (5, 7, 12), w=w_perm)
    f.close()
    f, (e2, F2, npairs2, st2) = _static("m2", prec, (5, 7, 12))
    f.close()
    assert npairs == npairs2 and st["list_entries"] == st2["list_entries"]
    err = (F[torch.as_tensor(perm)] - F2).abs().max().item()
    assert err <= FTOL[prec], err


# ---------------------------------------------------------------------------------------------------------------- (f)
@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_far_apart_open_clusters(prec, monkeypatch):
    """Two argon droplets 10 500 A apart in an open box: the 1 024-cells-per-axis clamp, 25 600 cells of which a few hundred hold
    atoms, the looped build (more than 16 384 cells) behind the four-launch binning.  No bracket here: coordinates of
    ~10 000 A have an fp32 spacing of 1e-3 A, and eight of them make a bracket wider than the 1e-3 its condition allows."""
    _env(monkeypatch)
    f, (e, F, npairs, st) = _static("clusters", prec)
    assert st["ncell"][0] == 1024 and st["ncell"] == (1024, 5, 5) and np.prod(st["ncell"]) > 16384
    _aged_leg(f, "clusters", prec, bracket=False)
    f.close()


# ---------------------------------------------------------------------------------------------------------------- (g)
def test_replicas_with_different_anisotropic_grids(monkeypatch):
    """One fp32 context, three replicas: the three axis placements of the 9 x 12 x 20 box scaled by 1.00, 1.03 and 1.06 —
    blockIdx.y = replica of the batched chain with per-replica cell counts."""
    from torchmd_amd.forces import Forces
    from torchmd_amd.integrator import Integrator, maxwell_boltzmann
    from torchmd_amd.systems import System

    dev, dt = torch.device("cuda:0"), torch.float32
    scale = [1.00, 1.03, 1.06]
    sys3 = [_system(f"m2/{r}") for r in range(3)]
    n = sys3[0].natoms
    pos = [s.pos * k for s, k in zip(sys3, scale)]
    box = [s.box * k for s, k in zip(sys3, scale)]
    cells = [ls.expected_cells(b, 2) for b in box]
    assert all(len(set(c)) == 3 and min(c) == 5 for c in cells) and len(set(cells)) == 3, cells
    terms = ["lj", "electrostatics", "bonds", "angles"]
    par = _par("m2/0", "f32")  # (molecule order: one topology for the three)
    w = _weights("m2/0")
    torch.manual_seed(7)
    vel = maxwell_boltzmann(par.masses, 300, 3)

    def context(idx):
        s = System(n, len(idx), dt, dev)
        s.set_positions(np.stack([pos[i] for i in idx], axis=2))
        s.set_box(np.stack([box[i] for i in idx], axis=1))
        s.set_velocities(vel[idx].clone())
        return s, Forces(par, terms=terms, algorithm="celllist", skin_weights=w, **KW)

    def run(batch):
        _env(monkeypatch, LPA=16, **({} if batch else {"BATCH_REPLICAS": 0}))  # (LPA: pinned, it follows the atoms that share a launch)
        s, f = context([0, 1, 2])
        f.compute(s.pos, s.box, s.forces)
        F0 = s.forces.clone()
        st0 = [f.stats(s.pos, r) for r in range(3)]
        integ = Integrator(s, f, 1.0, dev)
        integ.step(20)
        st = [f.stats(s.pos, r) for r in range(3)]
        out = (F0, s.pos.clone(), s.vel.clone(), st0, st)
        f.close()
        return out

    F0, pb, vb, st0, st = run(True)
    for r in range(3):
        assert st0[r]["ncell"] == cells[r] and st0[r]["algorithm"] == "celllist", (r, st0[r]["ncell"], cells[r])
        assert st[r]["n_rebuilds"] >= st0[r]["n_rebuilds"] + 1, (r, "no rebuild in 20 steps")
    assert st[0]["batched_launches"] > 0
    for r in range(3):  # one compute of the three = three single-replica contexts
        s1, f1 = context([r])
        f1.compute(s1.pos, s1.box, s1.forces)
        assert f1.stats(s1.pos)["ncell"] == cells[r]
        assert torch.equal(s1.forces[0], F0[r]), r
        f1.close()
    F0s, ps, vs, _, sts = run(False)
    assert sts[0]["batched_launches"] == 0
    assert torch.equal(F0, F0s) and torch.equal(pb, ps) and torch.equal(vb, vs)
    assert torch.isfinite(pb).all() and (pb - torch.as_tensor(np.stack(pos), dtype=dt, device=dev)).abs().max() > 0.05
