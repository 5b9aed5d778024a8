"""Smooth PME on the GPU at its edges: every spline order on odd, prime, minimal and anisotropic grids, unwrapped and
face-sitting coordinates, sparse and uncharged systems, exclusion sets, replicas with boxes of their own, a 98 304-atom
box and the MD loop's recovery paths.

The yardsticks are those of tests/test_gpu_pme.py: fp64 GPU against the host PME of tests/_ewald.py with the same beta, grid
and order — forces to 1e-8 kcal/mol/A, the energy to 1e-10 of the total (1e-12 of the self term when the total is mostly
cancellation) — and fp32 against fp64 GPU with the bounds of test_fp32_against_fp64 (forces 5e-3 kcal/mol/A, the energy
2e-5 of the self term).  Observed errors are printed (pytest -s) and recorded in the docstrings.
"""

import json

import numpy as np
import pytest
import torch

import _ewald as E
import _golden as G
from test_gpu_pme import DEV, EXCL, _atomic_par, _box_t, _integrator_against_loop, _ions, _tip3p, _water

pytestmark = pytest.mark.gpu

F64_FORCE, F64_ENERGY, F64_ENERGY_SELF = 1e-8, 1e-10, 1e-12
F32_FORCE, F32_ENERGY = 5e-3, 2e-5


def _report(tag, **errs):
    print("PME-EDGES " + json.dumps({"case": tag, **{k: float(f"{v:.3e}") for k, v in errs.items()}}))


def _compute(par, pos, box, dtype, terms, R=1, twice=False, **kw):
    """Forces + energies of one `compute` on a fresh context; `twice`: a second call on the same context must give the
    same forces — bit for bit on the cell-list path (PME has no float atomics; a context that keeps its list takes other
    launch paths then)."""
    from torchmd_amd.forces import Forces

    fo = Forces(par, terms=terms, **kw)
    p = torch.as_tensor(np.asarray(pos, np.float64), dtype=dtype, device=DEV)
    p = (p[None].repeat(R, 1, 1) if p.dim() == 2 else p).contiguous()
    b = box if torch.is_tensor(box) else _box_t(box, R, dtype)
    f = torch.zeros_like(p)
    e = fo.compute(p, b, f, returnDetails=True)
    if twice:
        f2 = torch.zeros_like(p)
        e2 = fo.compute(p, b, f2, returnDetails=True)
        if fo.stats(p)["algorithm"] == "celllist":
            assert torch.equal(f, f2), ("second call", (f - f2).abs().max().item())
        else:  # (the all-pairs kernels add their forces with atomics)
            tol = (1e-12 if dtype == torch.float64 else 1e-5) * max(1.0, f.abs().max().item())
            assert (f - f2).abs().max().item() <= tol, ("second call", (f - f2).abs().max().item())
        assert abs(e2[0]["electrostatics"] - e[0]["electrostatics"]) <= 1e-12 * max(1.0, abs(e[0]["electrostatics"]))
    return fo, e, f.double().cpu().numpy()


def _host(pos, q, box, beta, rc, grid, order, excl):
    return E.pme(pos, q, box, beta, rc, grid, order, excl, pairs="kdtree")


def _check64(tag, e, f, eh, fh, q, box, beta, term="electrostatics"):
    eself = abs(E.self_and_background(q, box, beta))
    bound = F64_ENERGY * abs(eh) if abs(eh) > 1e-2 * eself else F64_ENERGY_SELF * eself
    de, df = abs(e[term] - eh), np.abs(f - fh).max()
    _report(tag + " fp64-host", dE=de, dE_bound=bound, dF=df)
    assert de <= bound, (tag, e[term], eh)
    assert df <= F64_FORCE, (tag, df)


def _cutoff_allowance(pos, q, box, beta, rc, excl):
    """Per atom, the size of the real-space force of its pairs that lie so close to the cutoff that fp32 may count them on
    the other side: |r - rc| below 8 fp32 ulps of the largest coordinate (distances are formed from coordinates in the
    kernels).  Such a pair changes the fp32 force by its whole force at the cutoff, ~1e-2 kcal/mol/A for O-O — observed
    on water291 shifted by whole boxes, where one O-H pair lies 4.8e-6 A inside the cutoff in fp64 and 4.5e-6 A outside
    in fp32."""
    from scipy.spatial import cKDTree

    pos = np.asarray(pos, np.float64)
    delta = 8 * 2.0**-24 * max(np.abs(pos).max(), np.max(box))
    w = pos - box * np.floor(pos / box)
    w[w >= box] = 0.0
    allow = np.zeros(len(pos))
    pairs = cKDTree(w, boxsize=box).query_pairs(rc + delta, output_type="ndarray")
    if len(pairs) == 0:
        return allow
    i, j = np.minimum(pairs[:, 0], pairs[:, 1]), np.maximum(pairs[:, 0], pairs[:, 1])
    r = np.linalg.norm(E._min_image(pos[i] - pos[j], box), axis=1)
    keep = np.abs(r - rc) < delta
    ex = {tuple(sorted(e)) for e in excl}
    keep &= np.array([(a, b) not in ex for a, b in zip(i, j)], dtype=bool)
    i, j = i[keep], j[keep]
    fc = np.abs(E.KE * q[i] * q[j]) * (E.erfc(beta * rc) / rc**2 + 2 * beta / np.sqrt(np.pi) * np.exp(-(beta * rc) ** 2) / rc)
    np.add.at(allow, i, fc)
    np.add.at(allow, j, fc)
    return allow


def _check32(tag, e32, f32, e64, f64, q, box, beta, term="electrostatics", allow=None):
    """`allow`: per-atom force allowance of pairs at the cutoff (_cutoff_allowance), on top of the bound."""
    scale = max(abs(e64[term]), abs(E.self_and_background(q, box, beta)))
    err = np.abs(f32 - f64).max(axis=-1)
    allow = np.zeros(err.shape[-1]) if allow is None else allow
    de, df = abs(e32[term] - e64[term]) / scale, err.max()
    dfx = (err - allow).max()
    _report(tag + " fp32-fp64", dE_rel=de, dF=df, dF_beyond_cutoff_pairs=dfx, atoms_at_cutoff=float((allow > 0).sum()))
    assert de <= F32_ENERGY, (tag, de)
    assert dfx <= F32_FORCE, (tag, df, dfx)


def _both(tag, make_par, pos, q, box, rc, excl, terms=("electrostatics",), host_forces_offset=None, **kw):
    """fp64 GPU against the host PME and fp32 against fp64 on one input; returns the fp64 context, energies and forces."""
    terms = list(terms)
    fo, e64, f64 = _compute(make_par(torch.float64), pos, box, torch.float64, terms, twice=True, cutoff=rc, pme=True, **kw)
    _, e32, f32 = _compute(make_par(torch.float32), pos, box, torch.float32, terms, twice=True, cutoff=rc, pme=True, **kw)
    beta = fo.ewald_beta
    eh, fh = _host(pos, q, box, beta, rc, fo.pme_grid, fo.pme_order, excl)
    off = 0.0 if host_forces_offset is None else host_forces_offset
    _check64(tag, e64[0], f64[0] - off, eh, fh, q, box, beta)
    _check32(tag, e32[0], f32[0], e64[0], f64[0], q, box, beta, allow=_cutoff_allowance(pos, q, box, beta, rc, excl))
    return fo, e64, f64


def _par_of(system, **kw):
    return lambda dtype: system(dtype, **kw)[0]


def _small_ions(dtype=torch.float64):
    box = np.array([14.0, 15.0, 16.0])
    pos, q = E.random_ions(40, box, seed=8, min_dist=2.0)
    return _atomic_par(q, dtype), pos, q, box, ["electrostatics"], 6.9, []


SYSTEMS = {"ions": _ions, "water291": _water, "tip3p16": _tip3p}
GRIDS = {"odd_kz": (27, 30, 25), "primes": (31, 53, 97), "aniso": (16, 40, 97)}


# ---- spline order x grid ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", [4, 5, 6])
@pytest.mark.parametrize("name", list(SYSTEMS))
@pytest.mark.parametrize("grid", ["rule"] + list(GRIDS))
def test_order_and_grid(order, name, grid):
    """Orders 4, 5 and 6 on the rule's grid, a mixed grid with an odd innermost edge (the half-complex layout and the
    conjugate weight of pme_conv_kernel), prime edges up to 97 (other hipFFT paths) and a strongly anisotropic grid, on
    the all-pairs (ions, water291) and cell-list (tip3p_box(16)) real-space paths.  Observed on an MI355X over the 36 cases:
    fp64 forces <= 5.2e-13, energies <= 1.6e-8 (tip3p16, the self-term bound 2.3e-7) and <= 6.2e-11 elsewhere; fp32 forces
    <= 1.3e-4 (ions), 2.8e-5 (water291), 2.6e-4 (tip3p16), energies <= 1.6e-7 of the self term."""
    sysf = SYSTEMS[name]
    _, pos, q, box, terms, rc, excl = sysf()
    kw = {} if grid == "rule" else {"pme_grid": GRIDS[grid]}
    fo, _, _ = _both(f"{name} order {order} grid {grid}", _par_of(sysf), pos, q, box, rc, excl, pme_order=order, **kw)
    assert fo.pme_order == order
    if grid != "rule":
        assert fo.pme_grid == GRIDS[grid]
    assert fo.stats(G.pos_tensor(pos, 1, torch.float64, DEV))["algorithm"] == ("celllist" if name == "tip3p16" else "allpairs")


@pytest.mark.parametrize("order", [4, 5, 6])
def test_smallest_grid(order):
    """K = order on every axis: every z-run of the spread kernel wraps, every atom covers the whole grid.  Observed: fp64
    forces <= 7.1e-14, energies <= 6.8e-13; fp32 forces <= 8.4e-5."""
    _, pos, q, box, _, rc, excl = _small_ions()
    fo, _, _ = _both(f"small ions K = order = {order}", _par_of(_small_ions), pos, q, box, rc, excl, pme_order=order,
                     pme_grid=(order,) * 3)
    assert fo.pme_grid == (order,) * 3


# ---- coordinates -------------------------------------------------------------------------------------------------------------
def _molecules(par, n):
    """Connected components of the bond graph (atoms without bonds are molecules of their own)."""
    parent = np.arange(n)

    def root(i):
        while parent[i] != i:
            parent[i] = parent[parent[i]]
            i = parent[i]
        return i

    if getattr(par, "bond_params", None) is not None:
        for a, b in par.bond_params["idx"].cpu().numpy():
            parent[root(a)] = root(b)
    return np.array([root(i) for i in range(n)])


@pytest.mark.parametrize("name", list(SYSTEMS))
def test_unwrapped_molecules(name):
    """Each molecule moved as a whole by random integer box vectors of up to +-3 boxes per axis, both signs: fp64 against
    the host, fp32 against fp64, and fp64 against the same system wrapped atom by atom into [0, L) (which splits molecules
    across the faces, so excluded pairs straddle the box).  Observed: fp64 forces <= 5.2e-13 against the host and
    <= 1.9e-12 against the wrapped system; fp32 forces 4.0e-4 (ions), 3.3e-3 (tip3p16), and 1.1e-2 on water291, all of it
    on one O-H pair 4.8e-6 A inside the cutoff that fp32 puts outside (_cutoff_allowance); 2.6e-4 on the other atoms."""
    sysf = SYSTEMS[name]
    par, pos, q, box, terms, rc, excl = sysf()
    mol = _molecules(par, len(pos))
    rng = np.random.default_rng(17)
    _, inv = np.unique(mol, return_inverse=True)
    shift = rng.integers(-3, 4, size=(inv.max() + 1, 3))
    upos = pos + shift[inv] * box
    assert (upos < 0).any() and (upos > 2 * box).any()
    wpos = upos - box * np.floor(upos / box)
    fo, e64, f64 = _both(f"{name} unwrapped", _par_of(sysf), upos, q, box, rc, excl)
    _, ew, fw = _compute(par, wpos, box, torch.float64, terms, cutoff=rc, pme=True)
    eself = abs(E.self_and_background(q, box, fo.ewald_beta))
    de, df = abs(e64[0]["electrostatics"] - ew[0]["electrostatics"]), np.abs(f64 - fw).max()
    _report(f"{name} unwrapped vs wrapped fp64", dE=de, dF=df)
    eh = ew[0]["electrostatics"]
    assert de <= (F64_ENERGY * abs(eh) if abs(eh) > 1e-2 * eself else F64_ENERGY_SELF * eself)
    assert df <= F64_FORCE


def _edge_values(L, K):
    """Coordinates on grid planes k L / K, on the faces 0 and L, just below 0 (-1e-7 L; -1e-9 L, where fp32 rounds the
    fractional coordinate up to 1) and just below L (L (1 - 2^-24)) — all fp32 numbers, so both precisions see them."""
    f = np.float32
    L = f(L)
    vals = [f(k) * L / f(K) for k in (1, 2, K // 3, K // 2, K - 1)]
    vals += [f(0), L, -f(1e-7) * L, -f(1e-9) * L, L * (f(1) - f(2.0**-24))]
    return [float(v) for v in vals]


@pytest.mark.parametrize("name", ["ions", "tip3p16"])
def test_atoms_on_grid_planes_and_faces(name):
    """Per axis and edge value, the molecule whose first atom lies nearest to it (minimum image) is moved as a whole so
    that this atom sits exactly on the value.  The box is an fp32 number.  fp64 against the host, fp32 against fp64.
    x = L found a bug: frac_coord's s - floor(s) was contracted to fma(x, invL, -floor(x invL)), negative when x invL
    rounds up to 1 (L = 30 or 31 in fp64), and the atom was spread one grid spacing away (energy off by 23 kcal/mol,
    forces by 5.8).  Observed since: fp64 forces <= 2.6e-13; fp32 forces <= 1.5e-3."""
    from torchmd_amd.forces import pme_grid_size

    sysf = SYSTEMS[name]
    par, pos, q, box, terms, rc, excl = sysf()
    box = box.astype(np.float32).astype(np.float64)
    beta = E.ewald_beta(rc, 5e-4)
    grid = tuple(pme_grid_size(beta, float(box[d]), 5e-4) for d in range(3))
    mol = _molecules(par, len(pos))
    first = np.array([np.flatnonzero(mol == m)[0] for m in np.unique(mol)])
    pos = pos.copy()
    used = set()
    for d in range(3):
        for v in _edge_values(box[d], grid[d]):
            dist = np.abs(E._min_image(pos[first, d] - v, box[d]))
            dist[list(used)] = np.inf
            k = int(np.argmin(dist))
            used.add(k)
            a = first[k]
            members = mol == mol[a]
            pos[members, d] += v - pos[a, d]
            pos[a, d] = v
    pos = pos.astype(np.float32).astype(np.float64)
    fo, _, _ = _both(f"{name} on planes and faces", _par_of(sysf), pos, q, box, rc, excl, pme_grid=grid)
    assert fo.pme_grid == grid


# ---- occupancy and charges -------------------------------------------------------------------------------------------------
def _ions_at(pos, q):
    return lambda dtype: _atomic_par(q, dtype)


@pytest.mark.parametrize("order", [4, 5, 6])
def test_cluster_in_an_empty_box(order):
    """30 ions within a 7 A cube across a corner of a 30 A box: a few crowded bins (wrapped on every axis) and
    thousands of empty ones.  Observed: fp64 forces <= 1.4e-13; fp32 <= 8.9e-5."""
    box = np.array([30.0, 31.0, 32.0])
    pos, q = E.random_ions(30, np.full(3, 7.0), seed=12, min_dist=1.6)
    pos = pos - 3.5  # (the cube straddles the faces)
    _both(f"cluster order {order}", _ions_at(pos, q), pos, q, box, 9.0, [], pme_order=order)


@pytest.mark.parametrize("n", [1, 2])
def test_one_and_two_ions(n):
    """One Na+ (net charge: the background term; its force is the grid's self-force only) and an ion pair.  Observed:
    fp64 forces <= 2.5e-14; fp32 <= 4.9e-6."""
    box = np.array([20.0, 21.0, 22.0])
    pos = np.array([[3.1, 17.2, 0.4], [12.5, 2.2, 11.9]])[:n]
    q = np.array([1.0, -1.0])[:n]
    _both(f"{n} ion(s)", _ions_at(pos, q), pos, q, box, 9.0, [])


def _argon_ions(dtype):
    """40 ions and 120 uncharged argon-like atoms (LJ on all of them), with excluded pairs ion-argon, argon-argon and
    ion-ion (the `qq == 0` skip of pme_excl_kernel)."""
    box = np.array([26.0, 27.0, 28.0])
    pos, q = E.random_ions(160, box, seed=14, min_dist=2.4)
    q[40:] = 0.0
    types = np.array([0] * 40 + [1] * 120)
    g = {"par_charges": q, "par_masses": np.full(160, 30.0), "par_types": types,
         "par_nonbonded_params": np.array([[2.6, 0.1], [3.4, 0.238]])}
    par = G.GoldenParameters(g, precision=dtype, device=DEV)
    excl = [(0, 50), (41, 60), (2, 3), (70, 71), (5, 100)]
    par.get_exclusions = lambda types=EXCL: [list(e) for e in excl]
    return par, pos, q, box, excl


def test_uncharged_atoms_mixed_with_ions():
    """['lj', 'electrostatics']: the electrostatics energy against the host, the forces minus those of an LJ-only context
    against the host's electrostatic forces.  Observed: fp64 6.4e-14; fp32 (LJ included) 7.8e-4."""
    par, pos, q, box, excl = _argon_ions(torch.float64)
    _, elj, flj = _compute(par, pos, box, torch.float64, ["lj"], cutoff=9.0)
    _both("argon + ions", lambda dt: _argon_ions(dt)[0], pos, q, box, 9.0, excl, terms=("lj", "electrostatics"),
          host_forces_offset=flj[0])


@pytest.mark.parametrize("system", ["tip3p8", "ala2"])
@pytest.mark.parametrize("exclusions", [("bonds",), ("bonds", "angles"), ("bonds", "angles", "1-4")])
def test_exclusion_sets(system, exclusions):
    """Forces(exclusions=...) decides which pairs the excluded-pair correction removes: the host removes the same set.
    (TIP3P's H-H bond makes the three sets of water one set; alanine dipeptide has angles and 1-4 pairs of its own.)
    Observed: fp64 forces <= 9.3e-14; fp32 <= 8.3e-5."""
    if system == "tip3p8":
        sysf = lambda dtype=torch.float64: _tip3p(dtype, nside=8)  # noqa: E731
    else:
        from test_gpu_pme import _ala2 as sysf
    par, pos, q, box, terms, rc, _ = sysf()
    excl = [tuple(x) for x in par.get_exclusions(exclusions)]
    _both(f"{system} exclusions {exclusions}", lambda dt: sysf(dt)[0], pos, q, box, rc, excl, exclusions=exclusions)


# ---- replicas with boxes of their own ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["water291", "tip3p16"])
def test_replicas_with_distinct_boxes(name):
    """R = 3, boxes (and positions) scaled by 1.0, 1.04 and 0.97 in one `compute`: each replica against the host for its
    own box (each keeps its own influence function), the grid from the largest edge; then the boxes rotated among the
    replicas, so every influence function must be recomputed.  Observed: fp64 forces <= 2.1e-13."""
    from torchmd_amd.forces import pme_grid_size

    sysf = SYSTEMS[name]
    par, pos, q, box, terms, rc, excl = sysf()
    scales = [1.0, 1.04, 0.97]
    for rot in (0, 1):
        sc = scales[rot:] + scales[:rot]
        p = np.stack([pos * s for s in sc])
        boxes = [box * s for s in sc]
        bt = torch.zeros(3, 3, 3, dtype=torch.float64, device=DEV)
        for r in range(3):
            bt[r].diagonal().copy_(torch.as_tensor(boxes[r]))
        if rot == 0:
            from torchmd_amd.forces import Forces

            fo = Forces(par, terms=terms, cutoff=rc, pme=True)
        pt = torch.as_tensor(p, device=DEV).contiguous()
        f = torch.zeros_like(pt)
        e = fo.compute(pt, bt, f, returnDetails=True)
        assert fo.pme_grid == tuple(pme_grid_size(fo.ewald_beta, 1.04 * box[d], 5e-4) for d in range(3))
        assert fo.stats(pt)["algorithm"] == ("celllist" if name == "tip3p16" else "allpairs")
        for r in range(3):
            eh, fh = _host(p[r], q, boxes[r], fo.ewald_beta, rc, fo.pme_grid, 5, excl)
            _check64(f"{name} replica {r} scale {sc[r]}", e[r], f[r].cpu().numpy(), eh, fh, q, boxes[r], fo.ewald_beta)


# ---- size --------------------------------------------------------------------------------------------------------------------
def test_c3_water_box():
    """tip3p_box(32): 98 304 atoms, cutoff 9, the default tolerance -> a 90^3 grid and 20-bit sort keys.  fp64 against the
    full host PME; fp32 against the host with the fp32 bounds.  Observed: fp64 forces 3.6e-13, energy 7.4e-7 (the total,
    -958 kcal/mol, is left of parts of 1.9e6: the bound is 1e-12 of the self term, 1.9e-6); fp32 energy 1.5e-7 of the
    self term, forces 6.3e-3 on atoms of the 855 with a pair within 8 fp32 ulps of the cutoff (_cutoff_allowance), less
    5.8e-4 on all others."""
    par64, pos, q, box, terms, rc, excl = _tip3p(nside=32)
    fo, e64, f64 = _compute(par64, pos, box, torch.float64, terms, cutoff=rc, pme=True)
    assert fo.pme_grid == (90, 90, 90)
    assert fo.stats(G.pos_tensor(pos, 1, torch.float64, DEV))["algorithm"] == "celllist"
    eh, fh = _host(pos, q, box, fo.ewald_beta, rc, fo.pme_grid, 5, excl)
    _check64("C3 tip3p_box(32)", e64[0], f64[0], eh, fh, q, box, fo.ewald_beta)
    del par64
    par32 = _tip3p(torch.float32, nside=32)[0]
    _, e32, f32 = _compute(par32, pos, box, torch.float32, terms, cutoff=rc, pme=True)
    _check32("C3 tip3p_box(32) vs host", e32[0], f32[0], {"electrostatics": eh}, fh, q, box, fo.ewald_beta,
             allow=_cutoff_allowance(pos, q, box, fo.ewald_beta, rc, excl))


# ---- MD paths ------------------------------------------------------------------------------------------------------------
def test_fp32_md_run_equals_stepwise_loop(monkeypatch):
    """fp32, cell list, one replica, Langevin: tmdhip_md_run with PME reproduces the Integrator's step-by-step Python loop
    (first_vv -> compute -> langevin_second_vv) bit for bit (the pattern of test_fused_md_run_equals_stepwise_loop).
    The loop's `compute` calls keep a list of their own, so they also run the evaluation paths of a context that has one."""
    monkeypatch.setenv("TMDHIP_VSKIN", "0")
    from torchmd_amd.builders import tip3p_box, water_forcefield
    from torchmd_amd.forces import Forces
    from torchmd_amd.integrator import Integrator, maxwell_boltzmann
    from torchmd_amd.parameters import Parameters
    from torchmd_amd.systems import System

    class ZeroExternal:  # forces the Integrator onto its generic Python loop
        def calculate(self, pos, box):
            return torch.zeros(pos.shape[0], device=pos.device), torch.zeros_like(pos)

    dt = torch.float32
    mol, pos, box = tip3p_box(12, seed=21)
    terms = ["lj", "electrostatics", "bonds", "angles"]
    par = Parameters(water_forcefield(mol), mol, terms, precision=dt)
    torch.manual_seed(5)
    vel0 = maxwell_boltzmann(par.masses, 300, 1)
    out = []
    for ext in (None, ZeroExternal()):
        s = System(mol.numAtoms, 1, dt, DEV)
        s.set_positions(pos[:, :, None])
        s.set_box(box)
        s.set_velocities(vel0)
        f = Forces(par, terms=terms, cutoff=9.0, pme=True, external=ext)
        f.compute(s.pos, s.box, s.forces)
        torch.manual_seed(77)
        integ = Integrator(s, f, 1.0, DEV, gamma=1.0, T=300.0)
        res = [integ.step(7), integ.step(1), integ.step(12)]
        st = f.stats(s.pos)
        assert st["algorithm"] == "celllist" and st["n_rebuilds"] >= 2 and st["pme_evaluations"] >= 20
        out.append((s.pos.cpu(), s.vel.cpu(), s.forces.cpu(), res))
    (p0, v0, f0, r0), (p1, v1, f1, r1) = out
    _report("fp32 md_run vs stepwise loop", dpos=(p0 - p1).abs().max().item(), dvel=(v0 - v1).abs().max().item(),
            dF=(f0 - f1).abs().max().item())
    assert torch.equal(p0, p1) and torch.equal(v0, v1) and torch.equal(f0, f1)
    for a, b in zip(r0, r1):
        assert np.allclose(a[0], b[0], rtol=1e-12) and np.allclose(a[1], b[1], rtol=1e-12)


def test_integrator_equals_python_loop_celllist_two_replicas():
    """fp64 cell list with R = 2: the per-replica list branch of md_run and its pme_hook."""
    par, pos, q, box, _, rc, _ = _tip3p(nside=16)
    fo, system = _integrator_against_loop(par, pos, box, rc, 2, 1.0)
    assert fo.stats(system.pos)["algorithm"] == "celllist"
    assert fo.stats(system.pos)["n_rebuilds"] > 1


def test_list_overflow_is_replayed_with_pme(monkeypatch):
    """test_list_overflow_is_replayed_not_raised with PME: a list that overflows in the middle of a step() batch is
    replayed from the batch's entry state, and the final forces equal those of a fresh PME evaluation."""
    from torchmd_amd.builders import tip3p_box, water_forcefield
    from torchmd_amd.forces import Forces
    from torchmd_amd.integrator import Integrator, maxwell_boltzmann
    from torchmd_amd.parameters import Parameters
    from torchmd_amd.systems import System

    dt = torch.float32
    mol, pos, box = tip3p_box(14, seed=4)
    com = pos.reshape(-1, 3, 3).mean(axis=1, keepdims=True)
    pos = (pos.reshape(-1, 3, 3) + 0.15 * com).reshape(-1, 3)
    box = box * 1.15
    terms = ["lj", "electrostatics", "bonds", "angles"]
    par = Parameters(water_forcefield(mol), mol, terms, precision=dt)
    monkeypatch.setenv("TMDHIP_LPA", "8")

    def run(tight):
        if tight:
            monkeypatch.setenv("TMDHIP_DEBUG_LIST_SLACK", "0")
        else:
            monkeypatch.delenv("TMDHIP_DEBUG_LIST_SLACK", raising=False)
        s = System(mol.numAtoms, 1, dt, DEV)
        s.set_positions(pos[:, :, None])
        s.set_box(box)
        torch.manual_seed(5)
        s.set_velocities(maxwell_boltzmann(par.masses, 300.0, 1))
        f = Forces(par, terms=terms, cutoff=9.0, pme=True, algorithm="celllist")
        f.compute(s.pos, s.box, s.forces)
        cap0 = f.stats(s.pos)["max_neighbours"]
        torch.manual_seed(6)
        out = Integrator(s, f, 1.0, DEV, gamma=1.0, T=300.0).step(400)
        st = f.stats(s.pos)
        fresh = Forces(par, terms=terms, cutoff=9.0, pme=True, algorithm="celllist")
        F2 = torch.zeros_like(s.pos)
        fresh.compute(s.pos, s.box, F2)
        return out, cap0, st, (F2 - s.forces).abs().max().item()

    monkeypatch.delenv("TMDHIP_DEBUG_LIST_SLACK", raising=False)
    out_ref, cap_ref, st_ref, ferr_ref = run(False)
    out_t, cap_t, st_t, ferr_t = run(True)
    assert cap_t < cap_ref and st_t["max_neighbours"] > cap_t, (cap_t, cap_ref, st_t)
    assert st_t["overflow"] == 0 and st_ref["overflow"] == 0
    _report("PME list overflow replay: final forces vs a fresh evaluation", dF_tight=ferr_t, dF_ample=ferr_ref)
    assert ferr_t < 6e-4 and ferr_ref < 6e-4
    assert abs(out_t[2][0] - out_ref[2][0]) < 15.0
    assert abs(out_t[1][0] - out_ref[1][0]) < 0.01 * abs(out_ref[1][0])


def test_wrong_continuation_hint_is_rewound_with_pme(monkeypatch):
    """test_wrong_continuation_hint_is_rewound with PME: positions changed behind torch's version counter cost a rewind,
    and the final forces equal those of a fresh PME evaluation."""
    from torchmd_amd.builders import tip3p_box, water_forcefield
    from torchmd_amd.forces import Forces
    from torchmd_amd.integrator import Integrator, maxwell_boltzmann
    from torchmd_amd.parameters import Parameters
    from torchmd_amd.systems import System

    dt = torch.float32
    monkeypatch.setenv("TMDHIP_DEBUG_CHAIN_MIN_ENTRIES", "1")
    mol, pos, box = tip3p_box(14, seed=6)
    terms = ["lj", "electrostatics", "bonds", "angles"]
    par = Parameters(water_forcefield(mol), mol, terms, precision=dt)
    s = System(mol.numAtoms, 1, dt, DEV)
    s.set_positions(pos[:, :, None])
    s.set_box(box)
    torch.manual_seed(3)
    s.set_velocities(maxwell_boltzmann(par.masses, 300.0, 1))
    f = Forces(par, terms=terms, cutoff=9.0, pme=True, algorithm="celllist")
    f.compute(s.pos, s.box, s.forces)
    torch.manual_seed(9)
    integ = Integrator(s, f, 1.0, DEV, gamma=1.0, T=300.0)
    integ.step(12)
    integ.step(12)
    before = f.stats(s.pos)["chains_skipped"]
    for _ in range(6):
        integ.step(1)
    assert f.stats(s.pos)["chains_skipped"] > before
    skipped0 = f.stats(s.pos)["chains_skipped"]
    version = s.pos._version
    ox = s.pos[0, 0::3, 0]
    moved = (ox - torch.floor(ox / float(box[0])) * float(box[0])) > 0.5 * float(box[0])
    shift = torch.zeros_like(s.pos)
    shift[0, :, 1] = 0.9 * moved.repeat_interleave(3).to(dt)
    s.pos.data.add_(shift)
    assert s.pos._version == version
    integ.step(8)
    st = f.stats(s.pos)
    assert st["overflow"] == 0 and st["chains_skipped"] > skipped0
    fresh = Forces(par, terms=terms, cutoff=9.0, pme=True, algorithm="celllist")
    F2 = torch.zeros_like(s.pos)
    fresh.compute(s.pos, s.box, F2)
    err = (F2 - s.forces).abs().max().item()
    _report("PME wrong continuation hint: final forces vs a fresh evaluation", dF=err)
    assert torch.isfinite(s.forces).all()
    assert err < 2e-3


def test_side_stream_equals_the_default_stream_with_pme():
    """PME runs its hipcub sort and hipFFT plans on the caller's stream: a context created and used on a side stream
    gives the default stream's fp32 cell-list forces and Langevin trajectory bit for bit, and an fp64 all-pairs evaluation
    to the bounds of test_side_stream_equals_the_default_stream (energies are folded with fp64 atomics, and so are the
    all-pairs forces)."""
    from torchmd_amd.builders import tip3p_box, water_forcefield
    from torchmd_amd.forces import Forces
    from torchmd_amd.integrator import Integrator, maxwell_boltzmann
    from torchmd_amd.parameters import Parameters
    from torchmd_amd.systems import System

    dt = torch.float32
    mol, pos, box = tip3p_box(14, seed=2)
    terms = ["lj", "electrostatics", "bonds", "angles"]
    par = Parameters(water_forcefield(mol), mol, terms, precision=dt)
    torch.manual_seed(1)
    vel0 = maxwell_boltzmann(par.masses, 300.0, 1)
    wpar, wpos, _, wbox, _, wrc, _ = _water()

    def run():
        s = System(mol.numAtoms, 1, dt, DEV)
        s.set_positions(pos[:, :, None])
        s.set_box(box)
        s.set_velocities(vel0)
        f = Forces(par, terms=terms, cutoff=9.0, pme=True, algorithm="celllist")
        e0 = f.compute(s.pos, s.box, s.forces, returnDetails=True)
        F0 = s.forces.clone()
        torch.manual_seed(9)
        res = Integrator(s, f, 1.0, DEV, gamma=1.0, T=300.0).step(30)
        fw = Forces(wpar, terms=terms, cutoff=wrc, pme=True, algorithm="allpairs")
        pw = G.pos_tensor(wpos, 1, torch.float64, DEV)
        Fw = torch.zeros_like(pw)
        ew = fw.compute(pw, _box_t(wbox, 1, torch.float64), Fw, returnDetails=True)
        torch.cuda.current_stream(DEV).synchronize()
        out = (e0[0], F0.cpu(), s.pos.cpu(), s.forces.cpu(), res, ew[0], Fw.cpu())
        f.close()
        fw.close()
        return out

    a = run()
    side = torch.cuda.Stream(DEV)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        b = run()
    torch.cuda.synchronize()
    assert torch.equal(a[1], b[1]) and torch.equal(a[2], b[2]) and torch.equal(a[3], b[3])
    for k in a[0]:
        assert abs(a[0][k] - b[0][k]) <= 1e-12 * max(1.0, abs(a[0][k])), k
    for x, y in zip(a[4], b[4]):
        assert np.allclose(np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64), rtol=1e-12, atol=0)
    for k in a[5]:
        assert abs(a[5][k] - b[5][k]) <= 1e-12 * max(1.0, abs(a[5][k])), k
    assert (a[6] - b[6]).abs().max().item() < 1e-9
