"""Passive atoms (`Forces.update_atoms(par, nactive=k)`: the halo rows of a domain-decomposition brick) against the oracle.

Rows < k are active: they get a neighbour list and the complete force of every pair that touches them.  Rows >= k are
passive: they act on the active rows but get no list and a force of exactly zero; the energy counts active-active
pairs fully and active-passive pairs half (the other half belongs to the brick that owns the passive atom).  Checked
with energies (`Forces.compute` -> `tmdhip_compute`) and forces only (`tmdhip_compute_nonbonded`), in a periodic box and
in a zero box with explicit image rows, with the force buffer filled with NaN before every call, over three atom swaps
with other k and another atom order (stale per-context state).

Both calls run the separate pair kernels.  The fused fp32 evaluation of `tmdhip_compute` (compute_fused_eval, md_loop.hip)
is only taken when `bonded_inline_args` returns 1, i.e. for a context with bonded records, and `update_atoms` refuses any
context with bonded terms: an atomic context with passive rows cannot reach it.  (Its step blocks, FINAL == 2 in
md_step.h, do not write rows >= nactive; should the fused evaluation ever be opened to atomic contexts, this test is the
one that fails.)"""

import numpy as np
import pytest
import torch

from _golden import PREC
from test_gpu_parity import EFAC, ERTOL, FTOL

pytestmark = pytest.mark.gpu

CUTOFF = 9.0
KS = (1280, 2001, 333)  # (one multiple of 64, two that are not)


def _system(which, dt):
    from _oracle_sample import mixed_system
    from torchmd_amd.builders import argon_forcefield, lj_box
    from torchmd_amd.parameters import Parameters

    if which == "argon":
        mol, pos, box = lj_box(18, seed=5)  # 5 832 atoms, L = 64.9 A
        return pos, box, Parameters(argon_forcefield(mol), mol, ["lj"], precision=dt), ["lj"], {}
    _, pos, box, par, terms = mixed_system(18, dt, seed=9)  # 5 832 atoms, L = 64.8 A
    return pos, box, par, terms, {"rfa": True}


def _image_rows(pos, box, reach):
    """Wrapped positions followed by every periodic image that lies within `reach` outside the box: open boundaries with
    explicit images.  Returns (rows [M, 3], index of the original atom of every row)."""
    import itertools

    w = pos - np.floor(pos / box) * box
    rows, src = [w], [np.arange(len(w))]
    for s in itertools.product((-1, 0, 1), repeat=3):
        if s == (0, 0, 0):
            continue
        img = w + np.asarray(s) * box
        keep = ((img > -reach) & (img < box + reach)).all(axis=1)
        rows.append(img[keep])
        src.append(np.nonzero(keep)[0])
    return np.concatenate(rows), np.concatenate(src)


def _local_par(par, src, order):
    from torchmd_amd.domain import _local_parameters

    A, B = par.get_AB()
    sel = torch.as_tensor(src[order])
    return _local_parameters(par.charges[sel], par.mapped_atom_types[sel], par.masses.reshape(-1)[sel], A, B)


def _oracle(lpar, rows, box, k, terms, kw, dt):
    """Forces on the active rows (every pair touching them) and E(active-active) + 1/2 E(active-passive) per term, evaluated
    in the engine's precision `dt` (as the single-domain tests do: in fp32 the in-cutoff decision is then the engine's, pair
    for pair; an fp64 evaluation of fp32 positions can put a pair at r = 9 A on the other side)."""
    from oracle import torchmd_oracle as orc

    p = torch.as_tensor(rows).to(dt)[None]
    b = torch.diag(torch.as_tensor(box, dtype=dt))[None]
    pairs = orc.candidate_pairs(rows, box, CUTOFF + 0.6, None)
    aa = pairs[pairs[:, 1] < k]  # (i < j)
    ap = pairs[(pairs[:, 0] < k) & (pairs[:, 1] >= k)]
    e_aa, F_aa, _ = orc.compute(lpar, p, b, terms, pairs=aa, cutoff=CUTOFF, **kw)
    e_ap, F_ap, _ = orc.compute(lpar, p, b, terms, pairs=ap, cutoff=CUTOFF, **kw)
    return (F_aa + F_ap)[0, :k].double(), {t: e_aa[0][t] + 0.5 * e_ap[0][t] for t in terms}


@pytest.mark.timeout(300)
@pytest.mark.parametrize("boundary", ["periodic", "images"])
@pytest.mark.parametrize("prec", ["f32", "f64"])
@pytest.mark.parametrize("which", ["argon", "mixed"])
def test_passive_rows_get_zero_force_and_half_the_pair_energy(which, prec, boundary):
    from torchmd_amd.forces import Forces

    dev, dt = torch.device("cuda:0"), PREC[prec]
    pos, box, par, terms, kw = _system(which, dt)
    if boundary == "periodic":
        rows, src, obox = pos - np.floor(pos / box) * box, np.arange(len(pos)), box
    else:
        rows, src = _image_rows(pos, box, CUTOFF + 1.5)
        obox = np.zeros(3)
    m = len(rows)
    rows = rows.astype(np.float32 if prec == "f32" else np.float64).astype(np.float64)  # (what the engine stores)
    rng = np.random.default_rng(3)
    order = rng.permutation(m)
    f = Forces(_local_par(par, src, order), terms=terms, cutoff=CUTOFF, skin_weights=None, **kw)
    b = torch.diag(torch.as_tensor(obox, dtype=dt)).to(dev)[None].contiguous()
    f._engine(torch.empty(1, m, 3, dtype=dt, device=dev))
    report, errs = [], []
    for k in KS:
        order = rng.permutation(m)
        lpar = _local_par(par, src, order)
        f.update_atoms(lpar, nactive=k)
        r = rows[order]
        p = torch.as_tensor(r, dtype=dt, device=dev)[None].contiguous()
        Fo, Eo = _oracle(lpar, r, obox, k, terms, kw, dt)
        # energy + forces (the first call after the swap builds the list), forces only, energy again (on that list)
        for call in ("energy", "forces", "energy"):
            F = torch.full_like(p, float("nan"))
            if call == "energy":
                pots = f.compute(p, b, F, returnDetails=True)[0]
            else:
                f._evaluate(p, b, F, False, True)
            Fc = F[0].cpu()
            err = (Fc[:k].double() - Fo).abs().max().item()
            assert err < FTOL[prec], (k, call, err)
            errs.append(err)
            assert torch.equal(Fc[k:], torch.zeros_like(Fc[k:])), (k, call, "passive rows", Fc[k:].abs().nan_to_num(np.inf).max().item())
            if call == "energy":
                for t in terms:
                    rel = abs(pots[t] - Eo[t]) / max(1.0, abs(Eo[t]))
                    assert rel <= ERTOL[prec] * EFAC, (k, t, pots[t], Eo[t])
                    report.append(rel)
        assert f.stats(p)["algorithm"] == "celllist"
    print(f"{which} {prec} {boundary}: {m} rows, k = {KS}: max|dF| on the active rows {max(errs):.2e}, "
          f"energy rel. error <= {max(report):.2e}; passive rows exactly 0")
