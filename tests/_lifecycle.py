"""Helpers of tests/test_gpu_lifecycle.py: one comparison rule for a context that has lived against a fresh one.

The rule, in this order (`judge`):

1. the in-cutoff pair counts are equal, exactly (and equal the oracle's where the oracle counts the same set);
2. lived and fresh are EACH held to the reference (oracle + the side terms' numpy models) at the parity bars of
   tests/test_gpu_parity.py (FTOL, ERTOL * EFAC), so that "both wrong in the same way" cannot pass;
3. `bitwise=True`: forces (and whatever rows the caller hands in as `extra`) of lived and fresh are equal bit for bit;
4. `bitwise=False` (the caller's docstring says which state legitimately differs): max|lived - fresh| is at most twice the
   fresh context's own distance from the reference on that very input.  The per-term energies always go by rule 4: every
   kernel folds its fp64 energy partials into the energy row with atomic adds, whose order is free from run to run
   (tests/test_gpu_parity.py::test_padded_list_rows_are_bit_identical has seen the last bit move).

Everything here works on host tensors and plain numbers, so tests/test_lifecycle_host.py can run the rule on fakes."""

from __future__ import annotations

import math
from dataclasses import dataclass, field

import numpy as np
import torch

from test_gpu_parity import EFAC, ERTOL, FTOL  # the parity bars, not restated (as tests/test_gpu_passive_atoms.py takes them)

DEFAULT_SKIN = 1.2  # the library's default Verlet skin (engine.h); with TMDHIP_VSKIN=0 the list radius is cutoff + skin


def planned_cells(box, rlist, natoms):
    """Cells per axis that grid_plan.h plans for a periodic `box` [3] (no TMDHIP_STENCIL), or None where it plans none and
    an AUTO context falls back to all pairs."""
    box = [float(v) for v in box]
    if not all(v > 0 for v in box):
        return None
    for m in (2, 1):
        nc = [max(int(math.floor(v / (rlist / m))), 1) for v in box]
        if any(n < 2 * m + 1 for n in nc):
            continue
        nc = [min(n, 1024) for n in nc]
        if m == 2 and natoms / float(nc[0] * nc[1] * nc[2]) < 4.0 and all(int(math.floor(v / rlist)) >= 3 for v in box):
            continue
        return tuple(nc)
    return None


@dataclass
class Result:
    """What one context answered on one input: host tensors and plain numbers."""

    npairs: list                    # in-cutoff pairs per replica (count_pairs), or None
    energies: list                  # one {term: float} per replica (compute(returnDetails=True)), or None
    forces: torch.Tensor            # [R, N, 3] of compute(returnDetails=True)
    forces_only: torch.Tensor = None  # [R, N, 3] of the forces-only evaluation, or None
    extra: dict = field(default_factory=dict)  # name -> tensor: further rows that must agree (positions, velocities, side rows)


def stack(results):
    """Single-replica results of separate contexts as one result of R replicas."""
    cat = lambda ts: None if any(t is None for t in ts) else torch.cat(list(ts), dim=0)  # noqa: E731
    return Result(
        npairs=None if any(r.npairs is None for r in results) else [n for r in results for n in r.npairs],
        energies=None if any(r.energies is None for r in results) else [e for r in results for e in r.energies],
        forces=cat([r.forces for r in results]),
        forces_only=cat([r.forces_only for r in results]),
        extra={k: cat([r.extra[k] for r in results]) for k in results[0].extra},
    )


def force_distance(got, ref, rows=None):
    """max |got - ref| over the rows the reference speaks about, in double; NaN anywhere counts as infinite."""
    a, b = got.double(), ref.double()
    if rows is not None:
        a, b = a[:, rows], b[:, rows]
    d = (a - b).abs()
    return float("inf") if not bool(torch.isfinite(d).all()) else float(d.max()) if d.numel() else 0.0


def energy_distance(got, ref, terms):
    """max over replicas and terms of |got - ref| / max(1, |ref|)."""
    worst = 0.0
    for g, r in zip(got, ref):
        for t in terms:
            d = abs(g[t] - r[t]) / max(1.0, abs(r[t]))
            worst = max(worst, d if math.isfinite(d) else float("inf"))
    return worst


def judge(label, lived, fresh, ref, prec, terms, bitwise, rows=None, count_ref=True, ftol=None):
    """The comparison rule (module docstring).  `ref`: a Result holding the reference's pair count, energies and forces
    (`forces_only` unused); `rows`: the atoms the reference's forces speak about (None: all); `count_ref`: the reference's
    pair count is of the same pair set as the contexts'; `ftol`: the force bar of rule 2 where the reference has a bar of its
    own (PME in fp32: tests/test_gpu_pme.py), else FTOL.  The `extra` rows: bit for bit with `bitwise`; without it the ones
    named "forces..." are forces of the same input and go by rules 2 and 4 like the others, and any other row is an error
    (positions and velocities of a trajectory have no reference here: `rule4`).  Prints every distance before it asserts
    and returns them."""
    out = {}
    ftol = FTOL[prec] if ftol is None else ftol
    more = [k for k in lived.extra if k.startswith("forces")]
    assert bitwise or len(more) == len(lived.extra), (label, "rows that are bitwise-only in a rule-4 comparison", list(lived.extra))
    # 1. pair counts
    if lived.npairs is not None:
        assert lived.npairs == fresh.npairs, (label, "pair count", lived.npairs, fresh.npairs)
        if count_ref and ref.npairs is not None:
            assert fresh.npairs == list(ref.npairs), (label, "pair count against the reference", fresh.npairs, ref.npairs)
    # 2. each against the reference
    for name, res in (("lived", lived), ("fresh", fresh)):
        for kind in ("forces", "forces_only"):
            F = getattr(res, kind)
            if F is not None:
                out[f"{name}_{kind}"] = force_distance(F, ref.forces, rows)
        for k in more:
            out[f"{name}_{k}"] = force_distance(res.extra[k], ref.forces, rows)
        if res.energies is not None:
            out[f"{name}_energy"] = energy_distance(res.energies, ref.energies, terms)
    # 3. / 4. lived against fresh
    for kind in ("forces", "forces_only"):
        if getattr(lived, kind) is not None:
            out[f"diff_{kind}"] = force_distance(getattr(lived, kind), getattr(fresh, kind))
    if lived.energies is not None:
        out["diff_energy"] = energy_distance(lived.energies, fresh.energies, terms)
    print(f"{label} [{prec}, {'bitwise' if bitwise else 'rule 4'}]: " + ", ".join(f"{k} = {v:.3e}" for k, v in out.items()))
    for k, v in out.items():
        if k.endswith("_energy") and not k.startswith("diff"):
            assert v <= ERTOL[prec] * EFAC, (label, k, v)
        elif not k.startswith("diff"):
            assert v <= ftol, (label, k, v)
    for kind in ("forces", "forces_only"):
        a, b = getattr(lived, kind), getattr(fresh, kind)
        if a is None:
            continue
        if bitwise:
            assert torch.equal(a, b), (label, kind, "lived and fresh differ", out[f"diff_{kind}"])
        else:
            assert out[f"diff_{kind}"] <= 2.0 * out[f"fresh_{kind}"], (label, kind, out[f"diff_{kind}"], out[f"fresh_{kind}"])
    for k in lived.extra:
        a, b = lived.extra[k], fresh.extra[k]
        if bitwise:
            assert torch.equal(a, b), (label, k, "lived and fresh differ", force_distance(a, b))
        else:
            assert force_distance(a, b) <= 2.0 * out[f"fresh_{k}"], (label, k, force_distance(a, b), out[f"fresh_{k}"])
    if lived.energies is not None:
        assert out["diff_energy"] <= 2.0 * out["fresh_energy"], (label, "energies", out["diff_energy"], out["fresh_energy"])
    return out


def rule4(label, lived, fresh, ref):
    """Rule 4 for a single tensor (a trajectory's positions or velocities): returns (lived-fresh, fresh-reference)."""
    d, own = force_distance(lived, fresh), force_distance(fresh, ref)
    print(f"{label} [rule 4]: lived - fresh = {d:.3e}, fresh - reference = {own:.3e}")
    assert d <= 2.0 * own, (label, d, own)
    return d, own
