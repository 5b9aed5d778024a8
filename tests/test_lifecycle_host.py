"""The comparison rule of tests/_lifecycle.py on fake tensors, and its mirror of the grid planner (no GPU needed)."""

import numpy as np
import pytest
import torch

import _lifecycle as LC
from test_gpu_parity import EFAC, ERTOL, FTOL

TERMS = ["lj", "electrostatics"]


def _result(F, e, n=(100,), only=True):
    return LC.Result(npairs=list(n), energies=[dict(zip(TERMS, e))], forces=F.clone(), forces_only=F.clone() if only else None)


def _case(prec):
    g = torch.Generator().manual_seed(1)
    ref = torch.randn(1, 50, 3, generator=g, dtype=torch.float64) * 10
    noise = torch.randn(1, 50, 3, generator=g, dtype=torch.float64)
    noise = noise / noise.abs().max()
    return ref, noise, [-300.0, 200.0]


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_bitwise_rule_passes_on_equal_tensors_and_fails_on_one_ulp(prec):
    ref, noise, e = _case(prec)
    F = ref + 0.5 * FTOL[prec] * noise
    r = _result(ref, e)
    LC.judge("equal", _result(F, e), _result(F, e), r, prec, TERMS, bitwise=True)
    G = F.clone()
    G[0, 7, 1] = np.nextafter(G[0, 7, 1].item(), np.inf)
    with pytest.raises(AssertionError, match="lived and fresh differ"):
        LC.judge("one ulp", _result(G, e), _result(F, e), r, prec, TERMS, bitwise=True)
    lived = _result(F, e)
    lived.extra["vel"], fresh = G, _result(F, e)
    fresh.extra["vel"] = F
    with pytest.raises(AssertionError, match="lived and fresh differ"):
        LC.judge("an extra row", lived, fresh, r, prec, TERMS, bitwise=True)


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_both_wrong_in_the_same_way_does_not_pass(prec):
    """Lived and fresh agree bit for bit and both miss the parity bar: rule 2 comes before rule 3."""
    ref, noise, e = _case(prec)
    F = ref + 2.0 * FTOL[prec] * noise
    with pytest.raises(AssertionError):
        LC.judge("both wrong", _result(F, e), _result(F, e), _result(ref, e), prec, TERMS, bitwise=True)
    off = [e[0] * (1 + 2 * ERTOL[prec] * EFAC), e[1]]
    with pytest.raises(AssertionError):
        LC.judge("both energies wrong", _result(ref, off), _result(ref, off), _result(ref, e), prec, TERMS, bitwise=True)


def test_pair_counts_are_exact_and_come_first():
    ref, noise, e = _case("f64")
    with pytest.raises(AssertionError, match="pair count"):
        LC.judge("count", _result(ref, e, n=(101,)), _result(ref, e), _result(ref, e), "f64", TERMS, bitwise=True)
    with pytest.raises(AssertionError, match="against the reference"):
        LC.judge("count", _result(ref, e, n=(101,)), _result(ref, e, n=(101,)), _result(ref, e), "f64", TERMS, bitwise=True)
    LC.judge("count", _result(ref, e, n=(101,)), _result(ref, e, n=(101,)), _result(ref, e), "f64", TERMS, bitwise=True, count_ref=False)


def test_rule_four_is_twice_the_fresh_distance_from_the_reference_never_from_the_lived():
    ref, noise, e = _case("f32")
    d = 0.1 * FTOL["f32"]
    fresh = ref + d * noise  # max distance d from the reference
    ok, bad = fresh - 1.9 * d * noise, fresh - 2.1 * d * noise  # 1.9 d and 2.1 d from fresh (0.9 d and 1.1 d from the reference)
    r = _result(ref, e)
    out = LC.judge("rule 4", _result(ok, e), _result(fresh, e), r, "f32", TERMS, bitwise=False)
    assert abs(out["fresh_forces"] - d) < 1e-12 and abs(out["diff_forces"] - 1.9 * d) < 1e-12
    with pytest.raises(AssertionError):
        LC.judge("rule 4", _result(bad, e), _result(fresh, e), r, "f32", TERMS, bitwise=False)
    # a lived context far from the reference does not widen its own bar
    with pytest.raises(AssertionError):
        LC.judge("rule 4", _result(ref + 0.9 * FTOL["f32"] * noise, e), _result(ref, e), r, "f32", TERMS, bitwise=False)
    # energies go by rule 4 also where forces are bitwise
    ef = [e[0] * (1 + 1e-6), e[1]]
    LC.judge("energies", _result(ref, [e[0] * (1 + 2.5e-6), e[1]]), _result(ref, ef), r, "f32", TERMS, bitwise=True)
    with pytest.raises(AssertionError, match="energies"):
        LC.judge("energies", _result(ref, [e[0] * (1 - 1.5e-6), e[1]]), _result(ref, ef), r, "f32", TERMS, bitwise=True)
    with pytest.raises(AssertionError):
        LC.rule4("tensor", bad, fresh, ref)
    assert LC.rule4("tensor", ok, fresh, ref)[1] == pytest.approx(d)


def test_extra_rows_without_the_bitwise_rule_and_a_bar_of_the_reference_s_own():
    ref, noise, e = _case("f32")
    d = 0.1 * FTOL["f32"]
    r = _result(ref, e)

    def with_extra(F, X, name="forces_second_compute"):
        out = _result(F, e)
        out.extra[name] = X
        return out

    fresh = ref + d * noise
    LC.judge("extra by rule 4", with_extra(fresh, fresh - 1.9 * d * noise), with_extra(fresh, fresh), r, "f32", TERMS, bitwise=False)
    with pytest.raises(AssertionError):  # ... twice the fresh extra's distance from the reference, no more
        LC.judge("extra by rule 4", with_extra(fresh, fresh - 2.1 * d * noise), with_extra(fresh, fresh), r, "f32", TERMS, bitwise=False)
    with pytest.raises(AssertionError):  # ... and each extra within the parity bar of the reference (rule 2)
        LC.judge("extra by rule 2", with_extra(fresh, ref + 2 * FTOL["f32"] * noise), with_extra(fresh, ref + 2 * FTOL["f32"] * noise), r, "f32",
                 TERMS, bitwise=False)
    with pytest.raises(AssertionError, match="bitwise-only"):  # a trajectory's rows have no reference here
        LC.judge("pos", with_extra(fresh, fresh, "pos"), with_extra(fresh, fresh, "pos"), r, "f32", TERMS, bitwise=False)
    # a reference with a bar of its own (PME in fp32)
    far = ref + 10 * FTOL["f32"] * noise
    with pytest.raises(AssertionError):
        LC.judge("ftol", _result(far, e), _result(far, e), r, "f32", TERMS, bitwise=True)
    LC.judge("ftol", _result(far, e), _result(far, e), r, "f32", TERMS, bitwise=True, ftol=5e-3)


def test_rows_nobody_wrote_and_rows_the_reference_is_silent_about():
    ref, noise, e = _case("f64")
    F = ref.clone()
    F[0, 40:] = 0.0  # passive rows: the reference speaks about the first 40
    r = _result(ref, e)
    LC.judge("rows", _result(F, e), _result(F, e), r, "f64", TERMS, bitwise=True, rows=slice(0, 40))
    with pytest.raises(AssertionError):
        LC.judge("rows", _result(F, e), _result(F, e), r, "f64", TERMS, bitwise=True)
    G = F.clone()
    G[0, 3, 0] = float("nan")  # a row of the NaN-filled buffer that no kernel wrote
    assert LC.force_distance(G, ref, slice(0, 40)) == float("inf")
    with pytest.raises(AssertionError):
        LC.judge("nan", _result(G, e), _result(G, e), r, "f64", TERMS, bitwise=True, rows=slice(0, 40))


def test_stack_concatenates_single_replica_results():
    ref, noise, e = _case("f64")
    a, b = _result(ref, e, n=(5,)), _result(ref + 1, [1.0, 2.0], n=(6,))
    a.extra["pos"], b.extra["pos"] = ref, ref + 2
    s = LC.stack([a, b])
    assert s.npairs == [5, 6] and s.forces.shape == (2, 50, 3) and torch.equal(s.forces[1:], ref + 1)
    assert s.energies[1]["lj"] == 1.0 and torch.equal(s.extra["pos"][1:], ref + 2) and torch.equal(s.forces_only, s.forces)
    assert LC.stack([_result(ref, e), _result(ref, e, only=False)]).forces_only is None


def test_planned_cells_mirrors_the_grid_planner():
    """Values the suite already pins: the 5 184-atom water at cutoff 9 A has 7 cells per edge, the 2 187-atom one
    at cutoff 10.5 A has no grid (test_auto_falls_back_to_allpairs_in_small_boxes), liquid argon coarsens to half-width 1."""
    from torchmd_amd.builders import lj_box, tip3p_box

    _, _, b12 = tip3p_box(12, seed=3)
    _, _, b9 = tip3p_box(9, seed=8)
    assert LC.planned_cells(b12, 9.0 + LC.DEFAULT_SKIN, 5184) == (7, 7, 7)
    assert LC.planned_cells(b9, 10.5 + LC.DEFAULT_SKIN, 2187) is None
    assert LC.planned_cells(b9, 8.5 + LC.DEFAULT_SKIN, 2187) == (5, 5, 5) and LC.planned_cells(b9 * 1.05, 8.5 + LC.DEFAULT_SKIN, 2187) == (6, 6, 6)
    assert LC.planned_cells(b9, 9.8 + LC.DEFAULT_SKIN, 2187) == (5, 5, 5) and LC.planned_cells(b9 * 0.97, 9.8 + LC.DEFAULT_SKIN, 2187) is None
    _, _, bl = lj_box(22, seed=2)  # 10 648 atoms, L = 79.4: half-width 2 would leave 3.1 atoms per cell
    assert LC.planned_cells(bl, 10.2, 10648) == (7, 7, 7)
    assert LC.planned_cells([0.0, 0.0, 0.0], 10.2, 100) is None
