"""The numpy model of the fixed-order sum (tests/_reduce.py) on the CPU: that it is a sum at all (against math.fsum), and that
the inputs of the GPU cases tell the two meet orders apart — the condition under which those cases pin the order."""

import math

import numpy as np
import pytest

import _reduce as M

EPS64 = float(np.finfo(np.float64).eps)


def test_butterfly_gives_every_lane_the_same_bits():
    v = np.random.default_rng(0).standard_normal((5, 64))
    out = M.butterfly(v)
    assert (out == out[:, :1]).all()
    for r in range(5):
        assert abs(out[r, 0] - math.fsum(v[r])) <= 64 * EPS64 * np.abs(v[r]).sum()
    assert (M.butterfly(v, np.fmax)[:, 0] == v.max(axis=1)).all()


@pytest.mark.parametrize("order", [M.SEQUENTIAL, M.PAIRWISE])
@pytest.mark.parametrize("N", M.SHAPES + (1, 64, 256, 65536, 70001))
def test_model_is_a_sum(N, order):
    """Block stage and fold against math.fsum of the live items: any order of n additions stays within n eps64 sum |x|."""
    rng = np.random.default_rng(N)
    x = rng.standard_normal(N) * np.exp(rng.uniform(-3, 3, N))
    live = np.arange(N) % 3 != 2
    x[~live] = np.nan  # (a skipped item is never read into the sum)
    rows = M.partial_rows(x, live, order)
    assert rows.shape == (M.nblocks_of(N),)
    n, bar = int(live.sum()), EPS64 * np.abs(x[live]).sum()
    assert abs(M.fold(rows) - math.fsum(x[live])) <= n * bar
    # every row is the sum of its block's items
    nb = len(rows)
    block = (np.arange(N) // M.THREADS) % nb
    for b in (0, nb - 1):
        mine = live & (block == b)
        assert abs(rows[b] - math.fsum(x[mine])) <= max(int(mine.sum()), 1) * bar
    # the max: any order gives the maximum
    assert M.fold(M.partial_rows(np.abs(x), live, order, np.fmax), np.fmax) == np.abs(x[live]).max()


def test_fold_takes_rows_lane_by_lane():
    rows = np.random.default_rng(3).standard_normal(130)
    lanes = np.zeros(64)
    for b, v in enumerate(rows):
        lanes[b % 64] += v
    assert M.fold(rows) == M.butterfly(lanes)[0]
    assert M.fold(np.array([-0.0])) == 0.0 and not np.signbit(M.fold(np.array([-0.0])))  # (the fold starts from +0.0)


def _rows_of_the_gpu_cases(name, prec, order):
    N = M.SHAPES[-1]
    mass, vel = M.velocities(2, N, prec, 7)
    on = mass > 0
    out = []
    for r in range(2):
        if name == "exchange":
            out.append(M.partial_rows(M.mv2(mass, vel[r]), on, order))
        elif name == "thermostat":
            out.extend(M.partial_rows(c, on, order) for c in M.thermostat_columns(mass, vel[r]))
        elif name == "fire":
            cols = M.fire_columns(vel[r], M.forces(2, N, prec, 7)[r])
            out.extend(M.partial_rows(c, on, order, op) for c, op in zip(cols, M.FIRE_OPS))
        else:
            off, natoms = M.molecule_table(N)
            m, v = M.velocities(2, natoms, prec, 7)
            out.append(M.crescale_rows(m, v[r], off, order))
    return np.concatenate(out)


@pytest.mark.parametrize("prec", ["f32", "f64"])
@pytest.mark.parametrize("name", ["exchange", "thermostat", "fire", "crescale"])
def test_the_gpu_cases_tell_the_meet_orders_apart(name, prec):
    """At the largest shape of the GPU cases the partial rows of the two orders differ (at N <= 1025 none does: the small
    shapes test the indexing, not the order)."""
    seq, pair = _rows_of_the_gpu_cases(name, prec, M.SEQUENTIAL), _rows_of_the_gpu_cases(name, prec, M.PAIRWISE)
    differ = int((seq.view(np.int64) != pair.view(np.int64)).sum())
    print(f"{name} {prec}: {differ} of {len(seq)} partial rows differ between the two meet orders")
    assert differ >= 1
