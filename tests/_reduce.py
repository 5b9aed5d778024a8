"""A numpy model of the fixed-order sum of torchmd_amd/csrc/reduce.h (DESIGN, "The fixed-order sum"), addition by addition in
float64, so that a test can ask the device for the same BITS and not for a sum within a bar.

Block stage: thread t of block b takes the items b 256 + t + j nblocks 256 (j = 0, 1, ...) into an accumulator that starts at
0.0; the 64-lane xor butterfly makes one sum per wave; the four wave sums meet in one of two orders.  Fold stage: lane l of one
wave takes the rows l, l + 64, ... into an accumulator that starts at 0.0, then the butterfly.

Also the inputs of the GPU cases (tests/test_gpu_exchange.py, _thermostat.py, _fire.py, _crescale.py), so that
tests/test_reduce_host.py can check on the CPU that they tell the two meet orders apart."""

import numpy as np

THREADS, WAVE, MAX_BLOCKS = 256, 64, 256
SEQUENTIAL, PAIRWISE = "sequential", "pairwise"
NP = {"f32": np.float32, "f64": np.float64}
SHAPES = (65, 257, 16385, 65793)  # one block and a second wave with one live lane; two blocks; 65 rows; 256 rows and a second round
_LANE = np.arange(WAVE)


def butterfly(v, op=np.add):
    """v [..., 64] -> [..., 64]: v = v + v[lane ^ o] for o = 32 ... 1.  Every lane ends with the same bits."""
    v = np.asarray(v, dtype=np.float64)
    for o in (32, 16, 8, 4, 2, 1):
        v = op(v, v[..., _LANE ^ o])
    return v


def meet(p, order, op=np.add):
    """p [..., 4] wave sums -> [...] block sums."""
    if order == SEQUENTIAL:
        return op(op(op(p[..., 0], p[..., 1]), p[..., 2]), p[..., 3])
    assert order == PAIRWISE
    return op(op(p[..., 0], p[..., 1]), op(p[..., 2], p[..., 3]))


def nblocks_of(n):
    return min((n + THREADS - 1) // THREADS, MAX_BLOCKS)


def grid_stride(items, live, nblocks, op=np.add):
    """items [N], live [N] (bool: an item that is skipped does not reach the accumulator) -> lanes [nblocks, 256]."""
    items = np.asarray(items, dtype=np.float64)
    span = nblocks * THREADS
    rounds = (len(items) + span - 1) // span
    x = np.zeros(rounds * span)
    ok = np.zeros(rounds * span, dtype=bool)
    x[: len(items)], ok[: len(items)] = items, live
    acc = np.zeros(span)
    for j in range(rounds):
        sl = slice(j * span, (j + 1) * span)
        acc = np.where(ok[sl], op(acc, np.where(ok[sl], x[sl], 0.0)), acc)
    return acc.reshape(nblocks, THREADS)


def block_rows(lanes, order, op=np.add):
    """lanes [nblocks, 256] -> [nblocks]: the partial row of every block."""
    return meet(butterfly(lanes.reshape(len(lanes), THREADS // WAVE, WAVE), op)[..., 0], order, op)


def wave_rows(lanes, op=np.add):
    """lanes [nblocks, 64] of one-wave blocks -> [nblocks]."""
    return butterfly(lanes, op)[..., 0]


def fold(rows, op=np.add):
    """rows [nrows] -> the sum every lane of the folding wave holds."""
    rows = np.asarray(rows, dtype=np.float64)
    n = (len(rows) + WAVE - 1) // WAVE * WAVE
    x, ok = np.zeros(n), np.zeros(n, dtype=bool)
    x[: len(rows)], ok[: len(rows)] = rows, True
    acc = np.zeros(WAVE)
    for j in range(n // WAVE):
        sl = slice(j * WAVE, (j + 1) * WAVE)
        acc = np.where(ok[sl], op(acc, x[sl]), acc)
    return float(butterfly(acc, op)[0])


def partial_rows(items, live, order, op=np.add):
    """The whole block stage of a reduce kernel over N atoms: [nblocks] rows."""
    return block_rows(grid_stride(items, live, nblocks_of(len(items)), op), order, op)


# ----------------------------------------------------------------------------- the inputs of the GPU cases
def velocities(R, N, prec, seed):
    """test_gpu_exchange.py's `_start`: masses {1.008, 15.999, 0} in turn and velocities 0.05 N(0, 1) plus a drift, both already
    rounded to the precision (float64 arrays); every massless row holds NaNs."""
    rng = np.random.default_rng(seed)
    mass = np.array([1.008, 15.999, 0.0])[np.arange(N) % 3].astype(NP[prec]).astype(np.float64)
    vel = 0.05 * rng.standard_normal((R, N, 3)) + np.array([0.01, -0.02, 0.005])
    vel[:, mass == 0] = np.nan
    return mass, vel.astype(NP[prec]).astype(np.float64)


def forces(R, N, prec, seed):
    rng = np.random.default_rng(seed + 1000)
    return (3.0 * rng.standard_normal((R, N, 3))).astype(NP[prec]).astype(np.float64)


def mv2(mass, v):
    """exchange.hip, thermostat.hip: m * (vx*vx + vy*vy + vz*vz); crescale_mv2's m * ((vx*vx + vy*vy) + vz*vz) is the same."""
    return mass * (v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1] + v[:, 2] * v[:, 2])


def thermostat_columns(mass, v):
    """thermostat_reduce_kernel's five per-atom terms, [5][N]."""
    return np.stack([mass, mass * v[:, 0], mass * v[:, 1], mass * v[:, 2], mv2(mass, v)])


def fire_columns(v, f):
    """fire_reduce_kernel's four per-atom terms, [4][N]: |F|^2 (a max), F.v, v.v, F.F."""
    f2 = f[:, 0] * f[:, 0] + f[:, 1] * f[:, 1] + f[:, 2] * f[:, 2]
    return np.stack([f2, f[:, 0] * v[:, 0] + f[:, 1] * v[:, 1] + f[:, 2] * v[:, 2], v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1] + v[:, 2] * v[:, 2], f2])


FIRE_OPS = (np.fmax, np.add, np.add, np.add)

BIG_SIZES = (65, 130, 200)  # molecules of more than 64 atoms: one wave each
BIG_BLOCKS = 64


def molecule_table(N):
    """N molecules: the three of BIG_SIZES first, then N - 3 of one atom; atoms in table order.  Returns (offsets, natoms)."""
    sizes = np.concatenate([BIG_SIZES, np.ones(N - len(BIG_SIZES), dtype=np.int64)])
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    return off, int(off[-1])


def crescale_rows(mass, v, off, order):
    """rescale_molecules_kernel's rows of sum m v^2 for the table of `molecule_table`: ceil(nmol / 256) rows of the pass with one
    thread per molecule (a thread whose molecule is large, or massless, holds 0), then BIG_BLOCKS rows of one wave each."""
    nmol = len(off) - 1
    term = np.where(mass > 0, mv2(mass, np.where(mass[:, None] > 0, v, 0.0)), 0.0)
    small = (nmol + THREADS - 1) // THREADS
    lanes = np.zeros(small * THREADS)
    single = np.flatnonzero(np.diff(off) == 1)
    lanes[single] = term[off[single]]  # (0.0 + m v^2 of its atom)
    rows = list(block_rows(lanes.reshape(small, THREADS), order))
    for b in range(BIG_BLOCKS):
        acc = np.zeros(WAVE)
        if b < len(BIG_SIZES):
            for a in range(off[b], off[b + 1]):  # lane l takes the members first + l, first + l + 64, ...
                if mass[a] > 0:
                    acc[(a - off[b]) % WAVE] += term[a]
        rows.append(butterfly(acc)[0])
    return np.array(rows)
