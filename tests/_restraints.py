"""Shared pieces of the restraint tests: the velocity-Verlet / Langevin step of md_step.h transcribed to numpy in
double, run once with the restraint acceleration inside `a` and once as tmdhip_md_run applies it (impulses between the force
evaluations, a finishing kick, the force buffer carrying F_r across calls), and the random systems of the kernel tests."""

import numpy as np

from torchmd_amd.restraints import Restraints

EPS64 = np.finfo(np.float64).eps


# ----------------------------------------------------------------------------- the splitting, on the host
class Toy:
    """8 particles in open space, each bound to a site of its own by a harmonic "physical" force and to its neighbour in
    the ring by a weak spring; one position restraint with a displaced reference and one distance restraint."""

    def __init__(self, seed=5):
        rng = np.random.default_rng(seed)
        self.n = 8
        self.mass = np.array([1.008, 15.999, 12.011, 1.008, 14.007, 15.999, 1.008, 32.06])
        self.site = 3.0 * rng.standard_normal((self.n, 3))
        self.x0 = self.site + 0.3 * rng.standard_normal((self.n, 3))
        self.v0 = 0.02 * rng.standard_normal((self.n, 3))
        self.noise = rng.standard_normal((64, self.n, 3))  # row = noise step
        self.rs = Restraints(1)
        self.rs.add_position([2], self.x0[2:3] + np.array([[1.0, -0.5, 0.25]]), 40.0)
        self.rs.add_distance([[0, 5]], 2.5, 60.0)
        self.box = np.zeros(3)

    def f_phys(self, x):
        f = -25.0 * (x - self.site)
        d = x - np.roll(x, -1, axis=0)
        f -= 3.0 * d
        f += 3.0 * np.roll(d, 1, axis=0)
        return f

    def f_restraint(self, x):
        return self.rs.energy_forces(x[None], self.box)[1][0]


def run_inside(toy, x, v, f, niter, step0, dt, gamma, vc):
    """One tmdhip_md_run call, a_r inside `a`: the four lines of md_step_atom per iteration (it = 0 .. niter: the second half
    of step it - 1, then the first half of step it), `f` = the total force at `x` on entry and on return."""
    m = toy.mass[:, None]
    for it in range(niter + 1):
        a = f / m
        if it > 0:
            if gamma != 0.0:
                v = v + (-gamma * v * dt + toy.noise[step0 + it - 1] * vc)
            v = v + 0.5 * dt * a
        if it < niter:
            x = x + (v * dt + 0.5 * a * dt * dt)
            v = v + 0.5 * dt * a
            f = toy.f_phys(x) + toy.f_restraint(x)
    return x, v, f


def run_impulse(toy, x, v, f, niter, step0, dt, gamma, vc, interior_kick=None):
    """The same call as tmdhip_md_run makes it with restraints: the step sees the physical force only; before the force
    evaluation of every interior step the velocities of the restrained atoms take `interior_kick` * a_r(x) (default: the
    compensated impulse dt / (1 - gamma dt)); after the loop the finishing launch adds dt/2 a_r to the velocities and F_r to
    the force buffer, so `f` is total on return as it was on entry."""
    m = toy.mass[:, None]
    kick = dt / (1.0 - gamma * dt) if interior_kick is None else interior_kick
    for it in range(niter + 1):
        a = f / m
        if it > 0:
            if gamma != 0.0:
                v = v + (-gamma * v * dt + toy.noise[step0 + it - 1] * vc)
            v = v + 0.5 * dt * a
        if it < niter:
            x = x + (v * dt + 0.5 * a * dt * dt)
            v = v + 0.5 * dt * a
            if it + 1 < niter:
                v = v + kick * toy.f_restraint(x) / m
            f = toy.f_phys(x)
    fr = toy.f_restraint(x)
    return x, v + 0.5 * dt * fr / m, f + fr


def run_cut(run, toy, cuts, dt, gamma, **kw):
    vc = np.sqrt(2.0 * gamma * 0.596 * dt / toy.mass)[:, None] if gamma != 0.0 else 0.0
    x, v = toy.x0.copy(), toy.v0.copy()
    f = toy.f_phys(x) + toy.f_restraint(x)
    step0 = 0
    for n in cuts:
        x, v, f = run(toy, x, v, f, n, step0, dt, gamma, vc, **kw)
        step0 += n
    return x, v, f


# ----------------------------------------------------------------------------- the systems of the kernel tests
def kernel_case(R=3, N=200, seed=11, L=20.0):
    """R replicas of N random atoms in a cubic box of edge L, masses in {1.008, 15.999}; 17 position and 23 distance
    restraints with distinct k and r0 per replica.  Two pairs and two references lie across a face, atom 7 is in five
    distance restraints and position-restrained, one pair is coincident, one entry of each kind has k = 0 in replica 1.
    Returns (pos [R,N,3], box [3], mass [N], Restraints)."""
    rng = np.random.default_rng(seed)
    pos = rng.uniform(0.0, L, (R, N, 3))
    mass = np.where(rng.random(N) < 0.6, 1.008, 15.999)
    rs = Restraints(R)
    patoms = np.concatenate([[7], rng.choice(np.arange(40, N), 16, replace=False)])
    ref = pos[:, patoms] + rng.normal(0.0, 0.7, (R, 17, 3))
    ref[:, 1, 0] += L          # the same point, one box further: the minimum image brings it back
    ref[:, 2, 2] -= 2.0 * L
    pos[:, patoms[3], 1] = 0.2  # an atom near a face with its reference beyond it
    ref[:, 3, 1] = L - 0.4
    kp = rng.uniform(1.0, 120.0, (R, 17))
    kp[min(1, R - 1), 5] = 0.0
    rs.add_position(patoms, ref, kp)
    pairs = [(7, 8), (9, 7), (7, 10), (11, 7), (7, 12)]  # atom 7: five distance restraints, first and second of a pair
    free = rng.permutation(np.arange(13, 40))
    pairs += [(int(free[2 * k]), int(free[2 * k + 1])) for k in range(13)]
    pairs += [(int(patoms[4]), int(patoms[5])), (int(patoms[6]), 8), (3, 1), (0, 2), (5, 4)]
    pairs = np.asarray(pairs)
    assert len(pairs) == 23
    for q, (i, j) in ((5, pairs[5]), (6, pairs[6])):  # two pairs across a face
        pos[:, i, 0], pos[:, j, 0] = 0.3, L - 0.5
    pos[:, pairs[20, 1]] = pos[:, pairs[20, 0]]  # a coincident pair: r = 0
    r0 = rng.uniform(0.5, 6.0, (R, 23))
    r0[:, 7] = 30.0  # r < r0 for certain
    kd = rng.uniform(1.0, 150.0, (R, 23))
    kd[min(1, R - 1), 9] = 0.0
    rs.add_distance(pairs, r0, kd)
    return pos, np.full(3, L), mass, rs


def big_case(N=70001, nrestrained=30000, seed=3, L=60.0):
    """One replica, N atoms, `nrestrained` restrained atoms (many blocks): 10 000 position restraints and 10 000 distance
    restraints over 20 000 other atoms."""
    rng = np.random.default_rng(seed)
    pos = rng.uniform(0.0, L, (1, N, 3))
    mass = np.where(rng.random(N) < 0.6, 1.008, 15.999)
    pick = rng.choice(N, nrestrained, replace=False)
    third = nrestrained // 3
    rs = Restraints(1)
    rs.add_position(pick[:third], pos[0, pick[:third]] + rng.normal(0.0, 0.5, (third, 3)), rng.uniform(1.0, 100.0, third))
    rs.add_distance(pick[third:].reshape(-1, 2), rng.uniform(1.0, 30.0, third), rng.uniform(1.0, 100.0, third))
    assert len(rs.atoms()) == nrestrained
    return pos, np.full(3, L), mass, rs
