#!/usr/bin/env python
"""The cost of one Hamiltonian-exchange attempt on ONE GPU: `HamiltonianExchange.attempt` on the 5 184-atom TIP3P
box (fp32, cutoff 9 A, reaction field) with one water as the solute and one distance restraint, at 4 and 16 replicas (needs a
GPU).  Two kinds of attempt, each timed by the host clock between two device synchronisations:

    not moved   the cross energies of both terms (tmdhip_alchemical_states, tmdhip_restraint_states: one host synchronisation
                each) and the decision, every tried pair rejected: nothing further is launched
    moved       every tried pair accepted (u = 0): also the new assignment, its upload and one `forces.compute`

and the cross-energy calls alone.  Reported, compared with nothing.

    python tools/time_hrex.py [--rounds 5] [--attempts 50]
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from torchmd_amd.alchemy import Alchemical  # noqa: E402
from torchmd_amd.builders import tip3p_box, water_forcefield  # noqa: E402
from torchmd_amd.forces import Forces  # noqa: E402
from torchmd_amd.hrex import HamiltonianExchange  # noqa: E402
from torchmd_amd.integrator import Integrator, maxwell_boltzmann  # noqa: E402
from torchmd_amd.parameters import Parameters  # noqa: E402
from torchmd_amd.restraints import Restraints  # noqa: E402
from torchmd_amd.systems import System  # noqa: E402

TERMS = ["lj", "electrostatics", "bonds", "angles"]


class Zero:
    def random(self):
        return 0.0


def schedule(R):
    """The charges go first (lambda_elec 1 -> 0 at lambda_vdw = 1), then the spheres."""
    x = np.linspace(0.0, 2.0, R)
    return np.clip(2.0 - x, 0.0, 1.0), np.clip(1.0 - x, 0.0, 1.0)


def timed(fn, rounds, n):
    per = []
    for _ in range(rounds):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            fn()
        torch.cuda.synchronize()
        per.append((time.perf_counter() - t0) / n * 1e6)
    return [round(v, 1) for v in per], round(float(np.median(per)), 1)


def measure(R, rounds, nattempts):
    dev = torch.device("cuda:0")
    mol, pos, box = tip3p_box(12, seed=21)
    par = Parameters(water_forcefield(mol), mol, TERMS, precision=torch.float32)
    lv, le = schedule(R)
    al = Alchemical([300, 301, 302], lv, le)
    p = np.asarray(pos, dtype=np.float64)
    r = float(np.linalg.norm(p[0] - p[3]))
    rs = Restraints(R).add_distance([[0, 3]], np.array([[r + 0.1 * q] for q in range(R)]), 20.0)
    s = System(mol.numAtoms, R, torch.float32, dev)
    s.set_positions(np.repeat(p[:, :, None], R, axis=2))
    s.set_box(box)
    torch.manual_seed(1)
    s.set_velocities(maxwell_boltzmann(par.masses, 300, R))
    f = Forces(par, terms=TERMS, cutoff=9.0, rfa=True, alchemical=al, restraints=rs)
    f.compute(s.pos, s.box, s.forces)
    hx = HamiltonianExchange(frequency=100, seed=1)
    integ = Integrator(s, f, 1.0, dev, gamma=1.0, T=300.0, exchange=hx)
    integ.step(100)  # (one attempt inside a run: code objects, workspaces)
    inner = hx.decide

    def reject(M):
        states, accepted, delta, pairs, u = inner(M)
        return hx.states.copy(), np.zeros(len(pairs), dtype=bool), delta, pairs, u

    out = {"replicas": R, "natoms": int(mol.numAtoms)}
    hx.decide = reject
    for _ in range(3):
        hx.attempt(s, f)
    out["not_moved_us"], out["not_moved_us_median"] = timed(lambda: hx.attempt(s, f), rounds, nattempts)
    assert hx.accepted.sum() <= R  # (only the attempt inside the run may have accepted)
    hx.decide, hx.rng = inner, Zero()
    before = hx.accepted.sum()
    for _ in range(3):
        hx.attempt(s, f)
    out["moved_us"], out["moved_us_median"] = timed(lambda: hx.attempt(s, f), rounds, nattempts)
    assert hx.accepted.sum() - before >= (rounds * nattempts) * ((R - 1) // 2) and np.isfinite(hx.record["M"]).all()
    out["cross_energies_us"], out["cross_energies_us_median"] = timed(lambda: hx.cross_matrix(s, f), rounds, nattempts)
    out["compute_us"], out["compute_us_median"] = timed(lambda: f.compute(s.pos, s.box, s.forces), rounds, nattempts)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--attempts", type=int, default=50)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    print(json.dumps({"device": torch.cuda.get_device_name(0), "cases": [measure(R, args.rounds, args.attempts) for R in (4, 16)]}))


if __name__ == "__main__":
    main()
