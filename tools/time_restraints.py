#!/usr/bin/env python
"""What harmonic restraints cost an MD step on ONE GPU, fp32: microseconds per step of `Integrator.step` (NVE,
host clock around whole calls, two device synchronisations) with 0, 2 and 1 000 restrained atoms, in two settings: the
98 304-atom water box alone, and 16 replicas of the 5 184-atom box in the batched pair + step launch (needs a GPU).  The 0-atom
figure of the same session is the comparison: a `Forces` without the keyword, where no new launch is enqueued.  With restraints a
step gains one small launch (the impulse; in the batched pair + step path one for all replicas, in the replica-by-replica loop
one per replica) and a call one finishing launch + fold.

    python tools/time_restraints.py [--rounds 5] [--steps 200]
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from torchmd_amd.builders import tip3p_box, water_forcefield  # noqa: E402
from torchmd_amd.forces import Forces  # noqa: E402
from torchmd_amd.integrator import Integrator, maxwell_boltzmann  # noqa: E402
from torchmd_amd.parameters import Parameters  # noqa: E402
from torchmd_amd.restraints import Restraints  # noqa: E402
from torchmd_amd.systems import System  # noqa: E402

TERMS = ["lj", "electrostatics", "bonds", "angles"]


def restraints(pos, box, R, natoms_restrained):
    """Oxygens spread over the box: two atoms = one distance restraint; more = half of them held at their start, the other
    half paired up, every pair at its start distance."""
    if natoms_restrained == 0:
        return None
    ox = np.arange(0, len(pos), 3)
    pick = ox[np.linspace(0, len(ox) - 1, natoms_restrained).astype(int)]
    npos = natoms_restrained // 2 if natoms_restrained > 2 else 0
    rs = Restraints(R)
    if npos:
        rs.add_position(pick[:npos], pos[pick[:npos]], 10.0)
    pairs = pick[npos:npos + 2 * ((natoms_restrained - npos) // 2)].reshape(-1, 2)
    d = pos[pairs[:, 0]] - pos[pairs[:, 1]]
    d -= box * np.rint(d / box)
    rs.add_distance(pairs, np.sqrt((d * d).sum(axis=1)), 10.0)
    assert len(rs.atoms()) == natoms_restrained
    return rs


def measure(nside, R, counts, rounds, steps):
    dev = torch.device("cuda:0")
    mol, pos, box = tip3p_box(nside, seed=0)
    par = Parameters(water_forcefield(mol), mol, TERMS, precision=torch.float32)
    out = {"replicas": R, "natoms": mol.numAtoms, "steps_per_call": steps, "us_per_step": {}}
    for m in counts:
        rs = restraints(np.asarray(pos, dtype=np.float64), np.asarray(box, dtype=np.float64), R, m)
        s = System(mol.numAtoms, R, torch.float32, dev)
        s.set_positions(pos[:, :, None])
        s.set_box(box)
        torch.manual_seed(1)
        s.set_velocities(maxwell_boltzmann(par.masses, 300, R))
        f = Forces(par, terms=TERMS, cutoff=9.0, rfa=True, **({} if rs is None else {"restraints": rs}))
        f.compute(s.pos, s.box, s.forces)
        integ = Integrator(s, f, 1.0, dev)
        integ.step(steps)  # warm-up: code objects, list capacity
        per = []
        for _ in range(rounds):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            integ.step(steps)
            torch.cuda.synchronize()
            per.append((time.perf_counter() - t0) / steps * 1e6)
        st = f.stats(s.pos)
        out["us_per_step"][str(m)] = {"rounds": [round(v, 2) for v in per], "median": round(float(np.median(per)), 2),
                                      "steps_in_pair_launch": int(st["steps_in_pair_launch"]), "replays": int(integ.replays)}
        f.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=200)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    counts = (0, 2, 1000)
    out = {"device": torch.cuda.get_device_name(0),
           "cases": [measure(32, 1, counts, args.rounds, args.steps), measure(12, 16, counts, args.rounds, args.steps)]}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
