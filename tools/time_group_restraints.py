#!/usr/bin/env python
"""What group restraints cost an MD step on ONE GPU, fp32: microseconds per step of `Integrator.step` (NVE, host
clock around whole calls, two device synchronisations) without the term, with one Boresch set on six oxygens, and with a
distance between the centres of mass of two groups of 1 000 atoms, in two settings: the 98 304-atom water box alone, and 16
replicas of the 5 184-atom box in the batched pair + step launch (needs a GPU).  The figure without the term of the same session
is the comparison: a `Forces` without the keyword, where no new launch is enqueued.  With the term a step gains two small
launches (centres, forces; in the batched pair + step path two for all replicas, in the replica-by-replica loop two per
replica) and a call one finishing application with the energy kernel and its fold behind it.

    python tools/time_group_restraints.py [--rounds 3] [--steps 200]
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
from torchmd_amd.group_restraints import GroupRestraints  # noqa: E402
from torchmd_amd.integrator import Integrator, maxwell_boltzmann  # noqa: E402
from torchmd_amd.parameters import Parameters  # noqa: E402
from torchmd_amd.systems import System  # noqa: E402

TERMS = ["lj", "electrostatics", "bonds", "angles"]
CASES = ("none", "boresch", "com1000")


def _nearest_waters(pos, box, point, n):
    ox = np.arange(0, len(pos), 3)
    d = pos[ox] - point
    d -= box * np.rint(d / box)
    return ox[np.argsort((d * d).sum(axis=1))[:n]]


def group_restraints(pos, box, R, case):
    """boresch: six oxygens around the middle of the box, every target at its present value; com1000: two groups of 334 and 333
    whole waters (1 002 and 999 atoms) around two points 12 A apart, the distance at its present value."""
    if case == "none":
        return None
    if case == "boresch":
        six = [int(a) for a in _nearest_waters(pos, box, 0.5 * box, 6)]
        gr = GroupRestraints.boresch(R, six[:3], six[3:], 1.0, 1.0, 1.0, 0.0, 0.0, 0.0, 10.0, 10.0, 10.0)
        s = gr.values(np.repeat(pos[None], R, axis=0), box)
        s[:, 1:3] = np.clip(s[:, 1:3], 0.0, np.pi)
        gr.set_targets(s)
        return gr
    gr = GroupRestraints(R)
    ids = []
    for shift, n in ((-6.0, 334), (6.0, 333)):
        o = _nearest_waters(pos, box, 0.5 * box + np.array([shift, 0.0, 0.0]), n)
        ids.append(gr.add_group(np.concatenate([[a, a + 1, a + 2] for a in o]), weights=np.tile([15.9994, 1.008, 1.008], n)))
    assert gr.check_extent(pos, box)
    X = gr.centres(np.repeat(pos[None], R, axis=0), box)[0]
    gr.add_distance(ids, float(np.linalg.norm(X[0] - X[1])), 10.0)
    return gr


def measure(nside, R, rounds, steps):
    dev = torch.device("cuda:0")
    mol, pos, box = tip3p_box(nside, seed=0)
    par = Parameters(water_forcefield(mol), mol, TERMS, precision=torch.float32)
    out = {"replicas": R, "natoms": mol.numAtoms, "steps_per_call": steps, "us_per_step": {}}
    for case in CASES:
        gr = group_restraints(np.asarray(pos, dtype=np.float64), np.asarray(box, dtype=np.float64).reshape(-1)[:3], R, case)
        s = System(mol.numAtoms, R, torch.float32, dev)
        s.set_positions(pos[:, :, None])
        s.set_box(box)
        torch.manual_seed(1)
        s.set_velocities(maxwell_boltzmann(par.masses, 300, R))
        f = Forces(par, terms=TERMS, cutoff=9.0, rfa=True, **({} if gr is None else {"group_restraints": gr}))
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
        out["us_per_step"][case] = {"rounds": [round(v, 2) for v in per], "median": round(float(np.median(per)), 2),
                                    "steps_in_pair_launch": int(st["steps_in_pair_launch"]), "replays": int(integ.replays)}
        f.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=200)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    out = {"device": torch.cuda.get_device_name(0),
           "cases": [measure(32, 1, args.rounds, args.steps), measure(12, 16, args.rounds, args.steps)]}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
