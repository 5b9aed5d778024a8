#!/usr/bin/env python
"""What one `Integrator.pressure()` costs on ONE GPU (needs a GPU), beside `Forces.compute()` with energies on the same state:

* config C3 (the 98 304-atom TIP3P box, cutoff 9 A, 1 fs, fp32) with a reaction field and with PME,
* 16 replicas of the 5 184-atom box (tip3p_box(12)) with a reaction field.

Host clock around `reps` calls, each of which ends in its own read-back (pressure(): tmdhip_pressure's one synchronisation;
compute(): tmdhip_compute's), median of `rounds`, the two alternating.  The box is aged by a few MD steps first, so the lists
are ordinary ones.  With `--npt N` one more leg runs N steps of the C3 box (nside as given) under the Monte Carlo barostat and
prints the mean of the pressure sampled every `--every` steps with its block error (10 blocks), beside the barostat's target.

    python tools/time_pressure.py [--nside 32] [--reps 20] [--rounds 5] [--npt 0] [--every 10]
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from torchmd_amd.barostat import MonteCarloBarostat  # noqa: E402
from torchmd_amd.builders import tip3p_box, water_forcefield  # noqa: E402
from torchmd_amd.forces import Forces  # noqa: E402
from torchmd_amd.integrator import Integrator, maxwell_boltzmann  # noqa: E402
from torchmd_amd.parameters import Parameters  # noqa: E402
from torchmd_amd.systems import System  # noqa: E402

TERMS = ["lj", "electrostatics", "bonds", "angles"]


def setup(nside, replicas, barostat=None, **fkw):
    dev = torch.device("cuda:0")
    mol, pos, box = tip3p_box(nside, seed=0)
    par = Parameters(water_forcefield(mol), mol, TERMS, precision=torch.float32)
    s = System(mol.numAtoms, replicas, torch.float32, dev)
    s.set_positions(np.repeat(pos[:, :, None], replicas, axis=2))
    s.set_box(box)
    torch.manual_seed(1)
    s.set_velocities(maxwell_boltzmann(par.masses, 300.0, replicas))
    f = Forces(par, terms=TERMS, cutoff=9.0, **fkw)
    f.compute(s.pos, s.box, s.forces)
    return mol, s, f, Integrator(s, f, 1.0, dev, gamma=1.0, T=300.0, barostat=barostat)


def timed(fn, reps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps * 1e6


def leg(name, nside, replicas, reps, rounds, **fkw):
    mol, s, f, integ = setup(nside, replicas, **fkw)
    integ.step(20)
    scratch = torch.zeros_like(s.forces)
    press = lambda: integ.pressure()  # noqa: E731
    comp = lambda: f.compute(s.pos, s.box, scratch)  # noqa: E731
    press(), comp()  # warm-up: code objects, the molecule table
    tp, tc = [], []
    for _ in range(rounds):
        tp.append(timed(press, reps))
        tc.append(timed(comp, reps))
    return {"leg": name, "natoms": mol.numAtoms, "replicas": replicas, "algorithm": f.stats(s.pos)["algorithm"],
            "us_per_pressure": [round(v, 1) for v in tp], "us_per_compute": [round(v, 1) for v in tc],
            "us_per_pressure_median": round(float(np.median(tp)), 1), "us_per_compute_median": round(float(np.median(tc)), 1),
            "pressure_bar": [round(float(v), 1) for v in integ.pressure()[:2]]}


def npt_leg(nside, steps, every, target):
    bar = MonteCarloBarostat(target, 300.0, frequency=25, seed=1)
    mol, s, f, integ = setup(nside, 1, barostat=bar, rfa=True)
    integ.step(200)
    samples = []
    for _ in range(steps // every):
        integ.step(every)
        samples.append(float(integ.pressure()[0]))
    x = np.asarray(samples)
    nb = 10
    blocks = x[: len(x) // nb * nb].reshape(nb, -1).mean(axis=1) if len(x) >= nb else x
    return {"leg": "npt", "natoms": mol.numAtoms, "steps": steps, "every": every, "target_bar": target, "samples": len(x),
            "mean_pressure_bar": round(float(x.mean()), 1), "block_error_bar": round(float(blocks.std(ddof=1) / np.sqrt(len(blocks))), 1),
            "std_bar": round(float(x.std()), 1), "accepted": int(bar.accepted[0]), "attempts": int(bar.attempts[0])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nside", type=int, default=32)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--npt", type=int, default=0)
    ap.add_argument("--every", type=int, default=10)
    ap.add_argument("--target", type=float, default=1.0)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    out = {"device": torch.cuda.get_device_name(0), "legs": [
        leg("c3_rf", args.nside, 1, args.reps, args.rounds, rfa=True),
        leg("c3_pme", args.nside, 1, args.reps, args.rounds, pme=True),
        leg("16x5184_rf", 12, 16, args.reps, args.rounds, rfa=True),
    ]}
    if args.npt > 0:
        out["legs"].append(npt_leg(args.nside, args.npt, args.every, args.target))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
