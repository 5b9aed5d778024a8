#!/usr/bin/env python
"""What a metadynamics bias on CVs of groups of atoms costs an MD step on ONE GPU, fp32: microseconds per step of
`Integrator.step` (NVE, host clock around whole calls, two device synchronisations) on the 98 304-atom water box, the plain run
and every biased run alternated round by round in the same session (needs a GPU).  The bias is `frozen`, so that the figures
hold the impulse launches and the finishing launch alone.  The cases:

    group_distance   the distance of two groups of 1 000 atoms
    coordination 1   the coordination number of one oxygen with all others (r0 = 3.5, n = 6, d_max = 9)
    coordination 100 the same with 100 oxygens in the first set

    python tools/time_metad_groups.py [--rounds 3] [--steps 200] [--apply CASE]

With `--apply CASE` nothing is timed: the case is set up and its bias applied five times (tmdhip_metad_apply through
`Forces.compute`), for a kernel trace of one application taken from outside.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from torchmd_amd.builders import tip3p_box, water_forcefield  # noqa: E402
from torchmd_amd.forces import Forces  # noqa: E402
from torchmd_amd.integrator import Integrator, maxwell_boltzmann  # noqa: E402
from torchmd_amd.metadynamics import Metadynamics, min_image  # noqa: E402
from torchmd_amd.parameters import Parameters  # noqa: E402
from torchmd_amd.systems import System  # noqa: E402

WATER_TERMS = ["lj", "electrostatics", "bonds", "angles"]
SWITCH = {"r0": 3.5, "n": 6, "d_max": 9.0}
CASES = ("group_distance", "coordination 1", "coordination 100")


def nearest(p, centre, n, box):
    d = min_image(p - np.asarray(centre, dtype=np.float64), box)
    return [int(i) for i in np.argsort((d * d).sum(axis=1), kind="stable")[:n]]


def bias(name, p, b, masses):
    ox = [int(a) for a in np.arange(0, len(p), 3)]
    kw = dict(height=1.0, frequency=10 ** 9, temperature=300.0, bias_factor=6.0)
    if name == "group_distance":
        md = Metadynamics(("group_distance", (nearest(p, 0.25 * b, 1000, b), nearest(p, 0.6 * b, 1000, b))), sigma=0.3, grid_min=20.0,
                          grid_max=80.0, grid_bins=400, **kw)
    elif name == "coordination 1":
        md = Metadynamics(("coordination", (ox[:1], ox), SWITCH), sigma=0.2, grid_min=0.0, grid_max=16.0, grid_bins=160, **kw)
    else:
        md = Metadynamics(("coordination", (ox[:100], ox), SWITCH), sigma=2.0, grid_min=0.0, grid_max=1600.0, grid_bins=1600, **kw)
    md.masses = masses
    grid = np.zeros_like(md.grid)
    grid[0] += md.gauss_terms(md.cv_values(p, b)[0] + 0.3 * md.sigma[:1], 2.0)
    md.set_grid(grid)
    md.frozen = True
    return md


def system(mol, pos, box, par, dev):
    s = System(mol.numAtoms, 1, torch.float32, dev)
    s.set_positions(pos[:, :, None])
    s.set_box(box)
    torch.manual_seed(1)
    s.set_velocities(maxwell_boltzmann(par.masses, 300, 1))
    return s


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--nside", type=int, default=32)
    ap.add_argument("--apply", default=None, choices=CASES)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    dev = torch.device("cuda:0")
    mol, pos, box = tip3p_box(args.nside, seed=0)
    par = Parameters(water_forcefield(mol), mol, WATER_TERMS, precision=torch.float32)
    p, b = np.asarray(pos, dtype=np.float64).reshape(mol.numAtoms, 3), np.asarray(box, dtype=np.float64).reshape(-1)[:3]
    masses = par.masses.detach().cpu().double().reshape(-1).numpy()
    if args.apply:
        md = bias(args.apply, p, b, masses)
        s = system(mol, pos, box, par, dev)
        f = Forces(par, terms=[], metadynamics=md)
        for _ in range(5):
            f.compute(s.pos, s.box, s.forces)
        torch.cuda.synchronize()
        print(json.dumps({"applied": args.apply, "cv": md.cv.tolist(), "bias": md.energy.tolist()}))
        f.close()
        return
    runs = {}
    for name in ("plain",) + CASES:
        md = None if name == "plain" else bias(name, p, b, masses)
        s = system(mol, pos, box, par, dev)
        f = Forces(par, terms=WATER_TERMS, cutoff=9.0, rfa=True, **({} if md is None else {"metadynamics": md}))
        f.compute(s.pos, s.box, s.forces)
        integ = Integrator(s, f, 1.0, dev)
        integ.step(args.steps)  # warm-up: code objects, list capacity
        runs[name] = (s, f, integ, md, [])
    for _ in range(args.rounds):  # alternated: every round visits every run
        for name, (s, f, integ, md, per) in runs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            integ.step(args.steps)
            torch.cuda.synchronize()
            per.append((time.perf_counter() - t0) / args.steps * 1e6)
    out = {"device": torch.cuda.get_device_name(0), "natoms": mol.numAtoms, "steps_per_call": args.steps, "us_per_step": {}}
    for name, (s, f, integ, md, per) in runs.items():
        st = f.stats(s.pos)
        out["us_per_step"][name] = {"rounds": [round(v, 2) for v in per], "median": round(float(np.median(per)), 2),
                                    "steps_in_pair_launch": int(st["steps_in_pair_launch"])}
        if md is not None:
            out["us_per_step"][name]["cv"] = [round(float(v), 4) for v in md.cv[0]]
        f.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
