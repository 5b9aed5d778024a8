#!/usr/bin/env python
"""What a metadynamics bias costs an MD step on ONE GPU, fp32: microseconds per step of `Integrator.step` (NVE, host
clock around whole calls, two device synchronisations) with and without a bias in the same session, in two settings: 16 replicas
of alanine dipeptide in water (688 atoms, tests/golden/ala2.npz) under a phi / psi bias, and the 98 304-atom water box alone
under one O-O distance CV (needs a GPU).  The bias is `frozen` for the step figures, so that they hold the impulse launch and
the finishing launch alone; the cost of one deposition (the height launch and the node launch, 16 grids of 256 x 256 nodes) is
measured apart with device events.

    python tools/time_metad.py [--rounds 5] [--steps 200]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from torchmd_amd.builders import tip3p_box, water_forcefield  # noqa: E402
from torchmd_amd.forces import Forces  # noqa: E402
from torchmd_amd.integrator import Integrator, maxwell_boltzmann  # noqa: E402
from torchmd_amd.metadynamics import Metadynamics  # noqa: E402
from torchmd_amd.parameters import Parameters  # noqa: E402
from torchmd_amd.systems import System  # noqa: E402

WATER_TERMS = ["lj", "electrostatics", "bonds", "angles"]
ALL_TERMS = ["bonds", "angles", "dihedrals", "impropers", "1-4", "electrostatics", "lj"]
PHI, PSI = (4, 6, 8, 14), (6, 8, 14, 16)


def prefill(md, centre):
    grid = np.zeros_like(md.grid)
    for g in range(grid.shape[0]):
        grid[g] += md.gauss_terms(np.asarray(centre, dtype=np.float64) + 0.3, 2.0)
    md.set_grid(grid)
    md.frozen = True
    return md


def time_steps(s, f, rounds, steps):
    dev = s.pos.device
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
    out = {"rounds": [round(v, 2) for v in per], "median": round(float(np.median(per)), 2),
           "steps_in_pair_launch": int(st["steps_in_pair_launch"]), "replays": int(integ.replays)}
    f.close()
    return out


def ala2(R, rounds, steps):
    from _golden import GoldenParameters, load

    dev = torch.device("cuda:0")
    g = load("ala2")
    par = GoldenParameters(g, torch.float32)
    pos = np.asarray(g["pos"], dtype=np.float64).reshape(-1, 3)
    out = {"system": "ala2", "replicas": R, "natoms": len(pos), "steps_per_call": steps, "us_per_step": {}}
    for name in ("plain", "phi-psi bias"):
        md = None
        if name != "plain":
            md = Metadynamics([("dihedral", PHI), ("dihedral", PSI)], sigma=0.35, height=1.0, frequency=10 ** 9, temperature=300.0,
                              bias_factor=6.0, grid_bins=64, nreplicas=R)
            prefill(md, md.cv_values(pos, np.asarray(g["box"], dtype=np.float64).reshape(-1)[:3])[0])
        s = System(len(pos), R, torch.float32, dev)
        s.set_positions(np.repeat(pos[:, :, None], R, axis=2))
        s.set_box(np.asarray(g["box"], dtype=np.float64).reshape(-1)[:3])
        torch.manual_seed(1)
        s.set_velocities(maxwell_boltzmann(par.masses, 300, R))
        f = Forces(par, terms=ALL_TERMS, cutoff=9.0, switch_dist=7.5, rfa=True, **({} if md is None else {"metadynamics": md}))
        out["us_per_step"][name] = time_steps(s, f, rounds, steps)
    return out


def water(nside, rounds, steps):
    dev = torch.device("cuda:0")
    mol, pos, box = tip3p_box(nside, seed=0)
    par = Parameters(water_forcefield(mol), mol, WATER_TERMS, precision=torch.float32)
    p, b = np.asarray(pos, dtype=np.float64).reshape(mol.numAtoms, 3), np.asarray(box, dtype=np.float64).reshape(-1)[:3]
    out = {"system": "water", "replicas": 1, "natoms": mol.numAtoms, "steps_per_call": steps, "us_per_step": {}}
    for name in ("plain", "distance bias"):
        md = None
        if name != "plain":
            ox = np.arange(0, len(p), 3)
            i, j = int(ox[0]), int(ox[np.argsort(np.linalg.norm(p[ox] - p[ox[0]], axis=1))[1]])
            md = Metadynamics(("distance", (i, j)), sigma=0.3, height=1.0, frequency=10 ** 9, temperature=300.0, bias_factor=6.0,
                              grid_min=1.0, grid_max=13.0, grid_bins=96)
            prefill(md, md.cv_values(p, b)[0])
        s = System(mol.numAtoms, 1, torch.float32, dev)
        s.set_positions(pos[:, :, None])
        s.set_box(box)
        torch.manual_seed(1)
        s.set_velocities(maxwell_boltzmann(par.masses, 300, 1))
        f = Forces(par, terms=WATER_TERMS, cutoff=9.0, rfa=True, **({} if md is None else {"metadynamics": md}))
        out["us_per_step"][name] = time_steps(s, f, rounds, steps)
    return out


def deposition(R, bins, count):
    """One deposition on R grids of bins x bins nodes: device events around `count` back-to-back calls."""
    from _golden import GoldenParameters, load

    dev = torch.device("cuda:0")
    g = load("ala2")
    par = GoldenParameters(g, torch.float32)
    pos = np.asarray(g["pos"], dtype=np.float64).reshape(-1, 3)
    md = Metadynamics([("dihedral", PHI), ("dihedral", PSI)], sigma=2.0 * (2.0 * np.pi / bins), height=1.0, frequency=1, temperature=300.0,
                      bias_factor=6.0, grid_bins=bins, nreplicas=R)
    s = System(len(pos), R, torch.float32, dev)
    s.set_positions(np.repeat(pos[:, :, None], R, axis=2))
    s.set_box(np.asarray(g["box"], dtype=np.float64).reshape(-1)[:3])
    f = Forces(par, terms=ALL_TERMS, cutoff=9.0, switch_dist=7.5, rfa=True, metadynamics=md)
    f.compute(s.pos, s.box, s.forces)
    for _ in range(3):
        md.deposit(s)
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(count):
        md.deposit(s)
    b.record()
    torch.cuda.synchronize()
    f.close()
    return {"grids": R, "nodes": [bins, bins], "depositions": count, "us_per_deposition": round(a.elapsed_time(b) / count * 1e3, 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=200)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    out = {"device": torch.cuda.get_device_name(0),
           "cases": [ala2(16, args.rounds, args.steps), water(32, args.rounds, args.steps)],
           "deposition": deposition(16, 256, 50)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
