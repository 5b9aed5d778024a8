#!/usr/bin/env python
"""Four-site rigid water against three-site rigid water on ONE GPU (needs a GPU): the 131 072-site TIP4P-Ew box
(tip4p_box(32): 32^3 molecules) and the 98 304-atom TIP3P box (tip3p_box(32)) of the same 32 768 molecules, both rigid
(SETTLE), 2 fs, Langevin 300 K, cutoff 9 A, fp32 — with the reaction field and with PME.  The four runs live in one process and
alternate round by round, so that clock and box drift hit all of them alike.

Reports us/step of each (host clock around Integrator.step calls that end in a device synchronisation, after a warm-up under a
strong thermostat that has compiled the code objects, sized the lists and relaxed the lattice start), the median over the rounds, and rebuilds per
step.  The duration and register count of md_step_cons_vs_kernel come from a kernel trace of a run of this tool
(DESIGN §12), not from here.

    python tools/time_tip4p.py [--nside 32] [--steps 500] [--rounds 3] [--no-pme]
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from torchmd_amd.builders import tip3p_box, tip4p_box, tip4pew_forcefield, water_forcefield  # noqa: E402
from torchmd_amd.forces import Forces  # noqa: E402
from torchmd_amd.integrator import Integrator, maxwell_boltzmann  # noqa: E402
from torchmd_amd.parameters import Parameters  # noqa: E402
from torchmd_amd.systems import System  # noqa: E402

TERMS = ["lj", "electrostatics", "bonds", "angles"]


def setup(nside, four_site, pme):
    dev = torch.device("cuda:0")
    if four_site:
        mol, pos, box, vs = tip4p_box(nside, seed=0)
        par = Parameters(tip4pew_forcefield(mol), mol, TERMS, precision=torch.float32)
    else:
        mol, pos, box = tip3p_box(nside, seed=0)
        vs = None
        par = Parameters(water_forcefield(mol), mol, TERMS, precision=torch.float32)
    s = System(mol.numAtoms, 1, torch.float32, dev)
    s.set_positions(pos[:, :, None])
    s.set_box(box)
    torch.manual_seed(1)
    vel = maxwell_boltzmann(par.masses, 300.0, 1)
    if vs is not None:
        vel[:, torch.as_tensor(vs.sites.astype(np.int64))] = 0.0
    s.set_velocities(vel)
    kw = dict(cutoff=9.0, pme=True) if pme else dict(cutoff=9.0, rfa=True)
    if vs is not None:
        kw["virtual_sites"] = vs
    f = Forces(par, terms=TERMS, **kw)
    f.compute(s.pos, s.box, s.forces)
    return mol, s, f


def relaxed(s, f, steps):
    """The lattice start releases heat (randomly oriented molecules on a grid: several hundred kelvin within 200 steps, and
    with it list rebuilds and rewound batches that say nothing about a production run): `steps` steps under a strong
    thermostat (20 / ps) first, then the integrator that is timed (1 / ps)."""
    dev = s.pos.device
    Integrator(s, f, 2.0, dev, gamma=20.0, T=300.0, constraints="water").step(steps)
    return Integrator(s, f, 2.0, dev, gamma=1.0, T=300.0, constraints="water")


def timed(integ, steps, call=100):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps // call):
        integ.step(call)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / (steps // call * call) * 1e6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nside", type=int, default=32)
    ap.add_argument("--steps", type=int, default=500)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2000)
    ap.add_argument("--no-pme", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    runs = {}
    for pme in ([False] if args.no_pme else [False, True]):
        for four in (False, True):
            runs[("tip4p" if four else "tip3p") + ("_pme" if pme else "_rf")] = setup(args.nside, four, pme)
    runs = {k: (mol, s, f, relaxed(s, f, args.warmup)) for k, (mol, s, f) in runs.items()}
    temps = {k: float(integ.step(100)[2][0]) for k, (_, _, _, integ) in runs.items()}
    r0 = {k: f.stats(s.pos)["n_rebuilds"] for k, (_, s, f, _) in runs.items()}
    t = {k: [] for k in runs}
    for _ in range(args.rounds):
        for k, (_, s, f, integ) in runs.items():
            t[k].append(timed(integ, args.steps))
    total = args.rounds * args.steps
    out = {"device": torch.cuda.get_device_name(0), "timestep_fs": 2.0, "steps_per_round": args.steps, "rounds": args.rounds}
    for k, (mol, s, f, integ) in runs.items():
        out[k] = {
            "nsites": mol.numAtoms, "us_per_step": [round(v, 2) for v in t[k]], "us_per_step_median": round(float(np.median(t[k])), 2),
            "rebuilds_per_step": round((f.stats(s.pos)["n_rebuilds"] - r0[k]) / total, 4), "replays": integ.replays,
            "T_after_warmup_K": round(temps[k], 1),
        }
    print(json.dumps(out))


if __name__ == "__main__":
    main()
