#!/usr/bin/env python
"""Config C3 at constant pressure on ONE GPU: the 98 304-atom TIP3P box (tip3p_box(32)), cutoff 9 A, reaction field,
Langevin 300 K, 1 fs, fp32 — the same run with and without a Monte Carlo barostat (1 bar, a move every 25 steps), on the
same box in the same process, alternating (needs a GPU).

Reports us/step of both (host clock around Integrator.step calls that end in a device synchronisation), the cost of one
attempt split into accepted and rejected moves (host clock around `barostat.attempt`, which ends in the read-back of the
energies; a rejected move also makes the NEXT step re-plan and rebuild the list, which is in the step time, not here), and
the density after the run.

    python tools/time_npt.py [--nside 32] [--steps 500] [--rounds 3] [--frequency 25]
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


class TimedBarostat(MonteCarloBarostat):
    """Keeps the wall time of every attempt next to its outcome."""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.times = []

    def attempt(self, system, forces, epot):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        rec = super().attempt(system, forces, epot)
        torch.cuda.synchronize()
        self.times.append((time.perf_counter() - t0, bool(rec["accepted"][0])))
        return rec


def setup(nside, barostat):
    dev = torch.device("cuda:0")
    mol, pos, box = tip3p_box(nside, seed=0)
    par = Parameters(water_forcefield(mol), mol, TERMS, precision=torch.float32)
    s = System(mol.numAtoms, 1, torch.float32, dev)
    s.set_positions(pos[:, :, None])
    s.set_box(box)
    torch.manual_seed(1)
    s.set_velocities(maxwell_boltzmann(par.masses, 300.0, 1))
    f = Forces(par, terms=TERMS, cutoff=9.0, rfa=True)
    f.compute(s.pos, s.box, s.forces)
    return mol, s, f, Integrator(s, f, 1.0, dev, gamma=1.0, T=300.0, barostat=barostat)


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
    ap.add_argument("--frequency", type=int, default=25)
    ap.add_argument("--pressure", type=float, default=1.0)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    bar = TimedBarostat(args.pressure, 300.0, frequency=args.frequency, seed=1)
    mol, s_nvt, f_nvt, i_nvt = setup(args.nside, None)
    _, s_npt, f_npt, i_npt = setup(args.nside, bar)
    for integ in (i_nvt, i_npt):  # warm-up: code objects, list capacity, the first moves
        integ.step(200)
    bar.times.clear()
    r0 = {k: f.stats(s.pos)["n_rebuilds"] for k, f, s in (("nvt", f_nvt, s_nvt), ("npt", f_npt, s_npt))}
    nvt, npt = [], []
    for _ in range(args.rounds):
        nvt.append(timed(i_nvt, args.steps))
        npt.append(timed(i_npt, args.steps))
    total = args.rounds * args.steps
    acc = [t for t, ok in bar.times if ok]
    rej = [t for t, ok in bar.times if not ok]
    e = np.diagonal(s_npt.box[0].cpu().double().numpy())
    rho = mol.numAtoms / 3 * 18.0154 / 6.02214076e23 / (e.prod() * 1e-24)
    out = {
        "natoms": mol.numAtoms, "device": torch.cuda.get_device_name(0), "frequency": args.frequency, "pressure_bar": args.pressure,
        "us_per_step_nvt": [round(v, 2) for v in nvt], "us_per_step_npt": [round(v, 2) for v in npt],
        "us_per_step_nvt_median": round(float(np.median(nvt)), 2), "us_per_step_npt_median": round(float(np.median(npt)), 2),
        "attempts": len(bar.times), "accepted": len(acc),
        "us_per_accepted_attempt": round(float(np.median(acc)) * 1e6, 1) if acc else None,
        "us_per_rejected_attempt": round(float(np.median(rej)) * 1e6, 1) if rej else None,
        "rebuilds_per_step_nvt": round((f_nvt.stats(s_nvt.pos)["n_rebuilds"] - r0["nvt"]) / total, 4),
        "rebuilds_per_step_npt": round((f_npt.stats(s_npt.pos)["n_rebuilds"] - r0["npt"]) / total, 4),
        "box_edge_A": round(float(e[0]), 4), "density_g_cm3": round(float(rho), 4), "steps_npt_total": int(i_npt._nstep),
        "max_dv_A3": round(float(bar.max_dv[0]), 1),
    }
    print(json.dumps(out))


if __name__ == "__main__":
    main()
