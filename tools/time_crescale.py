#!/usr/bin/env python
"""Config C3 at constant pressure on ONE GPU: the 98 304-atom TIP3P box (tip3p_box(32)), cutoff 9 A, reaction field,
Langevin 300 K, 1 fs, fp32 — the same run at constant volume, under the C-rescale barostat every 10 and every 25 steps, and
under the Monte Carlo barostat every 25 steps (all at 1 bar), on the same box in the same process, alternating (needs a GPU).

Reports us/step of the four (host clock around Integrator.step calls that end in a device synchronisation), the cost of one
C-rescale application split into the pressure (`Forces._pressure_terms`, ends in its read-back), the rescale launch (host
clock to the end of the kernels) and `forces.compute` at the new box (which re-plans the grid and rebuilds the list with a
host synchronisation, and ends in the read-back of the energies), and the density of every box after every round, from the
lattice start.

    python tools/time_crescale.py [--nside 32] [--steps 500] [--rounds 3]
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from torchmd_amd import crescale as X  # noqa: E402
from torchmd_amd.barostat import MonteCarloBarostat  # noqa: E402
from torchmd_amd.builders import tip3p_box, water_forcefield  # noqa: E402
from torchmd_amd.forces import Forces  # noqa: E402
from torchmd_amd.integrator import Integrator, maxwell_boltzmann  # noqa: E402
from torchmd_amd.parameters import Parameters  # noqa: E402
from torchmd_amd.systems import System  # noqa: E402

TERMS = ["lj", "electrostatics", "bonds", "angles"]


class TimedForces(Forces):
    """Keeps the wall time of the pressure and of every `compute` made while `timing` is on (the barostat's)."""

    timing = False

    def _clock(self, key, fn, *a, **kw):
        if not self.timing:
            return fn(*a, **kw)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn(*a, **kw)
        torch.cuda.synchronize()
        self.times.setdefault(key, []).append(time.perf_counter() - t0)
        return out

    def _pressure_terms(self, *a, **kw):
        return self._clock("pressure", super()._pressure_terms, *a, **kw)

    def compute(self, *a, **kw):
        return self._clock("compute", super().compute, *a, **kw)


class TimedCRescale(X.CRescaleBarostat):
    def apply(self, system, forces, *a, **kw):
        forces.timing = True
        real = X.rescale_molecules

        def launch(*b, **k):
            return forces._clock("rescale", real, *b, **k)

        X.rescale_molecules = launch
        try:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            rec = super().apply(system, forces, *a, **kw)
            forces.times.setdefault("application", []).append(time.perf_counter() - t0)
            return rec
        finally:
            X.rescale_molecules = real
            forces.timing = False


def setup(nside, barostat):
    dev = torch.device("cuda:0")
    mol, pos, box = tip3p_box(nside, seed=0)
    par = Parameters(water_forcefield(mol), mol, TERMS, precision=torch.float32)
    s = System(mol.numAtoms, 1, torch.float32, dev)
    s.set_positions(pos[:, :, None])
    s.set_box(box)
    torch.manual_seed(1)
    s.set_velocities(maxwell_boltzmann(par.masses, 300.0, 1))
    f = TimedForces(par, terms=TERMS, cutoff=9.0, rfa=True)
    f.times = {}
    f.compute(s.pos, s.box, s.forces)
    return mol, s, f, Integrator(s, f, 1.0, dev, gamma=1.0, T=300.0, barostat=barostat)


def timed(integ, steps, call=100):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps // call):
        integ.step(call)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / (steps // call * call) * 1e6


def density(mol, s):
    e = np.diagonal(s.box[0].cpu().double().numpy())
    return round(float(mol.numAtoms / 3 * 18.0154 / 6.02214076e23 / (e.prod() * 1e-24)), 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nside", type=int, default=32)
    ap.add_argument("--steps", type=int, default=500)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--pressure", type=float, default=1.0)
    ap.add_argument("--tau", type=float, default=1.0)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    legs = {
        "nvt": None,
        "crescale10": TimedCRescale(args.pressure, 300.0, tau=args.tau, frequency=10, seed=1),
        "crescale25": TimedCRescale(args.pressure, 300.0, tau=args.tau, frequency=25, seed=1),
        "montecarlo25": MonteCarloBarostat(args.pressure, 300.0, frequency=25, seed=1),
    }
    runs = {k: setup(args.nside, b) for k, b in legs.items()}
    trace = {k: [density(runs[k][0], runs[k][1])] for k in legs}
    for k in legs:  # warm-up: code objects, list capacity, the first moves
        runs[k][3].step(200)
        runs[k][2].times.clear()
        trace[k].append(density(runs[k][0], runs[k][1]))
    us = {k: [] for k in legs}
    for _ in range(args.rounds):
        for k in legs:
            us[k].append(timed(runs[k][3], args.steps))
            trace[k].append(density(runs[k][0], runs[k][1]))
    out = {"natoms": runs["nvt"][0].numAtoms, "device": torch.cuda.get_device_name(0), "pressure_bar": args.pressure, "tau_ps": args.tau,
           "steps_per_leg": 200 + args.rounds * args.steps}
    for k in legs:
        out[k] = {"us_per_step": [round(v, 2) for v in us[k]], "us_per_step_median": round(float(np.median(us[k])), 2),
                  "density_g_cm3_trace": trace[k]}
        t = runs[k][2].times
        if t:
            out[k]["us_per_application"] = {p: round(float(np.median(v)) * 1e6, 1) for p, v in t.items()}
            out[k]["applications"] = len(t["application"])
    mc = legs["montecarlo25"]
    out["montecarlo25"].update(attempts=int(mc.attempts[0]), accepted=int(mc.accepted[0]))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
