#!/usr/bin/env python
"""Config C3 under the velocity-rescaling thermostat on ONE GPU: the 98 304-atom TIP3P box (tip3p_box(32)), cutoff 9 A,
reaction field, 1 fs, fp32 — NVE `step(100)` against the same run with a thermostat application every 10 steps, on the
same box in the same process, alternating (needs a GPU).

Reports us/step of both (host clock around Integrator.step calls that end in a device synchronisation), the cost of one
application alone (host clock around a batch of `apply` calls between two synchronisations), and the drift of the conserved
quantity E_kin + E_pot - heat of the thermostatted run beside the drift of E_kin + E_pot of the NVE run, both in
kcal/mol per atom per ns.

    python tools/time_thermostat.py [--nside 32] [--steps 500] [--rounds 3] [--frequency 10] [--tau 0.1]
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
from torchmd_amd.systems import System  # noqa: E402
from torchmd_amd.thermostat import VelocityRescale  # noqa: E402

TERMS = ["lj", "electrostatics", "bonds", "angles"]


def setup(nside, thermostat):
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
    return mol, s, f, Integrator(s, f, 1.0, dev, thermostat=thermostat)


def timed(integ, steps, energies, heat=None, call=100):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps // call):
        ek, pot, _ = integ.step(call)
        energies.append(float(ek[0]) + pot[0] - (float(heat()[0]) if heat else 0.0))
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / (steps // call * call) * 1e6


def drift(energies, natoms, call=100):
    """Slope of a straight line through the energies, kcal/mol per atom per ns (1 fs steps)."""
    t = np.arange(len(energies)) * call * 1e-6
    return float(np.polyfit(t, np.asarray(energies), 1)[0] / natoms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nside", type=int, default=32)
    ap.add_argument("--steps", type=int, default=500)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--frequency", type=int, default=10)
    ap.add_argument("--tau", type=float, default=0.1)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    th = VelocityRescale(300.0, tau=args.tau, frequency=args.frequency, seed=1)
    mol, s_nve, f_nve, i_nve = setup(args.nside, None)
    _, s_th, f_th, i_th = setup(args.nside, th)
    for integ in (i_nve, i_th):  # warm-up: code objects, list capacity
        integ.step(200)
    e_nve, e_th, nve, csvr = [], [], [], []
    for _ in range(args.rounds):
        nve.append(timed(i_nve, args.steps, e_nve))
        csvr.append(timed(i_th, args.steps, e_th, heat=th.heat))
    # one application alone: a third thermostat on a copy of the velocities (the run above is not disturbed)
    alone = VelocityRescale(300.0, tau=args.tau, frequency=args.frequency, seed=2)
    twin = type("S", (), {"vel": s_th.vel.clone()})()
    alone.apply(twin, i_th.masses, i_th.dt, 3 * mol.numAtoms)
    napply, per_apply = 200, []
    for _ in range(args.rounds):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(napply):
            alone.apply(twin, i_th.masses, i_th.dt, 3 * mol.numAtoms)
        torch.cuda.synchronize()
        per_apply.append((time.perf_counter() - t0) / napply * 1e6)
    out = {
        "natoms": mol.numAtoms, "device": torch.cuda.get_device_name(0), "frequency": args.frequency, "tau_ps": args.tau,
        "us_per_step_nve": [round(v, 2) for v in nve], "us_per_step_thermostat": [round(v, 2) for v in csvr],
        "us_per_step_nve_median": round(float(np.median(nve)), 2), "us_per_step_thermostat_median": round(float(np.median(csvr)), 2),
        "us_per_application_alone": [round(v, 2) for v in per_apply],
        "applications": th.applications, "heat_kcal_mol": round(float(th.heat()[0]), 3),
        "drift_nve_kcal_mol_atom_ns": round(drift(e_nve, mol.numAtoms), 4),
        "drift_conserved_kcal_mol_atom_ns": round(drift(e_th, mol.numAtoms), 4),
        "T_last_K": round(float(i_th._temperature(np.asarray(th.last[:, 2].cpu().numpy()))[0]), 2),
    }
    print(json.dumps(out))


if __name__ == "__main__":
    main()
