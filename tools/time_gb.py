"""Cost of the generalized-Born implicit solvent on the thrombin golden (4 676 atoms, no cutoff, all seven terms): one
compute() and us/step of step(100), with and without implicit_solvent=, fp32 and fp64; the median of 5 with the two legs
alternated (off, on, off, on, ...).  Figures for DESIGN §21: measurements, not targets."""
import os, sys, time
R = os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."); sys.path.insert(0, R); sys.path.insert(0, os.path.join(R, "tests"))
import numpy as np, torch
from _golden import GoldenParameters, load
from torchmd_amd.forces import Forces
from torchmd_amd.implicit import GeneralizedBorn
from torchmd_amd.integrator import Integrator, maxwell_boltzmann
from torchmd_amd.systems import System
g = load("thrombin"); dev = torch.device("cuda:0")
pos = np.asarray(g["pos"], dtype=np.float64)
terms = ["bonds", "angles", "dihedrals", "impropers", "1-4", "electrostatics", "lj"]
for dt in (torch.float32, torch.float64):
    par = GoldenParameters(g, dt)
    legs = {}
    for name in ("off", "on"):
        s = System(pos.shape[0], 1, dt, dev); s.set_positions(pos[:, :, None]); s.set_box(np.zeros(3))
        torch.manual_seed(1); s.set_velocities(maxwell_boltzmann(par.masses, 300.0, 1))
        f = Forces(par, terms=terms, **({"implicit_solvent": GeneralizedBorn.from_parameters(par)} if name == "on" else {}))
        f.compute(s.pos, s.box, s.forces)
        integ = Integrator(s, f, 0.5, dev, gamma=1.0, T=300.0)
        integ.step(100)
        legs[name] = (s, f, integ)
    tc, ts = {"off": [], "on": []}, {"off": [], "on": []}
    for rep in range(5):
        for name in ("off", "on"):
            s, f, integ = legs[name]
            torch.cuda.synchronize(); t0 = time.perf_counter()
            for _ in range(20):
                f.compute(s.pos, s.box, s.forces)
            torch.cuda.synchronize(); tc[name].append((time.perf_counter() - t0) / 20)
            torch.cuda.synchronize(); t0 = time.perf_counter(); integ.step(100); torch.cuda.synchronize()
            ts[name].append((time.perf_counter() - t0) / 100)
    p = "fp64" if dt == torch.float64 else "fp32"
    for name in ("off", "on"):
        print(f"thrombin {p} implicit_solvent {name}: compute() {np.median(tc[name]) * 1e6:.1f} us (min {min(tc[name]) * 1e6:.1f}, max {max(tc[name]) * 1e6:.1f}), "
              f"step(100) {np.median(ts[name]) * 1e6:.1f} us/step (min {min(ts[name]) * 1e6:.1f}, max {max(ts[name]) * 1e6:.1f})")
    for _, f, _ in legs.values():
        f.close()
