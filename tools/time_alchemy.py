"""Cost of the alchemical solute on the 98 304-atom TIP3P box (fp32, cutoff 9 A with reaction field, Langevin): us/step of
step(100) without `alchemical=` and with 10 and with 100 neighbouring waters (30 and 300 atoms) decoupling at lambda_vdw = 0.5, with the bounding-sphere early-outs forced
on and off (TMDHIP_ALCHEMY_SPHERE), one application alone, and the time of one alchemical_energies() call at 11 states; the median of
5 with the legs alternated.  Figures for DESIGN §22: measurements, not targets."""
import os, sys, time
R = os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."); sys.path.insert(0, R)
import numpy as np, torch
from torchmd_amd import Alchemical
from torchmd_amd.builders import tip3p_box, water_forcefield
from torchmd_amd.forces import Forces
from torchmd_amd.integrator import Integrator, maxwell_boltzmann
from torchmd_amd.parameters import Parameters
from torchmd_amd.systems import System
dev = torch.device("cuda:0")
terms = ["lj", "electrostatics", "bonds", "angles"]
mol, pos, box = tip3p_box(32, seed=0)
par = Parameters(water_forcefield(mol), mol, terms, precision=torch.float32)
ox = np.arange(0, len(pos), 3)
by_distance = ox[np.argsort(np.linalg.norm(pos[ox] - box / 2, axis=1))]


def make(name, solute):
    if name != "plain":
        os.environ["TMDHIP_ALCHEMY_SPHERE"] = "0" if name == "no_sphere" else "1"
    s = System(mol.numAtoms, 1, torch.float32, dev); s.set_positions(pos[:, :, None]); s.set_box(box)
    torch.manual_seed(1); s.set_velocities(maxwell_boltzmann(par.masses, 300.0, 1))
    kw = {} if name == "plain" else {"alchemical": Alchemical(solute, 0.5, 0.0)}
    f = Forces(par, terms=terms, cutoff=9.0, rfa=True, **kw)
    f.compute(s.pos, s.box, s.forces)
    integ = Integrator(s, f, 1.0, dev, gamma=0.1, T=300.0)
    integ.step(100)
    return s, f, integ


states = np.stack([np.linspace(0.0, 1.0, 11), np.zeros(11)], axis=1)
for nwat in (10, 100):  # neighbouring waters around the box centre: solutes of 30 and 300 atoms
    near = by_distance[:nwat]
    solute = np.sort(np.concatenate([near, near + 1, near + 2]))
    legs = {name: make(name, solute) for name in ("plain", "sphere", "no_sphere")}
    ts = {k: [] for k in legs}
    rebuilds = {k: legs[k][1].stats(legs[k][0].pos)["n_rebuilds"] for k in legs}
    for rep in range(5):
        for name, (s, f, integ) in legs.items():
            torch.cuda.synchronize(); t0 = time.perf_counter(); integ.step(100); torch.cuda.synchronize()
            ts[name].append((time.perf_counter() - t0) / 100)
    for name, (s, f, integ) in legs.items():
        nb = f.stats(s.pos)["n_rebuilds"] - rebuilds[name]
        print(f"98 304 atoms fp32, solute {3 * nwat} atoms, {name}: step(100) {np.median(ts[name]) * 1e6:.1f} us/step "
              f"(min {min(ts[name]) * 1e6:.1f}, max {max(ts[name]) * 1e6:.1f}), {nb} list rebuilds in 500 steps")
    for name in ("sphere", "no_sphere"):
        s, f, _ = legs[name]
        eng = f._engine(s.pos)
        boxes = f._replica_boxes(s.box, 1)
        F = torch.zeros_like(s.pos)
        t = []
        for rep in range(5):  # the launches of one application alone (forces += F, no energies), back to back
            torch.cuda.synchronize(); t0 = time.perf_counter()
            for _ in range(100):
                eng.apply_side(f.alchemical, s.pos, boxes, F, False)
            torch.cuda.synchronize(); t.append((time.perf_counter() - t0) / 100)
        f.alchemical_energies(s.pos, s.box, states)
        te = []
        for rep in range(5):
            torch.cuda.synchronize(); t0 = time.perf_counter(); f.alchemical_energies(s.pos, s.box, states); te.append(time.perf_counter() - t0)
        print(f"solute {3 * nwat} atoms, {name}: one application {np.median(t) * 1e6:.1f} us, alchemical_energies at 11 states "
              f"{np.median(te) * 1e6:.1f} us per call")
    for _, f, _ in legs.values():
        f.close()
