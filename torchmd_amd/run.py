"""MD driver with the reference's configuration surface (`torchmd/run.py:30-144`: same option names,
`--conf file.yaml`), built on this package's readers instead of moleculekit:

    python -m torchmd_amd.run --conf tests/water/water_conf.yaml [--device cuda:0] [--steps N]

Inputs: `structure: [file.psf, file.pdb]` (CHARMM) or `topology: file.prmtop` + `coordinates:
file.coor|.pdb` + `extended_system: file.xsc` (AMBER), `forcefield: *.yaml | *.prmtop`.
Outputs like the reference (`run.py:230-291`): `monitor_{k}.csv` (iter, ns, epot, ekin, etot, T, t),
`{output}_{k}.npy` trajectory `[N,3,frames]`, `input.yaml` echo.  Frames are staged through a pinned
host ring with asynchronous copies instead of a blocking `.cpu()` per period.
With `barostat_pressure` set (constant pressure) the box edges of every frame are saved as
`{output}_box_{k}.npy` `[frames,3]` and the monitor file gains a `volume` column; `barostat: crescale` (with `barostat_tau` in ps
and `barostat_compressibility` in 1/bar) replaces the Monte Carlo barostat by stochastic cell rescaling on the virial (DESIGN
§20), which also runs on a thermostat ladder.  With `exchange_frequency` set (temperature
replica exchange on the ladder of `thermostat: csvr`) every monitor file gains a `rung` column — the rung of the
ladder the replica slot holds at that row — and the acceptance counts are written to `exchange.json` at the end.  With
`restraints: file.npz` (harmonic position and distance restraints; arrays named as the fields of
tmdhip_restraint_desc without `_host`, per-replica leading axes optional) every monitor file gains a `restraints` column: the
restraint energy that `epot` contains.  With `group_restraints: file.npz` (restraints on the distance, angle and dihedral
between centres of groups of atoms; arrays group_off, member_atom, optionally member_weight, kind, groups, target, k,
optionally flat) every monitor file gains a `group_restraints` column likewise, and the start configuration is checked for groups
that are not whole.  With a `metadynamics:` mapping (the arguments of `metadynamics.Metadynamics`: cvs, sigma,
height, frequency, temperature, bias_factor, grid_min, grid_max, grid_bins, walkers) every monitor file gains a `bias`
column (V(s(x)), inside `epot`) and one column per CV (`cv0`, `cv1`), and the hills log and the grid are written to
`{output}_hills.npy` `[n,R,ncv+1]` and `{output}_bias_grid.npz` at the end.
With `implicit_solvent: obc2` (the generalized-Born / surface-area model of DESIGN §21, open boundaries only; optional
`gb_radii: file.npy` and `gb_scale: file.npy` replace the default tables, `solvent_dielectric` and `surface_tension` the default
78.5 and 0.0054 kcal/mol/A^2) every monitor file gains an `implicit_solvent` column: the GB + SA energy that `epot` contains.
With an `alchemical:` mapping (atoms, lambda_vdw, lambda_elec, alpha, and optionally states: [[lambda_vdw, lambda_elec], ...];
DESIGN §22) every monitor file gains the columns `alchemical` (the cross + intra energy inside `epot`), `dudl_vdw` and `dudl_elec`, and
with `states` the cross energy of every saved frame at those couplings is written to `{output}_states_{k}.npy` `[frames, K]`.
With `pressure: true` every monitor file gains a `pressure` column (bar): the instantaneous pressure of the force field from the
molecular virial, evaluated when a monitor row is written, with or without `barostat_pressure`.
With a `hamiltonian_exchange:` mapping (frequency, seed, temperature, keep_matrices; not together with
`exchange_frequency`) the replicas trade their alchemical couplings and restraint tables: every monitor file gains a `state`
column — the state the replica slot holds at that row — the acceptance counts are written to `hamiltonian_exchange.json`, and
with `keep_matrices` the reduced cross energies of every attempt to `hrex_u.npy` `[nattempts, R, R]` (slot, state) and the
assignment after it to `hrex_states.npy` `[nattempts, R]`.
"""

from __future__ import annotations

import argparse
import csv
import json
import os
import time

import numpy as np
import torch
import yaml

from . import io as tio
from .forcefields import ForceField
from .forces import Forces, active_side_terms
from .integrator import BOLTZMAN, Integrator, maxwell_boltzmann
from .minimizers import minimize_bfgs, minimize_fire
from .utils import LogWriter
from .parameters import Parameters
from .systems import System
from .wrapper import Wrapper

FS2NS = 1e-6
PRECISION = {"single": torch.float, "double": torch.double}

DEFAULTS = dict(
    timestep=1.0, temperature=300.0, langevin_temperature=0.0, langevin_gamma=0.1, device="cuda:0",
    structure=None, topology=None, coordinates=None, forcefield=None, seed=1, output_period=10,
    save_period=0, steps=10000, log_dir="./", output="output", forceterms=["LJ"], cutoff=None,
    switch_dist=None, precision="single", external=None, rfa=False, replicas=1, extended_system=None,
    minimize=None, exclusions=("bonds", "angles", "1-4"), pme=False, ewald_tolerance=5e-4, pme_order=5, pme_grid=None,
    constraints=None,  # None, "water" (rigid waters) or "hbonds" (rigid waters and X-H bonds): DESIGN §10
    barostat_pressure=None,  # bar; None: constant volume.  Monte Carlo barostat at langevin_temperature: DESIGN §11
    barostat_frequency=25,  # steps between two volume moves
    barostat="montecarlo",  # with barostat_pressure set: "montecarlo"  or "crescale" (stochastic cell rescaling on the virial: DESIGN §20)
    barostat_tau=1.0,  # ps: the relaxation time of barostat: crescale
    barostat_compressibility=4.5e-5,  # 1/bar: the isothermal compressibility barostat: crescale assumes (water)
    minimizer="bfgs",  # what `minimize: N` runs: "bfgs" (scipy L-BFGS-B, one replica) or "fire" (on the device, every replica): DESIGN §13
    thermostat=None,  # None or "csvr": stochastic velocity rescaling between batches of steps (instead of Langevin): DESIGN §14
    thermostat_tau=0.1,  # ps; 0 resamples the kinetic energy at every application
    thermostat_frequency=10,  # steps between two applications
    thermostat_temperature=None,  # K: a number, or a list with one target per replica; None: `temperature`
    remove_com=True,  # the thermostat also takes out the centre-of-mass motion
    exchange_frequency=None,  # steps between two replica-exchange attempts; None: none.  Needs thermostat: csvr with a list: DESIGN §16
    exchange_seed=None,  # seed of the exchange's random stream; None: drawn from torch's generator (so `seed` reproduces it)
    hamiltonian_exchange=None,  # None or a mapping {frequency, seed, temperature, keep_matrices}: replicas trade couplings / windows: DESIGN §24
    restraints=None,  # None or an .npz file: harmonic position / distance restraints (pos_atom, pos_ref, pos_k, dist_pair, dist_r0, dist_k): DESIGN §17
    group_restraints=None,  # None or an .npz file: restraints between centres of groups of atoms (group_off, member_atom, kind, groups, target, k, flat): DESIGN §25
    metadynamics=None,  # None or a mapping with the arguments of metadynamics.Metadynamics (cvs: [[kind, [atoms]], ...], ["group_distance", [[...], [...]]], ["coordination", [[...], [...]], {r0, n, d0, d_max}]; an atom list may be an .npy file): DESIGN §18, §26
    pressure=False,  # True: every monitor file gains a `pressure` column (bar): the instantaneous pressure from the molecular virial: DESIGN §19
    alchemical=None,  # None or a mapping with the arguments of alchemy.Alchemical (atoms, lambda_vdw, lambda_elec, alpha) and `states`: DESIGN §22
    implicit_solvent=None,  # None or "obc2": generalized-Born / surface-area implicit solvent, open boundaries only: DESIGN §21
    gb_radii=None,  # None (the defaults of GeneralizedBorn.from_parameters) or an .npy file with one intrinsic radius per atom (A)
    gb_scale=None,  # None or an .npy file with one descreening scale per atom
    solvent_dielectric=78.5,  # of implicit_solvent
    surface_tension=0.0054,  # kcal/mol/A^2, of implicit_solvent; 0: no surface-area term
    virtual_sites=None,  # None or "tip4p": four-site waters O,H1,H2,M; geometry from the force field's `virtual_sites` section: DESIGN §12
)


def get_args(arguments=None):
    ap = argparse.ArgumentParser(description="TorchMD on MI355X (torchmd_amd)")
    ap.add_argument("--conf", default=None, help="YAML configuration file (same keys as the options)")
    for key, val in DEFAULTS.items():
        opt = "--" + key.replace("_", "-")
        if isinstance(val, bool):
            ap.add_argument(opt, dest=key, action="store_true", default=None)
        elif key in ("forceterms", "structure"):
            ap.add_argument(opt, dest=key, nargs="+", default=None)
        elif key in ("external", "exclusions", "pme_grid", "metadynamics", "hamiltonian_exchange"):
            continue
        else:
            ap.add_argument(opt, dest=key, default=None, type=type(val) if val is not None else str)
    ns = ap.parse_args(arguments)
    cfg = dict(DEFAULTS)
    if ns.conf:
        with open(ns.conf) as fh:
            cfg.update({k: v for k, v in (yaml.safe_load(fh) or {}).items()})
    cfg.update({k: v for k, v in vars(ns).items() if k != "conf" and v is not None})
    args = argparse.Namespace(**cfg)
    for k in ("cutoff", "switch_dist", "timestep", "temperature", "langevin_temperature", "langevin_gamma"):
        if getattr(args, k) is not None:
            setattr(args, k, float(getattr(args, k)))
    args.ewald_tolerance = float(args.ewald_tolerance)
    args.pme = bool(args.pme)
    args.pressure = args.pressure.lower() in ("true", "yes", "1") if isinstance(args.pressure, str) else bool(args.pressure)
    if isinstance(args.constraints, str) and args.constraints.lower() in ("none", "null", ""):
        args.constraints = None
    if args.constraints not in (None, "water", "hbonds"):
        raise ValueError(f"constraints must be None, 'water' or 'hbonds', got {args.constraints!r}")
    if isinstance(args.virtual_sites, str) and args.virtual_sites.lower() in ("none", "null", ""):
        args.virtual_sites = None
    if args.virtual_sites not in (None, "tip4p"):
        raise ValueError(f"virtual_sites must be None or 'tip4p', got {args.virtual_sites!r}")
    args.minimizer = str(args.minimizer).lower()
    if args.minimizer not in ("bfgs", "fire"):
        raise ValueError(f"minimizer must be 'bfgs' or 'fire', got {args.minimizer!r}")
    if isinstance(args.barostat_pressure, str) and args.barostat_pressure.lower() in ("none", "null", ""):
        args.barostat_pressure = None
    if args.barostat_pressure is not None:
        args.barostat_pressure = float(args.barostat_pressure)
    args.barostat_frequency = int(args.barostat_frequency)
    if args.barostat_frequency < 1:
        raise ValueError(f"barostat_frequency must be a positive number of steps, got {args.barostat_frequency}")
    args.barostat = str(args.barostat).lower()
    if args.barostat not in ("montecarlo", "crescale"):
        raise ValueError(f"barostat must be 'montecarlo' or 'crescale', got {args.barostat!r}")
    args.barostat_tau = float(args.barostat_tau)
    args.barostat_compressibility = float(args.barostat_compressibility)
    if isinstance(args.thermostat, str) and args.thermostat.lower() in ("none", "null", ""):
        args.thermostat = None
    if args.thermostat is not None:
        args.thermostat = str(args.thermostat).lower()
        if args.thermostat != "csvr":
            raise ValueError(f"thermostat must be None or 'csvr', got {args.thermostat!r}")
        if args.langevin_temperature:
            raise ValueError("thermostat: csvr replaces the Langevin thermostat: leave langevin_temperature at 0")
    args.thermostat_tau = float(args.thermostat_tau)
    args.thermostat_frequency = int(args.thermostat_frequency)
    if isinstance(args.thermostat_temperature, str):
        tt = [float(v) for v in args.thermostat_temperature.replace(",", " ").split()]
        args.thermostat_temperature = tt[0] if len(tt) == 1 else tt
    elif isinstance(args.thermostat_temperature, (list, tuple)):
        args.thermostat_temperature = [float(v) for v in args.thermostat_temperature]
    elif args.thermostat_temperature is not None:
        args.thermostat_temperature = float(args.thermostat_temperature)
    for k in ("exchange_frequency", "exchange_seed"):
        v = getattr(args, k)
        if isinstance(v, str) and v.lower() in ("none", "null", ""):
            v = None
        setattr(args, k, int(v) if v is not None else None)
    if args.exchange_frequency is not None:
        if args.exchange_frequency < 1:
            raise ValueError(f"exchange_frequency must be a positive number of steps, got {args.exchange_frequency}")
        if args.thermostat != "csvr" or not isinstance(args.thermostat_temperature, list):
            raise ValueError("exchange_frequency needs thermostat: csvr with a list as thermostat_temperature (the ladder)")
    if isinstance(args.hamiltonian_exchange, str) and args.hamiltonian_exchange.lower() in ("none", "null", ""):
        args.hamiltonian_exchange = None
    if args.hamiltonian_exchange is not None:
        hx = args.hamiltonian_exchange
        if not isinstance(hx, dict):
            raise ValueError("hamiltonian_exchange must be a mapping (frequency, seed, temperature, keep_matrices)")
        unknown = set(hx) - {"frequency", "seed", "temperature", "keep_matrices"}
        if unknown:
            raise ValueError(f"hamiltonian_exchange: unknown keys {sorted(unknown)}")
        if args.exchange_frequency is not None:
            raise ValueError("hamiltonian_exchange and exchange_frequency are two exchanges: give one of them")
    if isinstance(args.restraints, str) and args.restraints.lower() in ("none", "null", ""):
        args.restraints = None
    if isinstance(args.group_restraints, str) and args.group_restraints.lower() in ("none", "null", ""):
        args.group_restraints = None
    if isinstance(args.metadynamics, str) and args.metadynamics.lower() in ("none", "null", ""):
        args.metadynamics = None
    if args.metadynamics is not None and not isinstance(args.metadynamics, dict):
        raise ValueError("metadynamics must be a mapping with the arguments of Metadynamics (cvs, sigma, height, frequency, ...)")
    if isinstance(args.alchemical, str):
        args.alchemical = None if args.alchemical.lower() in ("none", "null", "") else yaml.safe_load(args.alchemical)
    if args.alchemical is not None and not isinstance(args.alchemical, dict):
        raise ValueError("alchemical must be a mapping with the arguments of Alchemical (atoms, lambda_vdw, lambda_elec, alpha, states)")
    for k in ("implicit_solvent", "gb_radii", "gb_scale"):
        if isinstance(getattr(args, k), str) and getattr(args, k).lower() in ("none", "null", ""):
            setattr(args, k, None)
    if args.implicit_solvent is not None:
        args.implicit_solvent = str(args.implicit_solvent).lower()
        if args.implicit_solvent != "obc2":
            raise ValueError(f"implicit_solvent must be None or 'obc2', got {args.implicit_solvent!r}")
    args.solvent_dielectric = float(args.solvent_dielectric)
    args.surface_tension = float(args.surface_tension)
    if isinstance(args.remove_com, str):
        args.remove_com = args.remove_com.lower() not in ("false", "0", "no", "off")
    args.remove_com = bool(args.remove_com)
    if args.pme_grid is not None:
        args.pme_grid = tuple(int(v) for v in args.pme_grid)
    for k in ("steps", "output_period", "save_period", "replicas", "seed", "pme_order"):
        setattr(args, k, int(getattr(args, k)))
    if isinstance(args.forceterms, str):
        args.forceterms = [args.forceterms]
    if args.forceterms is None:
        args.forceterms = []
    if str(args.device) == "cuda":
        args.device = "cuda:0"
    if args.steps % args.output_period != 0:
        raise ValueError("Steps must be multiple of output-period.")
    if args.save_period == 0:
        args.save_period = 10 * args.output_period
    if args.save_period % args.output_period != 0:
        raise ValueError("save-period must be multiple of output-period.")
    os.makedirs(args.log_dir, exist_ok=True)
    with open(os.path.join(args.log_dir, "input.yaml"), "w") as fh:
        yaml.safe_dump({k: (list(v) if isinstance(v, tuple) else v) for k, v in vars(args).items()}, fh)
    return args


def load_molecule(args):
    """Topology + coordinates + box from the file kinds the reference's configs use."""
    files = []
    for f in (args.topology, args.structure, args.coordinates, args.extended_system):
        if f is None:
            continue
        files += list(f) if isinstance(f, (list, tuple)) else [f]
    mol, coords, box, prmtop = None, None, np.zeros(3), None
    for f in files:
        ext = os.path.splitext(f)[1].lower()
        if ext == ".psf":
            mol = tio.read_psf(f)
        elif ext in (".prmtop", ".parm7"):
            mol, prmtop = tio.read_prmtop(f)
        elif ext == ".pdb":
            xyz, pbox, names, elems = tio.read_pdb(f)
            coords = xyz.astype(np.float64)
            if np.any(pbox != 0):
                box = pbox.astype(np.float64)
            if mol is not None and mol.element is None:
                mol.element = elems
        elif ext == ".coor":
            coords = tio.read_namd_coor(f)
        elif ext == ".xsc":
            box = tio.read_xsc(f)
        else:
            raise RuntimeError(f"unsupported input file '{f}'")
    if mol is None or coords is None:
        raise RuntimeError("need a topology (.psf / .prmtop) and coordinates (.pdb / .coor)")
    if len(coords) != mol.numAtoms:
        raise RuntimeError("coordinate and topology atom counts differ")
    mol.coords = coords[:, :, None].astype(np.float32)
    mol.box = np.asarray(box, dtype=np.float64)
    if mol.element is None:
        mol.element = np.array([str(n)[:1] for n in (mol.name if mol.name is not None else mol.atomtype)], dtype=object)
    return mol, prmtop


def load_external(conf, replicas, device):
    """The reference's plugin hook (`torchmd/run.py:185-209`): `conf = {module, file, embeddings, ...}` ->
    `import_module(module).External(file, embeddings, device=device, **rest)`; `embeddings` is a list or the
    name of a `.npy` file, repeated per replica.  The object's `calculate(pos, box)` must return
    `(energy[R], forces[R,N,3])` (consumed by `Forces.compute`, reference `forces.py:321-326`)."""
    if conf is None:
        return None
    import importlib

    conf = dict(conf)
    try:
        module, file = conf.pop("module"), conf.pop("file")
    except KeyError as e:
        raise ValueError(f"external: missing key {e.args[0]!r} (needs 'module' and 'file')") from None
    emb = conf.pop("embeddings", None)
    if isinstance(emb, str):
        emb = np.load(emb).astype(int)
    embeddings = None if emb is None else torch.tensor(emb).repeat(replicas, 1)
    return importlib.import_module(module).External(file, embeddings, device=device, **conf)


def setup(args):
    torch.manual_seed(args.seed)
    device = torch.device(args.device)
    mol, prmtop = load_molecule(args)
    precision = PRECISION[args.precision]
    ff_src = args.forcefield
    if prmtop is not None and (ff_src is None or str(ff_src).endswith((".prmtop", ".parm7"))):
        from .forcefields import PrmtopForceField

        ff = PrmtopForceField(mol, prmtop)
    else:
        ff = ForceField.create(mol, ff_src)
    terms = args.forceterms if args.forceterms else ["bonds", "angles", "dihedrals", "impropers", "1-4", "electrostatics", "lj"]
    print("Force terms: ", terms)
    parameters = Parameters(ff, mol, terms, precision=precision, device=device)  # (on the device, as run.py:181-183 does)
    external = load_external(args.external, args.replicas, device)
    system = System(mol.numAtoms, args.replicas, precision, device)
    system.set_positions(mol.coords)
    system.set_box(mol.box)
    vel = maxwell_boltzmann(parameters.masses, args.temperature, args.replicas)
    vsites = None
    if args.virtual_sites == "tip4p":
        vsites = tip4p_sites(ff, mol)
        vel[:, torch.as_tensor(vsites.sites, dtype=torch.long)] = 0.0  # (massless: the draw divided by zero)
    system.set_velocities(vel)
    extra = {} if vsites is None else {"virtual_sites": vsites}
    if args.restraints is not None:
        from .restraints import Restraints

        extra["restraints"] = Restraints.from_npz(args.restraints, args.replicas)
    if args.metadynamics is not None:
        from .metadynamics import Metadynamics

        extra["metadynamics"] = Metadynamics.from_config(args.metadynamics, args.replicas)
    if args.implicit_solvent is not None:
        from .implicit import GeneralizedBorn

        kw = dict(solvent_dielectric=args.solvent_dielectric, surface_tension=args.surface_tension)
        gb = GeneralizedBorn.from_parameters(parameters, **kw)
        if args.gb_radii is not None or args.gb_scale is not None:
            gb = GeneralizedBorn(np.load(args.gb_radii) if args.gb_radii is not None else gb.radii,
                                 np.load(args.gb_scale) if args.gb_scale is not None else gb.scale, **kw)
        extra["implicit_solvent"] = gb
    if args.alchemical is not None:
        from .alchemy import Alchemical

        extra["alchemical"] = Alchemical.from_config(args.alchemical)
    if args.group_restraints is not None:
        from .group_restraints import GroupRestraints

        extra["group_restraints"] = GroupRestraints.from_npz(args.group_restraints, args.replicas)
    forces = Forces(parameters, terms=terms, external=external, cutoff=args.cutoff, rfa=args.rfa,
                    switch_dist=args.switch_dist, exclusions=tuple(args.exclusions), pme=args.pme,
                    ewald_tolerance=args.ewald_tolerance, pme_order=args.pme_order, pme_grid=args.pme_grid, **extra)
    if forces.group_restraints is not None and not forces.group_restraints.check_extent(
            system.pos.detach().cpu().numpy(), torch.diagonal(system.box, dim1=-2, dim2=-1).detach().cpu().numpy()):
        raise ValueError("group_restraints: an atom of a group lies half a box edge or more from the group's first atom "
                         "(make the groups whole before the run)")
    if forces.metadynamics is not None and forces.metadynamics.grouped:
        hbox = torch.diagonal(system.box, dim1=-2, dim2=-1).detach().cpu().numpy()
        forces.metadynamics.check_box(hbox, R=hbox.shape[0])
        if not forces.metadynamics.check_extent(system.pos.detach().cpu().numpy(), hbox):
            raise ValueError("metadynamics: an atom of a group of a centre CV lies half a box edge or more from the group's first "
                             "atom (make the groups whole before the run)")
    return mol, system, forces


def tip4p_sites(ff, mol):
    """`virtual_sites: tip4p` — the M sites of a system of four-site waters (atom order O,H1,H2,M), with the geometry the
    force-field file states: `virtual_sites: {tip4p: {r_om: ..., r_oh: ..., theta: ...}}` (Angstrom, degrees)."""
    from .vsites import VirtualSites

    geo = ((getattr(ff, "prm", None) or {}).get("virtual_sites") or {}).get("tip4p")
    if not geo or not all(k in geo for k in ("r_om", "r_oh", "theta")):
        raise ValueError("virtual_sites: tip4p needs a `virtual_sites: {tip4p: {r_om, r_oh, theta}}` section in the force-field file")
    return VirtualSites.tip4p(mol, geo["r_om"], geo["r_oh"], geo["theta"])


class FrameStager:
    """Trajectory frames leave the device through a pinned host ring with asynchronous copies on a side
    stream; the step loop never blocks on them (the reference does a blocking `.cpu()` each period and
    re-saves the whole trajectory with np.save, `run.py:267-274`)."""

    def __init__(self, system, nframes):
        R, N = system.pos.shape[0], system.pos.shape[1]
        self.buf = torch.empty((nframes, R, N, 3), dtype=system.pos.dtype).pin_memory()
        self.stream = torch.cuda.Stream(device=system.pos.device)
        self.events = []
        self.count = 0

    def push(self, pos):
        snap = pos.detach().clone()  # the integrator keeps mutating pos
        ready = torch.cuda.Event()   # recorded AFTER the clone: the side stream's copy must see the snapshot
        ready.record(torch.cuda.current_stream(pos.device))
        with torch.cuda.stream(self.stream):
            self.stream.wait_event(ready)
            self.buf[self.count].copy_(snap, non_blocking=True)
            done = torch.cuda.Event()
            done.record(self.stream)
        snap.record_stream(self.stream)
        self.events.append(done)
        self.count += 1

    def frames(self, replica):
        """[N,3,frames] numpy array of the frames copied so far (reference layout)."""
        for ev in self.events:
            ev.synchronize()
        return np.ascontiguousarray(self.buf[: self.count, replica].numpy().transpose(1, 2, 0))


def dynamics(args, mol, system, forces):
    torch.manual_seed(args.seed)
    device = torch.device(args.device)
    barostat = thermostat = exchange = None
    if args.thermostat is not None:
        from .thermostat import VelocityRescale

        target = args.thermostat_temperature if args.thermostat_temperature is not None else args.temperature
        thermostat = VelocityRescale(target, tau=args.thermostat_tau, frequency=args.thermostat_frequency,
                                     remove_com=args.remove_com)
    if args.barostat_pressure is not None and args.barostat == "crescale":
        from .crescale import CRescaleBarostat

        bath = thermostat.targets(args.replicas) if thermostat is not None else args.langevin_temperature
        if thermostat is None and not bath:
            raise ValueError("barostat: crescale needs a thermostat: set langevin_temperature, or thermostat: csvr")
        barostat = CRescaleBarostat(args.barostat_pressure, bath, tau=args.barostat_tau, compressibility=args.barostat_compressibility,
                                    frequency=args.barostat_frequency)
    elif args.barostat_pressure is not None:
        from .barostat import MonteCarloBarostat

        bath = thermostat.temperature if thermostat is not None else args.langevin_temperature
        if not bath:
            raise ValueError("barostat_pressure needs a thermostat at one temperature: set langevin_temperature, or "
                             "thermostat: csvr with a single thermostat_temperature")
        barostat = MonteCarloBarostat(args.barostat_pressure, bath, args.barostat_frequency)
    extra = {} if barostat is None else {"barostat": barostat}
    thermostat_ladder = list(thermostat.temperatures) if thermostat is not None else []  # (before any exchange permutes it)
    if args.exchange_frequency is not None:
        from .exchange import ReplicaExchange

        exchange = extra["exchange"] = ReplicaExchange(args.exchange_frequency, seed=args.exchange_seed)
    hrex = None
    if args.hamiltonian_exchange is not None:
        from .hrex import HamiltonianExchange

        hx = args.hamiltonian_exchange
        hrex = extra["exchange"] = HamiltonianExchange(hx.get("frequency", 500), temperature=hx.get("temperature"), seed=hx.get("seed"),
                                                       keep_matrices=bool(hx.get("keep_matrices", False)))
    if thermostat is not None:
        integrator = Integrator(system, forces, args.timestep, device, constraints=args.constraints, thermostat=thermostat, **extra)
    else:
        integrator = Integrator(system, forces, args.timestep, device, gamma=args.langevin_gamma,
                                T=args.langevin_temperature, constraints=args.constraints, **extra)
    wrapper = Wrapper(mol.numAtoms, mol.bonds if len(mol.bonds) else None, device)
    nper = args.steps // args.output_period
    stager = FrameStager(system, nper)
    columns = ("iter", "ns", "epot", "ekin", "etot", "T") + (("volume",) if barostat is not None else ())
    columns += ("pressure",) if args.pressure else ()
    columns += ("rung",) if exchange is not None else ()
    columns += ("state",) if hrex is not None else ()
    # each side term adds its columns: what of its energy `epot` contains, as of the last evaluation (the bias and its CVs last,
    # where the monitor files have always had them)
    side_terms = sorted(active_side_terms(forces), key=lambda t: t.side_name == "metadynamics")
    for term in side_terms:
        columns += term.monitor_columns()
    alch = getattr(forces, "alchemical", None)
    states = np.asarray(args.alchemical["states"], dtype=np.float64).reshape(-1, 2) if (alch is not None and args.alchemical.get("states")) else None
    foreign = []  # [frames][R, K] cross energies at `states`
    metad = getattr(forces, "metadynamics", None)
    logs = [LogWriter(args.log_dir, columns, name=f"monitor_{k}.csv") for k in range(args.replicas)]
    boxes = []  # [frames][R,3] box edges, constant-pressure runs only
    if args.minimize is not None:
        if args.minimizer == "fire":
            minimize_fire(system, forces, steps=int(args.minimize))
        else:
            minimize_bfgs(system, forces, steps=int(args.minimize))
    forces.compute(system.pos, system.box, system.forces)
    name, ext = os.path.splitext(args.output)
    t0 = time.time()
    for i in range(1, nper + 1):
        Ekin, Epot, T = integrator.step(niter=args.output_period)
        wrapper.wrap(system.pos, system.box)
        stager.push(system.pos)
        if barostat is not None:
            boxes.append(torch.diagonal(system.box, dim1=-2, dim2=-1).to("cpu", torch.float64).numpy().copy())
        pressure = integrator.pressure() if args.pressure else None  # (of the wrapped positions: molecules are whole)
        if states is not None:
            foreign.append(forces.alchemical_energies(system.pos, system.box, states))
        for k in range(args.replicas):
            if (i * args.output_period) % args.save_period == 0 or i == nper:
                np.save(os.path.join(args.log_dir, f"{name}_{k}{ext or '.npy'}"), stager.frames(k))
                if barostat is not None:
                    np.save(os.path.join(args.log_dir, f"{name}_box_{k}{ext or '.npy'}"), np.stack([b[k] for b in boxes]))
                if states is not None:
                    np.save(os.path.join(args.log_dir, f"{name}_states_{k}.npy"), np.stack([e[k] for e in foreign]))
            row = {"iter": i * args.output_period, "ns": FS2NS * i * args.output_period * args.timestep,
                   "epot": Epot[k], "ekin": float(Ekin[k]), "etot": Epot[k] + float(Ekin[k]), "T": float(T[k])}
            if barostat is not None:
                row["volume"] = float(np.prod(boxes[-1][k]))
            if pressure is not None:
                row["pressure"] = float(pressure[k])
            if exchange is not None:
                row["rung"] = int(exchange.rungs[k]) if exchange.rungs is not None else k
            if hrex is not None:
                row["state"] = int(hrex.states[k])
            for term in side_terms:
                row.update(term.monitor_row(k))
            logs[k].write_row(row)
    wall = time.time() - t0
    if metad is not None:
        np.save(os.path.join(args.log_dir, f"{name}_hills.npy"), metad.hills())
        metad.save(os.path.join(args.log_dir, f"{name}_bias_grid.npz"))
    if exchange is not None:
        with open(os.path.join(args.log_dir, "exchange.json"), "w") as fh:
            none = exchange.rungs is None  # (no attempt was made: the run was shorter than exchange_frequency)
            json.dump({"frequency": exchange.frequency, "seed": exchange.seed, "temperatures": [float(t) for t in thermostat_ladder],
                       "attempts": [] if none else exchange.attempts.tolist(), "accepted": [] if none else exchange.accepted.tolist(),
                       "rungs": list(range(args.replicas)) if none else exchange.rungs.tolist()}, fh)
    if hrex is not None:
        with open(os.path.join(args.log_dir, "hamiltonian_exchange.json"), "w") as fh:
            json.dump({"frequency": hrex.frequency, "seed": hrex.seed, "temperature": 1.0 / (BOLTZMAN * hrex.beta),
                       "attempts": hrex.attempts.tolist(), "accepted": hrex.accepted.tolist(), "states": hrex.states.tolist()}, fh)
        if hrex.keep_matrices:
            R = args.replicas
            np.save(os.path.join(args.log_dir, "hrex_u.npy"), np.asarray(hrex.matrices, dtype=np.float64).reshape(-1, R, R))
            np.save(os.path.join(args.log_dir, "hrex_states.npy"), np.asarray(hrex.history, dtype=np.int64).reshape(-1, R))
    print(f"{args.steps} steps in {wall:.2f} s = {args.steps * args.timestep * FS2NS / wall * 86400:.1f} ns/day per replica")
    return stager


def main(arguments=None):
    args = get_args(arguments)
    mol, system, forces = setup(args)
    dynamics(args, mol, system, forces)


if __name__ == "__main__":
    main()
