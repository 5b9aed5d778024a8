"""torchmd_amd — MI355X-native (gfx950) nonbonded force/energy + integrator hot path for TorchMD.

Public surface mirrors the reference package for this path:
    torchmd_amd.forces.Forces, torchmd_amd.integrator.Integrator, torchmd_amd.systems.System,
    torchmd_amd.parameters.Parameters, torchmd_amd.forcefields.ForceField
plus `torchmd_amd.MonteCarloBarostat` (constant pressure) and `torchmd_amd.CRescaleBarostat` (constant pressure from the
virial: stochastic cell rescaling, one target per replica) and `torchmd_amd.VelocityRescale` (stochastic velocity
rescaling, one target temperature per replica) and `torchmd_amd.ReplicaExchange` / `torchmd_amd.temperature_ladder`
(temperature replica exchange on that thermostat's ladder) and `torchmd_amd.Restraints` (harmonic position and distance
restraints with one target per replica) and `torchmd_amd.Metadynamics` (well-tempered metadynamics on distance and
dihedral collective variables) and `torchmd_amd.GeneralizedBorn` (OBC2 generalized-Born / surface-area implicit solvent for
systems with open boundaries) and `torchmd_amd.Alchemical` (alchemical decoupling of a solute: soft-core pairs with one coupling
per replica, dU/dlambda and foreign energies) and `torchmd_amd.HamiltonianExchange` (replicas trade those couplings and the
restraints' windows) and `torchmd_amd.GroupRestraints` (restraints on the distance, angle and dihedral between centres of groups
of atoms, the Boresch set among them); all imported on first use only,
backed by hand-written HIP kernels in `torchmd_amd/lib/libtmdhip.so` (C ABI: include/tmdhip.h).
"""

from .forces import Forces
from .integrator import Integrator, kinetic_energy, kinetic_to_temp, maxwell_boltzmann
from .parameters import Parameters
from .systems import System



def __getattr__(name):
    # the barostat and thermostat modules are loaded on first use: a run without them never imports them
    if name == "MonteCarloBarostat":
        from .barostat import MonteCarloBarostat

        return MonteCarloBarostat
    if name == "CRescaleBarostat":
        from .crescale import CRescaleBarostat

        return CRescaleBarostat
    if name == "VelocityRescale":
        from .thermostat import VelocityRescale

        return VelocityRescale
    if name in ("ReplicaExchange", "temperature_ladder"):
        from . import exchange

        return getattr(exchange, name)
    if name == "HamiltonianExchange":
        from .hrex import HamiltonianExchange

        return HamiltonianExchange
    if name == "Restraints":
        from .restraints import Restraints

        return Restraints
    if name == "GroupRestraints":
        from .group_restraints import GroupRestraints

        return GroupRestraints
    if name == "Metadynamics":
        from .metadynamics import Metadynamics

        return Metadynamics
    if name == "Alchemical":
        from .alchemy import Alchemical

        return Alchemical
    if name == "GeneralizedBorn":
        from .implicit import GeneralizedBorn

        return GeneralizedBorn
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")


__all__ = [
    "Alchemical",
    "CRescaleBarostat",
    "Forces",
    "GeneralizedBorn",
    "GroupRestraints",
    "HamiltonianExchange",
    "Integrator",
    "Metadynamics",
    "MonteCarloBarostat",
    "Parameters",
    "ReplicaExchange",
    "Restraints",
    "System",
    "VelocityRescale",
    "kinetic_energy",
    "kinetic_to_temp",
    "maxwell_boltzmann",
    "temperature_ladder",
]
__version__ = "0.1.0"
