#!/usr/bin/env python
"""The cost of one replica-exchange attempt on ONE GPU: `ReplicaExchange.attempt` — the host decision, the
permutation of the thermostat's temperatures and the two launches of tmdhip_velocity_rescale — enqueued 200 times between two
device synchronisations (host clock), fp32, on velocities and masses of water boxes of two sizes: 16 replicas of 5 184 atoms
and 2 replicas of 98 304 atoms (needs a GPU).  Every tried pair is accepted (u = 0), so an attempt rescales every slot that has
a partner: the most an attempt can cost.  Reported, compared with nothing.

    python tools/time_exchange.py [--rounds 5] [--attempts 200]
"""
import argparse
import json
import os
import sys
import time
import types

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from torchmd_amd.exchange import ReplicaExchange, temperature_ladder  # noqa: E402
from torchmd_amd.integrator import BOLTZMAN  # noqa: E402
from torchmd_amd.thermostat import VelocityRescale  # noqa: E402


class Zero:
    def random(self):
        return 0.0


def measure(R, natoms, rounds, nattempts):
    dev = torch.device("cuda:0")
    gen = torch.Generator().manual_seed(1)
    mass = torch.tensor([15.999, 1.008, 1.008]).repeat(natoms // 3)
    ladder = temperature_ladder(300.0, 330.0, R)
    vel = torch.randn(R, natoms, 3, generator=gen) * torch.sqrt(BOLTZMAN * torch.as_tensor(ladder, dtype=torch.float32).view(R, 1, 1)
                                                                / mass.view(1, -1, 1))
    s = types.SimpleNamespace(vel=vel.to(dev).contiguous())
    mass = mass.to(dev).contiguous()
    th = VelocityRescale(list(ladder), seed=1)
    ex = ReplicaExchange(frequency=1, seed=1)
    ex.rng = Zero()
    epot = -9.5 * natoms / 3 + np.arange(R)  # (any finite energies: u = 0 accepts every pair)
    for _ in range(10):  # warm-up: code objects, workspace
        ex.attempt(s, mass, th, epot)
    per = []
    for _ in range(rounds):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(nattempts):
            ex.attempt(s, mass, th, epot)
        torch.cuda.synchronize()
        per.append((time.perf_counter() - t0) / nattempts * 1e6)
    assert np.array_equal(ex.accepted, ex.attempts) and torch.isfinite(s.vel).all()
    return {"replicas": R, "natoms": natoms, "us_per_attempt": [round(v, 2) for v in per],
            "us_per_attempt_median": round(float(np.median(per)), 2), "attempts": int(ex.nattempts)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--attempts", type=int, default=200)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    out = {"device": torch.cuda.get_device_name(0),
           "cases": [measure(16, 5184, args.rounds, args.attempts), measure(2, 98304, args.rounds, args.attempts)]}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
