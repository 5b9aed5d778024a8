#!/usr/bin/env python
"""Config C3 with smooth PME on ONE GPU: the 98 304-atom TIP3P box (tip3p_box(32)), cutoff 9 A, Langevin 300 K, 1 fs, fp32 —
PME at ewald_tolerance 5e-4 and order 5 against reaction field on the same box (needs a GPU).

Reports us/step of Integrator.step(steps), the real-space list pair kernel (HIP events on its dispatch) and, per kernel,
the device time of the PME stages (spread = key + radix sort + bin starts + theta + spread, R2C / C2R FFT, convolution,
force gather, exclusion pass) from a short profiled run (torch.profiler's device trace).

    python tools/time_pme.py [--nside 32] [--steps 100]
"""
import argparse
import os
import sys
import time
from collections import defaultdict

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from torchmd_amd.builders import tip3p_box, water_forcefield  # noqa: E402
from torchmd_amd.forces import Forces  # noqa: E402
from torchmd_amd.integrator import Integrator, maxwell_boltzmann  # noqa: E402
from torchmd_amd.parameters import Parameters  # noqa: E402
from torchmd_amd.systems import System  # noqa: E402

TERMS = ["lj", "electrostatics", "bonds", "angles"]
STAGES = [("pme_key", "spread"), ("RadixSort", "spread"), ("radix_sort", "spread"), ("pme_start", "spread"), ("pme_theta", "spread"),
          ("pme_spread", "spread"), ("pme_conv", "convolution"), ("pme_force", "gather"), ("pme_excl", "exclusions"),
          ("pme_energy", "energy"), ("pme_influence", "influence"), ("list_pair_kernel", "real space (list)")]


def setup(nside, pme):
    dev = torch.device("cuda:0")
    mol, pos, box = tip3p_box(nside, seed=0)
    par = Parameters(water_forcefield(mol), mol, TERMS, precision=torch.float32)
    s = System(mol.numAtoms, 1, torch.float32, dev)
    s.set_positions(pos[:, :, None])
    s.set_box(box)
    torch.manual_seed(1)
    s.set_velocities(maxwell_boltzmann(par.masses, 300.0, 1))
    kw = dict(pme=True, ewald_tolerance=5e-4, pme_order=5) if pme else dict(rfa=True)
    f = Forces(par, terms=TERMS, cutoff=9.0, **kw)
    f.compute(s.pos, s.box, s.forces)
    return mol, s, f, Integrator(s, f, 1.0, dev, gamma=1.0, T=300.0)


def timed(s, f, integ, steps):
    integ.step(50)
    f.enable_timing(s.pos, True, every=4, interior_only=True)
    f.read_timing(s.pos)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    integ.step(steps)
    torch.cuda.synchronize()
    el = time.perf_counter() - t0
    ms, n = f.read_timing(s.pos)
    f.enable_timing(s.pos, False)
    return el / steps * 1e6, ms / max(n, 1) * 1e3


def stage_times(integ, steps):
    """Mean device time per step of each kernel family, from torch.profiler's device trace."""
    from torch.profiler import ProfilerActivity, profile

    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        integ.step(steps)
        torch.cuda.synchronize()
    out = defaultdict(float)
    for ev in prof.key_averages():
        dt = getattr(ev, "device_time_total", None)
        if dt is None:
            dt = getattr(ev, "cuda_time_total", 0.0)
        for key, stage in STAGES:
            if key in ev.key:
                out[stage] += dt / steps
                break
        else:
            if "fft" in ev.key.lower() or "rocfft" in ev.key.lower() or ev.key.startswith(("r2c", "c2r", "fft_")):
                out["FFT (R2C + C2R)"] += dt / steps
    return dict(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nside", type=int, default=32)
    ap.add_argument("--steps", type=int, default=100)
    args = ap.parse_args()
    mol, s, f, integ = setup(args.nside, pme=False)
    us_rf, pk_rf = timed(s, f, integ, args.steps)
    print(f"RF : N={mol.numAtoms} {us_rf:.1f} us/step, list pair kernel {pk_rf:.1f} us")
    del integ, f
    mol, s, f, integ = setup(args.nside, pme=True)
    us_pme, pk_pme = timed(s, f, integ, args.steps)
    print(f"PME: N={mol.numAtoms} {us_pme:.1f} us/step, real-space list pair kernel {pk_pme:.1f} us, beta={f.ewald_beta:.4f}/A, "
          f"grid={f.pme_grid}, order={f.pme_order}, PME buffers {f.stats(s.pos)['pme_bytes'] / 2**20:.1f} MiB")
    try:
        st = stage_times(integ, 20)
        print("PME stages, us/step (device time): " + ", ".join(f"{k} {v:.1f}" for k, v in sorted(st.items())))
    except Exception as e:  # (the profiler is a convenience: the step times above stand without it)
        print(f"per-kernel breakdown unavailable: {e}")
    import re

    maps = open("/proc/self/maps").read()
    libs = sorted(set(m for m in re.findall(r"\S*libhipfft\S*", maps)))
    print("libhipfft loaded: " + ", ".join(libs))


if __name__ == "__main__":
    main()
