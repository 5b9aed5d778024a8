"""Spatial domain decomposition (config C5) validated on ONE GPU: all ranks run inside one process
(`LocalTransport`), forces and a short trajectory must equal the single-domain periodic engine."""

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _system(nside, dtype):
    from torchmd_amd.builders import argon_forcefield, lj_box
    from torchmd_amd.parameters import Parameters

    mol, pos, box = lj_box(nside, seed=6)
    par = Parameters(argon_forcefield(mol), mol, ["lj"], precision=dtype)
    return mol, pos, box, par


@pytest.mark.parametrize("world,grid", [(8, None), (4, (2, 1, 2)), (2, None), (1, None)])
def test_forces_equal_single_domain(world, grid):
    from torchmd_amd.domain import DomainSet
    from torchmd_amd.forces import Forces

    dev, dt = torch.device("cuda:0"), torch.float64
    mol, pos, box, par = _system(22, dt)  # 10 648 atoms, L = 79.3 A
    rng = np.random.default_rng(0)
    pos = pos + rng.integers(-1, 2, size=pos.shape) * box  # scatter atoms over periodic images
    n = mol.numAtoms
    A, B = par.get_AB()
    ds = DomainSet(box, world, dev, dt, ["lj"], 9.0, A=A, B=B, skin=1.5, grid=grid)
    ds.scatter(pos, np.zeros_like(pos), par.charges.numpy(), par.mapped_atom_types.numpy(), par.masses.numpy().ravel())
    assert sum(d.nown for d in ds.domains.values()) == n
    ds.compute_forces()
    _, _, F = ds.gather(n)
    ref = Forces(par, terms=["lj"], cutoff=9.0)
    p = torch.tensor(pos, dtype=dt, device=dev)[None].contiguous()
    b = torch.diag(torch.tensor(box, dtype=dt, device=dev))[None].contiguous()
    Fr = torch.zeros_like(p)
    ref.compute(p, b, Fr)
    assert (F - Fr[0]).abs().max().item() < 1e-9
    halo = [d.local_pos.shape[1] - d.nown for d in ds.domains.values()]
    assert all(h > 0 for h in halo)
    # energy: halo atoms are passive, so a brick counts its own-own pairs fully and own-halo pairs half;
    # the bricks' energies add up to the single-domain total
    from torchmd_amd import _lib as L

    e_dd = sum(float(d.compute(want_energy=True)[0, L.ENERGY_SLOT["lj"]].item()) for d in ds.domains.values())
    e_ref = ref.compute(p, b, Fr, returnDetails=True)[0]["lj"]
    assert abs(e_dd - e_ref) <= 1e-9 * abs(e_ref)
    # and no force is computed on the halo atoms
    for d in ds.domains.values():
        assert d.local_forces[0, d.nown:].abs().max().item() == 0.0


def test_trajectory_equal_single_domain():
    """40 NVE steps (hot start so that atoms migrate between bricks): positions/velocities agree with
    the single-domain integrator to fp64 round-off."""
    from torchmd_amd.domain import DomainSet
    from torchmd_amd.forces import Forces
    from torchmd_amd.integrator import Integrator, maxwell_boltzmann
    from torchmd_amd.systems import System

    dev, dt = torch.device("cuda:0"), torch.float64
    mol, pos, box, par = _system(22, dt)
    n = mol.numAtoms
    torch.manual_seed(3)
    vel = maxwell_boltzmann(par.masses, 4000.0, 1)[0].numpy()  # hot: ~0.05 A per step
    A, B = par.get_AB()
    ds = DomainSet(box, 8, dev, dt, ["lj"], 9.0, A=A, B=B, skin=1.0)
    ds.scatter(pos, vel, par.charges.numpy(), par.mapped_atom_types.numpy(), par.masses.numpy().ravel())
    ds.compute_forces()
    ds.step(40, timestep_fs=2.0)
    P, V, F = ds.gather(n)

    s = System(n, 1, dt, dev)
    s.set_positions(pos[:, :, None])
    s.set_box(box)
    s.set_velocities(torch.tensor(vel)[None])
    f = Forces(par, terms=["lj"], cutoff=9.0)
    f.compute(s.pos, s.box, s.forces)
    Integrator(s, f, 2.0, dev).step(40)
    assert ds.migrations >= 1
    assert (P - s.pos[0]).abs().max().item() < 1e-7
    assert (V - s.vel[0]).abs().max().item() < 1e-7
    assert (F - s.forces[0]).abs().max().item() < 1e-6


@pytest.mark.timeout(300)
def test_native_exchange_and_step_loop_single_rank():
    """The C-driven path (`tmdhip_dd_run`: fused kick/drift kernel, device-side halo pack, grouped RCCL
    send/recv into the halo rows, forces — all enqueued from C) on a 1-rank RCCL communicator, where the brick
    exchanges its periodic images with itself: (i) `tmdhip_comm_exchange` reproduces the torch all-to-all,
    (ii) a 40-step NVE trajectory with migrations equals the single-domain integrator, (iii) and equals the
    Python-driven loop over torch.distributed (and its torch-made migrations) to 1e-9."""
    import os

    import torch.distributed as dist

    from torchmd_amd import _lib as L
    from torchmd_amd.domain import DistTransport, DomainSet
    from torchmd_amd.forces import Forces
    from torchmd_amd.integrator import Integrator, maxwell_boltzmann
    from torchmd_amd.systems import System

    dev, dt = torch.device("cuda:0"), torch.float64
    mol, pos, box, par = _system(22, dt)
    n = mol.numAtoms
    torch.manual_seed(3)
    vel = maxwell_boltzmann(par.masses, 4000.0, 1)[0].numpy()
    A, B = par.get_AB()
    import socket

    with socket.socket(socket.AF_INET, socket.SOCK_STREAM) as sk:  # a port nobody listens on right now
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    dist.init_process_group("nccl", init_method=f"tcp://127.0.0.1:{port}", rank=0, world_size=1, device_id=dev)
    try:
        results = {}
        for native in ("1", "0"):
            os.environ["TMDHIP_DD_NATIVE"] = native
            tr = DistTransport()
            ds = DomainSet(box, 1, dev, dt, ["lj"], 9.0, A=A, B=B, skin=1.0, transport=tr)
            ds.scatter(pos, vel, par.charges.numpy(), par.mapped_atom_types.numpy(), par.masses.numpy().ravel())
            assert (tr.native() is not None) == (native == "1")
            d = ds.domains[0]
            if native == "1":  # (i) one grouped exchange against torch's all_to_all_single
                import ctypes as C

                sent = d.pack_halo().clone()
                want = tr.all_to_all(sent, d.plan.send_counts, ds._recv_counts["halo"])
                got = torch.zeros_like(want)
                sc = (C.c_int64 * 1)(*d.plan.send_counts)
                rc = (C.c_int64 * 1)(*ds._recv_counts["halo"])
                L.check(L.load().tmdhip_comm_exchange(tr.native(), L.dtype_code(dt), sent.data_ptr(), sc, got.data_ptr(), rc, 3,
                                                      torch.cuda.current_stream(dev).cuda_stream))
                torch.cuda.synchronize()
                assert got.shape[0] > 0 and torch.equal(got, want)
            ds.compute_forces()
            ds.step(25, timestep_fs=2.0)
            ds.step(15, timestep_fs=2.0)
            results[native] = ds.gather(n) + (ds.migrations,)
            d.forces_engine.close()
            tr.close()
    finally:
        os.environ.pop("TMDHIP_DD_NATIVE", None)
        dist.destroy_process_group()
    P, V, F, mig = results["1"]
    assert mig >= 1
    s = System(n, 1, dt, dev)
    s.set_positions(pos[:, :, None])
    s.set_box(box)
    s.set_velocities(torch.tensor(vel)[None])
    f = Forces(par, terms=["lj"], cutoff=9.0)
    f.compute(s.pos, s.box, s.forces)
    Integrator(s, f, 2.0, dev).step(40)
    assert (P - s.pos[0]).abs().max().item() < 1e-7
    assert (V - s.vel[0]).abs().max().item() < 1e-7
    assert (F - s.forces[0]).abs().max().item() < 1e-6
    # the Python-driven loop migrates with torch operations and plans the engine's cell grid over the observed bounding
    # box; the library's migration (tmdhip_dd_migrate) plans it over brick + halo: same pairs, another summation order
    P0, V0, F0, mig0 = results["0"]
    assert mig0 == mig
    assert (P - P0).abs().max().item() < 1e-9 and (V - V0).abs().max().item() < 1e-9 and (F - F0).abs().max().item() < 1e-8


@pytest.mark.timeout(600)
@pytest.mark.parametrize("world", [2, 4, 8])
def test_native_loop_at_world_2_4_8_on_one_gpu(world):
    """The library's own brick loop (`tmdhip_dd_run`: kick/drift, halo pack, exchange into the halo rows, forces, the
    asynchronous migration trigger with its max-reduction over the ranks) at world 2 / 4 / 8 on ONE GPU: one host
    thread and one stream per rank, the ranks exchange through the library's in-process communicator
    (`tmdhip_comm_create_local`: device copies ordered by events around a host barrier — the stand-in for RCCL where
    there is one GPU).  (i) one grouped exchange from `world` threads equals the reference all-to-all; (ii) 40 hot NVE
    steps with migrations equal the single-domain integrator (fp64: 1e-7 / 1e-7 / 1e-6) and (iii) the Python-driven
    loop over the same kernels (same migration decisions; 1e-9)."""
    import ctypes as C
    import threading

    from torchmd_amd import _lib as L
    from torchmd_amd.domain import DomainSet, LocalTransport
    from torchmd_amd.forces import Forces
    from torchmd_amd.integrator import Integrator, maxwell_boltzmann
    from torchmd_amd.systems import System

    dev, dt = torch.device("cuda:0"), torch.float64
    mol, pos, box, par = _system(23, dt)  # (odd: brick faces pass through lattice planes, atoms change bricks)
    n = mol.numAtoms
    torch.manual_seed(3)
    vel = maxwell_boltzmann(par.masses, 4000.0, 1)[0].numpy()
    A, B = par.get_AB()
    results = {}
    for native in (True, False):
        tr = LocalTransport(world, native_threads=native)
        ds = DomainSet(box, world, dev, dt, ["lj"], 9.0, A=A, B=B, skin=1.0, transport=tr)
        ds.scatter(pos, vel, par.charges.numpy(), par.mapped_atom_types.numpy(), par.masses.numpy().ravel())
        if native:  # (i) tmdhip_comm_exchange from one thread per rank
            lib = L.load()
            comms, streams = tr.native(dev)
            sent = {r: d.pack_halo().clone() for r, d in ds.domains.items()}
            counts = {r: d.plan.send_counts for r, d in ds.domains.items()}
            want = ds._all_to_all("probe", sent, counts)
            got = {r: torch.zeros_like(want[r]) for r in ds.domains}
            torch.cuda.synchronize()
            rcs = {}

            def work(r):
                sc = (C.c_int64 * world)(*counts[r])
                rc = (C.c_int64 * world)(*[counts[src][r] for src in range(world)])
                with torch.cuda.device(dev):
                    rcs[r] = lib.tmdhip_comm_exchange(comms[r], L.dtype_code(dt), sent[r].data_ptr(), sc, got[r].data_ptr(),
                                                      rc, 3, streams[r].cuda_stream)

            ths = [threading.Thread(target=work, args=(r,)) for r in ds.domains]
            [th.start() for th in ths]
            [th.join() for th in ths]
            torch.cuda.synchronize()
            assert all(v == 0 for v in rcs.values()), rcs
            for r in ds.domains:
                assert got[r].shape[0] > 0 and torch.equal(got[r], want[r]), r
        ds.compute_forces()
        ds.step(25, timestep_fs=2.0)
        ds.step(15, timestep_fs=2.0)
        results[native] = ds.gather(n) + (ds.migrations,)
        for d in ds.domains.values():
            d.forces_engine.close()
        tr.close()
    P, V, F, mig = results[True]
    assert mig >= 1
    s = System(n, 1, dt, dev)
    s.set_positions(pos[:, :, None])
    s.set_box(box)
    s.set_velocities(torch.tensor(vel)[None])
    f = Forces(par, terms=["lj"], cutoff=9.0)
    f.compute(s.pos, s.box, s.forces)
    Integrator(s, f, 2.0, dev).step(40)
    ep, ev, ef = (P - s.pos[0]).abs().max().item(), (V - s.vel[0]).abs().max().item(), (F - s.forces[0]).abs().max().item()
    P0, V0, F0, mig0 = results[False]
    same = torch.equal(P, P0) and torch.equal(V, V0) and torch.equal(F, F0)
    print(f"world {world}: migrations {mig} (Python-driven loop: {mig0}), vs single domain max|dx| {ep:.2e} max|dv| {ev:.2e} "
          f"max|dF| {ef:.2e}; bit-identical to the Python-driven loop: {same}")
    assert ep < 1e-7 and ev < 1e-7 and ef < 1e-6
    assert (P - P0).abs().max().item() < 1e-9 and (V - V0).abs().max().item() < 1e-9 and (F - F0).abs().max().item() < 1e-8


@pytest.mark.timeout(600)
@pytest.mark.parametrize("world", [1, 2, 4, 8])
def test_native_loop_over_rccl_ranks(world):
    """`tmdhip_comm_exchange` and `tmdhip_dd_run` between REAL ranks, one GPU each (tests/_dd_ranks.py under
    torch.distributed.run): the library's grouped RCCL send/recv equals torch's all_to_all_single, and 40 NVE steps
    with migrations equal the single-domain integrator.  World sizes the box has no GPUs for are skipped (the
    1-GPU pool runs world = 1: the brick exchanges its periodic images with itself over RCCL)."""
    import os
    import socket
    import subprocess
    import sys

    if torch.cuda.device_count() < world:
        pytest.skip(f"needs {world} GPUs, this box has {torch.cuda.device_count()}")
    with socket.socket(socket.AF_INET, socket.SOCK_STREAM) as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    here = os.path.dirname(os.path.abspath(__file__))
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    env.pop("TMDHIP_DD_NATIVE", None)
    res = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={world}",
                          "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.join(here, "_dd_ranks.py")],
                         capture_output=True, text=True, timeout=550, env=env)
    assert res.returncode == 0, (res.stdout[-1500:], res.stderr[-3000:])
    assert f"DD-RANKS OK world={world}" in res.stdout, res.stdout[-1500:]


@pytest.mark.parametrize("dt", [torch.float32, torch.float64])
@pytest.mark.parametrize("langevin", [False, True])
def test_dd_step_equals_the_separate_integrator_kernels(dt, langevin):
    """`tmdhip_dd_step` (kick of the previous step + drift of this one in one launch) is bit-identical to
    tmdhip_[langevin_]second_vv followed by tmdhip_first_vv, and its displacement maximum is max |x - ref|^2;
    `tmdhip_halo_pack` equals index_select + shift."""
    from torchmd_amd import _lib as L

    lib, dev = L.load(), torch.device("cuda:0")
    code = L.dtype_code(dt)
    n = 5000
    g = torch.Generator(device="cpu").manual_seed(4)
    mk = lambda *shape: torch.randn(*shape, generator=g, dtype=torch.float64).to(dt).to(dev).contiguous()  # noqa: E731
    pos, vel, frc = mk(n, 3) * 10, mk(n, 3), mk(n, 3) * 5
    mass = (1.0 + 15.0 * torch.rand(n, generator=g, dtype=torch.float64)).to(dt).to(dev)
    vc = (0.01 * torch.rand(n, generator=g, dtype=torch.float64)).to(dt).to(dev)
    ref = (pos + 0.1 * mk(n, 3)).contiguous()
    tstep, gamma, seed, step = 0.02, 0.3, 1234, 77
    st = torch.cuda.current_stream(dev).cuda_stream
    p1, v1 = pos.clone(), vel.clone()
    if langevin:
        L.check(lib.tmdhip_langevin_second_vv(code, 1, n, v1.data_ptr(), frc.data_ptr(), mass.data_ptr(), vc.data_ptr(),
                                              tstep, gamma, seed, step, st))
    else:
        L.check(lib.tmdhip_second_vv(code, 1, n, v1.data_ptr(), frc.data_ptr(), mass.data_ptr(), tstep, st))
    L.check(lib.tmdhip_first_vv(code, 1, n, p1.data_ptr(), v1.data_ptr(), frc.data_ptr(), mass.data_ptr(), tstep, st))
    p2, v2 = pos.clone(), vel.clone()
    disp2 = torch.zeros(1, dtype=torch.float32, device=dev)
    L.check(lib.tmdhip_dd_step(code, n, p2.data_ptr(), v2.data_ptr(), frc.data_ptr(), mass.data_ptr(),
                               vc.data_ptr() if langevin else 0, tstep, gamma, seed, step, 3, ref.data_ptr(),
                               disp2.data_ptr(), st))
    torch.cuda.synchronize()
    assert torch.equal(p1, p2) and torch.equal(v1, v2)
    want = ((p2 - ref) ** 2).sum(dim=1).max().item()
    assert abs(disp2.item() - want) <= 2e-6 * want and disp2.item() >= want * (1 - 1e-6)
    # the two phases one at a time give the same state as both together
    p3, v3 = pos.clone(), vel.clone()
    for phases in (1, 2):
        L.check(lib.tmdhip_dd_step(code, n, p3.data_ptr(), v3.data_ptr(), frc.data_ptr(), mass.data_ptr(),
                                   vc.data_ptr() if langevin else 0, tstep, gamma, seed, step, phases, 0, 0, st))
    torch.cuda.synchronize()
    assert torch.equal(p3, p2) and torch.equal(v3, v2)
    # halo pack
    idx = torch.randint(0, n, (777,), generator=g).to(torch.int32).to(dev)
    shift = (mk(777, 3) * 3).contiguous()
    out = torch.empty(777, 3, dtype=dt, device=dev)
    L.check(lib.tmdhip_halo_pack(code, 777, p2.data_ptr(), idx.data_ptr(), shift.data_ptr(), out.data_ptr(), st))
    torch.cuda.synchronize()
    assert torch.equal(out, p2.index_select(0, idx.long()) + shift)


@pytest.mark.timeout(600)
@pytest.mark.parametrize("world", [1, 2, 8])
def test_brick_loop_variants_are_bit_identical(world, monkeypatch):
    """`tmdhip_dd_run` makes a brick step (a) as separate launches (TMDHIP_DD_FUSED=0: kick/drift, pack, displacement test,
    rebuild chain, pair kernel), (b) as three launches (=1: dd_own_kernel, dd_halo_kernel, the pair kernel with the chain
    left out while nobody is near its limit) or (c) with the owned atoms' update made by the step blocks of the previous
    pair launch (=2, the default; fp32 bricks on the lean kernel).  Same arithmetic, same rebuild and migration decisions:
    positions, velocities and forces must agree bit for bit — fp32, Langevin, hot enough for migrations (made by
    tmdhip_dd_migrate) and device-side list rebuilds inside the window; in-process ranks, one host thread each."""
    from torchmd_amd.domain import DomainSet, LocalTransport
    from torchmd_amd.integrator import maxwell_boltzmann

    dev, dt = torch.device("cuda:0"), torch.float32
    mol, pos, box, par = _system(23, dt)  # (odd: brick faces pass through lattice planes, atoms change bricks at once)
    n = mol.numAtoms
    torch.manual_seed(3)
    vel = maxwell_boltzmann(par.masses, 600.0, 1)[0].numpy()
    A, B = par.get_AB()
    monkeypatch.setenv("TMDHIP_DEBUG_CHAIN_MIN_ENTRIES", "1")
    out = {}
    for mode in ("2", "1", "0"):
        monkeypatch.setenv("TMDHIP_DD_FUSED", mode)
        tr = LocalTransport(world, native_threads=True)
        ds = DomainSet(box, world, dev, dt, ["lj"], 9.0, A=A, B=B, skin=1.0, transport=tr)
        ds.scatter(pos, vel, par.charges.numpy(), par.mapped_atom_types.numpy(), par.masses.numpy().ravel())
        ds.compute_forces()
        ds.step(45, timestep_fs=2.0, gamma_ps=1.0, T=600.0, seed=11)
        ds.step(36, timestep_fs=2.0, gamma_ps=1.0, T=600.0, seed=11)
        stats = [d.forces_engine.stats(d.local_pos) for d in ds.domains.values()]
        out[mode] = ds.gather(n) + (ds.migrations, sum(s["steps_in_pair_launch"] for s in stats),
                                    sum(s["n_rebuilds"] for s in stats), sum(s["chains_skipped"] for s in stats))
        for d in ds.domains.values():
            d.forces_engine.close()
        tr.close()
    P, V, F, mig, fused_steps, rebuilds, skipped = out["2"]
    assert torch.isfinite(P).all() and mig >= 2
    assert fused_steps > 40 * world and skipped > 20 * world, (fused_steps, skipped)
    for mode in ("1", "0"):
        P1, V1, F1, mig1, fs1, rb1, sk1 = out[mode]
        assert fs1 == 0 and mig1 == mig and rb1 == rebuilds, (mode, mig1, rb1)
        assert torch.equal(P, P1) and torch.equal(V, V1) and torch.equal(F, F1), mode
    assert out["1"][6] == skipped and out["0"][6] == 0


@pytest.mark.timeout(600)
def test_library_migration_equals_the_torch_migration_with_mixed_types():
    """`tmdhip_dd_migrate` against the torch migration of domain.py on a mixture: three atom types of which two share
    their LJ parameters (the engine merges them into one class: the type -> class map travels to the library), different
    masses, charges and a reaction field, so that every field of a migrating atom's state row matters.  World 4
    (2 x 1 x 2), in-process ranks; the library's loop with the library's migration against the same loop with
    TMDHIP_DD_MIGRATE=python: same migration decisions, same owners, positions / velocities / forces to 1e-9 (the two plan
    the engine's cell grid over different bounds: another summation order), and both equal the single-domain run."""
    import os

    from _oracle_sample import mixed_system
    from torchmd_amd.domain import DomainSet, LocalTransport
    from torchmd_amd.forces import Forces
    from torchmd_amd.integrator import Integrator, maxwell_boltzmann
    from torchmd_amd.systems import System

    dev, dt = torch.device("cuda:0"), torch.float64
    # nside 21, a = 3.6 (odd: the faces of the 2 x 1 x 2 bricks pass THROUGH lattice planes, atoms cross them at once)
    mol, pos, box, par, terms = mixed_system(21, dt)
    n = len(pos)
    torch.manual_seed(5)
    vel = maxwell_boltzmann(par.masses, 3000.0, 1)[0].numpy()
    A, B = par.get_AB()
    out = {}
    growths = 0
    try:
        for how in ("native", "python", "native-tight"):
            os.environ["TMDHIP_DD_MIGRATE"] = how.split("-")[0]
            # third pass: capacity buffers without headroom — every brick that gains an atom, a halo row or a send row makes
            # tmdhip_dd_migrate return 2 (need_*); the caller grows its arrays and the call resumes where it stopped
            os.environ.pop("TMDHIP_DD_TEST_TIGHT_CAPS", None)
            if how == "native-tight":
                os.environ["TMDHIP_DD_TEST_TIGHT_CAPS"] = "1"
            tr = LocalTransport(4, native_threads=True)
            ds = DomainSet(box, 4, dev, dt, terms, 9.0, A=A, B=B, skin=1.0, grid=(2, 1, 2), transport=tr, rfa=True)
            ds.scatter(pos, vel, par.charges.numpy(), par.mapped_atom_types.numpy(), par.masses.numpy().ravel())
            eng = next(iter(ds.domains.values())).forces_engine._engine(next(iter(ds.domains.values())).local_pos)
            assert eng.type_map is not None and eng.ntypes == 2  # A1 and A2 are one LJ class
            owners0 = torch.zeros(n, dtype=torch.long, device=dev)
            for r, d in ds.domains.items():
                owners0[d.ids] = r
            ds.compute_forces()
            ds.step(30, timestep_fs=2.0)
            owners = torch.zeros(n, dtype=torch.long, device=dev)
            for r, d in ds.domains.items():
                owners[d.ids] = r
            out[how] = ds.gather(n) + (ds.migrations, owners.cpu())
            assert int((owners != owners0).sum()) >= 20  # atoms really changed bricks
            if how == "native-tight":
                growths = sum(getattr(d, "capacity_growths", 0) for d in ds.domains.values())
            for d in ds.domains.values():
                d.forces_engine.close()
            tr.close()
    finally:
        os.environ.pop("TMDHIP_DD_MIGRATE", None)
        os.environ.pop("TMDHIP_DD_TEST_TIGHT_CAPS", None)
    assert growths >= 3, growths
    for a, b in zip(out["native"][:3], out["native-tight"][:3]):  # resumed calls give the same state, bit for bit
        assert torch.equal(a, b)
    assert out["native"][3] == out["native-tight"][3] and torch.equal(out["native"][4], out["native-tight"][4])
    P, V, F, mig, own = out["native"]
    P0, V0, F0, mig0, own0 = out["python"]
    assert mig >= 3 and mig == mig0 and torch.equal(own, own0)
    assert (P - P0).abs().max().item() < 1e-9 and (V - V0).abs().max().item() < 1e-9 and (F - F0).abs().max().item() < 1e-8
    s = System(n, 1, dt, dev)
    s.set_positions(pos[:, :, None])
    s.set_box(box)
    s.set_velocities(torch.tensor(vel)[None])
    f = Forces(par, terms=terms, cutoff=9.0, rfa=True)
    f.compute(s.pos, s.box, s.forces)
    Integrator(s, f, 2.0, dev).step(30)
    assert (P - s.pos[0]).abs().max().item() < 1e-7 and (V - s.vel[0]).abs().max().item() < 1e-7
    assert (F - s.forces[0]).abs().max().item() < 1e-6


@pytest.mark.timeout(600)
def test_halo_overrun_is_recovered_from_the_saved_state():
    """A `check_every` far too large for the temperature: the first displacement that is looked at lies beyond the halo's
    half skin already, so the steps since the last migration ran with halo atoms missing.  The loop must notice (the
    measured value, not the extrapolation), go back to the state saved at the entry of `step` / at the last migration,
    halve `check_every` and repeat — in the Python-driven loop, in the library's loop over the in-process communicator
    (world 4: `tmdhip_dd_run` returns TMDHIP_DD_OVERRUN on every rank at the same iteration) and over RCCL (one rank) —
    and still arrive at the single-domain trajectory.  With `recover` off the same run raises."""
    import socket

    import torch.distributed as dist

    from torchmd_amd.domain import DistTransport, DomainSet, HaloOverrun, LocalTransport
    from torchmd_amd.forces import Forces
    from torchmd_amd.integrator import Integrator, maxwell_boltzmann
    from torchmd_amd.systems import System

    dev, dt = torch.device("cuda:0"), torch.float64
    mol, pos, box, par = _system(23, dt)
    n = mol.numAtoms
    torch.manual_seed(3)
    vel = maxwell_boltzmann(par.masses, 4000.0, 1)[0].numpy()
    A, B = par.get_AB()
    s = System(n, 1, dt, dev)
    s.set_positions(pos[:, :, None])
    s.set_box(box)
    s.set_velocities(torch.tensor(vel)[None])
    f = Forces(par, terms=["lj"], cutoff=9.0)
    f.compute(s.pos, s.box, s.forces)
    Integrator(s, f, 2.0, dev).step(40)

    def run(transport, world, recover=True):
        ds = DomainSet(box, world, dev, dt, ["lj"], 9.0, A=A, B=B, skin=1.0, transport=transport)
        ds.check_every, ds.recover = 32, recover
        ds.scatter(pos, vel, par.charges.numpy(), par.mapped_atom_types.numpy(), par.masses.numpy().ravel())
        ds.compute_forces()
        try:
            ds.step(25, timestep_fs=2.0)
            ds.step(15, timestep_fs=2.0)
            moved = ds.verify_halo()
            return ds.gather(n), ds.recoveries, ds.check_every, ds.migrations, moved
        finally:
            for d in ds.domains.values():
                d.forces_engine.close()
            transport.close()

    with pytest.raises(HaloOverrun, match="half skin"):
        run(LocalTransport(4), 4, recover=False)
    legs = {"python loop": lambda: run(LocalTransport(4), 4), "library loop, world 4": lambda: run(LocalTransport(4, native_threads=True), 4)}
    for name, leg in legs.items():
        (P, V, F), rec, every, mig, moved = leg()
        ep, ev, ef = (P - s.pos[0]).abs().max().item(), (V - s.vel[0]).abs().max().item(), (F - s.forces[0]).abs().max().item()
        print(f"{name}: {rec} recoveries, check_every 32 -> {every}, {mig} migrations, max|dx| {ep:.2e} max|dv| {ev:.2e} max|dF| {ef:.2e}")
        assert rec >= 1 and every < 32 and mig >= 1 and moved <= 0.5
        assert ep < 1e-7 and ev < 1e-7 and ef < 1e-6, name

    with socket.socket(socket.AF_INET, socket.SOCK_STREAM) as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    dist.init_process_group("nccl", init_method=f"tcp://127.0.0.1:{port}", rank=0, world_size=1, device_id=dev)
    try:
        (P, V, F), rec, every, mig, moved = run(DistTransport(), 1)
    finally:
        dist.destroy_process_group()
    ep, ev, ef = (P - s.pos[0]).abs().max().item(), (V - s.vel[0]).abs().max().item(), (F - s.forces[0]).abs().max().item()
    print(f"library loop over RCCL, one rank: {rec} recoveries, check_every 32 -> {every}, {mig} migrations, max|dx| {ep:.2e}")
    assert rec >= 1 and every < 32 and mig >= 1
    assert ep < 1e-7 and ev < 1e-7 and ef < 1e-6


# ---- fp32 bricks (the precision the bench runs) against the ORACLE ----------------------------------------------------------
# Tolerances are the single-domain engine's (test_gpu_parity.py): a brick evaluates the same pairs with the same kernels, only
# with explicit images on open boundaries.
SKIN = 2.5  # the bench's (bench.py --config c5)
GRIDS = [(1, None), (2, None), (4, (2, 1, 2)), (8, None), (6, (6, 1, 1))]  # (6, 1, 1): thin bricks, see _brick_system
GRID_IDS = ["w1", "w2", "w4", "w8", "thin6"]


def _brick_system(which, dt):
    """argon: 23^3 = 12 167 atoms, L = 82.98 A; mixed: the LJ + reaction-field mixture, 21^3 = 9 261 atoms, L = 75.6 A.
    On the (6, 1, 1) grid a brick is 13.8 (12.6) A thick against a halo of cutoff + skin = 11.5 A: atoms near both faces go
    to both neighbours, and in the box's other two directions (one brick) a brick is its own neighbour with two shifts."""
    from _oracle_sample import mixed_system
    from torchmd_amd.builders import argon_forcefield, lj_box
    from torchmd_amd.parameters import Parameters

    if which == "argon":
        mol, pos, box = lj_box(23, seed=6)
        return pos, box, Parameters(argon_forcefield(mol), mol, ["lj"], precision=dt), ["lj"], {}
    _, pos, box, par, terms = mixed_system(21, dt)
    return pos, box, par, terms, {"rfa": True}


def _bricks(which, world, grid, vel_T=None, seed=3):
    from torchmd_amd.domain import DomainSet, LocalTransport
    from torchmd_amd.integrator import maxwell_boltzmann

    dev, dt = torch.device("cuda:0"), torch.float32
    pos, box, par, terms, kw = _brick_system(which, dt)
    if vel_T:
        torch.manual_seed(seed)
        vel = maxwell_boltzmann(par.masses, vel_T, 1)[0].numpy()
    else:
        vel = np.zeros_like(pos)
    A, B = par.get_AB()
    tr = LocalTransport(world, native_threads=True)
    ds = DomainSet(box, world, dev, dt, terms, 9.0, A=A, B=B, skin=SKIN, grid=grid, transport=tr, **kw)
    ds.scatter(pos, vel, par.charges.numpy(), par.mapped_atom_types.numpy(), par.masses.numpy().ravel())
    return ds, tr, pos, vel, box, par, terms, kw


def _close(ds, tr):
    for d in ds.domains.values():
        d.forces_engine.close()
    tr.close()


def _oracle_box(par, pos, box, terms, kw):
    """Oracle forces and per-term energies of the whole periodic box at `pos` ([N, 3] fp32 tensor), evaluated in fp32 like the
    single-domain tests (test_lj_box_vs_oracle): the in-cutoff decision is then the bricks' own, pair for pair.  (An fp64
    evaluation of the same fp32 positions puts single pairs at r = 9 A on the other side: 1.3e-3 kcal/mol/A of LJ force and
    2.8e-3 kcal/mol of energy each, observed in the argon box.)"""
    from oracle import torchmd_oracle as orc

    pairs = orc.candidate_pairs(pos.double().numpy(), box, 9.6, None)
    po, Fo, npairs = orc.compute(par, pos[None], torch.diag(torch.as_tensor(box, dtype=pos.dtype))[None], terms, pairs=pairs,
                                 cutoff=9.0, **kw)
    return po[0], Fo[0].double(), npairs[0]


def _brick_energies(ds, terms):
    from torchmd_amd import _lib as L

    tot = {t: 0.0 for t in terms}
    for d in ds.domains.values():
        e = d.compute(want_energy=True)
        for t in terms:
            tot[t] += float(e[0, L.ENERGY_SLOT[t]].item())
    return tot


def _energy_errors(e_dd, e_or, terms):
    from test_gpu_parity import EFAC, ERTOL

    rel = {t: abs(e_dd[t] - e_or[t]) / max(1.0, abs(e_or[t])) for t in terms}
    for t in terms:
        assert rel[t] <= ERTOL["f32"] * EFAC, (t, e_dd[t], e_or[t])
    return max(rel.values())


def _brick_counts(ds, cutoff=9.0):
    """Per brick: the engine's in-cutoff pair count and the open-boundary count (own-own, own-halo) of its own rows.
    The engine counts over full neighbour lists and halves the sum (pair_generic.hip: halve_pair_count); halo rows are
    passive and have no list, so an own-halo pair is seen once: the engine reports own-own + floor(own-halo / 2)."""
    from _oracle_sample import open_count

    out = []
    for r, d in ds.domains.items():
        n_eng = d.forces_engine.count_pairs(d.local_pos, d.zero_box)[0]
        oo, oh = open_count(d.local_pos[0].cpu(), d.nown, cutoff)
        out.append((r, n_eng, oo, oh))
    return out


def _check_counts(ds, pos32, box, cutoff=9.0):
    """Exact per-brick counts; the whole box within the pairs whose decision may flip between images (see EPS_ULPS)."""
    from _oracle_sample import periodic_count, shell_count

    per = _brick_counts(ds, cutoff)
    for r, n_eng, oo, oh in per:
        assert n_eng == oo + oh // 2, (r, n_eng, oo, oh)
    # every own-halo pair is the own-halo pair of the brick that owns its other atom as well: half of it belongs here
    total_dd = sum(oo + 0.5 * oh for _, _, oo, oh in per)
    total_or = periodic_count(pos32, box, cutoff)
    eps = EPS_ULPS * float(np.spacing(np.float32(max(box))))
    shell = shell_count(pos32.double().numpy(), box, cutoff, eps)
    assert abs(total_dd - total_or) <= shell, (total_dd, total_or, shell)
    return per, total_dd, total_or, shell, eps


# A halo row is the fp32 sum (wrapped position + shift), the oracle's minimum image the fp32 expression d - L round(d / L):
# each coordinate difference carries up to two roundings of at most ulp(2L) / 2 = ulp(L) on either side, so |dr| <= sqrt(3) x
# 2 ulp(L) < 4 ulp(L); with the roundings of the distance itself (ulp(9 A) << ulp(L)) eps = 8 ulp(L) covers it twice over
# (L = 83 A: 6.1e-5 A; L = 360.8 A: 2.4e-4 A).  Pairs farther than eps from the cutoff cannot change sides.
EPS_ULPS = 8


@pytest.mark.timeout(300)
@pytest.mark.parametrize("which", ["argon", "mixed"])
@pytest.mark.parametrize("world,grid", GRIDS, ids=GRID_IDS)
def test_fp32_bricks_static_vs_oracle(world, grid, which):
    """fp32 bricks (in-process native ranks, default TMDHIP_DD_FUSED) right after `scatter`: forces on every atom equal the
    oracle's on the whole box within FTOL['f32'], the bricks' energies add up to the oracle's within ERTOL['f32'] x EFAC, the
    halo rows get exactly zero force (the buffer is filled with NaN first), every brick's in-cutoff pair count equals the
    open-boundary count of its own rows exactly, and the sum equals the oracle's minimum-image count up to the pairs within
    eps of the cutoff."""
    from test_gpu_parity import FTOL

    ds, tr, pos, _, box, par, terms, kw = _bricks(which, world, grid)
    try:
        n = len(pos)
        assert sorted(torch.cat([d.ids for d in ds.domains.values()]).tolist()) == list(range(n))
        for d in ds.domains.values():
            d.local_forces.fill_(float("nan"))
        ds.compute_forces()
        for d in ds.domains.values():
            assert d.local_pos.shape[1] > d.nown
            assert torch.equal(d.local_forces[0, d.nown:], torch.zeros_like(d.local_forces[0, d.nown:])), d.rank
        P, _, F = ds.gather(n)
        p32 = P.cpu()
        e_or, Fo, npairs = _oracle_box(par, p32, box, terms, kw)
        err = (F.cpu().double() - Fo).abs().max().item()
        e_dd = _brick_energies(ds, terms)
        erel = _energy_errors(e_dd, e_or, terms)
        per, total_dd, total_or, shell, eps = _check_counts(ds, p32, box)
        print(f"{which} {world} {grid}: max|dF| {err:.2e}, energy rel. error {erel:.2e}; counts per brick (engine, own-own, own-halo) "
              f"{[c[1:] for c in per]}; whole box: bricks {total_dd}, oracle {total_or} (oracle's own list {npairs}), "
              f"shell |r - rc| <= {eps:.1e}: {shell} pairs")
        assert err < FTOL["f32"]
    finally:
        _close(ds, tr)


@pytest.mark.timeout(600)
@pytest.mark.parametrize("which,world,grid", [("argon", 8, None), ("mixed", 4, (2, 1, 2)), ("argon", 6, (6, 1, 1))],
                         ids=["argon-w8", "mixed-w4", "argon-thin6"])
def test_fp32_bricks_dynamic_vs_oracle(which, world, grid):
    """The bench's integrator settings (1 fs, Langevin, gamma = 1/ps, skin 2.5 A) from a warm start (600 K: the library's own
    trigger migrates within the window, and lists are rebuilt on the device meanwhile), 240 steps; then every atom id is owned
    exactly once, forces equal the oracle's on the gathered positions within FTOL_HOT['f32'], energies meet the static bar,
    and the per-brick counts are exact again."""
    from test_gpu_parity import FTOL_HOT

    ds, tr, pos, _, box, par, terms, kw = _bricks(which, world, grid, vel_T=600.0)
    try:
        n = len(pos)
        ds.compute_forces()
        rb0 = sum(d.forces_engine.stats(d.local_pos)["n_rebuilds"] for d in ds.domains.values())
        ds.step(120, timestep_fs=1.0, gamma_ps=1.0, T=600.0, seed=5)
        ds.step(120, timestep_fs=1.0, gamma_ps=1.0, T=600.0, seed=5)
        rb1 = sum(d.forces_engine.stats(d.local_pos)["n_rebuilds"] for d in ds.domains.values())
        ids = torch.cat([d.ids for d in ds.domains.values()])
        assert sum(d.nown for d in ds.domains.values()) == n and torch.equal(torch.sort(ids).values.cpu(), torch.arange(n))
        P, _, F = ds.gather(n)
        p32 = P.cpu()
        assert torch.isfinite(p32).all()
        e_or, Fo, _ = _oracle_box(par, p32, box, terms, kw)
        err = (F.cpu().double() - Fo).abs().max().item()
        e_dd = _brick_energies(ds, terms)
        erel = _energy_errors(e_dd, e_or, terms)
        per, total_dd, total_or, shell, _ = _check_counts(ds, p32, box)
        print(f"{which} {world} {grid} after 240 Langevin steps: {ds.migrations} migrations, list rebuilds {rb0} -> {rb1}, "
              f"max|dF| {err:.2e}, energies {e_dd} (oracle {e_or}, rel. error {erel:.2e}), whole-box count bricks {total_dd} oracle {total_or} "
              f"(shell {shell})")
        assert ds.migrations >= 1 and rb1 > rb0
        assert err < FTOL_HOT["f32"]
    finally:
        _close(ds, tr)


@pytest.mark.timeout(300)
@pytest.mark.parametrize("which,world,grid", [("argon", 8, None), ("mixed", 4, (2, 1, 2))], ids=["argon-w8", "mixed-w4"])
def test_fp32_brick_nve_step_vs_oracle_md_step(which, world, grid):
    """One NVE step of the fp32 bricks (`tmdhip_dd_run`: kick / drift with `nactive`, halo exchange, forces) against the
    oracle's velocity Verlet in fp64 (`orc.first_vv`, `orc.compute`, `orc.second_vv`: the pieces of `orc.md_step`; the forces
    evaluated as in `_oracle_box`) on the same fp32 start.  The oracle's forces of the new step are taken at the bricks' new positions: an fp32 rounding of a
    position (ulp(83 A) = 7.6e-6 A) would otherwise come back through the LJ stiffness of the closest contacts.
    Bars: positions 2 ulp(L) + dt^2 / (2 m_min) FTOL; velocities 4 ulp(max|v|) + dt / m_min FTOL; forces FTOL."""
    from oracle import torchmd_oracle as orc
    from test_gpu_parity import FTOL

    ds, tr, pos, vel, box, par, terms, kw = _bricks(which, world, grid, vel_T=300.0)
    try:
        n = len(pos)
        ds.compute_forces()
        P0, V0, F0 = (t.cpu().double() for t in ds.gather(n))
        ds.step(1, timestep_fs=1.0)
        P1, V1, F1 = (t.cpu().double() for t in ds.gather(n))
        m = par.masses.double().reshape(n, 1)
        dt = 1.0 / orc.TIMEFACTOR
        _, Fo0, _ = _oracle_box(par, P0.float(), box, terms, kw)
        x, v = P0.clone(), V0.clone()
        orc.first_vv(x, v, Fo0, m, dt)
        _, Fo1, _ = _oracle_box(par, P1.float(), box, terms, kw)
        orc.second_vv(v, Fo1, m, dt)
        ex, ev, ef = (P1 - x).abs().max().item(), (V1 - v).abs().max().item(), (F1 - Fo1).abs().max().item()
        mmin = float(m.min())
        bar_x = 2 * float(np.spacing(np.float32(max(box)))) + dt * dt / (2 * mmin) * FTOL["f32"]
        bar_v = 4 * float(np.spacing(np.float32(V0.abs().max().item()))) + dt / mmin * FTOL["f32"]
        print(f"{which} {world} {grid}: one NVE step against the oracle: max|dx| {ex:.2e} (bar {bar_x:.1e}), max|dv| {ev:.2e} "
              f"(bar {bar_v:.1e}), max|dF| {ef:.2e}")
        assert ex <= bar_x and ev <= bar_v and ef < FTOL["f32"]
    finally:
        _close(ds, tr)


@pytest.mark.timeout(1200)
def test_c5_bricks_vs_oracle():
    """Config C5 through the bricks: lj_box(100) = 10^6 argon atoms, L = 360.8 A, world 8 on a 2 x 2 x 2 grid of in-process
    native ranks, fp32, skin 2.5 A, Langevin at 85 K, gamma = 1/ps, 1 fs steps from a Maxwell-Boltzmann start at 85 K,
    stepped in batches of 100 until the library's trigger has made a migration (at most 1 000 steps).
    Measured: the first migration comes after 200 steps at 85 K (no warmer start needed).
    Then: (1) forces on 20 000 random atoms and on every atom within the halo of a brick vertex (1 101 atoms), against the
    oracle (every pair touching them): the oracle on each brick's own explicit rows (zero box, fp32) and the single-domain
    engine on the same positions within FTOL['f32'] (observed 1.7e-5 each), the bricks against the minimum-image oracle
    within FTOL_HOT['f32'] (observed 5.1e-4; bricks against the single-domain engine 9.4e-4 at worst).  The gap is the image
    rounding, not a brick error: a halo image is the fp32 sum (wrapped position + L), which at L = 360.8 A is rounded to
    ulp(L) / 2 = 1.5e-5 A, where the minimum-image arithmetic of the oracle and of the single-domain kernels rounds another
    difference; the closest contacts of this state (a lattice start after 200 steps) turn that into up to ~1e-3 of force.
    At 83 A (the static test) the same rounding is 4x smaller.  (2) every
    brick's pair count equals the open-boundary count of its rows exactly and the whole box the oracle's minimum-image count
    up to the shell |r - rc| <= eps; (3) every id is owned exactly once; (4) the bricks' LJ energy equals the oracle's over
    all pairs of the box (in chunks) within ERTOL['f32'] x EFAC."""
    import time

    from _oracle_sample import CHUNK, periodic_tree, sample_forces
    from oracle import torchmd_oracle as orc
    from test_gpu_parity import EFAC, ERTOL, FTOL, FTOL_HOT
    from torchmd_amd.builders import argon_forcefield, lj_box
    from torchmd_amd.domain import DomainSet, LocalTransport
    from torchmd_amd.integrator import maxwell_boltzmann
    from torchmd_amd.parameters import Parameters

    dev, dt = torch.device("cuda:0"), torch.float32
    mol, pos, box = lj_box(100, seed=4)
    n = mol.numAtoms
    par = Parameters(argon_forcefield(mol), mol, ["lj"], precision=dt)
    torch.manual_seed(2)
    vel = maxwell_boltzmann(par.masses, 85.0, 1)[0].numpy()
    A, B = par.get_AB()
    tr = LocalTransport(8, native_threads=True)
    ds = DomainSet(box, 8, dev, dt, ["lj"], 9.0, A=A, B=B, skin=SKIN, grid=(2, 2, 2), transport=tr)
    try:
        t0 = time.perf_counter()
        ds.scatter(pos, vel, par.charges.numpy(), par.mapped_atom_types.numpy(), par.masses.numpy().ravel())
        ds.compute_forces()
        steps = 0
        while ds.migrations == 0 and steps < 1000:
            ds.step(100, timestep_fs=1.0, gamma_ps=1.0, T=85.0, seed=3)
            steps += 100
        torch.cuda.synchronize()
        wall = time.perf_counter() - t0
        ids = torch.cat([d.ids for d in ds.domains.values()])
        assert sum(d.nown for d in ds.domains.values()) == n and torch.equal(torch.sort(ids).values.cpu(), torch.arange(n))
        P, _, F = ds.gather(n)
        p32, Fg = P.cpu(), F.cpu()
        b = torch.diag(torch.as_tensor(box, dtype=torch.float32))[None]
        tree = periodic_tree(p32.double().numpy(), box)
        # + every atom within the halo of a brick vertex: the atoms whose partners in the diagonal brick arrive only as corner
        # messages (a few hundred of 10^6: a random sample of 20 000 holds a handful of them at most)
        vertices = np.stack(np.meshgrid(*[np.arange(2) * box[k] / 2 for k in range(3)], indexing="ij"), axis=-1).reshape(-1, 3)
        corner = np.unique(np.concatenate([np.asarray(x, dtype=np.int64) for x in tree.query_ball_point(vertices, 9.0 + SKIN)]))
        pick, Fo, npairs, nin = sample_forces(par, p32[None], b, ["lj"], 20000, 7, rlist=9.5, tree=tree, extra=corner, cutoff=9.0)
        err = (Fg[pick] - Fo).abs().max().item()
        # the single-domain engine on the same positions against the same sample: is the gap to the oracle the bricks' own?
        from torchmd_amd.forces import Forces

        f1 = Forces(par, terms=["lj"], cutoff=9.0)
        p1 = P[None].contiguous()
        F1 = torch.zeros_like(p1)
        f1.compute(p1, b.to(dev), F1)
        F1 = F1[0].cpu()
        f1.close()
        err_single = (F1[pick] - Fo).abs().max().item()
        err_vs_single = (Fg - F1).abs().max().item()
        # the oracle on each brick's own explicit rows (own + halo images as the brick stores them, zero box, fp32) for the
        # picked atoms it owns: the brick's arithmetic, image rounding included
        from scipy.spatial import cKDTree

        from torchmd_amd.domain import _local_parameters

        err_open, picked = 0.0, torch.zeros(n, dtype=torch.bool)
        picked[torch.as_tensor(pick)] = True
        for d in ds.domains.values():
            rows = d.local_pos[0].cpu()
            mine = torch.nonzero(picked[d.ids.cpu()]).flatten().numpy()
            nb = cKDTree(rows.double().numpy()).query_ball_point(rows[mine].double().numpy(), 9.5, workers=-1)
            i = np.repeat(mine, [len(x) for x in nb])
            j = np.concatenate([np.asarray(x, dtype=np.int64) for x in nb])
            lo, hi = np.minimum(i[i != j], j[i != j]), np.maximum(i[i != j], j[i != j])
            key = np.unique(lo * np.int64(len(rows)) + hi)
            m = len(rows)
            lpar = _local_parameters(torch.zeros(m, dtype=dt), torch.zeros(m, dtype=torch.long), torch.ones(m, dtype=dt), A, B)
            _, Fl, _ = orc.compute(lpar, rows[None], torch.zeros(1, 3, 3, dtype=dt), ["lj"],
                                   pairs=np.stack([key // m, key % m], axis=1), cutoff=9.0)
            err_open = max(err_open, (d.local_forces[0, mine].cpu() - Fl[0, mine]).abs().max().item())
        per, total_dd, total_or, shell, eps = _check_counts(ds, p32, box)
        from torchmd_amd import _lib as L

        e_dd = sum(float(d.compute(want_energy=True)[0, L.ENERGY_SLOT["lj"]].item()) for d in ds.domains.values())
        allp = tree.query_pairs(9.05, output_type="ndarray")
        e_or = 0.0
        bb = b.double()
        for c in range(0, len(allp), CHUNK):
            po, _, _ = orc.compute(par, p32[None].double(), bb, ["lj"], pairs=allp[c: c + CHUNK].astype(np.int64), cutoff=9.0)
            e_or += po[0]["lj"]
        erel = abs(e_dd - e_or) / abs(e_or)
        print(f"C5 through 2x2x2 bricks: {steps} steps ({wall:.1f} s with scatter), {ds.migrations} migrations; max|dF| on {len(pick)} "
              f"picked atoms ({len(corner)} near brick vertices) {err:.3e} (single-domain engine on the same positions: {err_single:.3e}; bricks against it over all atoms "
              f"{err_vs_single:.3e}; the oracle on the bricks' own rows: {err_open:.3e}) ({nin} in-cutoff pairs); counts per brick (engine, own-own, own-halo) {[c[1:] for c in per]}; "
              f"whole box: bricks {total_dd}, oracle {total_or}, shell |r - rc| <= {eps:.1e}: {shell}; "
              f"E_lj bricks {e_dd:.2f} oracle {e_or:.2f} (rel. {erel:.2e})")
        assert ds.migrations >= 1
        assert err_open < FTOL["f32"] and err_single < FTOL["f32"]
        assert err < FTOL_HOT["f32"]
        assert erel <= ERTOL["f32"] * EFAC
    finally:
        _close(ds, tr)
