"""The rebuild chain's host decisions (torchmd_amd/csrc/chain_plan.h: read_chain_knobs, choose_binning, choose_build,
batch_single_block_per_cell, batch_covers) compiled for the host and run through their truth table — no GPU.

tests/chain_plan_host.cpp wraps the header behind a C interface; a module-scoped fixture compiles it with the system C++ compiler
and loads it with ctypes (the header needs no HIP).  Without a host compiler the module skips and says so.

The rules: a lone chain bins in ONE launch up to 8 192 atoms and 4 096 cells (TMDHIP_PREP_SMALL=0: never), else in TWO launches up
to 12 288 cells when the replica has not fallen back after a cell overflow and holds the member arrays, else in FOUR.  A row of
the batched chain prefers two launches (one only with TMDHIP_BATCH_PREP_SMALL=1 or where two do not apply) and has no four-launch
form: such a replica, or one with more than 16 384 cells, keeps its own chain.  Only the two-launch binning makes the build
clear the cell counts.  Blocks per cell: TMDHIP_BUILD_SPLIT (1..8), in a batch then TMDHIP_BATCH_BUILD_SPLIT, else 2 up to 1 100
cells and 1 above; back to 1 when a lone grid has more than 16 384 CELLS (the looped kernel, 16 384 blocks) but when a batched
row has more than 16 384 BLOCKS.  A batch of >= 3 000 cells in all runs one block per cell unless a split knob is set."""

import ctypes as C
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "torchmd_amd", "csrc")
OWN, ONE, TWO, FOUR = -1, 0, 1, 2
ENV = ["TMDHIP_PREP_SMALL", "TMDHIP_BATCH_PREP_SMALL", "TMDHIP_BUILD_SPLIT", "TMDHIP_BATCH_BUILD_SPLIT", "TMDHIP_REPLICA_REBUILDS"]


@pytest.fixture(scope="module")
def cp(tmp_path_factory):
    cxx = next((c for c in (os.environ.get("CXX"), "g++", "c++", "clang++") if c and shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler (CXX, g++, c++, clang++) found: chain_plan.h is not checked on the CPU")
    out = str(tmp_path_factory.mktemp("chain_plan") / "libchain_plan_host.so")
    cmd = [cxx, "-std=c++17", "-O2", "-fPIC", "-shared", f"-I{CSRC}", os.path.join(HERE, "chain_plan_host.cpp"), "-o", out]
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, " ".join(cmd) + "\n" + res.stdout + res.stderr
    lib = C.CDLL(out)
    ip = C.POINTER(C.c_int)
    lib.cp_read_knobs.argtypes = [ip]
    lib.cp_binning.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, ip, C.c_int]
    lib.cp_clears_counts.argtypes = [C.c_int]
    lib.cp_build.argtypes = [C.c_int, ip, C.c_int, ip]
    lib.cp_batch_single_block_per_cell.argtypes = [C.c_long, ip]
    lib.cp_batch_covers.argtypes = [C.c_int, ip, ip, ip]
    return lib


def knobs(prep_small=1, batch_prep_small=0, build_split=0, batch_build_split=0, together=0):
    """The defaults: what read_chain_knobs returns with none of the five variables set (test_knob_parsing)."""
    return (C.c_int * 5)(prep_small, batch_prep_small, build_split, batch_build_split, together)


def binning(cp, n, ncell, batched, fallback=False, members=True, **kn):
    """-> (binning, the build clears the cell counts)"""
    b = cp.cp_binning(n, ncell, int(fallback), int(members), knobs(**kn), int(batched))
    return b, bool(cp.cp_clears_counts(b))


def build(cp, ncell, batched, **kn):
    """-> (split, blocks, looped)"""
    out = (C.c_int * 3)()
    cp.cp_build(ncell, knobs(**kn), int(batched), out)
    return out[0], out[1], bool(out[2])


def test_lone_binning_and_cut(cp):
    assert binning(cp, 5184, 343, False) == (ONE, False)
    assert build(cp, 343, False) == (2, 686, False)
    assert binning(cp, 12288, 729, False) == (TWO, True)
    assert build(cp, 729, False) == (2, 1458, False)
    for n, ncell in ((41472, 2197), (98304, 6859)):
        assert binning(cp, n, ncell, False) == (TWO, True)
        assert build(cp, ncell, False) == (1, ncell, False)
        assert binning(cp, n, ncell, False, fallback=True) == (FOUR, False)
        assert binning(cp, n, ncell, False, members=False) == (FOUR, False)
    assert binning(cp, 12288, 729, False, fallback=True) == (FOUR, False)
    assert binning(cp, 5184, 343, False, fallback=True) == (ONE, False)  # a small system needs no member arrays
    assert binning(cp, 5184, 343, False, members=False) == (ONE, False)
    assert binning(cp, 5184, 343, False, prep_small=0) == (TWO, True)
    assert binning(cp, 5184, 343, False, prep_small=0, fallback=True) == (FOUR, False)


def test_lone_thresholds(cp):
    assert binning(cp, 8192, 4096, False)[0] == ONE
    assert binning(cp, 8193, 4096, False)[0] == TWO
    assert binning(cp, 8192, 4097, False)[0] == TWO
    assert binning(cp, 200000, 12288, False) == (TWO, True)
    assert binning(cp, 200000, 12289, False) == (FOUR, False)
    assert build(cp, 1100, False) == (2, 2200, False)
    assert build(cp, 1101, False) == (1, 1101, False)
    assert build(cp, 12289, False) == (1, 12289, False)
    assert build(cp, 16384, False) == (1, 16384, False)
    assert binning(cp, 300000, 16385, False) == (FOUR, False)
    assert build(cp, 16385, False) == (1, 16384, True)
    assert build(cp, 16385, False, build_split=8) == (1, 16384, True)
    assert build(cp, 3000, False, build_split=8) == (8, 24000, False)  # a lone chain does not clamp its blocks
    assert build(cp, 343, False, batch_build_split=4) == (2, 686, False)  # the batch knob is the batch's


def test_batched_binning_and_cut(cp):
    assert binning(cp, 5184, 343, True) == (TWO, True)
    assert build(cp, 343, True) == (2, 686, False)
    assert binning(cp, 5184, 343, True, batch_prep_small=1) == (ONE, False)
    assert binning(cp, 5184, 343, True, fallback=True) == (ONE, False)  # two launches do not apply: one does
    assert binning(cp, 5184, 343, True, prep_small=0, batch_prep_small=1) == (TWO, True)
    assert binning(cp, 5184, 343, True, prep_small=0, fallback=True) == (OWN, False)
    assert binning(cp, 12288, 729, True) == (TWO, True)
    assert binning(cp, 12288, 729, True, batch_prep_small=1) == (TWO, True)
    assert binning(cp, 12288, 729, True, fallback=True) == (OWN, False)
    assert binning(cp, 12288, 729, True, members=False) == (OWN, False)
    assert binning(cp, 200000, 12289, True) == (OWN, False)
    assert binning(cp, 300000, 16385, True) == (OWN, False)
    assert binning(cp, 5184, 16385, True) == (OWN, False)
    assert build(cp, 3000, True, build_split=8) == (1, 3000, False)  # 24 000 blocks: a batched row falls back to one per cell
    assert build(cp, 2048, True, build_split=8) == (8, 16384, False)
    assert build(cp, 343, True, batch_build_split=4) == (4, 1372, False)
    assert build(cp, 343, True, build_split=1, batch_build_split=4) == (1, 343, False)  # TMDHIP_BUILD_SPLIT goes first
    assert build(cp, 2197, True) == (1, 2197, False)


def test_batch_of_many_cells_runs_one_block_per_cell(cp):
    assert not cp.cp_batch_single_block_per_cell(2999, knobs())
    assert cp.cp_batch_single_block_per_cell(3000, knobs())
    assert cp.cp_batch_single_block_per_cell(16 * 343, knobs(batch_prep_small=1, together=1))
    assert not cp.cp_batch_single_block_per_cell(16 * 343, knobs(build_split=2))
    assert not cp.cp_batch_single_block_per_cell(16 * 343, knobs(batch_build_split=2))


def covers(cp, rows):
    arr = [(C.c_int * len(rows))(*[r[i] for r in rows]) for i in range(3)]
    return bool(cp.cp_batch_covers(len(rows), *arr))


def test_batch_needs_several_uniform_covered_replicas(cp):
    assert not covers(cp, [(TWO, 0, 1)])  # a single replica is never a batch
    assert not covers(cp, [(ONE, 0, 1)])
    assert covers(cp, [(TWO, 0, 1)] * 2)
    assert covers(cp, [(ONE, 1, 0)] * 16)
    assert not covers(cp, [(TWO, 0, 1), (ONE, 0, 1)])
    assert not covers(cp, [(TWO, 0, 1), (TWO, 1, 1)])
    assert not covers(cp, [(TWO, 0, 1), (TWO, 0, 0)])
    assert not covers(cp, [(TWO, 0, 1), (TWO, 0, 1), (OWN, 0, 1)])
    assert not covers(cp, [(OWN, 0, 1)] * 2)
    assert not covers(cp, [(FOUR, 0, 1)] * 2)


def read(cp, monkeypatch, **env):
    for name in ENV:
        monkeypatch.delenv(name, raising=False)
    for name, val in env.items():
        monkeypatch.setenv("TMDHIP_" + name, val)
    out = (C.c_int * 5)()
    cp.cp_read_knobs(out)
    return list(out)


def test_knob_parsing(cp, monkeypatch):
    assert read(cp, monkeypatch) == list(knobs()) == [1, 0, 0, 0, 0]
    assert read(cp, monkeypatch, PREP_SMALL="0")[0] == 0
    assert read(cp, monkeypatch, PREP_SMALL="1")[0] == 1
    assert read(cp, monkeypatch, BATCH_PREP_SMALL="1")[1] == 1
    assert read(cp, monkeypatch, BATCH_PREP_SMALL="0")[1] == 0
    for val, want in (("0", 1), ("-3", 1), ("1", 1), ("4", 4), ("8", 8), ("9", 8), ("100", 8), ("x", 1)):  # set: 1..8, never "unset"
        assert read(cp, monkeypatch, BUILD_SPLIT=val)[2:4] == [want, 0], val
        assert read(cp, monkeypatch, BATCH_BUILD_SPLIT=val)[2:4] == [0, want], val
    assert read(cp, monkeypatch, REPLICA_REBUILDS="together")[4] == 1
    for val in ("Together", "together ", "1", "", "togethe", "together2"):
        assert read(cp, monkeypatch, REPLICA_REBUILDS=val)[4] == 0, val
    assert read(cp, monkeypatch, PREP_SMALL="0", BATCH_PREP_SMALL="2", BUILD_SPLIT="3", BATCH_BUILD_SPLIT="5", REPLICA_REBUILDS="together") == [0, 1, 3, 5, 1]
