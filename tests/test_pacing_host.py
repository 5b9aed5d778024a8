"""The chain-skip decision of the pacing host (torchmd_amd/csrc/pacing.h: pace_decide, next_seq) compiled for the host and run
through its truth table — no GPU.

tests/pacing_host.cpp wraps the header behind a C interface; a module-scoped fixture compiles it with the system C++ compiler
and loads it with ctypes (the header needs no HIP).  Without a host compiler the module skips and says so.

The rule (tmdhip_md_run and tmdhip_dd_run share it): a replica's host-mapped words are [0] progress, [1 + p] the last sequence
number in which an atom was near its displacement limit, [3 + p] the last one whose step rebuilt the list, p = seq & 1.  With a
valid report of the previous step `seq` that this step follows, and no timeout, the rebuild chain is left out when nobody was
near its limit in that step, or when that step rebuilt the list with its chain in place (prev_skipped false: every displacement
is one step old).  Otherwise the chain stays.  The step's own number is seq + 1, and never 0 (0 = nothing published yet).

The same header holds the grid geometry of a replica's share of a fused pair + step launch (fused_grid): pair blocks of four waves
rounded up to the 8 XCDs, and behind them the step blocks, which find their atoms from these numbers alone."""

import ctypes as C
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "torchmd_amd", "csrc")


@pytest.fixture(scope="module")
def pc(tmp_path_factory):
    cxx = next((c for c in (os.environ.get("CXX"), "g++", "c++", "clang++") if c and shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler (CXX, g++, c++, clang++) found: pacing.h is not checked on the CPU")
    out = str(tmp_path_factory.mktemp("pacing") / "libpacing_host.so")
    cmd = [cxx, "-std=c++17", "-O2", "-fPIC", "-shared", f"-I{CSRC}", os.path.join(HERE, "pacing_host.cpp"), "-o", out]
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, " ".join(cmd) + "\n" + res.stdout + res.stderr
    lib = C.CDLL(out)
    lib.pc_decide.argtypes = [C.POINTER(C.c_uint), C.c_uint, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_uint)]
    lib.pc_decide.restype = None
    lib.pc_next_seq.argtypes = [C.c_uint]
    lib.pc_next_seq.restype = C.c_uint
    lib.pc_fast_threads.argtypes = []
    lib.pc_fast_threads.restype = C.c_int
    lib.pc_fused_grid.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int)]
    lib.pc_fused_grid.restype = None
    return lib


def decide(pc, words, seq, seq_valid=True, follows=True, timed_out=False, prev_skipped=False):
    hp = (C.c_uint * 8)(*words)
    out = (C.c_uint * 2)()
    pc.pc_decide(hp, seq, int(seq_valid), int(follows), int(timed_out), int(prev_skipped), out)
    assert out[0] in (0, 1)
    return bool(out[0]), out[1]


def words(seq, near, rebuilt):
    """The eight words after step `seq`: its parity's slots hold `seq` where the event happened and the number of the step
    two before (the slot's previous owner) where it did not; the other parity's slots hold what would decide the opposite way —
    `seq` itself where the event did not happen — so that a look at the wrong slot shows."""
    p, old = seq & 1, (seq - 2) & 0xFFFFFFFF
    w = [seq, 0, 0, 0, 0, 0xDEAD, 0xDEAD, 0xDEAD]
    w[1 + p], w[1 + (1 - p)] = (seq if near else old), (old if near else seq)
    w[3 + p], w[3 + (1 - p)] = (seq if rebuilt else old), (old if rebuilt else seq)
    return w


# (near, rebuilt, prev_skipped) -> skip the chain, written out from the rule above
TABLE = [
    ((False, False, False), True),   # nobody near its limit: no chain
    ((False, False, True), True),
    ((False, True, False), True),
    ((False, True, True), True),
    ((True, False, False), False),   # somebody near, no fresh list: the chain stays
    ((True, False, True), False),
    ((True, True, False), True),     # near, but the previous step rebuilt with its chain in place: all displacements one step old
    ((True, True, True), False),     # ... a "rebuild" report of a step whose chain was left out is not one
]


@pytest.mark.parametrize("seq", [6, 7, 0xFFFFFFFE, 0xFFFFFFFF, 1, 2])
def test_truth_table(pc, seq):
    for (near, rebuilt, prev), want in TABLE:
        got, nxt = decide(pc, words(seq, near, rebuilt), seq, prev_skipped=prev)
        assert got is want, (seq, near, rebuilt, prev)
        assert nxt == (1 if seq == 0xFFFFFFFF else seq + 1), (seq, nxt)


@pytest.mark.parametrize("off", ["seq_valid", "follows", "timed_out"])
@pytest.mark.parametrize("seq", [6, 7])
def test_no_skip_without_a_usable_report(pc, off, seq):
    """No valid report, a first step that does not follow the previous call, or a device that did not report in time: the chain
    stays whatever the words say — and the sequence number still advances."""
    kw = {"seq_valid": True, "follows": True, "timed_out": False}
    kw[off] = off == "timed_out"
    for (near, rebuilt, prev), _ in TABLE:
        got, nxt = decide(pc, words(seq, near, rebuilt), seq, prev_skipped=prev, **kw)
        assert got is False, (off, seq, near, rebuilt, prev)
        assert nxt == seq + 1


def test_sequence_numbers_wrap_past_zero(pc):
    assert pc.pc_next_seq(0) == 1  # a fresh replica: nothing published yet
    assert pc.pc_next_seq(1) == 2
    assert pc.pc_next_seq(0xFFFFFFFE) == 0xFFFFFFFF
    assert pc.pc_next_seq(0xFFFFFFFF) == 1  # never 0
    _, nxt = decide(pc, words(0xFFFFFFFF, True, False), 0xFFFFFFFF)
    assert nxt == 1


K_FAST_THREADS = 256  # threads of a pair block (four waves); step blocks have as many


def parent_fused_grid(n, apw, lpa, bonded):
    """The formula as the two launchers each spelled it before they shared fused_grid, transcribed literally."""
    waves = (n + apw - 1) // apw
    wpb = K_FAST_THREADS // 64
    npair8 = ((waves + wpb - 1) // wpb + 7) // 8 * 8
    k, g8 = lpa * 64 // K_FAST_THREADS, npair8 // 8
    units = (g8 + k - 1) // k
    return npair8, units, 8 * (units if bonded == 1 else (units + 3) // 4)


@pytest.mark.parametrize("bonded", [0, 1, 2])
@pytest.mark.parametrize("lpa", [4, 8, 16, 32, 64])
def test_fused_grid_shape(pc, lpa, bonded):
    """What the step blocks rely on: whole rounds of 8 blocks (one per XCD) of either kind, and enough step blocks for the atoms
    of all pair blocks — a step block takes 64 atoms with inline bonded records (bonded = 1), 256 otherwise."""
    assert pc.pc_fast_threads() == K_FAST_THREADS
    apw = 64 // lpa  # atoms per wave (ListGeom::apw)
    per_block = K_FAST_THREADS // 64 * apw  # atoms of a pair block
    rnd = 8 * per_block  # atoms of one round of 8 pair blocks
    counts = {1, apw - 1, apw, apw + 1, rnd - apw, rnd - apw - 1, rnd - apw + 1, rnd - 1, rnd, rnd + 1, rnd + apw - 1, rnd + apw,
              rnd + apw + 1, 8232, 98304}  # (8 232: the tests' water box, 98 304: the benchmark's)
    for n in sorted(c for c in counts if c >= 1):
        out = (C.c_int * 3)()
        pc.pc_fused_grid(n, apw, lpa, bonded, out)
        pair_blocks, units, step_blocks = out
        assert pair_blocks % 8 == 0 and pair_blocks * per_block >= n > (pair_blocks - 8) * per_block, (n, lpa, pair_blocks)
        assert step_blocks % 8 == 0 and step_blocks > 0, (n, lpa, bonded, step_blocks)
        assert step_blocks * (64 if bonded == 1 else 256) >= pair_blocks * per_block, (n, lpa, bonded, pair_blocks, step_blocks)
        assert (pair_blocks, units, step_blocks) == parent_fused_grid(n, apw, lpa, bonded), (n, lpa, bonded)
