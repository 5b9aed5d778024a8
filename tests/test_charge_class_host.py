"""`charges_by_class` (torchmd_amd/csrc/charge_class.h) on the host — no GPU.  A context whose fp32 scaled charges are, BIT for
bit, a function of the LJ class lets the lean pair kernel take the charge products of a pair from its class table; this is the
test that decides it.

tests/charge_class_host.cpp is a stand-alone program around the header (stdin: types and charge bit patterns; stdout: the
answer and the class charges); a module-scoped fixture compiles it with the system C++ compiler.  Without a host compiler the
module skips and says so.  The expected answers are worked out here, in Python, from the same inputs."""

import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "torchmd_amd", "csrc")


def bits(x):
    return struct.unpack("<I", struct.pack("<f", x))[0]


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    cxx = next((c for c in (os.environ.get("CXX"), "g++", "c++", "clang++") if c and shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler (CXX, g++, c++, clang++) found: charge_class.h is not checked on the CPU")
    out = str(tmp_path_factory.mktemp("charge_class") / "charge_class_host")
    cmd = [cxx, "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", f"-I{CSRC}", os.path.join(HERE, "charge_class_host.cpp"), "-o", out]
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, " ".join(cmd) + "\n" + res.stdout + res.stderr
    return out


def ask(prog, ntypes, types, qbits, has_q=True):
    """(answer, class charges as bit patterns) of the program for these atoms"""
    text = f"{ntypes} {len(types)} {int(has_q)}\n" + "".join(f"{int(t)} {int(b):08x}\n" for t, b in zip(types, qbits))
    res = subprocess.run([prog], input=text, capture_output=True, text=True)
    assert res.returncode == 0, (res.returncode, res.stdout, res.stderr)
    words = res.stdout.split()
    return words[0] == "1", [int(w, 16) for w in words[1:]]


def expected(ntypes, types, qbits):
    first, ok = {}, True
    for t, b in zip(types, qbits):
        if first.setdefault(int(t), int(b)) != int(b):
            ok = False
    return ok, [first.get(t, 0) for t in range(ntypes)]


def test_water_like_charges_are_by_class(prog):
    types = np.tile([0, 1, 1], 100)
    q = np.tile([bits(-15.2), bits(7.6), bits(7.6)], 100)
    assert ask(prog, 2, types, q) == (True, [bits(-15.2), bits(7.6)])


def test_an_empty_class_gets_a_zero_charge_and_does_not_matter(prog):
    types = [0, 2, 2, 0, 4]
    q = [bits(1.5), bits(-2.0), bits(-2.0), bits(1.5), bits(0.25)]
    assert ask(prog, 6, types, q) == (True, [bits(1.5), 0, bits(-2.0), 0, bits(0.25), 0])
    assert ask(prog, 3, [], []) == (True, [0, 0, 0])  # no atoms at all


def test_minus_zero_is_not_plus_zero(prog):
    assert bits(-0.0) == 0x80000000 and bits(0.0) == 0
    assert ask(prog, 1, [0, 0, 0], [bits(0.0), bits(-0.0), bits(0.0)]) == (False, [0])
    assert ask(prog, 1, [0, 0], [bits(-0.0), bits(-0.0)]) == (True, [0x80000000])
    assert ask(prog, 2, [0, 1], [bits(0.0), bits(-0.0)]) == (True, [0, 0x80000000])  # (two classes: fine)


def test_nan_charges_compare_by_their_bits(prog):
    qnan, other = 0x7FC00000, 0x7FC00001  # two quiet NaNs with different payloads
    assert ask(prog, 2, [1, 1, 0], [qnan, qnan, bits(1.0)]) == (True, [bits(1.0), qnan])
    assert ask(prog, 2, [1, 1, 0], [qnan, other, bits(1.0)]) == (False, [bits(1.0), qnan])


def test_thirty_two_classes_and_one_mismatch_in_the_last_atom(prog):
    rng = np.random.default_rng(7)
    n = 4099
    types = rng.integers(0, 32, size=n)
    types[:32] = rng.permutation(32)  # every class occurs
    classq = rng.integers(0, 2**32, size=32, dtype=np.uint64)
    q = classq[types].copy()
    assert ask(prog, 32, types, q) == (True, [int(b) for b in classq]) == expected(32, types, q)
    q[-1] ^= 1  # one ulp, in the last atom
    ok, got = ask(prog, 32, types, q)
    assert (ok, got) == expected(32, types, q) and not ok
    assert got == [int(b) for b in classq]  # (the class charge is the FIRST atom's)
    q[-1] ^= 1
    q[0] ^= 0x80000000  # ... and in the first: the class charge moves with it
    ok, got = ask(prog, 32, types, q)
    assert (ok, got) == expected(32, types, q) and not ok and got[int(types[0])] == int(q[0])


def test_without_charges_every_class_is_zero(prog):
    assert ask(prog, 3, [0, 1, 2, 1], [bits(1.0)] * 4, has_q=False) == (True, [0, 0, 0])


def test_bad_arguments_say_no(prog):
    assert ask(prog, 2, [0, 2], [0, 0])[0] is False  # a type outside the table
    assert ask(prog, 2, [0, -1], [0, 0])[0] is False
    assert ask(prog, 0, [], []) == (False, [])
    assert ask(prog, 257, [0], [0])[0] is False  # more classes than a context may have
