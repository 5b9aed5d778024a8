"""The j split of the all-pairs launches (torchmd_amd/csrc/allpairs_split.h: allpairs_split, read_allpairs_waves) compiled for
the host — no GPU.  The force launch and the pressure's pair launch both take their grid from it, and the pressure sizes its
partial sums by it.

tests/allpairs_split_host.cpp wraps the header behind a C interface; a module-scoped fixture compiles it with the system C++
compiler and loads it with ctypes (the header needs no HIP).  Without a host compiler the module skips and says so.

For every n in 1 .. 4096, 1, 2, 16, 17 and 64 replicas, TMDHIP_ALLPAIRS_WAVES unset, 1 and 8192:
  - the j ranges tile 0 .. n: chunks of a multiple of 16, at least one, together they cover n, and the last one is not empty;
  - nb = ceil(n / 64);
  - the values are those of the formula launch_allpairs held before it moved into the header, written out again here."""

import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "torchmd_amd", "csrc")
NMAX = 4096


@pytest.fixture(scope="module")
def aps(tmp_path_factory):
    cxx = next((c for c in (os.environ.get("CXX"), "g++", "c++", "clang++") if c and shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler (CXX, g++, c++, clang++) found: allpairs_split.h is not checked on the CPU")
    out = str(tmp_path_factory.mktemp("allpairs_split") / "liballpairs_split_host.so")
    cmd = [cxx, "-std=c++17", "-O2", "-fPIC", "-shared", f"-I{CSRC}", os.path.join(HERE, "allpairs_split_host.cpp"), "-o", out]
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, " ".join(cmd) + "\n" + res.stdout + res.stderr
    lib = C.CDLL(out)
    lib.aps_split_range.argtypes = [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int)]
    lib.aps_split_range.restype = None
    return lib


def parent_split(n, nrep, waves_env):
    """launch_allpairs' arithmetic as it stood (integer division throughout; the wave target truncated like the C cast)"""
    nb = (n + 63) // 64
    pairs = float(n) * float(n) * float(nrep)
    want_waves = waves_env if waves_env > 0 else int(min(4096.0, max(1024.0, pairs / 512.0)))
    nsplit = max(1, min((n + 15) // 16, want_waves // max(nb * nrep, 1)))
    jchunk = ((n + nsplit - 1) // nsplit + 15) // 16 * 16
    nsplit = (n + jchunk - 1) // jchunk
    return nb, nsplit, jchunk


@pytest.mark.parametrize("override", [None, "1", "8192"])
def test_split_tiles_the_j_range_and_matches_the_previous_formula(aps, monkeypatch, override):
    if override is None:
        monkeypatch.delenv("TMDHIP_ALLPAIRS_WAVES", raising=False)
    else:
        monkeypatch.setenv("TMDHIP_ALLPAIRS_WAVES", override)
    knob = aps.aps_read_waves()
    assert knob == (0 if override is None else int(override))
    n = np.arange(1, NMAX + 1)
    for nrep in (1, 2, 16, 17, 64):
        buf = (C.c_int * (3 * NMAX))()
        aps.aps_split_range(NMAX, nrep, knob, buf)
        nb, nsplit, jchunk = np.array(list(buf)).reshape(NMAX, 3).T
        assert (jchunk % 16 == 0).all()
        assert (nsplit >= 1).all()
        assert (nsplit * jchunk >= n).all()
        assert ((nsplit - 1) * jchunk < n).all()
        assert (nb == (n + 63) // 64).all()
        want = np.array([parent_split(int(k), nrep, knob) for k in n])
        got = np.stack([nb, nsplit, jchunk], axis=1)
        bad = np.nonzero((want != got).any(axis=1))[0]
        assert bad.size == 0, (nrep, override, int(n[bad[0]]), want[bad[0]], got[bad[0]])
        if override == "1":
            assert (nsplit == 1).all()  # one block per 64 atoms walks every j: one add per atom
