"""The host reference of the thermostat's noise (tests/_philox.py) on its own: Philox4x32-10 known answers, the counter and
key mapping of `normal3` (torchmd_amd/csrc/rng.h), and the fp32 uniforms at their edges.  No GPU needed."""

import numpy as np
import pytest

import _philox as P


def _hex(ws):
    return [f"{int(w):08x}" for w in ws]


@pytest.mark.parametrize("ctr,key,want", [
    ([0, 0, 0, 0], [0, 0], "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ([0xFFFFFFFF] * 4, [0xFFFFFFFF] * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ([0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344], [0xA4093822, 0x299F31D0], "d16cfe09 94fdcceb 5001e420 24126ea1"),
], ids=["zero", "ones", "pi"])
def test_philox4x32_10_known_answers(ctr, key, want):
    """The Random123 known-answer vectors of Philox4x32-10."""
    assert _hex(P.philox4x32_10(*ctr, *key)) == want.split()


def test_counter_and_key_mapping_of_normal3():
    """Counter (row lo, row hi, step lo, step hi), key (seed lo, seed hi)."""
    assert _hex(P.philox_block(0x0123456789ABCDEF, 7, 5)) == "414da380 b7702af1 cd642c43 43dc5e58".split()
    assert _hex(P.philox_block(0x0123456789ABCDEF, 7, 5)) == _hex(P.philox4x32_10(5, 0, 7, 0, 0x89ABCDEF, 0x01234567))


def test_vectorised_equals_scalar():
    rows = np.array([0, 1, 2**32 - 1, 2**32, 2**63 + 12345], dtype=np.uint64)
    vec = np.stack(P.philox_block(2**40 + 3, 2**33 + 9, rows), axis=1)
    for r, got in zip(rows, vec):
        assert _hex(got) == _hex(P.philox_block(2**40 + 3, 2**33 + 9, int(r)))


@pytest.mark.parametrize("which", ["row", "step", "seed"])
@pytest.mark.parametrize("half", ["lo", "hi"])
def test_both_words_of_row_step_and_seed_matter(which, half):
    base = dict(seed=0x0123456789ABCDEF, step=0x0000000500000007, row=0x0000000300000011)
    bit = 1 << (0 if half == "lo" else 32)
    other = dict(base, **{which: base[which] ^ bit})
    a = np.array(P.philox_block(**base), dtype=np.uint64)
    b = np.array(P.philox_block(**other), dtype=np.uint64)
    assert (a != b).all()  # one flipped counter or key bit changes every output word
    ga, gb = np.array(P.normal3(**base)), np.array(P.normal3(**other))
    assert (np.abs(ga - gb) > 0).all()


def test_uniform_edges():
    """u = fp32(fp32(c) 2^-32 + 2^-33): c = 0 gives 2^-33 (never 0); c = 2^32 - 1 converts to 2^32 in fp32 and gives 1 + 2^-33,
    which rounds to 1.0f: the clamp of u0 / u2 takes it to 0.99999994f; u1 and u3 (revolutions) may be exactly 1."""
    c = np.array([0, 1, 2**24, 2**32 - 2**8, 2**32 - 129, 2**32 - 128, 2**32 - 1], dtype=np.uint32)
    u = P.uniform(c)
    assert u.dtype == np.float32
    assert u[0] == np.float32(2.0**-33) and u[1] == np.float32(1.5 * 2.0**-32)
    assert u[2] == np.float32(2.0**-8 + 2.0**-33)
    assert u[-1] == np.float32(1.0) and u[-2] == np.float32(1.0)  # (fp32(c) = 2^32 for c >= 2^32 - 128)
    assert u[-3] == np.float32(1.0 - 2.0**-24) and u[-4] == np.float32(1.0 - 2.0**-24)
    assert (np.diff(u.astype(np.float64)) >= 0).all()
    # exact: the float64 sum of fp32(c) 2^-32 and 2^-33 needs at most 24 + 9 significant bits
    cf = c.astype(np.float32).astype(np.float64)
    assert np.array_equal(u, np.float32(cf * 2.0**-32 + 2.0**-33))
    clamped = np.minimum(u, P.U_MAX)
    assert clamped.max() == np.float32(0.99999994) and clamped.max() < 1 and clamped.min() > 0
    assert np.isfinite(np.sqrt(-2.0 * np.log(clamped.astype(np.float64)))).all()


def test_uniforms_of_normal3_are_in_the_open_interval():
    rows = np.arange(200_000, dtype=np.uint64)
    u0, u1, u2, u3 = P.uniforms(2**62 + 17, 2**32 + 1, rows)
    for u in (u0, u2):
        assert u.min() > 0 and u.max() < 1
    for u in (u1, u3):
        assert u.min() > 0 and u.max() <= 1


def test_normal_fill_layout_and_moments():
    n = 3 * 100_000 + 2
    g = P.normal_fill(2**63 + 5, 2**40 + 1, n)
    assert g.shape == (n,) and g.dtype == np.float64
    g0, g1, g2 = P.normal3(2**63 + 5, 2**40 + 1, np.arange(100_001, dtype=np.uint64))
    # the tail row (n % 3 = 2) keeps g0 and g1 of its draw
    assert np.array_equal(g[0::3], g0) and np.array_equal(g[1::3], g1) and np.array_equal(g[2::3], g2[:-1])
    assert abs(g.mean()) < 1e-2 and abs(g.std() - 1) < 1e-2
    assert abs(np.corrcoef(g[0::3][:-1], g[1::3][:-1])[0, 1]) < 1e-2
