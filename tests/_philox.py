"""Host reference of the thermostat's noise (torchmd_amd/csrc/rng.h): Philox4x32-10 and the Box-Muller step of `normal3`.

`normal3(seed, step, row)` draws one Philox block with the counter words (row lo, row hi, step lo, step hi) and the key
words (seed lo, seed hi).  Its four 32-bit outputs become uniforms u = fp32(fp32(c) 2^-32 + 2^-33) (one fused multiply-add in
fp32: the float64 sum below is exact, so rounding it to fp32 once reproduces the device's uniforms bit for bit); u0 and u2 are
clamped to 0.99999994f.  The three Gaussians, with u1 and u3 in revolutions:

    g0 = r0 cos 2 pi u1,  g1 = r0 sin 2 pi u1,  g2 = r1 cos 2 pi u3,  r0 = sqrt(-2 ln u0),  r1 = sqrt(-2 ln u2)

are evaluated here in float64 from those fp32 uniforms; the device evaluates them in fp32 on the hardware transcendentals.
Everything is vectorised over numpy arrays of rows (and broadcasts over steps / seeds)."""

import numpy as np

M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
W0, W1 = np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)
MASK32 = np.uint64(0xFFFFFFFF)
U_MAX = np.float32(0.99999994)  # the largest fp32 below 1


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Ten rounds of Philox4x32 on 32-bit words (array-likes, broadcast): returns the four output words as uint32 arrays."""
    c0, c1, c2, c3, k0, k1 = np.broadcast_arrays(*(np.asarray(w, dtype=np.uint64) & MASK32 for w in (c0, c1, c2, c3, k0, k1)))
    c0, c1, c2, c3, k0, k1 = (np.array(w, dtype=np.uint64) for w in (c0, c1, c2, c3, k0, k1))
    for _ in range(10):
        p0 = M0 * c0  # (exact: both factors < 2^32)
        p1 = M1 * c2
        n0 = (p1 >> np.uint64(32)) ^ c1 ^ k0
        n1 = p1 & MASK32
        n2 = (p0 >> np.uint64(32)) ^ c3 ^ k1
        n3 = p0 & MASK32
        c0, c1, c2, c3 = n0, n1, n2, n3
        k0 = (k0 + W0) & MASK32
        k1 = (k1 + W1) & MASK32
    return tuple(w.astype(np.uint32) for w in (c0, c1, c2, c3))


def words(x):
    """(lo, hi) 32-bit words of unsigned 64-bit integers (Python ints or arrays)."""
    x = np.asarray(x, dtype=np.uint64)
    return x & MASK32, x >> np.uint64(32)


def philox_block(seed, step, row):
    """The Philox output block `normal3` draws for (seed, step, row): counter (row lo, row hi, step lo, step hi), key
    (seed lo, seed hi)."""
    r0, r1 = words(row)
    s0, s1 = words(step)
    k0, k1 = words(seed)
    return philox4x32_10(r0, r1, s0, s1, k0, k1)


def uniform(c):
    """u = fp32(fp32(c) * 2^-32 + 2^-33) of 32-bit words c, as float32 (no clamp)."""
    cf = np.asarray(c, dtype=np.uint32).astype(np.float32).astype(np.float64)  # (round to nearest even, like v_cvt_f32_u32)
    return (cf * 2.0**-32 + 2.0**-33).astype(np.float32)


def uniforms(seed, step, row):
    """The four fp32 uniforms of `normal3`, u0 and u2 clamped below 1."""
    c = philox_block(seed, step, row)
    u = [uniform(w) for w in c]
    u[0] = np.minimum(u[0], U_MAX)
    u[2] = np.minimum(u[2], U_MAX)
    return u


def normal3(seed, step, row):
    """(g0, g1, g2) float64 arrays of `normal3(seed, step, row)` evaluated exactly from the device's uniforms."""
    u0, u1, u2, u3 = (u.astype(np.float64) for u in uniforms(seed, step, row))
    r0 = np.sqrt(-2.0 * np.log(u0))
    r1 = np.sqrt(-2.0 * np.log(u2))
    t1, t3 = 2.0 * np.pi * u1, 2.0 * np.pi * u3
    return r0 * np.cos(t1), r0 * np.sin(t1), r1 * np.cos(t3)


def normal_fill(seed, step, n):
    """What `tmdhip_normal_fill(n, seed, step)` writes: row r fills entries 3r, 3r+1, 3r+2 (the tail row is cut at n)."""
    rows = np.arange((n + 2) // 3, dtype=np.uint64)
    g = np.stack(normal3(seed, step, rows), axis=1).reshape(-1)
    return g[:n]
