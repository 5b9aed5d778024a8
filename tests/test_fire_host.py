"""CPU tests (no GPU) of the FIRE minimiser: the two C symbols and their argument checks, the numpy model of tests/_fire.py
against hand-computed iterations of a 1-D harmonic well, the check-point / rewind logic of `minimize_fire` with a stubbed
list check, the refusals that need no device, and the driver's `minimizer` key."""

import ctypes as C
import os
import re

import numpy as np
import pytest

import _fire as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _params(L, **kw):
    p = L.FireParams()
    p.struct_size = C.sizeof(L.FireParams)
    p.n_min, p.f_tol, p.dt_start, p.dt_max, p.max_step = 5, 0.5, 0.02, 0.2, 0.1
    p.f_inc, p.f_dec, p.alpha_start, p.f_alpha = 1.1, 0.5, 0.1, 0.99
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def test_abi_symbols_and_argument_checks():
    from torchmd_amd import _build, _lib as L

    header = open(os.path.join(ROOT, "include", "tmdhip.h")).read()
    declared = set(re.findall(r"\b(tmdhip_[a-z0-9_]+)\s*\(", header))
    for name in ("tmdhip_fire_init", "tmdhip_fire_step"):
        assert name in declared and name in L.SIGNATURES
    assert int(re.search(r"#define\s+TMDHIP_ABI_VERSION\s+(\d+)", header).group(1)) == L.ABI_VERSION == 11
    assert int(re.search(r"#define\s+TMDHIP_FIRE_STATE_DOUBLES\s+(\d+)", header).group(1)) == L.FIRE_STATE_DOUBLES
    assert int(re.search(r"#define\s+TMDHIP_FIRE_MAX_BLOCKS\s+(\d+)", header).group(1)) == L.FIRE_MAX_BLOCKS
    assert "fire.hip" in _build.SOURCES
    lib = L.load()
    assert lib.tmdhip_abi_version() == 11
    # argument validation happens before any HIP call
    ok = _params(L)
    assert lib.tmdhip_fire_step(7, 1, 4, None, None, None, None, None, None, C.byref(ok), 0, None) < 0 and "dtype" in L.last_error()
    assert lib.tmdhip_fire_step(L.F64, 1, 4, None, None, None, None, None, None, C.byref(ok), 0, None) < 0 and "null" in L.last_error()
    assert lib.tmdhip_fire_step(L.F64, 0, 4, None, None, None, None, None, None, C.byref(ok), 0, None) < 0
    assert lib.tmdhip_fire_step(L.F64, 1, 4, None, None, None, None, None, None, None, 0, None) < 0
    assert lib.tmdhip_fire_init(1, None, C.byref(ok), None) < 0 and "null" in L.last_error()
    assert lib.tmdhip_fire_init(0, None, C.byref(ok), None) < 0
    for bad in (dict(struct_size=8), dict(f_tol=0.0), dict(f_dec=1.5), dict(dt_max=0.01), dict(max_step=0.0), dict(f_inc=0.9)):
        assert lib.tmdhip_fire_init(1, None, C.byref(_params(L, **bad)), None) < 0, bad
        assert "tmdhip_fire_params" in L.last_error() or "need f_tol" in L.last_error()


def _well(x=1.0, k=1.0, m=1.0, **kw):
    """One atom in U = k x^2 / 2 along x (and a massless row that must stay as it is)."""
    prm = M.Params(f_tol=1e-3, dt_start=0.1, dt_max=1.0, max_step=10.0, n_min=2, **kw)
    pos = np.array([[x, 0.0, 0.0], [5.0, 6.0, 7.0]])
    vel = np.array([[0.0, 0.0, 0.0], [8.0, 9.0, 10.0]])
    mass = np.array([m, 0.0])

    def force():
        f = -k * pos
        f[1] = 123.0  # a site row: whatever it holds, it is never read
        return f

    return prm, pos, vel, mass, force, M.init(prm)


def test_model_first_iterations_by_hand():
    prm, pos, vel, mass, force, st = _well()
    # iteration 0: v = 0, so P = 0 is not positive: dt halves; v = dt F / m = 0.05 * -1; x = 1 + 0.05 * -0.05
    assert M.step(pos, vel, force(), mass, st, prm) == "uphill"
    assert (st.dt, st.alpha, st.npos, st.nuphill, st.iterations, st.done, st.fmax) == (0.05, 0.1, 0, 1, 1, 0, 1.0)
    assert vel[0, 0] == pytest.approx(-0.05, abs=1e-17) and pos[0, 0] == pytest.approx(0.9975, abs=1e-16)
    # iteration 1: F = -0.9975, P > 0; in one dimension the mixing leaves v as it is (0.9 * -0.05 + 0.1 * 0.05 * -1)
    assert M.step(pos, vel, force(), mass, st, prm) == "downhill"
    assert (st.dt, st.alpha, st.npos, st.nuphill, st.iterations) == (0.05, 0.1, 1, 1, 2)
    assert st.fmax == pytest.approx(0.9975, abs=1e-16)
    assert vel[0, 0] == pytest.approx(-0.05 + 0.05 * -0.9975, abs=1e-16)  # -0.099875
    assert pos[0, 0] == pytest.approx(0.9975 - 0.05 * 0.099875, abs=1e-15)  # 0.99250625
    # iteration 2: npos = 2 is not above n_min = 2: dt and alpha stay
    assert M.step(pos, vel, force(), mass, st, prm) == "downhill"
    assert (st.dt, st.alpha, st.npos) == (0.05, 0.1, 2)
    # iteration 3: npos = 3 > n_min: dt grows, alpha shrinks, and the Euler step already uses the new dt
    v2, x2 = vel[0, 0], pos[0, 0]
    assert M.step(pos, vel, force(), mass, st, prm) == "downhill"
    assert st.dt == 0.05 * 1.1 and st.alpha == 0.1 * 0.99 and st.npos == 3
    v3 = v2 + (0.05 * 1.1) * -x2
    assert vel[0, 0] == pytest.approx(v3, abs=1e-15) and pos[0, 0] == pytest.approx(x2 + 0.05 * 1.1 * v3, abs=1e-15)
    # the massless row: never read, never written
    assert pos[1].tolist() == [5.0, 6.0, 7.0] and vel[1].tolist() == [8.0, 9.0, 10.0]


def test_model_uphill_reset_dt_ceiling_and_convergence():
    prm, pos, vel, mass, force, st = _well()
    branches, dts = [], []
    for it in range(400):
        before = (st.dt, pos[0, 0], vel[0, 0])
        b = M.step(pos, vel, force(), mass, st, prm)
        branches.append(b)
        dts.append(st.dt)
        if b == "uphill" and it > 0:  # the overshoot: F changed sign against v
            assert before[1] * before[2] > 0  # moving away from the minimum
            assert st.dt == before[0] * 0.5 and st.alpha == 0.1 and st.npos == 0
            assert vel[0, 0] == pytest.approx(st.dt * -before[1], abs=1e-15)  # v was dropped, then one kick
        if b == "converged":
            break
    assert branches[-1] == "converged" and st.done == 1 and st.fmax < prm.f_tol
    assert st.nuphill >= 2 and branches.count("uphill") == st.nuphill
    assert st.iterations == len(branches) - 1  # the converging call moves nothing
    assert max(dts) <= prm.dt_max
    snap = (pos.copy(), vel.copy(), st.as_row())
    assert M.step(pos, vel, force(), mass, st, prm) == "done"  # frozen
    assert np.array_equal(pos, snap[0]) and np.array_equal(vel, snap[1]) and np.array_equal(st.as_row(), snap[2])
    # dt stops at dt_max
    prm2, pos2, vel2, mass2, force2, st2 = _well(x=100.0, k=1e-4)
    prm2.dt_max = 0.1  # 0.05 * 1.1^8 > 0.1: reached at the tenth downhill iteration
    for _ in range(12):
        M.step(pos2, vel2, force2(), mass2, st2, prm2)
    assert st2.dt == 0.1 and st2.npos > prm2.n_min + 2


def test_model_step_cap_and_float32_store():
    prm, pos, vel, mass, force, st = _well()
    prm.max_step = 0.001
    M.step(pos, vel, force(), mass, st, prm)
    # dt = 0.05, v = -0.05: |v| dt = 0.0025 > 0.001, so v is scaled to max_step / dt = 0.02 and the atom moves max_step
    assert vel[0, 0] == pytest.approx(-0.02, abs=1e-16) and pos[0, 0] == pytest.approx(0.999, abs=1e-15)
    # three dimensions: the cap is on the norm, the direction stays
    prm3 = M.Params(f_tol=1e-3, dt_start=0.1, dt_max=1.0, max_step=0.01)
    p3, v3, m3 = np.array([[3.0, 4.0, 12.0]]), np.zeros((1, 3)), np.array([2.0])
    st3 = M.init(prm3)
    M.step(p3, v3, -p3.copy(), m3, st3, prm3)
    assert np.linalg.norm(v3[0]) * st3.dt == pytest.approx(0.01, rel=1e-14)
    assert np.allclose(v3[0] / np.linalg.norm(v3[0]), -np.array([3.0, 4.0, 12.0]) / 13.0, atol=1e-15)
    # float32 storage: computed in double, rounded once
    prm, pos, vel, mass, force, st = _well(x=1.0 / 3.0)
    pos32, vel32 = pos.astype(np.float32), vel.astype(np.float32)
    f32 = (-1.0 * pos32).astype(np.float32)
    M.step(pos32, vel32, f32, mass.astype(np.float32), st, prm, store=np.float32)
    assert pos32.dtype == np.float32 and vel32.dtype == np.float32
    x, f = float(np.float32(1.0 / 3.0)), float(f32[0, 0])
    assert vel32[0, 0] == np.float32(0.05 * f) and pos32[0, 0] == np.float32(x + 0.05 * (0.05 * f))


class _StubOps:
    """`_fire_segments` against a plain object: positions are one number, an iteration adds one."""

    def __init__(self, fail_at=(), done_at=None):
        self.x, self.saved, self.calls, self.log = 0, None, 0, []
        self.fail_at, self.done_at = list(fail_at), done_at

    def save(self):
        self.saved = self.x
        self.log.append(("save", self.x))

    def restore(self):
        self.x = self.saved
        self.log.append(("restore", self.x))

    def invalidate(self):
        self.log.append(("invalidate",))

    def advance(self, first, n):
        assert first == self.x  # a repeated stretch starts from its check point
        self.x += n
        self.log.append(("advance", first, n))

    def verify(self):
        self.calls += 1
        return self.calls not in self.fail_at

    def all_done(self):
        return self.done_at is not None and self.x >= self.done_at

    def error(self):
        return "a list outlived its skin"


def test_segments_checkpoints_rewind_and_second_failure():
    from torchmd_amd.minimizers import _fire_segments

    ops = _StubOps()
    assert _fire_segments(ops, 120, 50) == 120
    assert ops.log == [("save", 0), ("advance", 0, 50), ("save", 50), ("advance", 50, 50), ("save", 100), ("advance", 100, 20)]
    assert ops.calls == 3  # one list check per stretch, the last (short) one included
    # every replica done at the second look: the loop stops there
    ops = _StubOps(done_at=70)
    assert _fire_segments(ops, 1000, 50) == 100 and ops.calls == 2
    # the second stretch fails once: back to its check point, lists dropped, repeated, and on
    ops = _StubOps(fail_at=[2])
    assert _fire_segments(ops, 120, 50) == 120
    assert ops.log == [("save", 0), ("advance", 0, 50), ("save", 50), ("advance", 50, 50), ("restore", 50), ("invalidate",),
                       ("advance", 50, 50), ("save", 100), ("advance", 100, 20)]
    # it fails again: RuntimeError with the library's message, positions at the check point
    ops = _StubOps(fail_at=[2, 3])
    with pytest.raises(RuntimeError, match="a list outlived its skin"):
        _fire_segments(ops, 120, 50)
    assert ops.x == 50 and ops.log[-1] == ("restore", 50)


def test_refusals_that_need_no_device():
    from types import SimpleNamespace

    from torchmd_amd import minimizers
    from torchmd_amd.minimizers import FireResult, minimize_fire

    duck = SimpleNamespace(compute=lambda pos, box, forces: [0.0])
    assert minimize_fire(None, duck, steps=0) is None
    with pytest.raises(ValueError, match="Forces"):
        minimize_fire(SimpleNamespace(), duck, steps=10)
    assert {"converged", "iterations", "fmax", "nuphill"} <= set(FireResult.__dataclass_fields__)
    import torchmd_amd.compat as compat

    assert "minimizers" in compat.MIRRORS and hasattr(minimizers, "minimize_fire")


def test_run_py_minimizer_key(tmp_path):
    from torchmd_amd import run as driver

    base = ["--log-dir", str(tmp_path / "a"), "--steps", "100", "--output-period", "10"]
    args = driver.get_args(base)
    assert args.minimizer == "bfgs" and args.minimize is None  # the default: what `minimize` ran before
    args = driver.get_args(base + ["--minimizer", "fire", "--minimize", "200"])
    assert args.minimizer == "fire" and int(args.minimize) == 200
    conf = tmp_path / "conf.yaml"
    conf.write_text(f"minimizer: FIRE\nminimize: 50\nsteps: 100\noutput_period: 10\nlog_dir: {tmp_path / 'b'}\n")
    args = driver.get_args(["--conf", str(conf)])
    assert args.minimizer == "fire" and args.minimize == 50
    with pytest.raises(ValueError, match="minimizer"):
        driver.get_args(base + ["--minimizer", "sd"])
