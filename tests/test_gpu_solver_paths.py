"""Every solver path through the inverse-depth bound.  The non-default paths kept behind environment knobs (the fused evaluate + assemble
kernel, VIO_FUSE; residuals per thread of the evaluation, VIO_EVAL_RPT; the marginalisation's thread count; the streaming solver of windows
beyond W = 10; the persistent fallback solver) are otherwise tested on the canonical
workload only, whose depth is valid everywhere: it never reaches the bound and never runs Ceres' projected line search (ps_ls_kernel).  Here
they run the scenes of tests/test_gpu_depth_holes.py, where every solve is bounds-constrained, against the oracle with the bar the default path
meets there: every clamp, bounded landmark, line-search trial and contraction counted equal (vio_get_bound_stats), the landmark tables equal
after every frame, positions within 1e-5 m.

Each oracle sequence runs once per scene (it does not depend on the knobs), each HIP configuration once per scene; the knobs are read when the
handle is created."""
from types import SimpleNamespace

import numpy as np
import pytest

import test_gpu_depth_holes as T
import vio_ct

pytestmark = pytest.mark.gpu

KNOBS = ("VIO_FUSE", "VIO_EVAL_RPT", "VIO_MARG_THREADS", "VIO_SOLVE_MODE", "VIO_FLAGS", "VIO_BE_THREADS", "VIO_LINE_SEARCH")
OVF_CALIB_FULL, OVF_DEVIATION = 128, 512   # vio_status.overflow_flags (include/vio_abi.h)


@pytest.fixture(scope="module")
def P():
    return vio_ct.pkg()


SCENES = {
    "bound": lambda P: T._bound_scene(P),
    # (the extrinsic opens after the window fills: its solves leave the fused path.  estimate_td is not set: the drivers push the IMU 1.5
    # samples past each frame, so once td grows beyond that both sides wait for IMU and stop processing after frame 38, 26 solved frames.
    # 58 frames: at frame 58 one landmark's flags differ -- on the two-kernel default path as on the fused one, with every bound / line-search
    # count still equal: a borderline decision like the one that shortens test_near_depth_erasure_depth_holes_and_a_moving_object)
    "extrinsic": lambda P: T._bound_scene(P, n=58, estimate_extrinsic=1),
    "blind": lambda P: T._blind_scene(P),
    "max_cnt30": lambda P: T._bound_scene(P, max_cnt=30),
    "w11": lambda P: T._bound_scene(P, window_size=11),
    "w20": lambda P: T._bound_scene(P, window_size=20),
    "quirk8": lambda P: T._bound_scene(P, quirks=8),
}


class Runs:
    """scenes, oracle runs and HIP runs, each made once for the module"""

    def __init__(self, P):
        self.P, self._scene, self._oracle, self._hip = P, {}, {}, {}

    def scene(self, name):
        if name not in self._scene:
            self._scene[name] = SCENES[name](self.P)
        return self._scene[name]

    def oracle(self, name):
        if name not in self._oracle:
            cfg, sc, seq, n, frames = self.scene(name)
            lm_o, bounded = [], []

            def hook(f, orc):
                lm_o.append(orc.landmarks_ex())
                bounded.append(orc.bound_stats()[1])
            o = vio_ct.run_oracle_sequence(cfg, sc, seq, n, frames=frames, hook=hook)
            self._oracle[name] = SimpleNamespace(o=o, lm=lm_o, bound=tuple(o["oracle"].bound_stats()) + tuple(o["oracle"].line_search_stats()),
                                                 bounded=np.diff(bounded, prepend=0))
        return self._oracle[name]

    def hip(self, name, env, monkeypatch):
        key = (name, tuple(sorted(env.items())))
        if key not in self._hip:
            for k in KNOBS:
                monkeypatch.delenv(k, raising=False)
            for k, v in env.items():
                monkeypatch.setenv(k, v)
            cfg, sc, seq, n, frames = self.scene(name)
            lm, win, per_frame, kind = [], [], [], []

            def hook(f, bb):
                lm.append(bb.landmarks_ex(0))
                win.append(bb.window(0).copy())
                per_frame.append(bb.bound_stats(0))
                if f == 0:
                    kind.append(bb.solver_kind())
            b, traj, stat = vio_ct.run_hip_batch(self.P, cfg, sc, [seq], n, [frames], hook=hook)
            self._hip[key] = SimpleNamespace(traj=traj[0], stat=stat[0], lm=lm, win=np.array(win), bound=b.bound_stats(0), kind=kind[0],
                                             bounded=np.diff([x[1] for x in per_frame], prepend=0))
            del b
        return self._hip[key]


@pytest.fixture(scope="module")
def runs(P):
    return Runs(P)


def _oracle_bar(runs, name, h, pos_tol=1e-5, depth_tol=1e-4):
    """the bar of test_inverse_depth_bound_engages_identically: every count equal, tables equal, positions / depths within the tolerances"""
    r = runs.oracle(name)
    assert h.bound == r.bound, (name, "HIP (clamps, bounded, evals, contractions)", h.bound, "oracle", r.bound)
    n = runs.scene(name)[3]
    T._compare(r.o, r.lm, h.traj, h.stat, h.lm, n, pos_tol=pos_tol, depth_tol=depth_tol)


def _bound_reached(runs, name):
    """the oracle went through the branch: the bound cuts, landmarks under it in every solve, hundreds of shortened steps"""
    clamps, bounded, evals, contractions = runs.oracle(name).bound
    assert clamps > 1000 and bounded > 1000 and evals > 1000 and contractions > 500, (name, runs.oracle(name).bound)


def _same_bits(a, b):
    assert a.bound == b.bound, (a.bound, b.bound)
    assert a.win.shape == b.win.shape
    for f in range(len(a.win)):
        assert np.array_equal(a.win[f].view(np.uint64), b.win[f].view(np.uint64)), (f, float(np.abs(a.win[f] - b.win[f]).max()))


FUSE_ENVS = [{"VIO_FUSE": "1"}, {"VIO_FUSE": "2"}, {"VIO_FUSE": "3"}, {"VIO_FUSE": "1", "VIO_EVAL_RPT": "1"}]


@pytest.mark.parametrize("env", FUSE_ENVS + [{"VIO_EVAL_RPT": "1"}, {"VIO_EVAL_RPT": "4"}, {"VIO_MARG_THREADS": "256"}, {"VIO_MARG_THREADS": "512"}])
def test_solver_paths_meet_the_oracle_through_the_bound(P, runs, monkeypatch, env):
    """The bound scene (W = 10) on each path.  The fused kernel's line search must evaluate every projection residual whatever its chunking
    (VIO_FUSE = 2 / 3: two / three chunk workgroups that loop; VIO_EVAL_RPT = 1: roles of 256 residuals): a partial cost passes the Armijo
    test at once and the search is silently skipped -- far fewer contractions than the oracle.  With VIO_FUSE the canonical configuration
    makes the handle fused-only, so no flag on any frame (no 256) also says every solve ran the fused kernel."""
    _bound_reached(runs, "bound")
    h = runs.hip("bound", env, monkeypatch)
    assert h.kind == 1
    _oracle_bar(runs, "bound", h)
    if "VIO_FUSE" in env:
        assert all(s.overflow_flags == 0 for s in h.stat), [s.overflow_flags for s in h.stat]


@pytest.mark.parametrize("env,ref", [({"VIO_FUSE": "2"}, {"VIO_FUSE": "1"}), ({"VIO_FUSE": "3"}, {"VIO_FUSE": "1"})])
def test_bit_identical_paths_stay_identical_through_the_bound(P, runs, monkeypatch, env, ref):
    """The knob whose test in test_gpu_batch.py claims the same BITS on the canonical workload (fused chunk workgroups) keeps that claim on
    constrained solves: the window after every frame to the bit and every bound / line-search count equal."""
    _same_bits(runs.hip("bound", env, monkeypatch), runs.hip("bound", ref, monkeypatch))


@pytest.mark.parametrize("env", [{}, {"VIO_FUSE": "2"}])
def test_solves_that_leave_the_fused_path_meet_the_oracle(P, runs, monkeypatch, env):
    """estimate_extrinsic = 1: the extrinsic block opens once the window is full and stays open; from then on the solves need the 42-double
    records of the two-kernel path, before that (VIO_FUSE = 2) they run the fused kernel -- both inside one handle, through the bound."""
    _bound_reached(runs, "extrinsic")
    _oracle_bar(runs, "extrinsic", runs.hip("extrinsic", env, monkeypatch))


@pytest.mark.parametrize("env", [{"VIO_FUSE": "1"}, {"VIO_FUSE": "3"}])
def test_fused_paths_on_the_blinded_sensor(P, runs, monkeypatch, env):
    """The 3 m blinded scene (test_depthless_landmarks_of_a_blinded_sensor_match_the_oracle): constrained in nearly every solve, mostly one
    trial per step; its own bar (depths within 1e-6 relative)."""
    clamps, bounded, evals, contractions = runs.oracle("blind").bound
    assert bounded > 1000 and evals > 300, runs.oracle("blind").bound
    h = runs.hip("blind", env, monkeypatch)
    _oracle_bar(runs, "blind", h, depth_tol=1e-6)
    assert all(s.overflow_flags == 0 for s in h.stat), [s.overflow_flags for s in h.stat]


@pytest.mark.parametrize("env", [{}, {"VIO_FUSE": "1"}])
def test_residual_lists_within_one_fused_chunk(P, runs, monkeypatch, env):
    """max_cnt = 30: late in the sequence the residual lists fall below one fused chunk (PS_FUSE_CAP - W = 246 residuals), where the fused
    kernel runs the prior, the IMU and ONE chunk workgroup -- and its line search once evaluated no projection residual at all."""
    cfg = runs.scene("max_cnt30")[0]
    r = runs.oracle("max_cnt30")
    small = [f for f, s in enumerate(r.o["status"]) if 0 < int(s["n_residuals"]) <= 256 - cfg.window_size and r.bounded[f] > 0]
    assert len(small) >= 10, small
    _bound_reached(runs, "max_cnt30")
    h = runs.hip("max_cnt30", env, monkeypatch)
    _oracle_bar(runs, "max_cnt30", h)
    assert all(s.overflow_flags == 0 for s in h.stat), [s.overflow_flags for s in h.stat]


@pytest.mark.parametrize("name", ["w11", "w20"])
def test_streaming_solver_meets_the_oracle_through_the_bound(P, runs, monkeypatch, name):
    """Windows beyond W = 10: the phased solver with the Schur complement in HBM / L2 (ps_serial_big, solver_kind 2) and its line search."""
    _bound_reached(runs, name)
    h = runs.hip(name, {}, monkeypatch)
    assert h.kind == 2
    _oracle_bar(runs, name, h)


@pytest.mark.parametrize("env", [{"VIO_SOLVE_MODE": "0"}, {"VIO_FLAGS": "1"}])
def test_fallback_solver_clamp_only_treatment_matches_the_oracle(P, runs, monkeypatch, env):
    """reference_quirks bit 3 on both sides: the persistent fallback solver (VIO_SOLVE_MODE = 0; VIO_FLAGS = 1 forces it) treats the bound by
    clamping candidates only, as the oracle under the quirk does -- the bar of test_clamp_only_treatment_of_the_bound_is_still_available,
    with the bounded landmarks counted as well."""
    r = runs.oracle("quirk8")
    assert r.bound[2:] == (0, 0) and r.bound[0] > 1000 and r.bound[1] > 1000, r.bound
    h = runs.hip("quirk8", env, monkeypatch)
    assert h.kind == 0
    assert h.bound == r.bound, (h.bound, r.bound)
    _oracle_bar(runs, "quirk8", h, pos_tol=1e-4, depth_tol=1e-4)


def test_fallback_solver_flags_its_deviation_not_a_capacity_error(P, runs, monkeypatch):
    """Without the quirk the fallback solver still clamps only (no line search): every frame whose solve holds a bounded landmark carries
    overflow bit 512 (VIO_OVF_DEVIATION) -- never 128, which means "extrinsic-calibration history full" -- and that bit alone leaves the code
    VIO_OK and overflow_frames at 0."""
    h = runs.hip("bound", {"VIO_SOLVE_MODE": "0"}, monkeypatch)
    assert h.kind == 0
    constrained = h.bounded > 0
    assert constrained.sum() > 30, h.bounded
    flags = np.array([s.overflow_flags for s in h.stat])
    assert np.array_equal((flags & OVF_DEVIATION) != 0, constrained), (flags, h.bounded)
    assert not (flags & OVF_CALIB_FULL).any() and not (flags & ~OVF_DEVIATION).any(), flags
    assert all(s.code == P.VIO_OK for s, c in zip(h.stat, constrained) if c), [s.code for s in h.stat]
    assert h.stat[-1].overflow_frames == 0
