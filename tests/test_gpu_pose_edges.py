"""The pose solvers that run on the device inside be_ingest, at their geometric edges: cv::Rodrigues in both directions and its Jacobian
against 50-digit definitions (tests/pose_ref.py), the device solvePnP against the oracle and the host copy with the path CvLevMarq took
(vio_stage_pnp_trace), VO mode through vio_process_obs on the streams of backend_cases.VO_CASES, and solveRelativeR with what it decided
on the way (vio_stage_relative_r_detail) against the restatement on correspondences that its RANSAC rejects, pure translations, large
rotations and sizes around the 64-lane and 256-thread strides.  tests/test_pose_ref_cpu.py and tests/test_vo_cases_cpu.py hold the CPU
twins to the same tolerances and show that every case reaches its branch.  Every test prints its figures before it asserts (DESIGN.md
section 4b records them)."""
import os

import numpy as np
import pytest

import backend_cases as BC
import excalib_ref as X
import pose_cases as PC
import pose_ref as PR
import vio_ct

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pnp_stage_trials.npy")


@pytest.fixture(scope="module")
def L(P, orc):
    PC.bind(orc)
    return P.lib()


# ------------------------------------------------------------------------------------------------------------- cv::Rodrigues
def test_exponential_map_and_jacobian_match_the_definition(L):
    """every entry of R within 1e-14, det and orthogonality within 1e-14, the Jacobian within 4 max(16 eps, e(theta)) of mpmath"""
    wR, wJ = PC.check_exp(L.vio_stage_rodrigues)
    print("exp: worst |dR| %.2e, worst Jacobian error / tolerance %.3f" % (wR, wJ))


def test_logarithm_on_its_three_branches(L, orc):
    """regular branch: round trip within 16 eps (1 + max(theta, 1) / sn); shell near 0: exactly zero; shell near pi: round trip within
    8 (pi - theta) + 1e-7 and the oracle's vector to 1e-15 relative per component, the same hemisphere"""
    worst = PC.check_log(L.vio_stage_rodrigues, orc.ovio_rodrigues)
    print("log: worst round trip / tolerance, regular %.3f, shell near pi %.3f" % (worst["regular"], worst["pi"]))


# ------------------------------------------------------------------------------------------------------------- solvePnP
def test_stage_pnp_returns_the_bits_it_returned_before_the_jacobian_moved(L):
    """vio_stage_pnp on the six trials of test_gpu_vo.test_device_solvepnp_matches_oracle: the (rvec, tvec) recorded before the Jacobian of
    cv::Rodrigues moved out of pnp_refine_block's lambda into pnp_rodrigues_jac, bit for bit"""
    gold = np.load(GOLDEN)
    for i, tr in enumerate(PC.old_pnp_trials()):
        rd, td = tr["rvec0"].copy(), tr["tvec0"].copy()
        assert L.vio_stage_pnp(tr["n"], tr["obj"].ctypes.data, tr["img"].ctypes.data, rd.ctypes.data, td.ctypes.data) == 0
        assert np.array_equal(np.r_[rd, td].view(np.uint64), gold[i].view(np.uint64)), (i, np.r_[rd, td] - gold[i])
        r2, t2, _ = PC.call_pnp(L.vio_stage_pnp_trace, tr["obj"], tr["img"], tr["rvec0"], tr["tvec0"])
        assert np.array_equal(r2, rd) and np.array_equal(t2, td), i        # the traced entry runs the same arithmetic


@pytest.mark.parametrize("name", list(PC.pnp_cases()))
def test_device_solvepnp_takes_the_oracles_path(L, orc, name):
    """trace (iterations, lambda escalations, final exponent, finite) equal on device, oracle and host; poses within 1e-7 (two solves that
    both stop on FLT_EPSILON), or, where the 20-iteration cap ended the solve, a cost no larger than the oracle's x (1 + 1e-9); noise-free
    cases within twice the oracle's own distance from the truth"""
    c = PC.pnp_cases()[name]
    ro, to, tro = PC.call_pnp(orc.ovio_solve_pnp_trace, c)
    rh, th, trh = PC.call_pnp(L.vio_stage_host_pnp_trace, c)
    rd, td, trd = PC.call_pnp(L.vio_stage_pnp_trace, c)
    if not (tro[3] and trh[3] and trd[3]):      # a non-finite result: the same path, the same verdict, nothing finite to compare
        print("pnp %-24s trace device %s oracle %s host %s" % (name, trd, tro, trh))
        assert c["expect"](tro) and trd == tro and trd == trh, (name, trd, tro, trh)
        assert not np.isfinite(np.r_[rd, td]).all() and not np.isfinite(np.r_[ro, to]).all() and not np.isfinite(np.r_[rh, th]).all()
        return
    dR, dt = float(np.abs(PC.rot(rd) - PC.rot(ro)).max()), float(np.abs(td - to).max())
    print("pnp %-24s trace device %s oracle %s host %s |dR| %.2e |dt| %.2e" % (name, trd, tro, trh, dR, dt), end="")
    if c["noise_free"]:
        print(" from the truth: device %.3e oracle %.3e" % (PC.truth_distance(c, rd, td), PC.truth_distance(c, ro, to)), end="")
    print()
    assert c["expect"](tro), (name, tro)
    assert trd == tro and trd == trh, (name, trd, tro, trh)
    if name == "z_zero":      # NaN normal equations: nothing of them is kept, the step is zero and the start pose comes back, bit for bit
        assert np.array_equal(rd, c["rvec0"]) and np.array_equal(td, c["tvec0"]) and np.array_equal(ro, rd) and np.array_equal(to, td)
        return
    if trd[0] == 20:
        cd, co = PC.pnp_cost(c, rd, td), PC.pnp_cost(c, ro, to)
        print("    cost device %.12e oracle %.12e" % (cd, co))
        assert cd <= co * (1 + 1e-9), (cd, co)
    else:
        assert dR < 1e-7 and dt < 1e-7, (name, dR, dt)
    if c["noise_free"]:
        assert PC.truth_distance(c, rd, td) <= 2 * PC.truth_distance(c, ro, to), name


# ------------------------------------------------------------------------------------------------------------- VO streams
_oracle_vo = {}


def _run_hip_vo(P, st):
    b = P.VioBatch(st.cfg, 1)
    out = []
    for stamp, ids, obs, depth, _ in st.frames():
        b.process_obs(0, ids, obs, depth, stamp)
        s = b.status(0)
        out.append(dict(status={k: getattr(s, k) for k, _ in s._fields_}, window=b.window(0).copy()))
    b.close()
    return out


@pytest.mark.parametrize("name", list(BC.VO_CASES))
def test_vo_stream_matches_oracle(P, name):
    """after every frame: the status decisions equal, window positions within 5e-4 m of the oracle (test_vo_pipeline_matches_oracle's bound:
    each frame starts from a solvePnP pose the two reach with 1e-7 differences, and the solver's 1e-6 function tolerance turns those into
    1e-5 .. 1e-4 m), the first solve within 1e-9, no speed or bias state, no overflow; slot 0 (constant in VO mode) is, on a frame that
    drops the second-newest slot, the slot 0 of the frame before: the position bit for bit, the quaternion within 4 eps (the pose goes
    matrix -> quaternion -> matrix around every solve, on the oracle too, which moves the last bit of a component)"""
    st = BC.build_vo(name, P)
    if name not in _oracle_vo:
        _oracle_vo[name] = BC.run_oracle_vo(st)
    ref, hip = _oracle_vo[name], _run_hip_vo(P, st)
    W = st.cfg.window_size
    worst, first, bad = 0.0, None, []
    for k, (ro, rh) in enumerate(zip(ref, hip)):
        so, sh = ro["status"], rh["status"]
        for key in BC.STATUS_KEYS:
            if key == "marginalization_flag" and not (sh["solver_flag"] == 1 and sh["processed"]):
                continue
            if int(so[key]) != int(sh[key]):
                bad.append("frame %d: %s oracle %d hip %d" % (k, key, int(so[key]), int(sh[key])))
        d = float(np.abs(ro["window"][:, :3] - rh["window"][:, :3]).max())
        worst = max(worst, d)
        if k == W:
            first = d
        assert sh["overflow_flags"] == 0 and np.abs(rh["window"][:, 7:16]).max() == 0, k
        if k > W and sh["marginalization_flag"] == 1:       # position copied, attitude through matrix -> quaternion -> matrix (as the oracle's is)
            assert np.array_equal(rh["window"][0, :3], hip[k - 1]["window"][0, :3]), k
            assert np.abs(rh["window"][0, 3:7] - hip[k - 1]["window"][0, 3:7]).max() <= 4 * 2.2e-16, k
    print("vo %-22s %d frames, first solve |dP| %.2e, worst |dP| %.2e m" % (name, len(hip), first, worst))
    assert not bad, bad[:5]
    assert first < 1e-9 and worst < 5e-4, (first, worst)
    if name == "vo_half_turn":
        err = lambda run: max(float(np.abs(r["window"][-1, :3] - st.scene.pose(st.stamps[i])[0]).max()) for i, r in enumerate(run) if i >= W)   # noqa: E731
        print("    distance from the true trajectory: hip %.4e oracle %.4e m" % (err(hip), err(ref)))
        assert err(hip) <= 2 * err(ref)


def test_vo_first_solve_from_a_far_start(P):
    """vo_moving_start: the rig moves 0.4 m through the initialisation window, the first VO solve starts from copies of the first pose at
    cost 403.  One landmark enters that solve free, with depth -1 and, the poses being identical, no baseline: its gradient is a rounding
    residue, the damping 1e-14 is all its step is divided by, and the step comes out of order 1 with a size and sign that depend on how
    the factor is written (tests/test_vo_cases_cpu.py shows both on the oracle).  So the first ITERATION is what the
    two must share: with the solve capped at one iteration the decisions and counts are equal and every pose of the window agrees within 1e-9
    (measured on the MI355X: |dP| 2.6e-15 m, |dq| 2.3e-16, initial cost 403.4357537 on both; the landmark went to depth 0.286 on the oracle
    and -0.682 on the device).  Uncapped, the two then follow different paths to different minima (cost 1.63 against 29.7 after the same 7
    iterations, positions 4.2e-4 m apart, 0.23 m a frame later): that difference is the landmark's first step, not the pose solver's."""
    st = BC.vo_moving_start(P)
    st.cfg.max_iterations = 1
    W = st.cfg.window_size
    o = vio_ct.OraclePipeline(st.cfg)
    b = P.VioBatch(st.cfg, 1)
    for stamp, ids, obs, depth, _ in st.frames()[:W + 1]:
        o.process_obs(ids, obs, BC.oracle_depth(depth), stamp)
        b.process_obs(0, ids, obs, depth, stamp)
    so, s, wo, w = o.status(), b.status(0), o.window(), b.window(0)
    b.close()
    dP, dq = float(np.abs(wo[:, :3] - w[:, :3]).max()), float(np.abs(wo[:, 3:7] - w[:, 3:7]).max())
    print("vo far start, one iteration: cost %.10e / %.10e -> %.6e / %.6e, |dP| %.2e |dq| %.2e" % (so["initial_cost"], s.initial_cost,
                                                                                                  so["final_cost"], s.final_cost, dP, dq))
    assert [int(so[k]) for k in BC.STATUS_KEYS] == [int(getattr(s, k)) for k in BC.STATUS_KEYS]
    assert s.iterations == 1 and s.successful_steps == 1 and s.n_var_landmarks == 1 and s.initial_cost > 400
    assert abs(so["initial_cost"] - s.initial_cost) <= 1e-12 * s.initial_cost
    assert dP < 1e-9 and dq < 1e-9, (dP, dq)


# ------------------------------------------------------------------------------------------------------------- solveRelativeR
def _device_relative_r(L, co):
    R, d = np.full(9, 7.0), np.full(8, -1, np.int32)
    rc = L.vio_stage_relative_r_detail(len(co), co.ctypes.data, R.ctypes.data, d.ctypes.data)
    return rc, R.reshape(3, 3), dict(found=int(d[0]), inliers=int(d[1]), cnt=tuple(int(x) for x in d[2:6]), win=int(d[6]), flip=int(d[7]))


def _check_relative_r(P, L, orc, c):
    co = c["co"]
    mask = PR.ransac_mask(orc, P, co) if len(co) >= 9 else None
    ref, d = PR.solve_relative_r(co, mask)
    rc, dev, dd = _device_relative_r(L, co)
    diff = float(np.abs(dev - ref).max())
    print("relative_r %-30s n %4d inliers %4d votes %s win %d |dR| %.2e" % (c["name"], len(co), dd["inliers"], dd["cnt"], dd["win"], diff))
    assert rc == 0
    assert (dd["found"], dd["inliers"], dd["cnt"]) == (d["found"], d["inliers"], tuple(d["cnt"])), (c["name"], dd, d)
    near = d["F22"] is not None and abs(abs(d["F22"]) - X.FLT_EPS) <= 10 * X.FLT_EPS
    if not near:          # (a sign change of F swaps the labels R1 / R2 and the flip, not the answer)
        assert (dd["win"], dd["flip"]) == (d["win"], d["flip"]), (c["name"], dd, d)
    else:
        assert c["exact_translation"]
    assert diff < c["tol"], (c["name"], diff, c["tol"])
    if not d["found"]:
        assert np.array_equal(dev, np.eye(3))


def test_relative_r_matches_the_restatement_on_hard_inputs(P, L, orc):
    """found flag, RANSAC inlier count and the four votes equal the restatement's (its inlier mask is the oracle sampler's); R1 / R2 label
    and sign flip equal too, except in the noise-free pure translations where F(2,2) vanishes; the matrix within 1e-9 (noise-free, n >= 15)
    or 1e-6"""
    for c in PC.relative_r_cases().values():
        _check_relative_r(P, L, orc, c)


def test_relative_r_capacity_edge(P, L, orc):
    """vio_stage_relative_r needs 40 n + 64 bytes of dynamic LDS next to its static state: the largest n it accepts (found by bisection over
    the return code: a refused call launches nothing) still equals the restatement, n = 5000 (200 064 bytes, above the 160 KB a workgroup
    can have) returns VIO_ECAPACITY, leaves R9 untouched and leaves no error behind for the next call"""
    rs = np.random.RandomState(23)
    co = PC._relative_r_case(rs, 5000, 0.0, X.rodrigues([0.1, -0.05, 0.08]), np.array([0.3, 0.1, -0.2]))
    rc, R, _ = _device_relative_r(L, co)
    assert rc == -3        # VIO_ECAPACITY
    assert np.array_equal(R, np.full((3, 3), 7.0))
    R = np.full(9, 7.0)
    assert L.vio_stage_relative_r(5000, co.ctypes.data, R.ctypes.data) == -3 and np.array_equal(R, np.full(9, 7.0))
    lo, hi = 257, 5000                     # accepted, refused
    while hi - lo > 1:
        mid = (lo + hi) // 2
        sub = np.ascontiguousarray(co[:mid])
        if _device_relative_r(L, sub)[0] == 0:
            lo = mid
        else:
            hi = mid
    print("relative_r: largest n accepted %d (%d bytes of dynamic LDS)" % (lo, 40 * lo + 64))
    # a refusal leaves nothing behind in the runtime: an entry point that ends with hipGetLastError() (vio_process_obs) still succeeds
    _run_hip_vo(P, BC.build_vo("vo_identity_extrinsic", P))
    assert hi == lo + 1 and 40 * lo + 64 <= 160 * 1024          # (the static state comes on top of the dynamic bytes)
    _check_relative_r(P, L, orc, dict(name="largest_n", co=np.ascontiguousarray(co[:lo]), tol=1e-9, exact_translation=False))
