"""The named cases behind tests/test_pose_ref_cpu.py and tests/test_gpu_pose_edges.py: rotation vectors and matrices at the edges of
cv::Rodrigues, solvePnP problems built for one path of CvLevMarq each, correspondences for solveRelativeR.

Everything is generated from the seeds written here; the searched seeds (PNP_SIZE_SEEDS, FAR_START_SEED, CAP20_SEED) were found by running the
oracle and the host copy over seeds 0, 1, 2, ... until the oracle's trace showed the wanted path and the host's equalled it
(search_pnp_seed below shows the oracle half)."""
import mpmath as mp
import numpy as np

import pose_ref

PI = float(mp.pi)


def _rod(rv):
    th = np.linalg.norm(rv); k = rv / th
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K


def old_pnp_trials():
    """the six trials of test_gpu_vo.test_device_solvepnp_matches_oracle, draw for draw (default_rng(7))"""
    rng = np.random.default_rng(7)
    out = []
    for trial in range(6):
        n = [40, 150, 8, 220, 60, 4][trial]
        X = np.c_[rng.uniform(-2, 2, n), rng.uniform(-1.5, 1.5, n), rng.uniform(2, 6, n)]
        rv = rng.normal(0, 0.2, 3)
        R = _rod(rv)
        t = rng.normal(0, 0.3, 3)
        Y = (R @ X.T).T + t
        img = Y[:, :2] / Y[:, 2:3] + rng.normal(0, 1.0 / 460, (n, 2))
        rv0 = rv + rng.normal(0, 0.05, 3); t0 = t + rng.normal(0, 0.1, 3)
        out.append(dict(n=n, obj=np.ascontiguousarray(X), img=np.ascontiguousarray(img), rvec0=rv0, tvec0=t0))
    return out


# ------------------------------------------------------------------------------------------------------------- rotation maps
def axes():
    """name -> unit axis (float64): generic, the coordinate axes, one zero component (three ways), two components that differ in the last
    bit, all eight sign patterns"""
    g = np.array([0.3, -0.5, 0.8]); g /= np.linalg.norm(g)
    a = 0.5
    b = np.nextafter(a, 1.0)
    out = {"generic": g, "ex": np.array([1.0, 0, 0]), "ey": np.array([0, 1.0, 0]), "ez": np.array([0, 0, 1.0]),
           "zero_x": np.array([0, 0.6, 0.8]), "zero_y": np.array([0.6, 0, 0.8]), "zero_z": np.array([0.6, 0.8, 0]),
           "near_equal_xy": np.array([a, b, np.sqrt(1 - a * a - b * b)]), "near_equal_yz": np.array([np.sqrt(1 - a * a - b * b), b, a])}
    p = np.array([0.48, 0.6, 0.64])
    for s in range(8):
        sg = np.array([1 - 2 * (s & 1), 1 - 2 * ((s >> 1) & 1), 1 - 2 * ((s >> 2) & 1)], np.float64)
        out["signs_%d%d%d" % tuple(int(x < 0) for x in sg)] = sg * p
    return out


EXP_ANGLES = (0.0, 1e-16, 9e-13, 1.1e-12, 1e-8, 1.5e-8, 1e-4, 1.0, PI - 1e-9, PI, PI + 0.3, 2 * PI - 1e-6, 7.0)
LOG_ANGLES = ("0", "1e-9", "9e-6", "1.1e-5", "0.5", "pi/2", "pi-1.1e-5", "pi-9e-6", "pi-1e-7", "pi-1e-9", "pi")


def exp_cases():
    """[(name, r float64[3])]: r = angle * axis in double; the references take these doubles exactly"""
    return [("%s@%g" % (an, th), th * ax) for an, ax in axes().items() for th in EXP_ANGLES]


def _mp_angle(s):
    return mp.mpf(s) if "pi" not in s else (mp.pi / 2 if s == "pi/2" else mp.pi - mp.mpf(s[3:] or "0"))


def log_cases():
    """[(name, R float64[3][3], theta mpf)]: exp of angle * axis in mpmath (axis re-normalised there), rounded to double once"""
    out = []
    for an, ax in axes().items():
        k = [mp.mpf(float(x)) for x in ax]
        nk = mp.sqrt(sum(x * x for x in k))
        k = [x / nk for x in k]
        for s in LOG_ANGLES:
            th = _mp_angle(s)
            out.append(("%s@%s" % (an, s), pose_ref.to_np(pose_ref.exp_mp([th * x for x in k])), th))
    return out


def log_branch(R):
    """which branch of the matrix -> vector code a double matrix takes: 'regular', 'zero' (shell near 0) or 'pi' (shell near pi), and
    (sn, cs) as the code forms them"""
    r = np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    sn = np.sqrt((r @ r) * 0.25)
    cs = min(max((R[0, 0] + R[1, 1] + R[2, 2] - 1) * 0.5, -1.0), 1.0)
    return ("regular" if sn >= 1e-5 else ("zero" if cs > 0 else "pi")), float(sn), float(cs)


def jac_tolerance(th):
    """4 max(16 x 2.2e-16, e(theta)): e = theta below 1e-12 (the code returns the generators), min(theta / 2, 5.5e-17 / theta) above (the
    diagonal of I - R carries the rounding of cos theta)"""
    e = th if th < 1e-12 else min(th / 2, 5.5e-17 / th)
    return 4 * max(16 * 2.2e-16, e)


def check_exp(fn):
    """fn(mode, n, in, out) against exp_mp / dexp_mp on every exp case: (worst |dR|, worst Jacobian error / its tolerance)"""
    cases = exp_cases()
    R, dR = call_rodrigues(fn, 0, np.array([r for _, r in cases]))
    wR = wJ = 0.0
    for i, (name, r) in enumerate(cases):
        e = pose_ref.max_abs_diff(pose_ref.exp_mp(r), R[i])
        assert e <= 1e-14, (name, e)
        assert abs(np.linalg.det(R[i]) - 1) <= 1e-14 and np.abs(R[i] @ R[i].T - np.eye(3)).max() <= 1e-14, name
        dm = pose_ref.dexp_mp(r)
        ej = max(pose_ref.max_abs_diff(dm[k], dR[i][k]) for k in range(3))
        tol = jac_tolerance(float(np.linalg.norm(r)))
        assert ej <= tol, (name, ej, tol)
        wR, wJ = max(wR, e), max(wJ, ej / tol)
    return wR, wJ


def log_tolerance(branch, th, sn):
    """regular branch: 16 eps (1 + max(theta, 1) / sn): theta = acos(cs) moves by d cs / sin theta, and cs = (trace - 1) / 2 carries a few eps
    whatever the angle, so the term 1 / sn is present at small angles as it is near pi; shell near pi: 8 (pi - theta) + 1e-7"""
    return 16 * 2.2e-16 * (1 + max(th, 1.0) / sn) if branch == "regular" else 8 * (PI - th) + 1e-7


def check_log(fn, twin=None):
    cases = log_cases()
    r = call_rodrigues(fn, 1, np.array([R for _, R, _ in cases]))
    rt = None if twin is None else call_rodrigues(twin, 1, np.array([R for _, R, _ in cases]))
    seen, worst = set(), {"regular": 0.0, "pi": 0.0}
    for i, (name, R, th) in enumerate(cases):
        br, sn, _ = log_branch(R)
        seen.add(br)
        if br == "zero":
            assert not r[i].any(), (name, r[i])
            continue
        e = pose_ref.max_abs_diff(pose_ref.exp_mp(r[i]), R)
        tol = log_tolerance(br, float(th), sn)
        assert e <= tol, (name, br, e, tol)
        worst[br] = max(worst[br], e / tol)
        if br == "pi" and rt is not None:    # v and cs are exact functions of the input bits up to acos and one division: same hemisphere, same digits
            assert np.all(np.abs(r[i] - rt[i]) <= 1e-15 * np.abs(rt[i])), (name, r[i], rt[i])
    assert seen == {"regular", "zero", "pi"}
    return worst


# ------------------------------------------------------------------------------------------------------------- solvePnP
F32 = lambda a: np.asarray(a, np.float64).astype(np.float32).astype(np.float64)   # noqa: E731
PNP_SIZES = (4, 5, 63, 64, 65, 255, 256, 257, 1000)
# first seeds at which the oracle's trace shows the wanted path AND the host copy, which sums and eigen-solves in another order, shows the
# same trace: an escalation that rounding decides (a step at the optimum that changes the cost in its last bits) is not a path to compare
PNP_SIZE_SEEDS = {4: 0, 5: 0, 63: 0, 64: 1, 65: 0, 255: 0, 256: 2, 257: 0, 1000: 0}
# far_start: the first such seed whose solve also ends INSIDE the cap (seed 1 satisfies the criterion but runs into it: that is far_start_cap)
FAR_START_SEED, CAP20_SEED, FAR_START_CAP_SEED = 6, 1, 1


def _scene(rng, n, rv, t, noise=0.0, coplanar=False):
    """n points 2 .. 6 m in front of the camera of pose (rv, t); object points rounded to float as vio_stage_pnp rounds them, so that a
    noise-free image is the exact projection of the data the solvers see (up to the float rounding of the image itself)"""
    Y = np.c_[rng.uniform(-2, 2, n), rng.uniform(-1.5, 1.5, n), rng.uniform(2, 6, n)]
    if coplanar:
        Y[:, 2] = 4.0 + 0.3 * Y[:, 0] - 0.2 * Y[:, 1]
    R = np.eye(3) if np.linalg.norm(rv) == 0 else _rod(np.asarray(rv, np.float64))
    X = F32((Y - t) @ R)          # R^T (Y - t)
    Yc = X @ R.T + t
    img = Yc[:, :2] / Yc[:, 2:3] + (rng.normal(0, noise, (n, 2)) if noise > 0 else 0.0)
    return np.ascontiguousarray(X), np.ascontiguousarray(img)


def _case(name, obj, img, rv0, t0, truth, expect, about, noise_free):
    return dict(name=name, n=len(obj), obj=obj, img=img, rvec0=np.array(rv0, np.float64), tvec0=np.array(t0, np.float64), truth=truth,
                expect=expect, about=about, noise_free=noise_free)


def sized(n, seed):
    rng = np.random.default_rng(100 + n + 10000 * seed)
    rv, t = rng.normal(0, 0.2, 3), rng.normal(0, 0.3, 3)
    obj, img = _scene(rng, n, rv, t, noise=1.0 / 460)
    return obj, img, rv + rng.normal(0, 0.05, 3), t + rng.normal(0, 0.1, 3), (rv, t)


def far_start(seed):
    rng = np.random.default_rng(1000 + seed)
    rv, t = rng.normal(0, 0.2, 3), rng.normal(0, 0.3, 3)
    obj, img = _scene(rng, 40, rv, t)
    d = rng.normal(0, 1, 3); d *= 0.8 / np.linalg.norm(d)
    e = rng.normal(0, 1, 3); e *= 1.5 / np.linalg.norm(e)
    return obj, img, rv + d, t + e, (rv, t)


def cap20(seed):
    rng = np.random.default_rng(2000 + seed)
    rv, t = rng.normal(0, 0.2, 3), rng.normal(0, 0.3, 3)
    obj, img = _scene(rng, 12, rv, t, noise=2.0 / 460)
    d = rng.normal(0, 1, 3); d *= 2.5 / np.linalg.norm(d)
    e = rng.normal(0, 1, 3); e *= 4.0 / np.linalg.norm(e)
    return obj, img, rv + d, t + e, (rv, t)


def pnp_cases():
    """name -> case.  expect: predicate on the trace (iterations, lambda escalations, final lambda exponent, finite) that the oracle must
    show (tests/test_pose_ref_cpu.py) -- the path the case was built for."""
    out = []
    conv = lambda tr: 2 <= tr[0] < 20 and tr[3] == 1                                   # noqa: E731
    for n in PNP_SIZES:      # the stride loops (64 lanes, 256 threads) and the four-wave reduction; pixel noise, start as in test_gpu_vo
        obj, img, rv0, t0, truth = sized(n, PNP_SIZE_SEEDS[n])
        out.append(_case("n%d" % n, obj, img, rv0, t0, truth, lambda tr: conv(tr) and tr[1] == 0, "converges inside the cap without an escalation", False))
    rng = np.random.default_rng(31)
    rv, t = rng.normal(0, 0.2, 3), rng.normal(0, 0.3, 3)
    obj, img = _scene(rng, 60, rv, t, coplanar=True)
    out.append(_case("coplanar", obj, img, rv + rng.normal(0, 0.05, 3), t + rng.normal(0, 0.1, 3), (rv, t), conv, "object points on a plane", True))
    rng = np.random.default_rng(32)
    rv, t = rng.normal(0, 0.2, 3), rng.normal(0, 0.3, 3)
    obj, img = _scene(rng, 50, rv, t)
    out.append(_case("truth_start", obj, img, rv, t, (rv, t), lambda tr: tr[0] == 1 and tr[1] == 0 and tr[3] == 1,
                     "start at the truth: the first step is of the size of the image's float rounding, one iteration", True))
    rng = np.random.default_rng(33)
    rv, t = np.array([0.02, -0.03, 0.01]), np.array([0.05, -0.02, 0.04])
    obj, img = _scene(rng, 50, rv, t)
    out.append(_case("zero_start_small_motion", obj, img, np.zeros(3), np.zeros(3), (rv, t), conv, "prev = 0 at the first stop test, step > 0", True))
    # all zero, truth zero: Z a power of two and X, Y multiples of 1 / 8, so that the image is exact in float and every residual is exactly 0
    rng = np.random.default_rng(34)
    Z = rng.choice([2.0, 4.0], 30)
    obj = np.c_[rng.integers(-12, 13, 30) / 8.0, rng.integers(-10, 11, 30) / 8.0, Z]
    out.append(_case("zero_start_zero_truth", obj, np.ascontiguousarray(obj[:, :2] / obj[:, 2:3]), np.zeros(3), np.zeros(3),
                     (np.zeros(3), np.zeros(3)), lambda tr: tuple(tr) == (1, 0, -4, 1),
                     "prev = 0 and step = 0: cvNorm's |d| / (|prev| + DBL_EPSILON) = 0 stops after one iteration", True))
    obj, img, rv0, t0, truth = far_start(FAR_START_SEED)
    out.append(_case("far_start", obj, img, rv0, t0, truth, lambda tr: tr[1] >= 1 and tr[3] == 1, "0.8 rad and 1.5 m off: lambda escalates", True))
    obj, img, rv0, t0, truth = cap20(CAP20_SEED)
    out.append(_case("cap20", obj, img, rv0, t0, None, lambda tr: tr[0] == 20 and tr[3] == 1, "the 20-iteration cap ends the solve", False))
    for name, ang in (("truth_3rad", 3.0), ("truth_pi_plus", PI + 0.2)):
        rng = np.random.default_rng(35)
        ax = np.array([0.48, -0.6, 0.64])
        rv, t = ang * ax, rng.normal(0, 0.3, 3)
        obj, img = _scene(rng, 50, rv, t)
        out.append(_case(name, obj, img, rv + rng.normal(0, 0.05, 3), t + rng.normal(0, 0.1, 3), (rv, t), conv, "rotation vector of length %.2f" % ang, True))
    rng = np.random.default_rng(36)
    ax = np.array([0.6, 0.0, 0.8])
    rv, t = (PI - 0.05) * ax, rng.normal(0, 0.3, 3)
    obj, img = _scene(rng, 50, rv, t)
    out.append(_case("start_pi", obj, img, PI * ax, t + rng.normal(0, 0.1, 3), (rv, t), conv, "start vector of length exactly pi", True))
    # start R = I, t = (0.125, 0, 0.5): the first object point has Z = -0.5 exactly, camera z = 0 -> 1 / 0.  J^T J is all NaN, its
    # eigenvalues are NaN, the pseudo-inverse keeps none of them (cv::solve(DECOMP_SVD) back-substitutes only w_i > threshold, false for
    # NaN), the step is exactly zero, the NaN cost is not "larger", |d| / (|prev| + DBL_EPSILON) = 0: one iteration, the start pose returned
    rng = np.random.default_rng(37)
    obj, img = _scene(rng, 20, np.zeros(3), np.array([0.125, 0.0, 0.5]))
    obj[0] = [0.25, -0.125, -0.5]
    out.append(_case("z_zero", obj, img, np.zeros(3), [0.125, 0.0, 0.5], None, lambda tr: tuple(tr) == (1, 0, -4, 1),
                     "one point at camera z = 0 under the start pose: NaN normal equations, zero step, the start pose comes back", False))
    # the same far start at the first seed of all that satisfies the criterion, cap or not: 21 escalations and the cap together
    obj, img, rv0, t0, truth = far_start(FAR_START_CAP_SEED)
    out.append(_case("far_start_cap", obj, img, rv0, t0, None, lambda tr: tr[0] == 20 and tr[1] >= 20 and tr[3] == 1,
                     "0.8 rad and 1.5 m off: lambda escalates on nearly every iteration and the cap ends the solve", False))
    # a start that is not a number: every cost and every step is NaN, no test is ever true, 20 iterations, lambda down to its floor, and the
    # one case whose result is NOT finite (the finite flag's other value)
    rng = np.random.default_rng(38)
    rv, t = rng.normal(0, 0.2, 3), rng.normal(0, 0.3, 3)
    obj, img = _scene(rng, 20, rv, t)
    out.append(_case("nan_start", obj, img, [np.nan, rv[1], rv[2]], t, None, lambda tr: tuple(tr) == (20, 0, -16, 0),
                     "a NaN component in the start vector: non-finite result, every loop bounded", False))
    return {c["name"]: c for c in out}


def pnp_cost(c, rvec, tvec):
    """sum of squared residuals in float64 numpy on the data as the solvers round them"""
    X, m = F32(c["obj"]), F32(c["img"])
    R = np.eye(3) if np.linalg.norm(rvec) == 0 else _rod(np.asarray(rvec, np.float64))
    Y = X @ R.T + tvec
    return float((((Y[:, :2] / Y[:, 2:3]) - m) ** 2).sum())


def rot(rvec):
    return np.eye(3) if np.linalg.norm(rvec) == 0 else _rod(np.asarray(rvec, np.float64))


def truth_distance(c, rvec, tvec):
    """max |R - R_true|, |t - t_true| of a noise-free case"""
    return max(float(np.abs(rot(rvec) - rot(c["truth"][0])).max()), float(np.abs(tvec - c["truth"][1]).max()))


def search_pnp_seed(orc_solve, make, want, limit=2000):
    """first seed whose oracle trace satisfies want (how FAR_START_SEED / CAP20_SEED were found)"""
    for seed in range(limit):
        obj, img, rv0, t0, _ = make(seed)
        tr = orc_solve(obj, img, rv0, t0)[2]
        if want(tr):
            return seed, tr
    return None, None


# ------------------------------------------------------------------------------------------------------------- solveRelativeR
RR_SIZES = (8, 9, 63, 64, 65, 255, 256, 257)


def _relative_r_case(rs, n, noise_px, R, t, box=(3.0, 2.0, 3.0, 9.0), centre=(0.0, 0.0)):
    """test_gpu_ex_calib._relative_r_case with the cloud's box and centre as parameters"""
    Xl = np.stack([centre[0] + rs.uniform(-box[0], box[0], n), centre[1] + rs.uniform(-box[1], box[1], n), rs.uniform(box[2], box[3], n)], 1)
    Xr = (Xl - t) @ R
    xl, xr = Xl / Xl[:, 2:], Xr / Xr[:, 2:]
    xl[:, :2] += rs.normal(0, noise_px / 460.0, (n, 2))
    xr[:, :2] += rs.normal(0, noise_px / 460.0, (n, 2))
    return np.ascontiguousarray(np.hstack([xl, xr]))


def relative_r_cases():
    """name -> dict(co [n][6], tol, truth R or None, pure_translation_exact)"""
    import excalib_ref as X
    out = {}
    rs = np.random.RandomState(21)

    def add(name, co, noise_free, truth=None, exact_translation=False):
        out[name] = dict(name=name, co=co, tol=1e-9 if (noise_free and len(co) >= 15) else 1e-6, truth=truth, exact_translation=exact_translation)
    for n in RR_SIZES:
        for noise in (0.0, 0.5):
            R, t = X.rodrigues(rs.normal(0, 0.15, 3)), rs.normal(0, 0.3, 3)
            add("n%d_noise%g" % (n, noise), _relative_r_case(rs, n, noise, R, t), noise == 0.0, R if noise == 0.0 and n >= 9 else None)
    co = _relative_r_case(rs, 9, 0.0, X.rodrigues([0.1, -0.05, 0.08]), np.array([0.3, 0.1, -0.2]))
    co[8] = co[3]
    add("n9_duplicate", co, False)
    co = _relative_r_case(rs, 40, 0.0, X.rodrigues([0.1, -0.05, 0.08]), np.array([0.3, 0.1, -0.2]))
    co[:, 0:3] = co[0, 0:3]
    add("left_identical", co, False)
    for name, t in (("sideways", np.array([0.4, 0.0, 0.0])), ("forward", np.array([0.0, 0.0, 0.5]))):
        for noise in (0.0, 0.5):
            add("translation_%s_noise%g" % (name, noise), _relative_r_case(rs, 100, noise, np.eye(3), t), noise == 0.0, np.eye(3) if noise == 0.0 else None,
                exact_translation=noise == 0.0)
    for deg in (30, 60, 90):    # yaw about the camera's y axis; the cloud sits between the two optical axes so that both views see it in front
        a = np.radians(deg)
        R = X.rodrigues([0.0, a, 0.0])
        c = 6.0 * np.tan(a / 2)
        add("rot%d" % deg, _relative_r_case(rs, 100, 0.0, R, np.array([0.3, 0.1, -0.2]), box=(1.0, 1.5, 5.0, 7.0), centre=(c, 0.0)), True, R)
    # wide angle: normalised coordinates up to 20 (KB / MEI slots), 60 of the 300 right points exchanged at random
    R, t = X.rodrigues([0.05, 0.1, -0.02]), np.array([0.3, -0.1, 0.2])
    Xl = np.stack([rs.uniform(-20, 20, 300), rs.uniform(-20, 20, 300), np.ones(300)], 1) * rs.uniform(3, 9, (300, 1))
    Xr = (Xl - t) @ R
    co = np.ascontiguousarray(np.hstack([Xl / Xl[:, 2:], Xr / Xr[:, 2:]]))
    bad = rs.permutation(300)[:60]
    co[bad, 3:6] = co[np.roll(bad, 7), 3:6]
    add("wide_angle", co, False)
    return out


# ------------------------------------------------------------------------------------------------------------- callers
def call_pnp(fn, c_or_obj, img=None, rv0=None, t0=None):
    """fn(n, obj, img, rvec, tvec, trace4) of the oracle, the host or the device: (rvec, tvec, trace tuple)"""
    if img is None:
        c_or_obj, img, rv0, t0 = c_or_obj["obj"], c_or_obj["img"], c_or_obj["rvec0"], c_or_obj["tvec0"]
    obj, img = np.ascontiguousarray(c_or_obj, np.float64), np.ascontiguousarray(img, np.float64)
    r, t, tr = np.array(rv0, np.float64), np.array(t0, np.float64), np.zeros(4, np.int32)
    fn(len(obj), obj.ctypes.data, img.ctypes.data, r.ctypes.data, t.ctypes.data, tr.ctypes.data)
    return r, t, tuple(int(x) for x in tr)


def call_rodrigues(fn, mode, x):
    """fn(mode, n, in, out): mode 0 x [n][3] -> (R [n][3][3], dR [n][3][3][3]); mode 1 x [n][3][3] -> r [n][3]"""
    x = np.ascontiguousarray(x, np.float64)
    n = len(x)
    out = np.full((n, 36 if mode == 0 else 3), np.nan)
    fn(mode, n, x.ctypes.data, out.ctypes.data)
    return (out[:, :9].reshape(n, 3, 3), out[:, 9:].reshape(n, 3, 3, 3)) if mode == 0 else out


def bind(orc):
    """argument types of the oracle entries used here (the product's are in its ctypes table)"""
    import ctypes as C
    orc.ovio_solve_pnp_trace.argtypes = [C.c_int] + [C.c_void_p] * 5
    orc.ovio_rodrigues.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    orc.ovio_rodrigues.restype = None
