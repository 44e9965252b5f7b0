"""Named inputs for the factor tests (tests/test_factor_ref_cpu.py, tests/test_gpu_factor_edges.py): the smallest that reach each analytic edge of
the IMU pre-integration, the IMU factor, the projection factors and the pose operations.  Plain float64 numpy data; `cfg_kw` are the fields of the
default configuration a case overrides.  The constants below mirror vio_config_default (the CPU test pins them)."""
import functools

import numpy as np

import factor_ref as fr

G_NORM, HEIGHT, WIDTH, FOCAL, DEPTH_MAX = 9.805, 480, 640, 460.0, 6.0
NOISE = dict(acc_n=0.1, gyr_n=0.01, acc_w=0.001, gyr_w=0.0001)
TIC = np.array([0.17336835, 0.049596, -0.10574841])
RIC = np.array([0.02629567, -0.00713751, 0.99962873, -0.99934346, 0.02474397, 0.02646484, -0.02492368, -0.99966834, -0.00648216]).reshape(3, 3)
PI_CH, SLOT_CAP = 8, 64          # kernels.h PI_CH, vio_abi.h VIO_IMU_SLOT_CAP
INV_DEP_UB = 2.0 / DEPTH_MAX     # the solver's box on a depth-less landmark's inverse depth is (-inf, 2 / depth_max] (be_phased.h, estimator.cpp:1282-1297):
#                                  one finite end; the small side is covered by the 1e-3 case


# ---- quaternion helpers on the stored order (x y z w)
def qmul(a, b):
    ax, ay, az, aw = a
    bx, by, bz, bw = b
    return np.array([aw * bx + ax * bw + ay * bz - az * by, aw * by - ax * bz + ay * bw + az * bx, aw * bz + ax * by - ay * bx + az * bw,
                     aw * bw - ax * bx - ay * by - az * bz])


def qconj(q): return np.array([-q[0], -q[1], -q[2], q[3]])
def qrot(q, v): return qmul(qmul(q, np.r_[v, 0.0]), qconj(q))[:3]


def axis_angle(axis, deg):
    a = np.asarray(axis, float) / np.linalg.norm(axis)
    h = np.deg2rad(deg) / 2
    return np.r_[a * np.sin(h), np.cos(h)]


def q_from_R(R):
    w = np.sqrt(max(0.0, 1 + R[0, 0] + R[1, 1] + R[2, 2])) / 2
    q = np.array([(R[2, 1] - R[1, 2]) / (4 * w), (R[0, 2] - R[2, 0]) / (4 * w), (R[1, 0] - R[0, 1]) / (4 * w), w])
    return q / np.linalg.norm(q)


def rand_pose(rng, scale=1.0):
    """as tests/test_gpu_stages.py _rand_pose: qw >= 0 forced"""
    q = rng.normal(size=4); q /= np.linalg.norm(q)
    if q[3] < 0:
        q = -q
    return np.r_[rng.normal(size=3) * scale, q]


# ------------------------------------------------------------------------------------------------ IMU
def _imu_draw(seed, n, dt=None, acc_sigma=1.0, gyr_sigma=0.3):
    rng = np.random.default_rng(seed)
    dt = np.full(n, 0.005) if dt is None else np.asarray(dt, float)
    acc = rng.normal(0, acc_sigma, (n, 3)) + [0, 0, 9.8]
    gyr = rng.normal(0, gyr_sigma, (n, 3))
    acc0, gyr0 = acc[0] + 0.01, gyr[0] - 0.01
    ba, bg = rng.normal(0, 0.02, 3), rng.normal(0, 0.002, 3)
    pi, pj = rand_pose(rng), rand_pose(rng)
    sbi, sbj = rng.normal(0, 0.3, 9), rng.normal(0, 0.3, 9)
    sbi[3:] *= 0.05; sbj[3:] *= 0.05
    return dict(n=n, dt=dt, acc=acc, gyr=gyr, acc0=acc0, gyr0=gyr0, ba=ba, bg=bg, pi=pi, sbi=sbi, pj=pj, sbj=sbj, cfg_kw={}, longdouble=False)


def _float_dq(c):
    """delta_q of a case in plain float64 (x y z w), only to aim a construction; the tests measure what came out."""
    q = np.array([0.0, 0, 0, 1]); g0 = c["gyr0"]
    for k in range(c["n"]):
        w = 0.5 * (g0 + c["gyr"][k]) - c["bg"]
        q = qmul(q, np.r_[w * c["dt"][k] / 2, 1.0]); q /= np.linalg.norm(q)
        g0 = c["gyr"][k]
    return q


@functools.lru_cache(maxsize=None)
def imu_cases():
    out = {}
    b = _imu_draw(2, 20)                                  # the draw of test_gpu_stages.test_imu_factor_matches_oracle
    out["benign"] = b
    for n in (1, PI_CH - 1, PI_CH, PI_CH + 1, 2 * PI_CH + 1, SLOT_CAP, SLOT_CAP + 1):
        out["n%d" % n] = _imu_draw(100 + n, n)
    c = _imu_draw(500, 400); c["longdouble"] = True       # 2 s of samples: too long for mpmath, np.longdouble serves
    out["n400"] = c
    rng = np.random.default_rng(7)
    out["dt_spread"] = _imu_draw(8, 17, dt=np.exp(rng.uniform(np.log(1e-4), np.log(0.05), 17)))
    c = _imu_draw(9, 9)                                   # samples 4 and 8 (the last) repeat their predecessors at the same stamp: dt = 0
    for k in (4, 8):
        c["dt"][k] = 0.0; c["acc"][k] = c["acc"][k - 1]; c["gyr"][k] = c["gyr"][k - 1]
    out["dt_zero"] = c
    out["high_dynamics"] = _imu_draw(10, 17, acc_sigma=30.0, gyr_sigma=8.0)
    n = 20
    z3 = np.zeros(3)
    pose = np.r_[1.5, -2.0, 0.7, 0, 0, 0, 1.0]
    out["standstill"] = dict(n=n, dt=np.full(n, 0.005), acc=np.tile([0, 0, G_NORM], (n, 1)), gyr=np.zeros((n, 3)), acc0=np.array([0, 0, G_NORM]),
                             gyr0=z3.copy(), ba=z3.copy(), bg=z3.copy(), pi=pose.copy(), sbi=np.zeros(9), pj=pose.copy(), sbj=np.zeros(9), cfg_kw={},
                             longdouble=False)
    for name, si, sj in (("qw_neg_i", -1, 1), ("qw_neg_j", 1, -1), ("qw_neg_both", -1, -1)):
        c = _imu_draw(2, 20)
        c["pi"][3:] *= si; c["pj"][3:] *= sj
        out[name] = c
    c = _imu_draw(11, 17)                                 # corrected delta_q^-1 (Qi^-1 Qj) a rotation by 179.4 degrees
    c["pj"][3:] = qmul(qmul(c["pi"][3:], _float_dq(c)), axis_angle([0.3, -0.5, 0.8], 179.4))
    out["rot_near_pi"] = c
    c = _imu_draw(12, 17)                                 # biases far from the linearisation point: |dba| = 0.5, |dbg| = 0.2
    u, v = np.array([2.0, -1, 2]) / 3, np.array([-1.0, 2, 2]) / 3
    c["sbi"][3:6] = c["ba"] + 0.5 * u; c["sbi"][6:9] = c["bg"] + 0.2 * v
    out["bias_far"] = c
    c = _imu_draw(13, 17); c["cfg_kw"] = dict(acc_n=1.0, acc_w=1e-6, gyr_w=1e-6)
    out["noise_illcond"] = c
    c = _imu_draw(14, 17); c["cfg_kw"] = dict(acc_n=0.01, gyr_n=0.01, acc_w=0.01, gyr_w=0.01)
    out["noise_equal"] = c
    for name, c in out.items():
        c["name"] = name
        nz = dict(NOISE); nz.update(c["cfg_kw"])
        c["noise"] = (nz["acc_n"], nz["gyr_n"], nz["acc_w"], nz["gyr_w"])
        c["dbg0"] = bool(np.all(c["sbi"][6:9] == c["bg"]))
    # the Jacobian's rotation rows are derivatives only at dbg = 0 (factor_ref docstring): give every second family a twin at Bg_i = bg
    for name in ("benign", "n9", "dt_spread", "high_dynamics", "qw_neg_both", "rot_near_pi", "noise_illcond"):
        c = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in out[name].items()}
        c["sbi"][6:9] = c["bg"]; c["name"] = name + "_dbg0"; c["dbg0"] = True; c["twin_of"] = name
        out[c["name"]] = c
    return out


RING_COUNTS = (1, 2, 7, 8, 9, 16, 17, 63, 64, 65)   # the PI_CH edges, and the slot buffer one short, full and one over
RING_CAP = 80


@functools.lru_cache(maxsize=None)
def ring_case(n):
    """The first n samples of the n65 draw as be_ingest meets them (vio_stage_preint_ring): in a ring of RING_CAP entries read from the
    unwrapped position head = 2 RING_CAP - 1, so that sample 0 lies in the last entry and the others from entry 0 on (head + n exceeds the
    capacity for every n); the entries outside the interval are NaN.  Stamps at irregular intervals near an epoch time, prevTime before the
    first stamp, curTime strictly between the last two (n = 1 has only prevTime to go by).  `dt` is what numpy forms from the same stamps by
    the same float64 subtractions.  The world state is a draw of its own; its biases are the case's."""
    c = imu_cases()["n%d" % (SLOT_CAP + 1)]
    rng = np.random.default_rng(4242)
    t = 1403636580.0 + np.cumsum(0.005 * (1 + 0.2 * rng.uniform(-1, 1, SLOT_CAP + 1)))[:n]
    prev = t[0] - 0.0031
    cur = t[n - 2] + 0.4 * (t[n - 1] - t[n - 2]) if n >= 2 else t[0] - 0.001
    dt = np.r_[t[0] - prev, t[1:] - t[:-1]]
    if n >= 2:
        dt[n - 1] = cur - t[n - 2]
    head = 2 * RING_CAP - 1
    idx = (head + np.arange(n)) % RING_CAP
    rt, ra, rg = np.full(RING_CAP, np.nan), np.full((RING_CAP, 3), np.nan), np.full((RING_CAP, 3), np.nan)
    rt[idx], ra[idx], rg[idx] = t, c["acc"][:n], c["gyr"][:n]
    q = rand_pose(rng)[3:]
    R = np.array([[float(x) for x in r] for r in fr.q2R((q[3], q[0], q[1], q[2]))])
    return dict(c, n=n, dt=dt, acc=np.ascontiguousarray(c["acc"][:n]), gyr=np.ascontiguousarray(c["gyr"][:n]), name="ring%d" % n, head=head, prev=prev,
                cur=cur, ring_t=rt, ring_acc=ra, ring_gyr=rg, Ps=rng.normal(0, 2.0, 3), Vs=rng.normal(0, 0.5, 3), Rs=R, g=np.array([0.0, 0.0, G_NORM]))


@functools.lru_cache(maxsize=None)
def imu_preint_ref(name):
    """The reference pre-integration of a case, computed once per process."""
    c = imu_cases()[name]
    if "twin_of" in c:
        return imu_preint_ref(c["twin_of"])
    return fr.preint(c["dt"], c["acc"], c["gyr"], c["acc0"], c["gyr0"], c["ba"], c["bg"], c["noise"], longdouble=c["longdouble"])


# ------------------------------------------------------------------------------------------------ projection
def _proj_draw(seed, tr=0.01):
    """the recipe of test_gpu_stages.test_projection_factor_matches_oracle"""
    rng = np.random.default_rng(seed)
    pi = rand_pose(rng, 0.5); pj = pi.copy(); pj[:3] += rng.normal(0, 0.1, 3)
    dq = np.r_[rng.normal(0, 0.05, 3), 1.0]; dq /= np.linalg.norm(dq)
    pj[3:] = qmul(pi[3:], dq)
    qe = np.r_[0.5, -0.5, 0.5, -0.5] + rng.normal(0, 0.02, 4); qe /= np.linalg.norm(qe)
    ex = np.r_[TIC, qe]
    oi = np.r_[rng.uniform(-0.4, 0.4, 2), 1.0, rng.uniform(0, 640), rng.uniform(0, 480), rng.normal(0, 0.1, 2), 0.001, 2.0]
    oj = np.r_[rng.uniform(-0.4, 0.4, 2), 1.0, rng.uniform(0, 640), rng.uniform(0, 480), rng.normal(0, 0.1, 2), -0.002, 2.0]
    return dict(pi=pi, pj=pj, ex=ex, inv_dep=1.0 / rng.uniform(1.5, 6.0), td=0.003, oi=oi, oj=oj, cfg_kw=dict(tr=tr))


def _cam_j(c, pts_i=None):
    """float64 point of frame i's observation in camera j (to aim constructions)"""
    p = (c["oi"][:3] if pts_i is None else pts_i) / c["inv_dep"]
    p = qrot(c["ex"][3:], p) + c["ex"][:3]
    p = qrot(c["pi"][3:], p) + c["pi"][:3]
    p = qrot(qconj(c["pj"][3:]), p - c["pj"][:3])
    return qrot(qconj(c["ex"][3:]), p - c["ex"][:3])


def _aim_dep_j(c, dep):
    """move P_j so that the point lies at (0.1 dep, -0.2 dep, dep) in camera j (up to float64 rounding of this construction)"""
    p = c["oi"][:3] / c["inv_dep"]
    p = qrot(c["ex"][3:], p) + c["ex"][:3]
    pw = qrot(c["pi"][3:], p) + c["pi"][:3]
    pcj = np.array([0.1 * dep, -0.2 * dep, dep])
    c["pj"][:3] = pw - qrot(c["pj"][3:], qrot(c["ex"][3:], pcj) + c["ex"][:3])
    return c


@functools.lru_cache(maxsize=None)
def proj_cases():
    out = {}
    for k in range(3):
        out["draw%d" % k] = _proj_draw(3 + k)
    for tr_ in (0.0, 0.01, 0.033):                       # rolling shutter: the row term TR / ROW * (v - ROW / 2) at the image's top, centre, bottom
        for v in (0.0, HEIGHT / 2, HEIGHT - 1.0):
            c = _proj_draw(20, tr=tr_)
            c["oi"][4] = v; c["oj"][4] = HEIGHT - 1.0 - v if v != HEIGHT / 2 else v
            c["oi"][5:7] = [2.0, -1.3]; c["oj"][5:7] = [-2.0, 1.7]        # velocities up to +-2, cur_td != td on both
            out["tr%g_v%g" % (tr_, v)] = c
    for name, lam in (("invdep_ub", INV_DEP_UB), ("invdep_1e-3", 1e-3), ("invdep_10", 10.0)):
        c = _proj_draw(30); c["inv_dep"] = lam
        out[name] = c
    for name, dep in (("depj_0.05", 0.05), ("depj_0.2", 0.2), ("depj_neg", -0.7)):
        out[name] = _aim_dep_j(_proj_draw(31), dep)
    c = _proj_draw(32); c["pj"] = c["pi"].copy()          # zero baseline, Q_i = Q_j: r = sq (pts_i - pts_j), inverse-depth column 0
    out["zero_baseline"] = c
    for name, key in (("qw_neg_i", "pi"), ("qw_neg_j", "pj"), ("qw_neg_ic", "ex")):
        c = _proj_draw(33)
        if c[key][6] > 0:                                 # (the recipe's q_ic near (0.5 -0.5 0.5 | -0.5) has qw < 0 already; ex_default has qw > 0)
            c[key][3:] *= -1.0
        out[name] = c
    c = _proj_draw(34)                                    # 179 degrees between the frames, about camera i's viewing ray of the point (it stays in front of j)
    ray_body = qrot(c["ex"][3:], c["oi"][:3])
    c["pj"][3:] = qmul(c["pi"][3:], axis_angle(ray_body, 179.0)); c["pj"][:3] = c["pi"][:3] + [0.05, -0.02, 0.03]
    out["rot179"] = c
    c = _proj_draw(35); c["pi"][:3] += 1e4; c["pj"][:3] += 1e4
    out["far_origin"] = c
    c = _proj_draw(36); c["ex"] = np.r_[0, 0, 0, 0, 0, 0, 1.0]
    out["ex_identity"] = c
    c = _proj_draw(36); c["ex"] = np.r_[TIC, q_from_R(RIC)]
    out["ex_default"] = c
    for name, off in (("cauchy_r0", 0.0), ("cauchy_r1", 1.0 / (FOCAL / 1.5)), ("cauchy_r300", 1.0)):
        c = _proj_draw(37)
        p = _cam_j(c)                                     # aimed without td (with td the residual moves by the velocity terms, a few pixels)
        c["oj"][:2] = p[:2] / p[2] + [off, 0.0]
        out[name] = c
    for name, c in out.items():
        c["name"] = name
    return out


# ------------------------------------------------------------------------------------------------ pose operations
@functools.lru_cache(maxsize=None)
def plus_cases():
    """(names, x7 [n][7], d6 [n][6])"""
    rng = np.random.default_rng(50)
    x = rand_pose(rng)
    xn = rand_pose(rng); xn[3:] *= -1
    u = np.array([1.0, -2, 2]) / 3
    rows = [("d_zero", x, np.zeros(6)), ("d_1e-20", x, np.r_[6e-21 * u, 8e-21 * u]), ("rot_norm3", x, np.r_[0.1, -0.2, 0.3, 3.0 * u]),
            ("qw_neg", xn, np.r_[rng.normal(0, 0.1, 3), rng.normal(0, 0.1, 3)]), ("benign", rand_pose(rng), rng.normal(0, 0.05, 6)),
            ("unnormalised", np.r_[x[:3], 1.0000001 * x[3:]], np.zeros(6))]
    return [r[0] for r in rows], np.array([r[1] for r in rows]), np.array([r[2] for r in rows])


@functools.lru_cache(maxsize=None)
def delta_cases():
    """(names, x7, x07, expected flip): the prior's pose delta"""
    rng = np.random.default_rng(51)
    x0 = rand_pose(rng)
    ident = np.r_[0.3, -0.1, 0.2, 0, 0, 0, 1.0]
    tiny = np.array([1.0, 0, 0, -1e-9]); tiny /= np.linalg.norm(tiny)
    tinyp = np.array([1.0, 0, 0, 1e-9]); tinyp /= np.linalg.norm(tinyp)
    near = x0.copy(); near[:3] += 0.01; near[3:] = qmul(x0[3:], axis_angle([1, 2, 3], 2.0))
    rows = [("x_eq_x0", x0, x0, False), ("w_exactly_0", np.r_[0.5, 0.1, -0.2, 1.0, 0, 0, 0], ident, False),
            ("w_slightly_neg", np.r_[0.5, 0.1, -0.2, tiny], ident, True), ("w_slightly_pos", np.r_[0.5, 0.1, -0.2, tinyp], ident, False),
            ("near", near, x0, False), ("near_negated", np.r_[near[:3], -near[3:]], x0, True),
            ("far_190deg", np.r_[x0[:3], qmul(x0[3:], axis_angle([0, 1, 0], 190.0))], x0, True)]
    return [r[0] for r in rows], np.array([r[1] for r in rows]), np.array([r[2] for r in rows]), [r[3] for r in rows]


ROUND_TRIP_D = np.array([[0.0] * 6, [0.1, 0.2, -0.3, 1e-3, -2e-3, 5e-4], [0, 0, 0, 0.3, -0.2, 0.4], [1, 2, 3, 1.0, -2.0, 2.0], [0, 0, 0, 6e-21, 0, 8e-21]])


# ------------------------------------------------------------------------------------------------ running the oracle and the device on a case
def _p(a):
    return a.ctypes.data


def j20_of_46(J46):
    """[Ji(2x7) Jj(2x7) Jex(2x7) Jl(2) Jtd(2)] -> 2 x 20 rows [pose_i(6) pose_j(6) ex(6) td inv_depth]; the three 7th columns must be 0"""
    J = np.zeros((2, 20))
    for b in range(3):
        blk = J46[14 * b:14 * b + 14].reshape(2, 7)
        assert np.all(blk[:, 6] == 0)
        J[:, 6 * b:6 * b + 6] = blk[:, :6]
    J[:, 19] = J46[42:44]; J[:, 18] = J46[44:46]
    return J


def j30_of_480(J480):
    Ji, Jsi, Jj, Jsj = J480[:105].reshape(15, 7), J480[105:240].reshape(15, 9), J480[240:345].reshape(15, 7), J480[345:].reshape(15, 9)
    assert np.all(Ji[:, 6] == 0) and np.all(Jj[:, 6] == 0)
    return np.hstack([Ji[:, :6], Jsi, Jj[:, :6], Jsj])


class OraclePreint:
    """ovio_preint_* handle of a case; `set_state` replaces the integrated state (not the biases) by 461 values from elsewhere."""

    def __init__(self, orc, cfg, c, push=True):
        import ctypes as C
        self.orc, self.cfg, self.c = orc, cfg, c
        self.h = C.c_void_p(orc.ovio_preint_create(C.byref(cfg), _p(c["acc0"]), _p(c["gyr0"]), _p(c["ba"]), _p(c["bg"])))
        if push:
            for k in range(c["n"]):
                a, g = np.ascontiguousarray(c["acc"][k]), np.ascontiguousarray(c["gyr"][k])
                orc.ovio_preint_push(self.h, float(c["dt"][k]), _p(a), _p(g))

    def close(self):
        if self.h:
            self.orc.ovio_preint_destroy(self.h)
            self.h = None

    __del__ = close

    def get(self):
        o = np.zeros(461)
        self.orc.ovio_preint_get(self.h, _p(o))
        return o

    def set_state(self, o461):
        o = np.ascontiguousarray(o461, np.float64)
        self.orc.ovio_preint_set(self.h, _p(o))

    def raw(self):
        c, r, J = self.c, np.zeros(15), np.zeros(450)
        self.orc.ovio_eval_imu_raw(self.h, self.cfg.g_norm, _p(c["pi"]), _p(c["sbi"]), _p(c["pj"]), _p(c["sbj"]), _p(r), _p(J))
        return r, J.reshape(15, 30)

    def whitened(self):
        c, r, J = self.c, np.zeros(15), np.zeros(480)
        self.orc.ovio_eval_imu(self.h, self.cfg.g_norm, _p(c["pi"]), _p(c["sbi"]), _p(c["pj"]), _p(c["sbj"]), _p(r), _p(J))
        return r, j30_of_480(J)

    def sqrt_info(self):
        S = np.zeros((15, 15))
        self.orc.ovio_imu_sqrt_info(self.h, _p(S))
        return S


def oracle_projection(orc, cfg, c, use_td):
    import ctypes as C
    r, J = np.zeros(2), np.zeros(46)
    orc.ovio_eval_projection(C.byref(cfg), _p(c["pi"]), _p(c["pj"]), _p(c["ex"]), c["inv_dep"], c["td"], _p(c["oi"]), _p(c["oj"]), use_td, _p(r), _p(J))
    J = j20_of_46(J)
    if not use_td:
        J[:, 18] = 0.0          # the factor without td has no such block; the oracle leaves its slot as passed in
    return r, J


def block_ratio(got, ref, scale_of_block):
    """5 x 5: per 3 x 3 block of a 15 x 15 matrix, max |got - ref| / (eps * scale of the block); a block whose reference is exactly 0 must be
    exactly 0 (inf otherwise)."""
    out = np.zeros((5, 5))
    for i in range(5):
        for j in range(5):
            sl = (slice(3 * i, 3 * i + 3), slice(3 * j, 3 * j + 3))
            d, s = np.abs(got[sl] - ref[sl]).max(), scale_of_block(ref, sl)
            out[i, j] = 0.0 if d == 0 else (np.inf if s == 0 else d / (fr.EPS * s))
    return out


def preint_ratios(o461, ref):
    """Errors of a pre-integration against the reference in units of eps * scale: dict of dp, dq, dv (scalars: scale = the largest term that entered
    dp / dv, 1 for the unit quaternion), sum_dt, jac (5 x 5 per block, scale = the block's largest reference entry) and cov (5 x 5 per block of the
    entry-wise error over sqrt(cov_ii cov_jj))."""
    p = fr.pre_from_461(o461, ref["ba"], ref["bg"])
    d = np.sqrt(np.diag(ref["cov"]))
    D = np.outer(d, d)
    with np.errstate(divide="ignore", invalid="ignore"):
        covn = np.where(p["cov"] == ref["cov"], 0.0, np.abs(p["cov"] - ref["cov"]) / D) / fr.EPS
    return dict(dp=np.abs(p["dp"] - ref["dp"]).max() / (fr.EPS * ref["scale_p"]), dq=np.abs(p["dq"] - ref["dq"]).max() / fr.EPS,
                dv=np.abs(p["dv"] - ref["dv"]).max() / (fr.EPS * ref["scale_v"]),
                sum_dt=abs(p["sum_dt"] - ref["sum_dt"]) / (fr.EPS * max(ref["sum_dt"], np.finfo(float).tiny)),
                jac=block_ratio(p["jac"], ref["jac"], lambda R, sl: np.abs(R[sl]).max()),
                cov=np.array([[covn[3 * i:3 * i + 3, 3 * j:3 * j + 3].max() for j in range(5)] for i in range(5)]))


def gram_scaled_error(G, Gref):
    """max over entries of |G - Gref| / sqrt(Gref_ii Gref_jj), in units of eps"""
    d = np.sqrt(np.abs(np.diag(Gref)))
    D = np.outer(d, d)
    with np.errstate(divide="ignore", invalid="ignore"):
        return float(np.where(G == Gref, 0.0, np.abs(G - Gref) / D).max() / fr.EPS)


def without_last(c):
    """the case without its last sample"""
    return dict(c, n=c["n"] - 1, dt=c["dt"][:-1].copy(), acc=np.ascontiguousarray(c["acc"][:-1]), gyr=np.ascontiguousarray(c["gyr"][:-1]))


def same_but_dq(a461, b461):
    """True if two pre-integrations agree bit for bit in everything but delta_q, and there within 2 eps (a step with dt = 0 changes nothing but
    re-normalises a unit quaternion, which may move its last bit)"""
    a, b = np.asarray(a461), np.asarray(b461)
    m = np.ones(461, bool); m[3:7] = False
    return bool(np.array_equal(a[m], b[m]) and np.abs(a[3:7] - b[3:7]).max() <= 2 * fr.EPS)
