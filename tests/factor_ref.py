"""The back end's factors from their definitions, in extended precision (tests/test_factor_ref_cpu.py, tests/test_gpu_factor_edges.py).

Written from the upstream sources the device code cites -- integration_base.h (midPointIntegration, propagate, evaluate), imu_factor.h,
projection_factor.cpp / projection_td_factor.cpp, pose_local_parameterization.cpp, marginalization_factor.cpp:374-393, utility.h (deltaQ, Qleft,
Qright) -- not from csrc/be_factors.h and not from oracle/.  Everything runs in mpmath at DPS = 40 significant digits on the float64 inputs as
given, so the reference carries no float64 round-off of its own; `preint(..., longdouble=True)` is the same recursion in np.longdouble (64-bit
mantissa) for sample counts at which mpmath would take more than about ten seconds.

Eigen semantics are kept where they matter at the edges: `q * v` and toRotationMatrix() do not normalise q (the pre-integration rotates with the
un-normalised result_delta_q before propagate() normalises it), inverse() is conjugate / squared norm, deltaQ is (1, theta / 2) un-normalised.

Every formula is written once over a generic scalar.  With `S` (a value with a scale) the same code also yields the cancellation-aware scale of
each entry: a leaf's scale is its magnitude, a sum's the largest scale among its terms (and at least its own magnitude); through a product or a
quotient the scale propagates like a first-order error, scale(a b) = max(|a| scale(b), scale(a) |b|), scale(a / b) = max(scale(a) / |b|,
|a| scale(b) / b^2), so that cancellation inside a factor or a denominator (P_i - P_j at 1e4 m, a small dep_j) is carried to the entry it
amplifies.  Without cancellation the scale is the magnitude of the largest term.  A float64 evaluation of a short sum of products errs by a
small multiple of eps * scale in any association.

Jacobians are derivatives: central differences of the residuals, perturbed through `plus` in the tangent space, at 70 digits with a step of
1e-20 (truncation ~ h^2 f''' / 6, far below 1e-20 relative even for the 1 / lambda^4 third derivative at inverse depth 1e-3).  The upstream
Jacobian formulas (`imu_jacobian_formula`, `proj_jacobian_formula`) are restated as well; they supply the scales, and they ARE the reference where
upstream is not a derivative:

  * IMU factor, rotation rows (imu_factor.h:105-110, :142-145, :172-177): first-order formulas.  With dbg = Bg_i - linearized_bg != 0 the
    corrected delta_q = delta_q * deltaQ(dq_dbg dbg) is not a unit quaternion; the derivative of 2 vec(corrected^-1 (Qi^-1 Qj)) with respect to
    theta_i carries the factor 1 / |corrected|^2 of the true inverse, which -(Qleft(Qj^-1 Qi) Qright(corrected)) omits, and the Bg_i column uses
    delta_q in place of corrected (the commented-out line above it) and ignores d(1 / |corrected|^2) / dBg.  Both differ from the derivative by
    O(|dq_dbg dbg|); they are equal to it at dbg = 0.  The pose_j block, Qleft(corrected^-1 Qi^-1 Qj), is exact.
  * every other block (position, velocity and bias rows of the IMU factor; all projection columns) is an exact derivative
    (tests/test_factor_ref_cpu.py checks this on every case).
"""
import mpmath
import numpy as np
from mpmath import mpf

DPS = 40
DPS_DIFF = 70
H_DIFF = mpf(10) ** -20
EPS = float(np.finfo(np.float64).eps)
mpmath.mp.dps = max(mpmath.mp.dps, DPS)


# ------------------------------------------------------------------------------------------------ a value with its scale
class S:
    __slots__ = ("v", "s")

    def __init__(self, v, s=None):
        self.v = v
        self.s = abs(v) if s is None else s

    @staticmethod
    def of(x):
        return x if isinstance(x, S) else S(mpf(x))

    def __add__(self, o):
        o = S.of(o)
        v = self.v + o.v
        return S(v, max(self.s, o.s, abs(v)))

    __radd__ = __add__

    def __sub__(self, o):
        o = S.of(o)
        v = self.v - o.v
        return S(v, max(self.s, o.s, abs(v)))

    def __rsub__(self, o):
        return S.of(o) - self

    def __neg__(self):
        return S(-self.v, self.s)

    def __mul__(self, o):
        o = S.of(o)
        return S(self.v * o.v, max(abs(self.v) * o.s, self.s * abs(o.v)))

    __rmul__ = __mul__

    def __truediv__(self, o):
        o = S.of(o)
        return S(self.v / o.v, max(self.s / abs(o.v), abs(self.v) * o.s / (o.v * o.v)))

    def __rtruediv__(self, o):
        return S.of(o) / self


def val(x):
    return x.v if isinstance(x, S) else x


def _sqrt(x):
    if isinstance(x, S):
        return S(mpmath.sqrt(x.v), mpmath.sqrt(x.s))
    if isinstance(x, np.longdouble):
        return np.sqrt(x)
    return mpmath.sqrt(x)


# ------------------------------------------------------------------------------------------------ small algebra over a generic scalar
def add(a, b): return [x + y for x, y in zip(a, b)]
def sub(a, b): return [x - y for x, y in zip(a, b)]
def scl(s, a): return [s * x for x in a]
def dot(a, b): return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]
def cross(a, b): return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]
def skew(a): return [[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]]
def tr(A): return [[A[j][i] for j in range(len(A))] for i in range(len(A[0]))]
def mv(A, v): return [sum((A[i][k] * v[k] for k in range(1, len(v))), A[i][0] * v[0]) for i in range(len(A))]
def madd(A, B): return [[x + y for x, y in zip(r, q)] for r, q in zip(A, B)]
def msub(A, B): return [[x - y for x, y in zip(r, q)] for r, q in zip(A, B)]
def mscl(s, A): return [[s * x for x in r] for r in A]
def eye3(): return [[1, 0, 0], [0, 1, 0], [0, 0, 1]]


def _is0(x):
    return isinstance(x, int) and x == 0


def mm(A, B):
    """Matrix product that skips structural zeros (the int 0), so that block-sparse F and V stay cheap."""
    n, m, p = len(A), len(B), len(B[0])
    out = [[0] * p for _ in range(n)]
    for i in range(n):
        Ai = A[i]
        nz = [k for k in range(m) if not _is0(Ai[k])]
        for j in range(p):
            acc = 0
            for k in nz:
                b = B[k][j]
                if _is0(b):
                    continue
                t = Ai[k] * b
                acc = t if _is0(acc) else acc + t
            out[i][j] = acc
    return out


# quaternions are (w, x, y, z)
def qmul(a, b):
    return (a[0] * b[0] - a[1] * b[1] - a[2] * b[2] - a[3] * b[3], a[0] * b[1] + a[1] * b[0] + a[2] * b[3] - a[3] * b[2],
            a[0] * b[2] + a[2] * b[0] + a[3] * b[1] - a[1] * b[3], a[0] * b[3] + a[3] * b[0] + a[1] * b[2] - a[2] * b[1])


def qn2(q): return q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]
def qinv(q): n2 = qn2(q); return (q[0] / n2, -q[1] / n2, -q[2] / n2, -q[3] / n2)          # Eigen inverse(): conjugate / squaredNorm
def qnormalized(q): n = _sqrt(qn2(q)); return (q[0] / n, q[1] / n, q[2] / n, q[3] / n)
def delta_q(th): return (1, th[0] / 2, th[1] / 2, th[2] / 2)                                  # utility.h deltaQ: not normalised
def qvec(q): return [q[1], q[2], q[3]]


def qrot(q, v):
    """Eigen `q * v` (QuaternionBase::_transformVector): v + w (2 u x v) + u x (2 u x v), no normalisation of q."""
    u = qvec(q)
    uv = cross(u, v)
    uv = add(uv, uv)
    return add(add(v, scl(q[0], uv)), cross(u, uv))


def q2R(q):
    """Eigen toRotationMatrix(), no normalisation of q."""
    w, x, y, z = q
    tx, ty, tz = 2 * x, 2 * y, 2 * z
    twx, twy, twz = tx * w, ty * w, tz * w
    txx, txy, txz = tx * x, ty * x, tz * x
    tyy, tyz, tzz = ty * y, tz * y, tz * z
    return [[1 - (tyy + tzz), txy - twz, txz + twy], [txy + twz, 1 - (txx + tzz), tyz - twx], [txz - twy, tyz + twx, 1 - (txx + tyy)]]


def qleft_br(q):
    """bottom-right 3 x 3 of utility.h Qleft: w I + skew(vec)"""
    return madd(mscl(q[0], eye3()), skew(qvec(q)))


def qleft4(q):
    w, x, y, z = q
    return [[w, -x, -y, -z], [x, w, -z, y], [y, z, w, -x], [z, -y, x, w]]


def qright4(q):
    w, x, y, z = q
    return [[w, -x, -y, -z], [x, w, z, -y], [y, -z, w, x], [z, y, -x, w]]


def _num(kind):
    if kind == "mp":
        return lambda x: mpf(float(x))
    if kind == "S":
        return lambda x: S(mpf(float(x)))
    if kind == "ld":
        return lambda x: np.longdouble(float(x))
    raise ValueError(kind)


def _vec(num, a): return [num(x) for x in np.asarray(a, np.float64).ravel()]
def pose_q(p): return (p[6], p[3], p[4], p[5])          # storage (x y z qx qy qz qw)


# ------------------------------------------------------------------------------------------------ pre-integration (integration_base.h:56-162)
def _midpoint_FV(dt, dq, rq, a0, a1, w):
    """F (15 x 15) and V (15 x 18) of integration_base.h:80-127; structural zeros are the int 0."""
    Rq, Rr = q2R(dq), q2R(rq)
    Rw, Ra0, Ra1 = skew(w), skew(a0), skew(a1)
    I = eye3()
    ImW = msub(I, mscl(dt, Rw))
    RrA1 = mm(Rr, Ra1)
    F = [[0] * 15 for _ in range(15)]
    V = [[0] * 18 for _ in range(15)]

    def put(M, r, c, B):
        for i in range(3):
            for j in range(3):
                M[r + i][c + j] = B[i][j]
    put(F, 0, 0, I)
    put(F, 0, 3, madd(mscl(-0.25 * dt * dt, mm(Rq, Ra0)), mscl(-0.25 * dt * dt, mm(RrA1, ImW))))
    put(F, 0, 6, mscl(dt, I))
    put(F, 0, 9, mscl(-0.25 * dt * dt, madd(Rq, Rr)))
    put(F, 0, 12, mscl(0.25 * dt * dt * dt, RrA1))
    put(F, 3, 3, ImW)
    put(F, 3, 12, mscl(-dt, I))
    put(F, 6, 3, madd(mscl(-0.5 * dt, mm(Rq, Ra0)), mscl(-0.5 * dt, mm(RrA1, ImW))))
    put(F, 6, 6, I)
    put(F, 6, 9, mscl(-0.5 * dt, madd(Rq, Rr)))
    put(F, 6, 12, mscl(0.5 * dt * dt, RrA1))
    put(F, 9, 9, I)
    put(F, 12, 12, I)
    V03 = mscl(-0.125 * dt * dt * dt, RrA1)
    V63 = mscl(-0.25 * dt * dt, RrA1)
    put(V, 0, 0, mscl(0.25 * dt * dt, Rq)); put(V, 0, 3, V03); put(V, 0, 6, mscl(0.25 * dt * dt, Rr)); put(V, 0, 9, V03)
    put(V, 3, 3, mscl(0.5 * dt, I)); put(V, 3, 9, mscl(0.5 * dt, I))
    put(V, 6, 0, mscl(0.5 * dt, Rq)); put(V, 6, 3, V63); put(V, 6, 6, mscl(0.5 * dt, Rr)); put(V, 6, 9, V63)
    put(V, 9, 12, mscl(dt, I)); put(V, 12, 15, mscl(dt, I))
    for M in (F, V):      # scaled identities leave int zeros off the diagonal as 0 * dt: restore the structural zero
        for r in M:
            for j, x in enumerate(r):
                if not isinstance(x, int) and x == 0:
                    r[j] = 0
    return F, V


def preint(dt, acc, gyr, acc0, gyr0, ba, bg, noise, longdouble=False):
    """n x IntegrationBase::propagate from the constructor's state.  noise = (acc_n, gyr_n, acc_w, gyr_w).  Returns a dict of float64 arrays
    dp(3) dq(4: w x y z) dv(3) sum_dt jac(15 x 15) cov(15 x 15), `scale_p` / `scale_v` (the largest term that entered dp / dv), `source`, and
    `hi`: the unrounded state for the factor functions below."""
    kind = "ld" if longdouble else "mp"
    num = _num(kind)
    dt, acc, gyr = np.asarray(dt, np.float64), np.asarray(acc, np.float64).reshape(-1, 3), np.asarray(gyr, np.float64).reshape(-1, 3)
    a0, g0, lba, lbg = _vec(num, acc0), _vec(num, gyr0), _vec(num, ba), _vec(num, bg)
    nn = [num(x) * num(x) for x in noise]
    N = [nn[0]] * 3 + [nn[1]] * 3 + [nn[0]] * 3 + [nn[1]] * 3 + [nn[2]] * 3 + [nn[3]] * 3
    one, zero = num(1.0), num(0.0)
    dp, dv, dq, sdt = [zero] * 3, [zero] * 3, (one, zero, zero, zero), zero
    J = [[one if i == j else 0 for j in range(15)] for i in range(15)]
    P = [[0] * 15 for _ in range(15)]
    sp = sv = 0.0
    with mpmath.workdps(DPS):
        for k in range(len(dt)):
            h, a1, g1 = num(dt[k]), _vec(num, acc[k]), _vec(num, gyr[k])
            un_acc_0 = qrot(dq, sub(a0, lba))
            un_gyr = sub(scl(0.5, add(g0, g1)), lbg)
            rq = qmul(dq, (one, un_gyr[0] * h / 2, un_gyr[1] * h / 2, un_gyr[2] * h / 2))
            un_acc_1 = qrot(rq, sub(a1, lba))
            un_acc = scl(0.5, add(un_acc_0, un_acc_1))
            F, V = _midpoint_FV(h, dq, rq, sub(a0, lba), sub(a1, lba), un_gyr)
            inc_p, inc_v = scl(0.5 * h * h, un_acc), scl(h, un_acc)
            sp = max([sp] + [abs(float(x)) for x in dp + scl(h, dv) + inc_p])
            sv = max([sv] + [abs(float(x)) for x in dv + inc_v])
            dp = add(add(dp, scl(h, dv)), inc_p)
            dv = add(dv, inc_v)
            dq = qnormalized(rq)
            J = mm(F, J)
            VN = [[0 if _is0(V[i][c]) else V[i][c] * N[c] for c in range(18)] for i in range(15)]
            P = madd(mm(mm(F, P), tr(F)), mm(VN, tr(V)))
            sdt = sdt + h
            a0, g0 = a1, g1
    f = lambda M: np.array([[float(x) for x in r] for r in M])
    return dict(dp=np.array([float(x) for x in dp]), dq=np.array([float(x) for x in dq]), dv=np.array([float(x) for x in dv]), sum_dt=float(sdt),
                jac=f(J), cov=f(P), scale_p=max(sp, np.finfo(float).tiny), scale_v=max(sv, np.finfo(float).tiny),
                source="longdouble" if longdouble else "mpmath", ba=np.asarray(ba, np.float64), bg=np.asarray(bg, np.float64))


def process_imu(dt, acc, gyr, acc0, gyr0, P, R, V, ba, bg, g):
    """Estimator::processIMU's world-state recursion over n samples (estimator.cpp:142-152): R <- R toRotationMatrix(deltaQ(un_gyr dt)) with the
    un-normalised deltaQ, midpoint acceleration in the world frame less g.  R is 3 x 3.  Returns float64 P(3), R(3 x 3), V(3) and scale_p /
    scale_v / scale_r, the largest term that entered a sum of P / V / an entry of R (or the sum itself, if larger)."""
    num = _num("mp")
    dt, acc, gyr = np.asarray(dt, np.float64), np.asarray(acc, np.float64).reshape(-1, 3), np.asarray(gyr, np.float64).reshape(-1, 3)
    a0, g0, Ba, Bg, G = _vec(num, acc0), _vec(num, gyr0), _vec(num, ba), _vec(num, bg), _vec(num, g)
    P, V = _vec(num, P), _vec(num, V)
    R = [[num(x) for x in r] for r in np.asarray(R, np.float64).reshape(3, 3)]
    sp = sv = sr = 0.0
    with mpmath.workdps(DPS):
        for k in range(len(dt)):
            h, a1, g1 = num(dt[k]), _vec(num, acc[k]), _vec(num, gyr[k])
            un_acc_0 = sub(mv(R, sub(a0, Ba)), G)
            un_gyr = sub(scl(0.5, add(g0, g1)), Bg)
            D = q2R(delta_q(scl(h, un_gyr)))
            sr = max([sr] + [abs(float(R[i][m] * D[m][j])) for i in range(3) for j in range(3) for m in range(3)])
            R = mm(R, D)
            un_acc_1 = sub(mv(R, sub(a1, Ba)), G)
            un_acc = scl(0.5, add(un_acc_0, un_acc_1))
            inc_p, inc_v = scl(0.5 * h * h, un_acc), scl(h, un_acc)
            terms_p, terms_v = P + scl(h, V) + inc_p, V + inc_v
            P = add(add(P, scl(h, V)), inc_p)
            V = add(V, inc_v)
            sp = max([sp] + [abs(float(x)) for x in terms_p + P])
            sv = max([sv] + [abs(float(x)) for x in terms_v + V])
            a0, g0 = a1, g1
    tiny = np.finfo(float).tiny
    return dict(P=np.array([float(x) for x in P]), R=np.array([[float(x) for x in r] for r in R]), V=np.array([float(x) for x in V]),
                scale_p=max(sp, tiny), scale_v=max(sv, tiny), scale_r=max(sr, tiny))


def pre_from_461(o461, ba, bg):
    """The same dict from the 461 doubles the stage entries and the oracle return."""
    o = np.asarray(o461, np.float64)
    return dict(dp=o[0:3].copy(), dq=o[3:7].copy(), dv=o[7:10].copy(), sum_dt=float(o[10]), jac=o[11:236].reshape(15, 15).copy(),
                cov=o[236:461].reshape(15, 15).copy(), ba=np.asarray(ba, np.float64), bg=np.asarray(bg, np.float64))


def pre_to_461(pre):
    return np.r_[pre["dp"], pre["dq"], pre["dv"], pre["sum_dt"], pre["jac"].ravel(), pre["cov"].ravel()]


# ------------------------------------------------------------------------------------------------ IMU factor (integration_base.h:164-195, imu_factor.h)
O_P, O_R, O_V, O_BA, O_BG = 0, 3, 6, 9, 12


def _pre_terms(num, pre):
    Jm = [[num(x) for x in r] for r in np.asarray(pre["jac"], np.float64)]
    blk = lambda r, c: [[Jm[r + i][c + j] for j in range(3)] for i in range(3)]
    dq = tuple(_vec(num, pre["dq"]))
    return (_vec(num, pre["dp"]), dq, _vec(num, pre["dv"]), num(pre["sum_dt"]), blk(O_P, O_BA), blk(O_P, O_BG), blk(O_R, O_BG), blk(O_V, O_BA),
            blk(O_V, O_BG), _vec(num, pre["ba"]), _vec(num, pre["bg"]))


def _imu_residual_g(num, T, G, pi, sbi, pj, sbj):
    """IntegrationBase::evaluate on generic scalars (pi, sbi, pj, sbj already of the scalar type)."""
    dp, dq, dv, sdt, dp_dba, dp_dbg, dq_dbg, dv_dba, dv_dbg, lba, lbg = T
    Pi, Qi, Vi, Bai, Bgi = pi[:3], pose_q(pi), sbi[:3], sbi[3:6], sbi[6:9]
    Pj, Qj, Vj, Baj, Bgj = pj[:3], pose_q(pj), sbj[:3], sbj[3:6], sbj[6:9]
    dba, dbg = sub(Bai, lba), sub(Bgi, lbg)
    cq = qmul(dq, delta_q(mv(dq_dbg, dbg)))
    cv = add(add(dv, mv(dv_dba, dba)), mv(dv_dbg, dbg))
    cp = add(add(dp, mv(dp_dba, dba)), mv(dp_dbg, dbg))
    Qi_inv = qinv(Qi)
    rp = sub(qrot(Qi_inv, sub(sub(add(scl(0.5 * sdt * sdt, G), Pj), Pi), scl(sdt, Vi))), cp)
    rq = scl(2, qvec(qmul(qinv(cq), qmul(Qi_inv, Qj))))
    rv = sub(qrot(Qi_inv, sub(add(scl(sdt, G), Vj), Vi)), cv)
    return rp + rq + rv + sub(Baj, Bai) + sub(Bgj, Bgi)


def imu_residual(pre, g_norm, pi, sbi, pj, sbj):
    """(r15, scale15) as float64 arrays: the raw, un-whitened residual."""
    with mpmath.workdps(DPS):
        num = _num("S")
        r = _imu_residual_g(num, _pre_terms(num, pre), [0, 0, num(g_norm)], _vec(num, pi), _vec(num, sbi), _vec(num, pj), _vec(num, sbj))
        return np.array([float(x.v) for x in r]), np.array([float(x.s) for x in r])


def imu_jacobian_formula(pre, g_norm, pi, sbi, pj, sbj):
    """(J, scale), 15 x 30: the blocks of imu_factor.h:92-201 before `sqrt_info *`, in tangent coordinates (the 7th pose column dropped)."""
    with mpmath.workdps(DPS):
        num = _num("S")
        dp, dq, dv, sdt, dp_dba, dp_dbg, dq_dbg, dv_dba, dv_dbg, lba, lbg = _pre_terms(num, pre)
        G = [0, 0, num(g_norm)]
        pi, sbi, pj, sbj = _vec(num, pi), _vec(num, sbi), _vec(num, pj), _vec(num, sbj)
        Pi, Qi, Vi, Bgi, Pj, Qj, Vj = pi[:3], pose_q(pi), sbi[:3], sbi[6:9], pj[:3], pose_q(pj), sbj[:3]
        Qi_inv, Qj_inv = qinv(Qi), qinv(Qj)
        RiT = q2R(Qi_inv)
        cq = qmul(dq, delta_q(mv(dq_dbg, sub(Bgi, lbg))))
        J = [[0] * 30 for _ in range(15)]

        def put(r, c, B):
            for i in range(3):
                for j in range(3):
                    J[r + i][c + j] = B[i][j]
        neg = lambda B: mscl(-1, B)
        put(O_P, 0, neg(RiT))
        put(O_P, 3, skew(qrot(Qi_inv, sub(sub(add(scl(0.5 * sdt * sdt, G), Pj), Pi), scl(sdt, Vi)))))
        LR = mm(qleft4(qmul(Qj_inv, Qi)), qright4(cq))
        put(O_R, 3, neg([r[1:] for r in LR[1:]]))
        put(O_V, 3, skew(qrot(Qi_inv, sub(add(scl(sdt, G), Vj), Vi))))
        put(O_P, 6, mscl(-1 * sdt, RiT)); put(O_P, 9, neg(dp_dba)); put(O_P, 12, neg(dp_dbg))
        put(O_R, 12, neg(mm(qleft_br(qmul(qmul(Qj_inv, Qi), dq)), dq_dbg)))
        put(O_V, 6, neg(RiT)); put(O_V, 9, neg(dv_dba)); put(O_V, 12, neg(dv_dbg))
        put(O_BA, 9, neg(eye3())); put(O_BG, 12, neg(eye3()))
        put(O_P, 15, RiT)
        put(O_R, 18, qleft_br(qmul(qmul(qinv(cq), Qi_inv), Qj)))
        put(O_V, 21, RiT); put(O_BA, 24, eye3()); put(O_BG, 27, eye3())
        Jv = np.array([[float(val(S.of(x))) for x in r] for r in J])
        Js = np.array([[float(S.of(x).s) for x in r] for r in J])
        return Jv, Js


IMU_ZERO = np.ones((15, 30), bool)     # structurally zero entries of the raw Jacobian
for _r, _c in ((O_P, 0), (O_P, 3), (O_R, 3), (O_V, 3), (O_P, 6), (O_P, 9), (O_P, 12), (O_R, 12), (O_V, 6), (O_V, 9), (O_V, 12), (O_BA, 9),
               (O_BG, 12), (O_P, 15), (O_R, 18), (O_V, 21), (O_BA, 24), (O_BG, 27)):
    IMU_ZERO[_r:_r + 3, _c:_c + 3] = False
IMU_ROT_ROWS = np.zeros((15, 30), bool)    # the first-order blocks (module docstring): derivatives only at dbg = 0
IMU_ROT_ROWS[O_R:O_R + 3, 3:6] = True
IMU_ROT_ROWS[O_R:O_R + 3, 12:15] = True


def plus(x, d):
    """PoseLocalParameterization::Plus on generic scalars: x = (p, qx qy qz qw), d = (dp, dtheta)."""
    q = qnormalized(qmul(pose_q(x), delta_q(d[3:6])))
    return add(x[:3], d[:3]) + [q[1], q[2], q[3], q[0]]


def _central(f, args, sizes):
    """d f / d (tangent of args), central differences at DPS_DIFF digits; sizes[b] = 6: a pose perturbed through plus(), else additive."""
    cols = []
    h = H_DIFF
    for b, dim in enumerate(sizes):
        for k in range(dim):
            out = []
            for sgn in (1, -1):
                a2 = list(args)
                if dim == 6:
                    d = [mpf(0)] * 6
                    d[k] = sgn * h
                    a2[b] = plus(args[b], d)
                elif dim == 1:
                    a2[b] = args[b] + sgn * h
                else:
                    v = list(args[b])
                    v[k] = v[k] + sgn * h
                    a2[b] = v
                out.append(f(*a2))
            cols.append([(p - m) / (2 * h) for p, m in zip(out[0], out[1])])
    return np.array([[float(cols[c][r]) for c in range(len(cols))] for r in range(len(cols[0]))])


def imu_jacobian_derivative(pre, g_norm, pi, sbi, pj, sbj):
    """15 x 30: d residual / d (pose_i, speedbias_i, pose_j, speedbias_j) in the tangent space."""
    with mpmath.workdps(DPS_DIFF):
        num = _num("mp")
        T = _pre_terms(num, pre)
        G = [0, 0, num(g_norm)]
        f = lambda a, b, c, d: _imu_residual_g(num, T, G, a, b, c, d)
        return _central(f, [_vec(num, pi), _vec(num, sbi), _vec(num, pj), _vec(num, sbj)], (6, 9, 6, 9))


# ------------------------------------------------------------------------------------------------ projection (projection_td_factor.cpp:34-146)
def _proj_g(num, K, pi, pj, ex, inv_dep, td, oi, oj, use_td, want_J=False, want_dep=False):
    """K = (focal_length, ROW, TR).  oi / oj = (x y z u v vx vy cur_td depth).  Returns r (2) or (r, J 2 x 20) with columns pose_i(6) pose_j(6)
    ex(6) td inv_depth; sqrt_info = focal_length / 1.5 * I (projection_factor.cpp, ProjectionFactor::sqrt_info as the estimator sets it)."""
    sq = num(K[0]) / num(1.5)
    Pi, Qi, Pj, Qj, tic, qic = pi[:3], pose_q(pi), pj[:3], pose_q(pj), ex[:3], pose_q(ex)
    pts_i, pts_j = list(oi[:3]), list(oj[:3])
    vel_i, vel_j = [oi[5], oi[6], 0], [oj[5], oj[6], 0]
    if use_td:
        ROW, TR = num(K[1]), num(K[2])
        row_i, row_j = oi[4] - ROW / 2, oj[4] - ROW / 2          # projection_td_factor.cpp:12-13: row = pixel row - ROW / 2
        pts_i = sub(pts_i, scl(td - oi[7] + TR / ROW * row_i, vel_i))
        pts_j = sub(pts_j, scl(td - oj[7] + TR / ROW * row_j, vel_j))
    pc_i = [x / inv_dep for x in pts_i]
    p_imu_i = add(qrot(qic, pc_i), tic)
    p_w = add(qrot(Qi, p_imu_i), Pi)
    p_imu_j = qrot(qinv(Qj), sub(p_w, Pj))
    pc_j = qrot(qinv(qic), sub(p_imu_j, tic))
    dep_j = pc_j[2]
    if want_dep:
        return dep_j
    r = [sq * (pc_j[0] / dep_j - pts_j[0]), sq * (pc_j[1] / dep_j - pts_j[1])]
    if not want_J:
        return r
    Ri, Rj, ric = q2R(Qi), q2R(Qj), q2R(qic)
    red = [[sq / dep_j, 0, -1 * sq * pc_j[0] / (dep_j * dep_j)], [0, sq / dep_j, -1 * sq * pc_j[1] / (dep_j * dep_j)]]
    ricT, RjT = tr(ric), tr(Rj)
    A1 = mm(ricT, RjT)
    A2 = mm(A1, Ri)
    tmp_r = mm(A2, ric)
    J = [[0] * 20 for _ in range(2)]

    def put(c, B):
        RB = mm(red, B)
        for i in range(2):
            for j in range(len(B[0])):
                J[i][c + j] = RB[i][j]
    put(0, A1)
    put(3, mm(A2, mscl(-1, skew(p_imu_i))))
    put(6, mscl(-1, A1))
    put(9, mm(ricT, skew(p_imu_j)))
    put(12, mm(ricT, msub(mm(RjT, Ri), eye3())))
    put(15, madd(madd(mscl(-1, mm(tmp_r, skew(pc_i))), skew(mv(tmp_r, pc_i))),
                 skew(mv(ricT, sub(mv(RjT, sub(add(mv(Ri, tic), Pi), Pj)), tic)))))
    put(19, [[x * (-1 / (inv_dep * inv_dep))] for x in mv(tmp_r, pts_i)])
    if use_td:
        put(18, [[x / inv_dep * -1] for x in mv(tmp_r, vel_i)])
        J[0][18] = J[0][18] + sq * vel_j[0]
        J[1][18] = J[1][18] + sq * vel_j[1]
    return r, J


def proj_consts(cfg):
    return (float(cfg.focal_length), float(cfg.height), float(cfg.tr))


def proj_residual(K, pi, pj, ex, inv_dep, td, oi, oj, use_td):
    """(r2, scale2)"""
    with mpmath.workdps(DPS):
        num = _num("S")
        a = [_vec(num, x) for x in (pi, pj, ex)]
        r = _proj_g(num, K, a[0], a[1], a[2], num(inv_dep), num(td), _vec(num, oi), _vec(num, oj), use_td)
        return np.array([float(x.v) for x in r]), np.array([float(x.s) for x in r])


def proj_dep_j(K, pi, pj, ex, inv_dep, td, oi, oj, use_td):
    """depth of the point in camera j (pts_camera_j.z), float64"""
    with mpmath.workdps(DPS):
        num = _num("mp")
        a = [_vec(num, x) for x in (pi, pj, ex)]
        return float(_proj_g(num, K, a[0], a[1], a[2], num(inv_dep), num(td), _vec(num, oi), _vec(num, oj), use_td, want_dep=True))


def proj_jacobian_formula(K, pi, pj, ex, inv_dep, td, oi, oj, use_td):
    """(J, scale), 2 x 20, from the upstream formulas; the td column is 0 without use_td (the factor without td has no such block)."""
    with mpmath.workdps(DPS):
        num = _num("S")
        a = [_vec(num, x) for x in (pi, pj, ex)]
        _, J = _proj_g(num, K, a[0], a[1], a[2], num(inv_dep), num(td), _vec(num, oi), _vec(num, oj), use_td, True)
        return np.array([[float(val(S.of(x))) for x in r] for r in J]), np.array([[float(S.of(x).s) for x in r] for r in J])


def proj_jacobian_derivative(K, pi, pj, ex, inv_dep, td, oi, oj, use_td):
    """2 x 20 by central differences; the td column is 0 without use_td."""
    with mpmath.workdps(DPS_DIFF):
        num = _num("mp")
        oi_, oj_ = _vec(num, oi), _vec(num, oj)
        f = lambda a, b, c, t, l: _proj_g(num, K, a, b, c, l, t, oi_, oj_, use_td)
        J = _central(f, [_vec(num, pi), _vec(num, pj), _vec(num, ex), num(td), num(inv_dep)], (6, 6, 6, 1, 1))
        if not use_td:
            J[:, 18] = 0.0
        return J


def cauchy_weight(r2):
    """sqrt(rho'(|r|^2)) of ceres::CauchyLoss(1): 1 / sqrt(1 + |r|^2), from the unweighted float64 residual as given."""
    with mpmath.workdps(DPS):
        return float(1 / mpmath.sqrt(1 + mpf(float(r2[0])) ** 2 + mpf(float(r2[1])) ** 2))


# ------------------------------------------------------------------------------------------------ pose operations
def pose_plus(x7, d6):
    """(x', scale) of PoseLocalParameterization::Plus."""
    with mpmath.workdps(DPS):
        num = _num("S")
        o = plus(_vec(num, x7), _vec(num, d6))
        return np.array([float(x.v) for x in o]), np.array([float(x.s) for x in o])


def pose_delta(x7, x07):
    """(dx6, scale, w): marginalization_factor.cpp:374-393 -- x - x0 and 2 vec(q0^-1 q), negated when !(w >= 0); w = scalar part of q0^-1 q, exact
    sign included (an mpf)."""
    with mpmath.workdps(DPS):
        num = _num("S")
        x, x0 = _vec(num, x7), _vec(num, x07)
        d = qmul(qinv(pose_q(x0)), pose_q(x))
        v = scl(2, qvec(d))
        if not (d[0].v >= 0):
            v = [-c for c in v]
        o = sub(x[:3], x0[:3]) + v
        return np.array([float(c.v) for c in o]), np.array([float(c.s) for c in o]), d[0].v


# ------------------------------------------------------------------------------------------------ whitening
def _mpm(A):
    A = np.asarray(A, np.float64)
    return mpmath.matrix([[mpf(float(x)) for x in r] for r in A])


def whiten_identity_error(M, cov):
    """max |M C M^T - I| with C = (cov + cov^T) / 2 (what both whitening routes factor), in mpmath."""
    with mpmath.workdps(DPS):
        Mm, C = _mpm(M), _mpm(cov)
        C = (C + C.T) / 2
        E = Mm * C * Mm.T - mpmath.eye(15)
        return float(max(abs(E[i, j]) for i in range(15) for j in range(15)))


def gram_ref(Jraw, rraw, cov):
    """[J r]^T C^-1 [J r] (31 x 31) in mpmath from float64 raw J (15 x 30), r (15), and C = (cov + cov^T) / 2."""
    with mpmath.workdps(DPS):
        A = _mpm(np.hstack([np.asarray(Jraw, np.float64), np.asarray(rraw, np.float64)[:, None]]))
        C = _mpm(cov)
        C = (C + C.T) / 2
        G = A.T * (C ** -1) * A
        return np.array([[float(G[i, j]) for j in range(31)] for i in range(31)])


DIFF_SLACK = 1e-30     # absolute error of a central difference above (truncation and the 70-digit rounding over 2 h), orders above what was seen


def ratio(got, ref, scale, slack=0.0):
    """|got - ref| / (eps * scale) entry-wise; where the scale is 0 (an entry made of exact zeros) any difference is infinite.  slack: the
    reference's own absolute error (DIFF_SLACK when it is a numerical derivative), taken off the difference first."""
    d = np.maximum(0.0, np.abs(np.asarray(got, np.float64) - np.asarray(ref, np.float64)) - slack)
    s = EPS * np.asarray(scale, np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(d == 0, 0.0, d / s)
