"""numpy restatement of camodocal's liftProjective / spaceToPlane for the three camera models the tracker supports, the
CPU reference of tests/test_camera_models_cpu.py and tests/test_gpu_camera_models.py.

KANNALA_BRANDT (EquidistantCamera.cc:428-464, backprojectSymmetric :716-817): the lift takes the smallest real, non-negative root of the
companion-matrix eigenvalues (np.roots is the same method), |imag| <= 1e-10 counts as real, [-1e-10, 0) becomes 0, theta = |p_u| without
a root, and the polynomial has degree 9 - 2 x (number of zero coefficients among k2..k5), filled from k2 upward.
MEI (CataCamera.cc:556-662): the 8 fixed-point steps of the radial-tangential inverse (skipped without distortion), xi == 1 closed form."""
import numpy as np

# the test lenses at 640 x 480
KB_LENS = dict(k2=-0.012, k3=0.0035, k4=-0.0007, k5=0.00005, mu=330.0, mv=330.0, u0=321.26, v0=239.71)
MEI_LENS = dict(xi=1.2, k1=-0.12, k2=0.02, p1=2e-4, p2=-3e-4, gamma1=900.0, gamma2=900.0, u0=321.26, v0=239.71)
KB_EDGE = {   # (k2, k3, k4, k5) with KB_LENS's mu mv u0 v0
    "three_roots": (-0.3, 0.03, 0.0, 0.0),     # three positive roots for |p_u| in (0.55, 0.75): the smallest is taken
    "no_root": (-0.2, 0.0, 0.0, 0.0),          # no root for |p_u| > 0.86: theta = |p_u|
    "dropped_k5": (-0.01, 0.0, 0.001, 0.0002),  # the lift's degree is 7: k5 is dropped (the projection keeps it)
    "zero": (0.0, 0.0, 0.0, 0.0),
}


def _rt_distortion(k1, k2, p1, p2, x, y):
    mx2, my2, mxy = x * x, y * y, x * y
    rho2 = mx2 + my2
    rad = k1 * rho2 + k2 * rho2 * rho2
    return x * rad + 2.0 * p1 * mxy + p2 * (rho2 + 2.0 * mx2), y * rad + 2.0 * p2 * mxy + p1 * (rho2 + 2.0 * my2)


def _rt_undistort(k1, k2, p1, p2, mx_d, my_d):
    dx, dy = _rt_distortion(k1, k2, p1, p2, mx_d, my_d)
    mx_u, my_u = mx_d - dx, my_d - dy
    for _ in range(1, 8):
        dx, dy = _rt_distortion(k1, k2, p1, p2, mx_u, my_u)
        mx_u, my_u = mx_d - dx, my_d - dy
    return mx_u, my_u


def kb_theta(k2, k3, k4, k5, rn):
    kk = [k2, k3, k4, k5]
    npow = 9 - 2 * sum(1 for k in kk if k == 0.0)
    if npow == 1:
        return rn
    coeffs = np.zeros(npow + 1)
    coeffs[0], coeffs[1] = -rn, 1.0
    for j, k in zip((3, 5, 7, 9), kk):
        if npow >= j:
            coeffs[j] = k
    roots = np.roots(coeffs[::-1])   # np.roots wants the highest power first
    th = [max(r.real, 0.0) for r in roots if abs(r.imag) <= 1e-10 and r.real >= -1e-10]
    return min(th) if th else rn


def kb_lift(c, u, v):
    pux, puy = (1.0 / c["mu"]) * u + (-c["u0"] / c["mu"]), (1.0 / c["mv"]) * v + (-c["v0"] / c["mv"])
    rn = np.hypot(pux, puy)
    phi = 0.0 if rn < 1e-10 else np.arctan2(puy, pux)
    th = kb_theta(c["k2"], c["k3"], c["k4"], c["k5"], rn)
    return np.array([np.sin(th) * np.cos(phi), np.sin(th) * np.sin(phi), np.cos(th)])


def kb_project(c, P):
    th = np.arccos(P[2] / np.linalg.norm(P))
    phi = np.arctan2(P[1], P[0])
    r = th + c["k2"] * th ** 3 + c["k3"] * th ** 5 + c["k4"] * th ** 7 + c["k5"] * th ** 9
    return np.array([c["mu"] * r * np.cos(phi) + c["u0"], c["mv"] * r * np.sin(phi) + c["v0"]])


def mei_lift(c, u, v):
    mx_d = (1.0 / c["gamma1"]) * u + (-c["u0"] / c["gamma1"])
    my_d = (1.0 / c["gamma2"]) * v + (-c["v0"] / c["gamma2"])
    if c["k1"] == 0 and c["k2"] == 0 and c["p1"] == 0 and c["p2"] == 0:
        mx_u, my_u = mx_d, my_d
    else:
        mx_u, my_u = _rt_undistort(c["k1"], c["k2"], c["p1"], c["p2"], mx_d, my_d)
    xi = c["xi"]
    if xi == 1.0:
        return np.array([mx_u, my_u, (1.0 - mx_u * mx_u - my_u * my_u) / 2.0])
    rho2 = mx_u * mx_u + my_u * my_u
    return np.array([mx_u, my_u, 1.0 - xi * (rho2 + 1.0) / (xi + np.sqrt(1.0 + (1.0 - xi * xi) * rho2))])


def mei_project(c, P):
    z = P[2] + c["xi"] * np.linalg.norm(P)
    px, py = P[0] / z, P[1] / z
    dx, dy = _rt_distortion(c["k1"], c["k2"], c["p1"], c["p2"], px, py)
    return np.array([c["gamma1"] * (px + dx) + c["u0"], c["gamma2"] * (py + dy) + c["v0"]])


def pinhole_lift(c, u, v):
    mx_d = (1.0 / c["fx"]) * u + (-c["cx"] / c["fx"])
    my_d = (1.0 / c["fy"]) * v + (-c["cy"] / c["fy"])
    x, y = _rt_undistort(c["k1"], c["k2"], c["p1"], c["p2"], mx_d, my_d)
    return np.array([x, y, 1.0])


def pinhole_project(c, P):
    px, py = P[0] / P[2], P[1] / P[2]
    dx, dy = _rt_distortion(c["k1"], c["k2"], c["p1"], c["p2"], px, py)
    return np.array([c["fx"] * (px + dx) + c["cx"], c["fy"] * (py + dy) + c["cy"]])


LIFT = {0: pinhole_lift, 1: kb_lift, 2: mei_lift}
PROJECT = {0: pinhole_project, 1: kb_project, 2: mei_project}


def lift(model, params, uv):
    return np.array([LIFT[model](params, float(u), float(v)) for u, v in np.asarray(uv, np.float64).reshape(-1, 2)])


def project(model, params, rays):
    return np.array([PROJECT[model](params, r) for r in np.asarray(rays, np.float64).reshape(-1, 3)])


def grid(width=640, height=480, step=16):
    """pixel grid incl. the last row and column, plus the principal-point neighbourhood"""
    xs = np.unique(np.r_[np.arange(0, width, step), width - 1]).astype(np.float64)
    ys = np.unique(np.r_[np.arange(0, height, step), height - 1]).astype(np.float64)
    return np.stack(np.meshgrid(xs, ys), -1).reshape(-1, 2)


def random_points(n, seed, width=640, height=480):
    r = np.random.default_rng(seed)
    return np.stack([r.uniform(0, width - 1, n), r.uniform(0, height - 1, n)], -1)
