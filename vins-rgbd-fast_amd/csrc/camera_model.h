// Camera models of camodocal (camera_model/src/camera_models/) as the tracker uses them: liftProjective (pixel -> projective ray) and
// spaceToPlane (ray -> pixel) of PINHOLE (PinholeCamera.cc), KANNALA_BRANDT (EquidistantCamera.cc) and MEI (CataCamera.cc).  One text for
// host and device: the lifts use only + - * / sqrt and dmath.h's sincos_det, so with -ffp-contract=off every IEEE-754
// double implementation returns the same bits (the renderer's ray tables and vio_stage_host_camera rely on it).  The projections call
// atan2 (KANNALA_BRANDT only), whose last place differs between math libraries; the tracker's projection runs on the device alone.
// Parameter order of vio_camera::p (include/vio_abi.h): PINHOLE fx fy cx cy k1 k2 p1 p2, KANNALA_BRANDT k2 k3 k4 k5 mu mv u0 v0,
// MEI xi k1 k2 p1 p2 gamma1 gamma2 u0 v0.
#pragma once
#include <math.h>
#include "dmath.h"
#include "../../include/vio_abi.h"

namespace vcam {

// radial-tangential distortion (PinholeCamera.cc:645-662, CataCamera.cc:766-782: the same formula)
DM_HD void rt_distortion(double k1, double k2, double p1, double p2, double x, double y, double &dx, double &dy) {
    double mx2 = x * x, my2 = y * y, mxy = x * y;
    double rho2 = mx2 + my2;
    double rad = k1 * rho2 + k2 * rho2 * rho2;
    dx = x * rad + 2.0 * p1 * mxy + p2 * (rho2 + 2.0 * mx2);
    dy = y * rad + 2.0 * p2 * mxy + p1 * (rho2 + 2.0 * my2);
}
// the recursive inverse of both models: 8 fixed-point steps (PinholeCamera.cc:489-507, CataCamera.cc:598-612)
DM_HD void rt_undistort(double k1, double k2, double p1, double p2, double mx_d, double my_d, double &mx_u, double &my_u) {
    double dx, dy;
    rt_distortion(k1, k2, p1, p2, mx_d, my_d, dx, dy);
    mx_u = mx_d - dx;
    my_u = my_d - dy;
    for (int i = 1; i < 8; i++) {
        rt_distortion(k1, k2, p1, p2, mx_u, my_u, dx, dy);
        mx_u = mx_d - dx;
        my_u = my_d - dy;
    }
}

// ---- PINHOLE (PinholeCamera.cc:449-542): the ray is (x, y, 1)
DM_HD void pinhole_lift(double fx, double fy, double cx, double cy, double k1, double k2, double p1, double p2, double u, double v, double &x,
                        double &y) {
    double inv_K11 = 1.0 / fx, inv_K13 = -cx / fx, inv_K22 = 1.0 / fy, inv_K23 = -cy / fy;
    double mx_d = inv_K11 * u + inv_K13, my_d = inv_K22 * v + inv_K23;
    rt_undistort(k1, k2, p1, p2, mx_d, my_d, x, y);
}
DM_HD void pinhole_project(double fx, double fy, double cx, double cy, double k1, double k2, double p1, double p2, double X, double Y, double Z,
                           double &u, double &v) {
    double px = X / Z, py = Y / Z, dx, dy;
    rt_distortion(k1, k2, p1, p2, px, py, dx, dy);
    u = fx * (px + dx) + cx;
    v = fy * (py + dy) + cy;
}

// ---- KANNALA_BRANDT (EquidistantCamera.cc)
// r(theta) = theta + k2 theta^3 + k3 theta^5 + k4 theta^7 + k5 theta^9, the products written as EquidistantCamera::r writes them
DM_HD double kb_r(double k2, double k3, double k4, double k5, double th) {
    return th + k2 * th * th * th + k3 * th * th * th * th * th + k4 * th * th * th * th * th * th * th +
           k5 * th * th * th * th * th * th * th * th * th;
}
// f(theta) = theta + a[0] theta^3 + ... + a[3] theta^9 - rn and f'(theta), Horner in theta^2
DM_HD void kb_poly(const double *a, double rn, double th, double &f, double &df) {
    const double s = th * th;
    const double g = 1.0 + s * (a[0] + s * (a[1] + s * (a[2] + s * a[3])));
    df = 1.0 + s * (3.0 * a[0] + s * (5.0 * a[1] + s * (7.0 * a[2] + s * (9.0 * a[3]))));
    f = th * g - rn;
}
enum { KB_SCAN = 256, KB_REFINE = 64 };
// backprojectSymmetric (:716-817): the smallest non-negative root of r(theta) = |p_u|, theta = |p_u| when there is none.  The reference takes
// the eigenvalues of the companion matrix; here the first sign change of f on [0, pi] in KB_SCAN uniform steps (f(0) = -|p_u| <= 0, so the
// first crossing is the smallest non-negative root), refined by Newton's method safeguarded by bisection (at most KB_REFINE steps).
// Tangential (double) roots and two roots closer together than pi / KB_SCAN are not detected; roots beyond pi are not searched (a ray there
// points behind the camera).  The reference's degree rule is kept: the polynomial has degree 9 - 2 x (number of zero coefficients among
// k2..k5) and is filled from k2 upward, so an interior zero drops the highest coefficient from the lift (the projection keeps it).
DM_HD double kb_theta(double k2, double k3, double k4, double k5, double rn) {
    const double kk[4] = {k2, k3, k4, k5};
    int used = 4;
    for (int i = 0; i < 4; i++) used -= kk[i] == 0.0 ? 1 : 0;
    if (used == 0) return rn;   // npow == 1
    double a[4];
    for (int i = 0; i < 4; i++) a[i] = i < used ? kk[i] : 0.0;
    const double step = 3.14159265358979311600 / KB_SCAN;
    double lo = 0, hi = -1, f, df;
    kb_poly(a, rn, 0.0, f, df);
    if (f >= 0) return 0.0;   // rn == 0
#pragma unroll 1
    for (int k = 1; k <= KB_SCAN; k++) {
        const double th = step * k;
        kb_poly(a, rn, th, f, df);
        if (f >= 0) { hi = th; break; }
        lo = th;
    }
    if (hi < 0) return rn;   // no root
    if (f == 0) return hi;
    double x = 0.5 * (lo + hi);
#pragma unroll 1
    for (int it = 0; it < KB_REFINE; it++) {
        kb_poly(a, rn, x, f, df);
        if (f == 0) break;
        if (f < 0) lo = x; else hi = x;
        double xn = x - f / df;
        if (!(xn > lo && xn < hi)) xn = 0.5 * (lo + hi);   // (also a NaN step)
        if (xn == x) break;
        x = xn;
    }
    return x;
}
DM_HD void kb_lift(double k2, double k3, double k4, double k5, double mu, double mv, double u0, double v0, double u, double v, double &x,
                   double &y, double &z) {
    double inv_K11 = 1.0 / mu, inv_K13 = -u0 / mu, inv_K22 = 1.0 / mv, inv_K23 = -v0 / mv;
    double pux = inv_K11 * u + inv_K13, puy = inv_K22 * v + inv_K23;
    double rn = sqrt(pux * pux + puy * puy);
    // (cos phi, sin phi) of phi = atan2(p_u.y, p_u.x) as p_u / |p_u|; phi = 0 below 1e-10 as the reference
    double cphi = 1.0, sphi = 0.0;
    if (!(rn < 1e-10)) { cphi = pux / rn; sphi = puy / rn; }
    double theta = kb_theta(k2, k3, k4, k5, rn), st, ct;
    dm::sincos_det(theta, &st, &ct);
    x = st * cphi;
    y = st * sphi;
    z = ct;
}
// spaceToPlane (:451-464) with theta = atan2(rho, z) for acos(z / |P|) (better conditioned near the axis) and (cos phi, sin phi) = (x, y) / rho
DM_HD void kb_project(double k2, double k3, double k4, double k5, double mu, double mv, double u0, double v0, double X, double Y, double Z,
                      double &u, double &v) {
    double rho = sqrt(X * X + Y * Y);
    double theta = atan2(rho, Z);
    double cphi = 1.0, sphi = 0.0;
    if (rho > 0) { cphi = X / rho; sphi = Y / rho; }
    double r = kb_r(k2, k3, k4, k5, theta);
    double pux = r * cphi, puy = r * sphi;
    u = mu * pux + u0;
    v = mv * puy + v0;
}

// ---- MEI (CataCamera.cc)
DM_HD void mei_lift(double xi, double k1, double k2, double p1, double p2, double g1, double g2, double u0, double v0, double u, double v,
                    double &x, double &y, double &z) {
    double inv_K11 = 1.0 / g1, inv_K13 = -u0 / g1, inv_K22 = 1.0 / g2, inv_K23 = -v0 / g2;
    double mx_d = inv_K11 * u + inv_K13, my_d = inv_K22 * v + inv_K23, mx_u, my_u;
    if (k1 == 0.0 && k2 == 0.0 && p1 == 0.0 && p2 == 0.0) { mx_u = mx_d; my_u = my_d; }   // m_noDistortion
    else rt_undistort(k1, k2, p1, p2, mx_d, my_d, mx_u, my_u);
    x = mx_u;
    y = my_u;
    if (xi == 1.0) {
        z = (1.0 - mx_u * mx_u - my_u * my_u) / 2.0;
    } else {
        double rho2 = mx_u * mx_u + my_u * my_u;
        z = 1.0 - xi * (rho2 + 1.0) / (xi + sqrt(1.0 + (1.0 - xi * xi) * rho2));
    }
}
DM_HD void mei_project(double xi, double k1, double k2, double p1, double p2, double g1, double g2, double u0, double v0, double X, double Y,
                       double Z, double &u, double &v) {
    double zz = Z + xi * sqrt(X * X + Y * Y + Z * Z);
    double pux = X / zz, puy = Y / zz, pdx = pux, pdy = puy;
    if (!(k1 == 0.0 && k2 == 0.0 && p1 == 0.0 && p2 == 0.0)) {
        double dx, dy;
        rt_distortion(k1, k2, p1, p2, pux, puy, dx, dy);
        pdx = pux + dx;
        pdy = puy + dy;
    }
    u = g1 * pdx + u0;
    v = g2 * pdy + v0;
}

// ---- dispatch on vio_camera::model (an unknown model lifts / projects to NaN)
DM_HD void lift(const vio_camera &c, double u, double v, double &x, double &y, double &z) {
    const double *p = c.p;
    if (c.model == VIO_CAMERA_PINHOLE) {
        pinhole_lift(p[0], p[1], p[2], p[3], p[4], p[5], p[6], p[7], u, v, x, y);
        z = 1.0;
    } else if (c.model == VIO_CAMERA_KANNALA_BRANDT) {
        kb_lift(p[0], p[1], p[2], p[3], p[4], p[5], p[6], p[7], u, v, x, y, z);
    } else if (c.model == VIO_CAMERA_MEI) {
        mei_lift(p[0], p[1], p[2], p[3], p[4], p[5], p[6], p[7], p[8], u, v, x, y, z);
    } else {
        x = y = z = NAN;
    }
}
DM_HD void project(const vio_camera &c, double X, double Y, double Z, double &u, double &v) {
    const double *p = c.p;
    if (c.model == VIO_CAMERA_PINHOLE) pinhole_project(p[0], p[1], p[2], p[3], p[4], p[5], p[6], p[7], X, Y, Z, u, v);
    else if (c.model == VIO_CAMERA_KANNALA_BRANDT) kb_project(p[0], p[1], p[2], p[3], p[4], p[5], p[6], p[7], X, Y, Z, u, v);
    else if (c.model == VIO_CAMERA_MEI) mei_project(p[0], p[1], p[2], p[3], p[4], p[5], p[6], p[7], p[8], X, Y, Z, u, v);
    else u = v = NAN;
}
// the tracker's normalised point of a pixel (undistortedPoints, feature_tracker.cpp:555): b.x / b.z, b.y / b.z (z = 1 for PINHOLE)
DM_HD void lift_plane(const vio_camera &c, double u, double v, double &x, double &y) {
    double X, Y, Z;
    lift(c, u, v, X, Y, Z);
    x = X / Z;
    y = Y / Z;
}

}  // namespace vcam
