// fba_ray.h -- the inverse of the projection model: the image ray of one measurement, fp64, for the forward
// intersection of the tie points (k_rays, fba_intersect.hip) and, the same arithmetic, for the host
// (fba_unproject_host).  No reference counterpart: main.m takes every object point's starting value from the .cnt file.
//
// The model (BuildAwG.m:163-213, obs_model in fba_kernels.hip) evaluates its distortion at the MEASURED coordinates, so
// the ray is closed-form -- no fixed-point iteration:
//   xb = x - xp, yb = y - yp, r^2 = xb^2 + yb^2, dr = sum K_j r^2j, decx = P1 (yb^2 + 3 xb^2) + 2 P2 xb yb,
//   decy = P2 (xb^2 + 3 yb^2) + 2 P1 xb yb; the condition w = 0 reads
//   xu = xb - dr xb - decx = -c s U,  yu = yb - dr yb - decy = -c ydir s V,  s = g(t) / R,  t = atan(R / W),
//   so rho = hypot(xu, yu) = c |g(t)| and t = ginv(q), q = rho / c:
//   q (fisheye) | atan q (pinhole) | 2 asin(q / 2) (equisolid) | asin q (orthographic) | 2 atan(q / 2) (stereographic).
//   out  (xu, yu) and the unit direction in the camera frame d = (-sin t xu / rho, -ydir sin t yu / rho, cos t)
//        rho = 0: the axis (0, 0, 1).  FBA_RAY_DOMAIN and d = 0: |q| > 1 (orthographic), |q| > 2 (equisolid), or
//        anything non-finite (a NaN pixel, c = 0).
// The ray is a LINE through the projection centre: W > 0 and W < 0 (synth.py's scenes) give the same line with the
// direction reversed, and every user of d is independent of that sign.
//
// ray_project: the forward model's part that depends on the object point, px = -c s U, py = -c ydir s V (the
// misclosure is w = (px - xu, py - yu): obs_model's fx - x with the distortion terms moved to the other side), and its
// derivative to X Y Z, obs_model's tie columns by the same chain rule.  Like obs_model it has no guard at R = 0.
#pragma once
#include <cmath>

#include "../../include/fba.h"

#ifndef FBA_HD
#if defined(__HIPCC__) || defined(__CUDACC__)
#define FBA_HD __host__ __device__
#else
#define FBA_HD
#endif
#endif

namespace fba {

// K[nk]; NK > 0 fixes the trip count at compile time (the device's instantiations), NK = 0 reads nk
template <int NK>
FBA_HD inline int ray_unproject(double x, double y, double xp, double yp, double c, double ydir, double P1, double P2,
                                const double* K, int nk, int type, double& xu, double& yu, double& d0, double& d1,
                                double& d2) {
    const int n = NK > 0 ? NK : nk;
    const double xb = x - xp, yb = y - yp;
    const double r2 = xb * xb + yb * yb;
    double dr = 0.0, r2j = 1.0;
#pragma unroll
    for (int j = 0; j < n; ++j) {
        r2j *= r2;
        dr += K[j] * r2j;
    }
    const double decx = P1 * (yb * yb + 3.0 * xb * xb) + 2.0 * P2 * xb * yb;
    const double decy = P2 * (xb * xb + 3.0 * yb * yb) + 2.0 * P1 * xb * yb;
    xu = xb - dr * xb - decx;
    yu = yb - dr * yb - decy;
    d0 = d1 = d2 = 0.0;
    const double rho = sqrt(xu * xu + yu * yu);
    const double q = rho / c;
    // !(|q| <= max) is true for a NaN as well
    if (!(fabs(q) <= 1.79769313486231570815e308) || ydir != ydir) return FBA_RAY_DOMAIN;
    double t;
    if (type == FBA_TYPE_FISHEYE) {
        t = q;
    } else if (type == FBA_TYPE_PINHOLE) {
        t = atan(q);
    } else if (type == FBA_TYPE_EQUISOLID) {
        if (!(fabs(q) <= 2.0)) return FBA_RAY_DOMAIN;
        t = 2.0 * asin(0.5 * q);
    } else if (type == FBA_TYPE_ORTHOGRAPHIC) {
        if (!(fabs(q) <= 1.0)) return FBA_RAY_DOMAIN;
        t = asin(q);
    } else {
        t = 2.0 * atan(0.5 * q);
    }
    if (rho == 0.0) {
        d2 = 1.0;
        return FBA_RAY_OK;
    }
    const double st = sin(t), ct = cos(t), ir = 1.0 / rho;
    d0 = -st * (xu * ir);
    d1 = -ydir * st * (yu * ir);
    d2 = ct;
    return FBA_RAY_OK;
}

// M[9] the image's rotation (rows U V W), (e0, e1, e2) = X - C; jp[6]: d px / d(X Y Z), d py / d(X Y Z)
FBA_HD inline void ray_project(int type, const double* M, double e0, double e1, double e2, double c, double ydir,
                               double& px, double& py, double* jp) {
    const double U = M[0] * e0 + M[1] * e1 + M[2] * e2;
    const double V = M[3] * e0 + M[4] * e1 + M[5] * e2;
    const double W = M[6] * e0 + M[7] * e1 + M[8] * e2;
    const double R = sqrt(U * U + V * V);
    const double iR = 1.0 / R;
    double s, sR, sW;  // the radial factor s(R, W) and its derivatives (BuildAwG.m:184-208)
    if (type == FBA_TYPE_PINHOLE) {
        s = 1.0 / W; sR = 0.0; sW = -1.0 / (W * W);
    } else {
        const double t = atan(R / W);
        const double iq = 1.0 / (R * R + W * W);
        const double tR = W * iq, tW = -R * iq;
        double g, gt;
        if (type == FBA_TYPE_FISHEYE) { g = t; gt = 1.0; }
        else if (type == FBA_TYPE_EQUISOLID) { g = 2.0 * sin(0.5 * t); gt = cos(0.5 * t); }
        else if (type == FBA_TYPE_ORTHOGRAPHIC) { g = sin(t); gt = cos(t); }
        else { const double ch = cos(0.5 * t); g = 2.0 * tan(0.5 * t); gt = 1.0 / (ch * ch); }
        s = g * iR;
        sR = (gt * tR - s) * iR;
        sW = gt * tW * iR;
    }
    const double cys = c * ydir;
    px = -c * s * U;
    py = -cys * V * s;
#pragma unroll
    for (int q = 0; q < 3; ++q) {  // d(U V W) / dX_q = M[:, q]
        const double dU = M[q], dV = M[3 + q], dW = M[6 + q];
        const double dR = (U * dU + V * dV) * iR;
        const double ds = (type == FBA_TYPE_PINHOLE) ? sW * dW : sR * dR + sW * dW;
        jp[q] = -c * (dU * s + U * ds);
        jp[3 + q] = -cys * (dV * s + V * ds);
    }
}

}  // namespace fba
