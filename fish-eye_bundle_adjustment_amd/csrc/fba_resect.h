// fba_resect.h -- space resection of one image from object points and their image rays, fp64: the per-image routines
// of k_resect (fba_resect.hip) and, the same arithmetic, of the host (fba_resect_host).  No reference counterpart:
// Buildxhat.m:22-63 copies the .ext rows.
//
// The forward model (BuildAwG.m:163-213) is a function of the LINE through the projection centre: every g is odd, so
// (U, V, W) -> -(U, V, W) gives the same pixel.  For a measurement with the camera-frame direction d (ray_unproject,
// fba_ray.h) and a known object point X the constraint d x (M (X - C)) = 0 is independent of d's sign and linear in the
// 12 entries of P = [M | -M C] (row-major, p[4 i + j]):
//   1  Hartley: m the centroid of the usable points, s their mean distance to it, X~ = ((X - m) / s, 1);
//   2  G = sum (I - d d') (x) (X~ X~'), 12 x 12: 6 x 10 distinct products per measurement ([d]x'[d]x = I - d d');
//   3  P = the eigenvector of G's smallest eigenvalue (cyclic Jacobi, resect_jacobi12); the quality of the solution is
//      lambda_1 / lambda_11, the second smallest over the largest eigenvalue: 0 for coplanar points or fewer than 6;
//   4  P's sign so that det(P[:, :3]) > 0 -- the one remaining sign, so W < 0 and W > 0 scenes both resolve;
//   5  M = A (A'A)^(-1/2), the polar factor of A = P[:, :3] (eig3 of A'A); lambda = the mean singular value of A;
//   6  t~ = P[:, 3] / lambda, C = m - s M' t~;
//   7  phi = asin(clamp(M20)), omega = atan2(-M21, M22), kappa = atan2(-M10, M00) (BuildAwG.m:163-165); where
//      cos^2 phi = M21^2 + M22^2 <= RESECT_GIMBAL (M's entries carry ~1e-14 of noise, so below cos phi ~ 1e-7 the
//      two quotients are noise): omega = 0, kappa = atan2(M01, M11).
// Refinement: Gauss-Newton on (Xc Yc Zc omega phi kappa) of the image alone, w = (px - xu, py - yu) through
// resect_eval_add -- ray_project's arithmetic with the six exterior-orientation columns: -jp for C, the chain rule
// through dM / d(omega, phi, kappa) for the angles -- N = J'PJ (21 sums), g = J'Pw, a 6 x 6 Cholesky (resect_chol6).
//
// resect_solve is the whole per-image procedure over a source of sums S: the device's S (one wave64 per image, fixed
// xor trees) and the host's (index order) differ in the order of the sums alone.  Per-thread arrays are indexed by
// constants after unrolling (no scratch on the device); the 12 x 12 matrix and its eigenvectors live in memory the
// caller provides (LDS on the device), indexed at run time.
#pragma once
#include <cmath>
#include <cstdint>

#include "../../include/fba.h"
#include "fba_eig3.h"
#include "fba_layout.h"
#include "fba_ray.h"

namespace fba {

constexpr int RESECT_GRAM = 60;       // distinct products of G
constexpr int RESECT_EVAL = 30;       // N 21 (packed lower, a (a + 1) / 2 + b) | g 6 | ssq | dsum | d . M(X - C) > 0
constexpr int RESECT_MIN_PTS = 6;
constexpr int RESECT_SWEEPS = 40;     // cyclic Jacobi converges quadratically; a 12 x 12 matrix takes 6 to 10
constexpr double RESECT_GIMBAL = 1e-14;
constexpr double RESECT_F64_MAX = 1.79769313486231570815e308;

FBA_HD constexpr int resect_sym4(int j, int l) {
    return j > l ? resect_sym4(l, j) : (j == 0 ? l : (j == 1 ? 3 + l : (j == 2 ? 5 + l : 9)));
}

// one record [xu yu d0 d1 d2 X Y Z] into the six blocks of G's distinct products: block a holds the (I - d d') entry a
// (00 01 02 11 12 22) times the ten X~ X~' entries (00 01 02 03 11 12 13 22 23 33).  Six arrays of 10, not one of
// 60: the device keeps each in registers
FBA_HD inline void resect_gram_add(const double* r, double m0, double m1, double m2, double is, double* g0, double* g1,
                                   double* g2, double* g3, double* g4, double* g5) {
    const double d0 = r[2], d1 = r[3], d2 = r[4];
    const double x0 = (r[5] - m0) * is, x1 = (r[6] - m1) * is, x2 = (r[7] - m2) * is;
    const double q0 = 1.0 - d0 * d0, q1 = -d0 * d1, q2 = -d0 * d2, q3 = 1.0 - d1 * d1, q4 = -d1 * d2, q5 = 1.0 - d2 * d2;
    const double xx[10] = {x0 * x0, x0 * x1, x0 * x2, x0, x1 * x1, x1 * x2, x1, x2 * x2, x2, 1.0};
#pragma unroll
    for (int b = 0; b < 10; ++b) {
        g0[b] += q0 * xx[b]; g1[b] += q1 * xx[b]; g2[b] += q2 * xx[b];
        g3[b] += q3 * xx[b]; g4[b] += q4 * xx[b]; g5[b] += q5 * xx[b];
    }
}

// block (I, K) of (I - d d'), I <= K, into the full symmetric 12 x 12 G (row-major):
// G[(4 I + j), (4 K + l)] = G[(4 K + j), (4 I + l)] = g[sym4(j, l)]
template <int I, int K>
FBA_HD inline void resect_gram_fill(const double* g, double* A) {
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int l = 0; l < 4; ++l) {
            A[12 * (4 * I + j) + 4 * K + l] = g[resect_sym4(j, l)];
            A[12 * (4 * K + j) + 4 * I + l] = g[resect_sym4(j, l)];
        }
}

// cyclic Jacobi on the symmetric 12 x 12 A (both triangles kept): eigenvalues on A's diagonal, eigenvector k in V's
// column k.  Rutishauser's rotation as in fba_eig3.h; stops when off <= 1e-18 x the diagonal's norm, tested before
// every sweep.  A NaN ends it at once (the caller sees it in the ratio).
FBA_HD inline void resect_jacobi12(double* A, double* V) {
    for (int i = 0; i < 144; ++i) V[i] = 0.0;
    for (int i = 0; i < 12; ++i) V[13 * i] = 1.0;
    for (int sweep = 0; sweep < RESECT_SWEEPS; ++sweep) {
        double off2 = 0.0, dg2 = 0.0;
        for (int p = 0; p < 12; ++p) {
            dg2 += A[13 * p] * A[13 * p];
            for (int q = p + 1; q < 12; ++q) off2 += A[12 * p + q] * A[12 * p + q];
        }
        if (!(off2 > 1e-36 * dg2)) break;
        for (int p = 0; p < 11; ++p)
            for (int q = p + 1; q < 12; ++q) {
                const double apq = A[12 * p + q];
                if (apq == 0.0) continue;
                const double app = A[13 * p], aqq = A[13 * q];
                const double th = (aqq - app) / (2.0 * apq);
                const double t = (th < 0.0 ? -1.0 : 1.0) / (fabs(th) + sqrt(th * th + 1.0));
                const double c = 1.0 / sqrt(t * t + 1.0), s = t * c, tau = s / (1.0 + c);
                A[13 * p] = app - t * apq;
                A[13 * q] = aqq + t * apq;
                A[12 * p + q] = 0.0;
                A[12 * q + p] = 0.0;
                // all loads of the two columns first, then all stores: no store of the loop touches an entry a later
                // load reads, and issued together the loads overlap their latency (the matrices live in LDS)
                double g[12], h[12];
#pragma unroll
                for (int r = 0; r < 12; ++r) { g[r] = A[12 * r + p]; h[r] = A[12 * r + q]; }
#pragma unroll
                for (int r = 0; r < 12; ++r) {
                    const double gn = g[r] - s * (h[r] + tau * g[r]), hn = h[r] + s * (g[r] - tau * h[r]);
                    if (r != p && r != q) {
                        A[12 * r + p] = gn; A[12 * p + r] = gn;
                        A[12 * r + q] = hn; A[12 * q + r] = hn;
                    }
                }
#pragma unroll
                for (int r = 0; r < 12; ++r) { g[r] = V[12 * r + p]; h[r] = V[12 * r + q]; }
#pragma unroll
                for (int r = 0; r < 12; ++r) {
                    V[12 * r + p] = g[r] - s * (h[r] + tau * g[r]);
                    V[12 * r + q] = h[r] + s * (g[r] - tau * h[r]);
                }
            }
    }
}

FBA_HD inline bool resect_finite6(const double* v) {
    bool ok = true;
#pragma unroll
    for (int q = 0; q < 6; ++q) ok = ok && fabs(v[q]) <= RESECT_F64_MAX;
    return ok;
}

// the angles of M (row-major) in BuildAwG.m:163-165's convention
FBA_HD inline void resect_angles(const double* M, double& om, double& ph, double& ka) {
    const double m20 = fmin(fmax(M[6], -1.0), 1.0);
    ph = asin(m20);
    if (M[7] * M[7] + M[8] * M[8] <= RESECT_GIMBAL) {
        om = 0.0;
        ka = atan2(M[1], M[4]);
    } else {
        om = atan2(-M[7], M[8]);
        ka = atan2(-M[3], M[0]);
    }
}

// steps 3 to 7 from the Jacobi result: lin[6] = Xc Yc Zc omega phi kappa, ratio = lambda_1 / lambda_11
FBA_HD inline void resect_linear(const double* A, const double* V, double m0, double m1, double m2, double s, double* lin,
                                 double& ratio) {
    int k0 = 0;
    double l0 = A[0], lmax = A[0];
    for (int k = 1; k < 12; ++k) {
        const double l = A[13 * k];
        if (l < l0) { l0 = l; k0 = k; }
        lmax = fmax(lmax, l);
    }
    double l1 = lmax;
    for (int k = 0; k < 12; ++k)
        if (k != k0) l1 = fmin(l1, A[13 * k]);
    ratio = l1 / lmax;
    double p[12];
#pragma unroll
    for (int r = 0; r < 12; ++r) p[r] = V[12 * r + k0];
    const double det = p[0] * (p[5] * p[10] - p[6] * p[9]) - p[1] * (p[4] * p[10] - p[6] * p[8]) +
                       p[2] * (p[4] * p[9] - p[5] * p[8]);
    if (det < 0.0) {
#pragma unroll
        for (int r = 0; r < 12; ++r) p[r] = -p[r];
    }
    // B = A'A, its eigen-decomposition, (A'A)^(-1/2) = sum v v' / sigma
    const double b00 = p[0] * p[0] + p[4] * p[4] + p[8] * p[8], b01 = p[0] * p[1] + p[4] * p[5] + p[8] * p[9];
    const double b02 = p[0] * p[2] + p[4] * p[6] + p[8] * p[10], b11 = p[1] * p[1] + p[5] * p[5] + p[9] * p[9];
    const double b12 = p[1] * p[2] + p[5] * p[6] + p[9] * p[10], b22 = p[2] * p[2] + p[6] * p[6] + p[10] * p[10];
    double s0, s1, s2, v00, v01, v02, v10, v11, v12, v20, v21, v22;
    eig3(b00, b01, b02, b11, b12, b22, s0, s1, s2, v00, v01, v02, v10, v11, v12, v20, v21, v22);
    const double i0 = 1.0 / s0, i1 = 1.0 / s1, i2 = 1.0 / s2;
    const double h00 = v00 * v00 * i0 + v10 * v10 * i1 + v20 * v20 * i2, h01 = v00 * v01 * i0 + v10 * v11 * i1 + v20 * v21 * i2;
    const double h02 = v00 * v02 * i0 + v10 * v12 * i1 + v20 * v22 * i2, h11 = v01 * v01 * i0 + v11 * v11 * i1 + v21 * v21 * i2;
    const double h12 = v01 * v02 * i0 + v11 * v12 * i1 + v21 * v22 * i2, h22 = v02 * v02 * i0 + v12 * v12 * i1 + v22 * v22 * i2;
    double M[9];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const double a0 = p[4 * i], a1 = p[4 * i + 1], a2 = p[4 * i + 2];
        M[3 * i] = a0 * h00 + a1 * h01 + a2 * h02;
        M[3 * i + 1] = a0 * h01 + a1 * h11 + a2 * h12;
        M[3 * i + 2] = a0 * h02 + a1 * h12 + a2 * h22;
    }
    const double il = 3.0 / (s0 + s1 + s2);
    const double t0 = p[3] * il, t1 = p[7] * il, t2 = p[11] * il;
    lin[0] = m0 - s * (M[0] * t0 + M[3] * t1 + M[6] * t2);
    lin[1] = m1 - s * (M[1] * t0 + M[4] * t1 + M[7] * t2);
    lin[2] = m2 - s * (M[2] * t0 + M[5] * t1 + M[8] * t2);
    resect_angles(M, lin[3], lin[4], lin[5]);
}

// the rotation of (omega, phi, kappa) and its three derivatives (BuildAwG.m:163-165), the centre beside them
struct ResectPose {
    double C[3], M[9], Mw[9], Mp[9], Mk[9];
};
FBA_HD inline void resect_pose(const double* eop, ResectPose& P) {
    const double cw = cos(eop[3]), sw = sin(eop[3]), cp = cos(eop[4]), sp = sin(eop[4]), ck = cos(eop[5]), sk = sin(eop[5]);
    P.C[0] = eop[0]; P.C[1] = eop[1]; P.C[2] = eop[2];
    P.M[0] = ck * cp; P.M[1] = cw * sk + ck * sp * sw; P.M[2] = sk * sw - ck * cw * sp;
    P.M[3] = -cp * sk; P.M[4] = ck * cw - sk * sp * sw; P.M[5] = ck * sw + cw * sk * sp;
    P.M[6] = sp; P.M[7] = -cp * sw; P.M[8] = cp * cw;
    P.Mw[0] = 0.0; P.Mw[1] = -sw * sk + ck * sp * cw; P.Mw[2] = sk * cw + ck * sw * sp;
    P.Mw[3] = 0.0; P.Mw[4] = -ck * sw - sk * sp * cw; P.Mw[5] = ck * cw - sw * sk * sp;
    P.Mw[6] = 0.0; P.Mw[7] = -cp * cw; P.Mw[8] = -cp * sw;
    P.Mp[0] = -ck * sp; P.Mp[1] = ck * cp * sw; P.Mp[2] = -ck * cw * cp;
    P.Mp[3] = sp * sk; P.Mp[4] = -sk * cp * sw; P.Mp[5] = cw * sk * cp;
    P.Mp[6] = cp; P.Mp[7] = sp * sw; P.Mp[8] = -sp * cw;
    P.Mk[0] = P.M[3]; P.Mk[1] = P.M[4]; P.Mk[2] = P.M[5];
    P.Mk[3] = -P.M[0]; P.Mk[4] = -P.M[1]; P.Mk[5] = -P.M[2];
    P.Mk[6] = 0.0; P.Mk[7] = 0.0; P.Mk[8] = 0.0;
}

// one record at the pose: the forward model (ray_project's arithmetic; like it no guard at R = 0) with the six
// exterior-orientation columns, added into acc[RESECT_EVAL]; wx, wy the weights 1 / std^2
FBA_HD inline void resect_eval_add(int type, const ResectPose& P, const double* r, double c, double ydir, double wx,
                                   double wy, double* acc) {
    const double e0 = r[5] - P.C[0], e1 = r[6] - P.C[1], e2 = r[7] - P.C[2];
    const double U = P.M[0] * e0 + P.M[1] * e1 + P.M[2] * e2;
    const double V = P.M[3] * e0 + P.M[4] * e1 + P.M[5] * e2;
    const double W = P.M[6] * e0 + P.M[7] * e1 + P.M[8] * e2;
    const double R = sqrt(U * U + V * V);
    const double iR = 1.0 / R;
    double s, sR, sW;
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
    const double w0 = -c * s * U - r[0], w1 = -cys * V * s - r[1];
    // d (U V W) / d (Xc Yc Zc) = -M[:, q]; d / d angle = (dM / d angle) e
    double dU[6], dV[6], dW[6];
#pragma unroll
    for (int q = 0; q < 3; ++q) { dU[q] = -P.M[q]; dV[q] = -P.M[3 + q]; dW[q] = -P.M[6 + q]; }
    dU[3] = P.Mw[0] * e0 + P.Mw[1] * e1 + P.Mw[2] * e2; dV[3] = P.Mw[3] * e0 + P.Mw[4] * e1 + P.Mw[5] * e2;
    dW[3] = P.Mw[6] * e0 + P.Mw[7] * e1 + P.Mw[8] * e2;
    dU[4] = P.Mp[0] * e0 + P.Mp[1] * e1 + P.Mp[2] * e2; dV[4] = P.Mp[3] * e0 + P.Mp[4] * e1 + P.Mp[5] * e2;
    dW[4] = P.Mp[6] * e0 + P.Mp[7] * e1 + P.Mp[8] * e2;
    dU[5] = P.Mk[0] * e0 + P.Mk[1] * e1 + P.Mk[2] * e2; dV[5] = P.Mk[3] * e0 + P.Mk[4] * e1 + P.Mk[5] * e2;
    dW[5] = 0.0;
    double jx[6], jy[6];
#pragma unroll
    for (int q = 0; q < 6; ++q) {
        const double dR = (U * dU[q] + V * dV[q]) * iR;
        const double ds = (type == FBA_TYPE_PINHOLE) ? sW * dW[q] : sR * dR + sW * dW[q];
        jx[q] = -c * (dU[q] * s + U * ds);
        jy[q] = -cys * (dV[q] * s + V * ds);
    }
#pragma unroll
    for (int a = 0; a < 6; ++a) {
        const double ax = wx * jx[a], ay = wy * jy[a];
#pragma unroll
        for (int b = 0; b <= a; ++b) acc[a * (a + 1) / 2 + b] += ax * jx[b] + ay * jy[b];
        acc[21 + a] += ax * w0 + ay * w1;
    }
    acc[27] += w0 * w0 + w1 * w1;
    acc[28] += sqrt(e0 * e0 + e1 * e1 + e2 * e2);
    acc[29] += (r[2] * U + r[3] * V + r[4] * W > 0.0) ? 1.0 : 0.0;
}

// x = N^-1 g by Cholesky, N packed lower (a (a + 1) / 2 + b); false: a non-positive (or NaN) pivot
FBA_HD inline bool resect_chol6(const double* N, const double* g, double* x) {
    double L[21], y[6];
    bool ok = true;
#pragma unroll
    for (int i = 0; i < 6; ++i) {
#pragma unroll
        for (int j = 0; j <= i; ++j) {
            double sum = N[i * (i + 1) / 2 + j];
#pragma unroll
            for (int k = 0; k < j; ++k) sum -= L[i * (i + 1) / 2 + k] * L[j * (j + 1) / 2 + k];
            if (i == j) {
                ok = ok && sum > 0.0;
                L[i * (i + 1) / 2 + i] = sqrt(sum);
            } else {
                L[i * (i + 1) / 2 + j] = sum / L[j * (j + 1) / 2 + j];
            }
        }
    }
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        double sum = g[i];
#pragma unroll
        for (int k = 0; k < i; ++k) sum -= L[i * (i + 1) / 2 + k] * y[k];
        y[i] = sum / L[i * (i + 1) / 2 + i];
    }
#pragma unroll
    for (int i = 5; i >= 0; --i) {
        double sum = y[i];
#pragma unroll
        for (int k = i + 1; k < 6; ++k) sum -= L[k * (k + 1) / 2 + i] * x[k];
        x[i] = sum / L[i * (i + 1) / 2 + i];
    }
    return ok;
}

// The resection of one image over a source of sums S:
//   S::moments(o[4])              count, sum X, sum Y, sum Z of the usable records
//   S::spread(m0, m1, m2)         sum |X - m|
//   S::gram(m0, m1, m2, is, A)    the 12 x 12 G into A
//   S::eval(type, P, wx, wy, acc) acc[RESECT_EVAL]
// A, V: 144 doubles each; cur[6]: the image's current values (FEW, WEAK); eop[6], qual[5], status: the outputs of
// fba_resect (include/fba.h)
template <class S>
FBA_HD inline void resect_solve(S& src, int type, double wx, double wy, int refine_iters, double min_ratio,
                                double refine_tol, double* A, double* V, const double* cur, double* eop, double* qual,
                                int& status) {
#pragma unroll
    for (int q = 0; q < 6; ++q) eop[q] = cur[q];
    qual[0] = qual[1] = qual[2] = qual[3] = qual[4] = 0.0;
    status = FBA_RESECT_FEW;
    double mo[4];
    src.moments(mo);
    const double n = mo[0];
    qual[0] = n;
    if (!(n >= (double)RESECT_MIN_PTS)) return;
    status = FBA_RESECT_WEAK;
    const double m0 = mo[1] / n, m1 = mo[2] / n, m2 = mo[3] / n;
    const double s = src.spread(m0, m1, m2) / n;
    src.gram(m0, m1, m2, 1.0 / s, A);
    resect_jacobi12(A, V);
    double lin[6], ratio;
    resect_linear(A, V, m0, m1, m2, s, lin, ratio);
    qual[1] = ratio;
    if (!(ratio >= min_ratio) || !resect_finite6(lin)) return;  // false for a NaN as well
    ResectPose P;
    double acc[RESECT_EVAL];
    resect_pose(lin, P);
    src.eval(type, P, wx, wy, acc);
    if (!(acc[27] <= RESECT_F64_MAX)) return;
    const double rms_lin = sqrt(acc[27] / n), pos_lin = acc[29] / n;
    double rms_fin = rms_lin, pos_fin = pos_lin;
    double x[6];
#pragma unroll
    for (int q = 0; q < 6; ++q) x[q] = lin[q];
    status = FBA_RESECT_OK;
    bool bad = false;
    for (int iter = 0; iter < refine_iters && !bad; ++iter) {
        double st[6], nx[6];
        if (!resect_chol6(acc, acc + 21, st)) { bad = true; break; }
        const double tol = refine_tol * (acc[28] / n);
#pragma unroll
        for (int q = 0; q < 6; ++q) nx[q] = x[q] - st[q];
        if (!resect_finite6(nx)) { bad = true; break; }
        resect_pose(nx, P);
        src.eval(type, P, wx, wy, acc);
        if (!(acc[27] <= RESECT_F64_MAX) || !(acc[28] <= RESECT_F64_MAX)) { bad = true; break; }
#pragma unroll
        for (int q = 0; q < 6; ++q) x[q] = nx[q];
        rms_fin = sqrt(acc[27] / n);
        pos_fin = acc[29] / n;
        if (fmax(fmax(fabs(st[0]), fabs(st[1])), fabs(st[2])) <= tol &&
            fmax(fmax(fabs(st[3]), fabs(st[4])), fabs(st[5])) <= refine_tol)
            break;
    }
    if (bad || !(rms_fin <= rms_lin + 1e-9)) {  // the linear solution stands
        status = FBA_RESECT_REFINE;
#pragma unroll
        for (int q = 0; q < 6; ++q) x[q] = lin[q];
        rms_fin = rms_lin;
        pos_fin = pos_lin;
    }
#pragma unroll
    for (int q = 0; q < 6; ++q) eop[q] = x[q];
    qual[2] = rms_lin;
    qual[3] = rms_fin;
    qual[4] = pos_fin;
}

// the host's source of sums: n records [RESECT_REC] in index order, one camera
struct ResectHostSrc {
    const double* rec;
    const int32_t* use;  // [n] != 0: usable; nullptr: all
    int64_t n;
    double c, ydir;
    bool on(int64_t i) const { return !use || use[i]; }
    void moments(double* o) const {
        o[0] = o[1] = o[2] = o[3] = 0.0;
        for (int64_t i = 0; i < n; ++i)
            if (on(i)) {
                const double* r = rec + RESECT_REC * i;
                o[0] += 1.0; o[1] += r[5]; o[2] += r[6]; o[3] += r[7];
            }
    }
    double spread(double m0, double m1, double m2) const {
        double d = 0.0;
        for (int64_t i = 0; i < n; ++i)
            if (on(i)) {
                const double* r = rec + RESECT_REC * i;
                d += sqrt((r[5] - m0) * (r[5] - m0) + (r[6] - m1) * (r[6] - m1) + (r[7] - m2) * (r[7] - m2));
            }
        return d;
    }
    void gram(double m0, double m1, double m2, double is, double* A) const {
        double g[RESECT_GRAM] = {0.0};
        for (int64_t i = 0; i < n; ++i)
            if (on(i)) resect_gram_add(rec + RESECT_REC * i, m0, m1, m2, is, g, g + 10, g + 20, g + 30, g + 40, g + 50);
        resect_gram_fill<0, 0>(g, A); resect_gram_fill<0, 1>(g + 10, A); resect_gram_fill<0, 2>(g + 20, A);
        resect_gram_fill<1, 1>(g + 30, A); resect_gram_fill<1, 2>(g + 40, A); resect_gram_fill<2, 2>(g + 50, A);
    }
    void eval(int type, const ResectPose& P, double wx, double wy, double* acc) const {
        for (int q = 0; q < RESECT_EVAL; ++q) acc[q] = 0.0;
        for (int64_t i = 0; i < n; ++i)
            if (on(i)) resect_eval_add(type, P, rec + RESECT_REC * i, c, ydir, wx, wy, acc);
    }
};

}  // namespace fba
