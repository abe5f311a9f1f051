// fba_eig3.h -- eigen-decomposition of a symmetric 3 x 3 block by cyclic Jacobi, fp64, for the error
// ellipsoids of the object points (k_ellipsoid, fba_cov.hip) and, the same arithmetic, for the host
// (fba_eig3_host).  No reference counterpart: main.m:460-482 keeps the diagonal of Cx.
//
//   in   blk[6]   XX XY XZ YY YZ ZZ
//   out  ell[12]  the semi-axes a >= b >= c, a = sqrt(max(lambda, 0)), then the three unit axis vectors as
//                 rows in the same order, each with its largest-magnitude component positive (on ties the
//                 first component wins).  A non-finite block gives 12 NaNs.
//
// The block is scaled by a power of two to a largest entry in [0.5, 1) first (exact), so neither the squares
// of the stopping rule nor the rotations over- or underflow.  A sweep rotates (0,1), (0,2), (1,2) in turn
// (Rutishauser's formulas: t from the smaller root, the other entries updated through tau = s / (1 + c)).
// Stopping rule, relative: off = sqrt(a01^2 + a02^2 + a12^2) <= 1e-18 sqrt(a00^2 + a11^2 + a22^2), tested
// before every sweep -- below one ulp of the diagonal by a factor of 200, so what is left changes no
// eigenvalue.  At most FBA_EIG3_SWEEPS = 12 sweeps: cyclic Jacobi converges quadratically, a 3 x 3 block
// takes 4 to 7.  Everything lives in named scalars: no array is indexed dynamically (no scratch on the device).
#pragma once
#include <cmath>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define FBA_HD __host__ __device__
#else
#define FBA_HD
#endif

#define FBA_EIG3_SWEEPS 12

namespace fba {

// one Jacobi rotation in the (p, q) plane: app, aqq, apq the 2 x 2, (arp, arq) the third row's entries,
// (v0p, v0q) .. (v2p, v2q) the eigenvector matrix's columns p and q
#define FBA_EIG3_ROT(app, aqq, apq, arp, arq, v0p, v0q, v1p, v1q, v2p, v2q)               \
    if (apq != 0.0) {                                                                      \
        const double th_ = (aqq - app) / (2.0 * apq);                                      \
        const double t_ = (th_ < 0.0 ? -1.0 : 1.0) / (fabs(th_) + sqrt(th_ * th_ + 1.0)); \
        const double c_ = 1.0 / sqrt(t_ * t_ + 1.0), s_ = t_ * c_, tau_ = s_ / (1.0 + c_); \
        app -= t_ * apq;                                                                   \
        aqq += t_ * apq;                                                                   \
        apq = 0.0;                                                                         \
        double g_ = arp, h_ = arq;                                                         \
        arp = g_ - s_ * (h_ + tau_ * g_); arq = h_ + s_ * (g_ - tau_ * h_);                \
        g_ = v0p; h_ = v0q;                                                                \
        v0p = g_ - s_ * (h_ + tau_ * g_); v0q = h_ + s_ * (g_ - tau_ * h_);                \
        g_ = v1p; h_ = v1q;                                                                \
        v1p = g_ - s_ * (h_ + tau_ * g_); v1q = h_ + s_ * (g_ - tau_ * h_);                \
        g_ = v2p; h_ = v2q;                                                                \
        v2p = g_ - s_ * (h_ + tau_ * g_); v2q = h_ + s_ * (g_ - tau_ * h_);                \
    }

// (lambda, column) pairs in descending order of lambda
#define FBA_EIG3_SWAP(la, lb, xa, ya, za, xb, yb, zb)                  \
    if (lb > la) {                                                      \
        double t_ = la; la = lb; lb = t_;                               \
        t_ = xa; xa = xb; xb = t_;                                      \
        t_ = ya; ya = yb; yb = t_;                                      \
        t_ = za; za = zb; zb = t_;                                      \
    }

// the largest-magnitude component positive; on ties the first wins
#define FBA_EIG3_SIGN(x, y, z)                                          \
    {                                                                   \
        double m_ = fabs(x), p_ = x;                                    \
        if (fabs(y) > m_) { m_ = fabs(y); p_ = y; }                     \
        if (fabs(z) > m_) { p_ = z; }                                   \
        if (p_ < 0.0) { x = -x; y = -y; z = -z; }                       \
    }

FBA_HD inline void eig3(double b00, double b01, double b02, double b11, double b12, double b22, double& ax0,
                        double& ax1, double& ax2, double& d00, double& d01, double& d02, double& d10, double& d11,
                        double& d12, double& d20, double& d21, double& d22) {
    const double big = fmax(fmax(fmax(fabs(b00), fabs(b11)), fabs(b22)), fmax(fmax(fabs(b01), fabs(b02)), fabs(b12)));
    if (!(big <= 1.79769313486231570815e308) || b00 != b00 || b01 != b01 || b02 != b02 || b11 != b11 || b12 != b12 ||
        b22 != b22) {
        const double n = __builtin_nan("");
        ax0 = ax1 = ax2 = d00 = d01 = d02 = d10 = d11 = d12 = d20 = d21 = d22 = n;
        return;
    }
    int ex = 0;
    if (big > 0.0) (void)frexp(big, &ex);
    double a00 = ldexp(b00, -ex), a01 = ldexp(b01, -ex), a02 = ldexp(b02, -ex);
    double a11 = ldexp(b11, -ex), a12 = ldexp(b12, -ex), a22 = ldexp(b22, -ex);
    // eigenvector k is column k: (v0k, v1k, v2k)
    double v00 = 1.0, v01 = 0.0, v02 = 0.0, v10 = 0.0, v11 = 1.0, v12 = 0.0, v20 = 0.0, v21 = 0.0, v22 = 1.0;
    for (int sweep = 0; sweep < FBA_EIG3_SWEEPS; ++sweep) {
        const double off2 = a01 * a01 + a02 * a02 + a12 * a12, dg2 = a00 * a00 + a11 * a11 + a22 * a22;
        if (off2 <= 1e-36 * dg2) break;
        FBA_EIG3_ROT(a00, a11, a01, a02, a12, v00, v01, v10, v11, v20, v21)
        FBA_EIG3_ROT(a00, a22, a02, a01, a12, v00, v02, v10, v12, v20, v22)
        FBA_EIG3_ROT(a11, a22, a12, a01, a02, v01, v02, v11, v12, v21, v22)
    }
    FBA_EIG3_SWAP(a00, a11, v00, v10, v20, v01, v11, v21)
    FBA_EIG3_SWAP(a00, a22, v00, v10, v20, v02, v12, v22)
    FBA_EIG3_SWAP(a11, a22, v01, v11, v21, v02, v12, v22)
    FBA_EIG3_SIGN(v00, v10, v20)
    FBA_EIG3_SIGN(v01, v11, v21)
    FBA_EIG3_SIGN(v02, v12, v22)
    ax0 = sqrt(fmax(ldexp(a00, ex), 0.0));
    ax1 = sqrt(fmax(ldexp(a11, ex), 0.0));
    ax2 = sqrt(fmax(ldexp(a22, ex), 0.0));
    d00 = v00; d01 = v10; d02 = v20;
    d10 = v01; d11 = v11; d12 = v21;
    d20 = v02; d21 = v12; d22 = v22;
}

// blk[6] -> ell[12] (constant indices only)
FBA_HD inline void eig3_block(const double* blk, double* ell) {
    double a0, a1, a2, d00, d01, d02, d10, d11, d12, d20, d21, d22;
    eig3(blk[0], blk[1], blk[2], blk[3], blk[4], blk[5], a0, a1, a2, d00, d01, d02, d10, d11, d12, d20, d21, d22);
    ell[0] = a0; ell[1] = a1; ell[2] = a2;
    ell[3] = d00; ell[4] = d01; ell[5] = d02;
    ell[6] = d10; ell[7] = d11; ell[8] = d12;
    ell[9] = d20; ell[10] = d21; ell[11] = d22;
}

#undef FBA_EIG3_ROT
#undef FBA_EIG3_SWAP
#undef FBA_EIG3_SIGN

}  // namespace fba
