// fba_intersect.hip -- forward intersection of the tie points from the measured image rays, for gfx950 (MI355X).
// No reference counterpart: Buildxhat.m:107-134 copies the object points' starting values from the .cnt file.
//
//   k_rays       one thread per local observation (tie and control alike): the closed-form image ray of the
//                measurement (ray_unproject, fba_ray.h) from k_params' camera table, rotated into the object frame
//                with M' of the image table; stores [C | d] (6 doubles), the status and the corrected image
//                coordinates (xu, yu) -- all the refinement needs of the measurement, the distortion being a function
//                of the measured coordinates alone
//   k_intersect  a group of 8 lanes per local tie point, regular (lp_start) and general (GenPlan::g_obs) alike:
//                (a) A = sum (I - d d'), b = sum (I - d d')(C - C0) over the rays with status OK, C0 the first ray's
//                    centre (against cancellation); lambda_min / lambda_max of A (eig3, fba_eig3.h); X by the
//                    symmetric adjugate, as k_lin_point inverts V;
//                (b) point-only Gauss-Newton passes X <- X - V^-1 g, V = Jp'PJp, g = Jp'Pw (ray_project: obs_model's
//                    tie columns), P = diag(px, py), stopped at |dX|_inf <= tol x the mean distance to the centres;
//                (c) the RMS reprojection residual through the forward model at the linear and the final solution.
// Every sum is taken in a fixed order that does not depend on the launch geometry: lane l of the group adds the
// point's rays l, l + 8, ... in ascending order, then a fixed xor tree (4, 2, 1) over the 8 lanes -- a sub-wave shuffle,
// no LDS, no __syncthreads, no atomics; fp addition commutes, so all 8 lanes hold bitwise the same sums and take the
// same branches.  Two calls are bitwise equal.
//
// The rays are LINES: a point intersected on the wrong half-line of a camera (the camera looking away from it) is a
// valid solution of (a); the forward model's atan(R / W) folds it back, so it shows up as a huge RMS in (c).  Nothing
// here guesses the camera's sign convention.
#include "fba_eig3.h"
#include "fba_internal.h"
#include "fba_ray.h"

namespace fba {

constexpr int IS_LANES = 8;  // lanes per tie point (k_intersect)

template <int NK>
__global__ __launch_bounds__(256) void k_rays(const double* __restrict__ xy, const int32_t* __restrict__ img,
                                              const int32_t* __restrict__ cam, const double* __restrict__ img_tab,
                                              const double* __restrict__ cam_tab, int64_t n_obs, int type, int cam_stride,
                                              double* __restrict__ ray, int32_t* __restrict__ rst,
                                              double* __restrict__ xuo) {
    const int64_t o = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (o >= n_obs) return;
    const double2 xyv = *reinterpret_cast<const double2*>(xy + 2 * o);
    const double* it = img_tab + (int64_t)img[o] * IMG_TAB;
    const double* ct = cam_tab + (int64_t)cam[o] * cam_stride;
    double xu, yu, c0, c1, c2;
    const int st = ray_unproject<NK>(xyv.x, xyv.y, ct[0], ct[1], ct[2], ct[3], ct[4], ct[5], ct + CAM_TAB_HDR, NK, type,
                                     xu, yu, c0, c1, c2);
    const double* M = it + 6;  // d_obj = M' d_cam
    double2* r = reinterpret_cast<double2*>(ray + RAY_REC * o);
    r[0] = double2{it[0], it[1]};
    r[1] = double2{it[2], M[0] * c0 + M[3] * c1 + M[6] * c2};
    r[2] = double2{M[1] * c0 + M[4] * c1 + M[7] * c2, M[2] * c0 + M[5] * c1 + M[8] * c2};
    *reinterpret_cast<double2*>(xuo + 2 * o) = double2{xu, yu};
    rst[o] = st;
}

// sum over the 8 lanes of the group, the same value in all of them
__device__ __forceinline__ double group_sum(double v) {
    v += __shfl_xor(v, 4, IS_LANES);
    v += __shfl_xor(v, 2, IS_LANES);
    v += __shfl_xor(v, 1, IS_LANES);
    return v;
}

// the group's sums at X over the point's usable rays: V = Jp'PJp (00 01 02 11 12 22), g = Jp'Pw, ssq = sum wx^2 + wy^2
// (pixels), dsum = sum |X - C|
struct IsectEval {
    double V00, V01, V02, V11, V12, V22, g0, g1, g2, ssq, dsum;
};
__device__ __forceinline__ void isect_eval(int lane, int o0, int o1, const double* __restrict__ ray,
                                           const int32_t* __restrict__ rst, const double* __restrict__ xuo,
                                           const int32_t* __restrict__ img, const int32_t* __restrict__ cam,
                                           const double* __restrict__ img_tab, const double* __restrict__ cam_tab,
                                           int cam_stride, int type, double px, double py, double X0, double X1, double X2,
                                           IsectEval& e) {
    double V00 = 0, V01 = 0, V02 = 0, V11 = 0, V12 = 0, V22 = 0, g0 = 0, g1 = 0, g2 = 0, ssq = 0, dsum = 0;
    for (int i = o0 + lane; i < o1; i += IS_LANES) {
        if (rst[i] != FBA_RAY_OK) continue;
        const double* r = ray + RAY_REC * (int64_t)i;
        const double* ct = cam_tab + (int64_t)cam[i] * cam_stride;
        const double2 u = *reinterpret_cast<const double2*>(xuo + 2 * (int64_t)i);
        const double e0 = X0 - r[0], e1 = X1 - r[1], e2 = X2 - r[2];
        double fx, fy, jp[6];
        ray_project(type, img_tab + (int64_t)img[i] * IMG_TAB + 6, e0, e1, e2, ct[2], ct[3], fx, fy, jp);
        const double w0 = fx - u.x, w1 = fy - u.y;
        const double a0 = px * jp[0], a1 = px * jp[1], a2 = px * jp[2];
        const double b0 = py * jp[3], b1 = py * jp[4], b2 = py * jp[5];
        V00 += a0 * jp[0] + b0 * jp[3]; V01 += a0 * jp[1] + b0 * jp[4]; V02 += a0 * jp[2] + b0 * jp[5];
        V11 += a1 * jp[1] + b1 * jp[4]; V12 += a1 * jp[2] + b1 * jp[5]; V22 += a2 * jp[2] + b2 * jp[5];
        g0 += a0 * w0 + b0 * w1; g1 += a1 * w0 + b1 * w1; g2 += a2 * w0 + b2 * w1;
        ssq += w0 * w0 + w1 * w1;
        dsum += sqrt(e0 * e0 + e1 * e1 + e2 * e2);
    }
    e.V00 = group_sum(V00); e.V01 = group_sum(V01); e.V02 = group_sum(V02);
    e.V11 = group_sum(V11); e.V12 = group_sum(V12); e.V22 = group_sum(V22);
    e.g0 = group_sum(g0); e.g1 = group_sum(g1); e.g2 = group_sum(g2);
    e.ssq = group_sum(ssq);
    e.dsum = group_sum(dsum);
}

// x = S^-1 r of a symmetric 3 x 3 S by the adjugate (k_lin_point's inverse)
__device__ __forceinline__ void sym3_solve(double S00, double S01, double S02, double S11, double S12, double S22, double r0,
                                           double r1, double r2, double& x0, double& x1, double& x2) {
    const double c00 = S11 * S22 - S12 * S12, c01 = S02 * S12 - S01 * S22, c02 = S01 * S12 - S02 * S11;
    const double id = 1.0 / (S00 * c00 + S01 * c01 + S02 * c02);
    const double I00 = c00 * id, I01 = c01 * id, I02 = c02 * id;
    const double I11 = (S00 * S22 - S02 * S02) * id, I12 = (S01 * S02 - S00 * S12) * id, I22 = (S00 * S11 - S01 * S01) * id;
    x0 = I00 * r0 + I01 * r1 + I02 * r2;
    x1 = I01 * r0 + I11 * r1 + I12 * r2;
    x2 = I02 * r0 + I12 * r1 + I22 * r2;
}

__device__ __forceinline__ bool finite3(double a, double b, double c) {
    return fabs(a) <= 1.79769313486231570815e308 && fabs(b) <= 1.79769313486231570815e308 &&
           fabs(c) <= 1.79769313486231570815e308;
}

__global__ __launch_bounds__(256) void k_intersect(
    const double* __restrict__ ray, const int32_t* __restrict__ rst, const double* __restrict__ xuo,
    const int32_t* __restrict__ img, const int32_t* __restrict__ cam, const double* __restrict__ img_tab,
    const double* __restrict__ cam_tab, const int32_t* __restrict__ lp_start, const int32_t* __restrict__ g_obs,
    const int32_t* __restrict__ lp_tie, int64_t n_lp, int64_t n_gp, int64_t u_c, int cam_stride, int type, double px,
    double py, int refine_iters, double min_ratio, double refine_tol, int write, double* __restrict__ xfull,
    double* __restrict__ xyz, double* __restrict__ qual, int32_t* __restrict__ stat) {
    const int64_t p = ((int64_t)blockIdx.x * 256 + threadIdx.x) / IS_LANES;  // whole groups leave together
    if (p >= n_lp + n_gp) return;
    const int lane = threadIdx.x & (IS_LANES - 1);
    const int o0 = p < n_lp ? lp_start[p] : g_obs[p - n_lp], o1 = p < n_lp ? lp_start[p + 1] : g_obs[p - n_lp + 1];
    const int64_t tie = lp_tie[p];
    double* xcur = xfull + u_c + 3 * tie;
    double X0 = xcur[0], X1 = xcur[1], X2 = xcur[2];  // FEW, WEAK: the point's current value
    double nray = 0.0, ratio = 0.0, rms_lin = 0.0, rms_fin = 0.0;
    int status = FBA_ISECT_FEW;
    if (o1 > o0) {
        // (a) the linear solution, relative to the first ray's centre
        const double C0 = ray[RAY_REC * (int64_t)o0], C1 = ray[RAY_REC * (int64_t)o0 + 1], C2 = ray[RAY_REC * (int64_t)o0 + 2];
        double A00 = 0, A01 = 0, A02 = 0, A11 = 0, A12 = 0, A22 = 0, b0 = 0, b1 = 0, b2 = 0, cnt = 0;
        for (int i = o0 + lane; i < o1; i += IS_LANES) {
            if (rst[i] != FBA_RAY_OK) continue;
            const double* r = ray + RAY_REC * (int64_t)i;
            const double d0 = r[3], d1 = r[4], d2 = r[5];
            const double m00 = 1.0 - d0 * d0, m01 = -d0 * d1, m02 = -d0 * d2, m11 = 1.0 - d1 * d1, m12 = -d1 * d2,
                         m22 = 1.0 - d2 * d2;
            const double e0 = r[0] - C0, e1 = r[1] - C1, e2 = r[2] - C2;
            A00 += m00; A01 += m01; A02 += m02; A11 += m11; A12 += m12; A22 += m22;
            b0 += m00 * e0 + m01 * e1 + m02 * e2;
            b1 += m01 * e0 + m11 * e1 + m12 * e2;
            b2 += m02 * e0 + m12 * e1 + m22 * e2;
            cnt += 1.0;
        }
        A00 = group_sum(A00); A01 = group_sum(A01); A02 = group_sum(A02);
        A11 = group_sum(A11); A12 = group_sum(A12); A22 = group_sum(A22);
        b0 = group_sum(b0); b1 = group_sum(b1); b2 = group_sum(b2);
        nray = group_sum(cnt);
        if (nray >= 2.0) {
            double ax0, ax1, ax2, v00, v01, v02, v10, v11, v12, v20, v21, v22;
            eig3(A00, A01, A02, A11, A12, A22, ax0, ax1, ax2, v00, v01, v02, v10, v11, v12, v20, v21, v22);
            ratio = (ax2 * ax2) / (ax0 * ax0);  // eig3 returns sqrt(max(lambda, 0)), descending
            status = FBA_ISECT_WEAK;
            if (ratio >= min_ratio) {  // false for a NaN as well
                double L0, L1, L2;
                sym3_solve(A00, A01, A02, A11, A12, A22, b0, b1, b2, L0, L1, L2);
                L0 += C0; L1 += C1; L2 += C2;
                IsectEval e;
                isect_eval(lane, o0, o1, ray, rst, xuo, img, cam, img_tab, cam_tab, cam_stride, type, px, py, L0, L1, L2, e);
                X0 = L0; X1 = L1; X2 = L2;
                rms_lin = rms_fin = sqrt(e.ssq / nray);
                status = FBA_ISECT_OK;
                // (b) point-only Gauss-Newton from the linear solution
                bool bad = !finite3(L0, L1, L2);
                for (int iter = 0; iter < refine_iters && !bad; ++iter) {
                    double s0, s1, s2;
                    sym3_solve(e.V00, e.V01, e.V02, e.V11, e.V12, e.V22, e.g0, e.g1, e.g2, s0, s1, s2);
                    const double tol = refine_tol * (e.dsum / nray);
                    const double N0 = X0 - s0, N1 = X1 - s1, N2 = X2 - s2;
                    isect_eval(lane, o0, o1, ray, rst, xuo, img, cam, img_tab, cam_tab, cam_stride, type, px, py, N0, N1, N2, e);
                    if (!finite3(N0, N1, N2) || !finite3(e.ssq, e.dsum, e.V00 + e.V11 + e.V22)) {
                        bad = true;
                        break;
                    }
                    X0 = N0; X1 = N1; X2 = N2;
                    rms_fin = sqrt(e.ssq / nray);
                    if (fmax(fmax(fabs(s0), fabs(s1)), fabs(s2)) <= tol) break;
                }
                if (bad || !(rms_fin <= rms_lin + 1e-9)) {  // the linear solution stands
                    status = FBA_ISECT_REFINE;
                    X0 = L0; X1 = L1; X2 = L2;
                    rms_fin = rms_lin;
                }
            }
        }
    }
    if (lane == 0) {
        const bool have = status == FBA_ISECT_OK || status == FBA_ISECT_REFINE;
        xyz[3 * tie] = X0; xyz[3 * tie + 1] = X1; xyz[3 * tie + 2] = X2;
        *reinterpret_cast<double2*>(qual + 4 * tie) = double2{nray, status == FBA_ISECT_FEW ? 0.0 : ratio};
        *reinterpret_cast<double2*>(qual + 4 * tie + 2) = double2{have ? rms_lin : 0.0, have ? rms_fin : 0.0};
        stat[tie] = status;
        if (write && have) { xcur[0] = X0; xcur[1] = X1; xcur[2] = X2; }
    }
}

#define FBA_IS_NK_DISPATCH(nk, F)     \
    switch (nk) {                     \
        case 1: F(1); break;          \
        case 2: F(2); break;          \
        case 3: F(3); break;          \
        case 4: F(4); break;          \
        case 5: F(5); break;          \
        case 6: F(6); break;          \
        case 7: F(7); break;          \
        case 8: F(8); break;          \
        default: set_error("num_radial out of range"); return FBA_ERR_UNSUPPORTED; \
    }

int launch_rays(Ctx& c, double* ray, int32_t* rst, double* xu) {
    if (c.n_obs <= 0) return FBA_OK;
    const unsigned nblk = (unsigned)((c.n_obs + 255) / 256);
#define RY(NKV)                                                                                                      \
    k_rays<NKV><<<nblk, 256, 0, c.stream>>>(c.d_xy, c.d_img, c.d_cam, c.d_img_tab, c.d_cam_tab, c.n_obs, c.set.type, \
                                            c.cam_tab_stride, ray, rst, xu)
    FBA_IS_NK_DISPATCH(c.L.nk, RY);
#undef RY
    FBA_HIP(hipGetLastError());
    return FBA_OK;
}

int launch_intersect(Ctx& c, const double* ray, const int32_t* rst, const double* xu, int refine_iters, double min_ratio,
                     double refine_tol, bool write, double* xyz, double* qual, int32_t* st) {
    const int64_t np = c.n_lp + c.gen.n_gp;
    if (np <= 0) return FBA_OK;
    const unsigned nblk = (unsigned)((np * IS_LANES + 255) / 256);
    const double px = 1.0 / (c.set.meas_std_x * c.set.meas_std_x), py = 1.0 / (c.set.meas_std_y * c.set.meas_std_y);
    k_intersect<<<nblk, 256, 0, c.stream>>>(ray, rst, xu, c.d_img, c.d_cam, c.d_img_tab, c.d_cam_tab, c.d_lp_start,
                                            c.d_acc + c.gen.g_obs, c.d_lp_tie, c.n_lp, c.gen.n_gp, c.L.u_c,
                                            c.cam_tab_stride, c.set.type, px, py, refine_iters, min_ratio, refine_tol,
                                            write ? 1 : 0, c.d_xfull, xyz, qual, st);
    FBA_HIP(hipGetLastError());
    return FBA_OK;
}

}  // namespace fba
