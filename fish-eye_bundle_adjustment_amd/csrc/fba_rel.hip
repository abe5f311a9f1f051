// fba_rel.hip -- observation reliability on the device (gfx950 / MI355X): Baarda's redundancy numbers
// and standardised residuals (w-test) of every image measurement.
//
// No reference counterpart: main.m stops at BuildRSD's raw residuals.  Both quantities need the
// variance of the adjusted observation, a Cx a' of its Jacobian row a with the cofactor Cx = the
// upper-left u x u of the bordered inverse (main.m:428-444) BEFORE the distortion de-scaling and the
// sigma0^2 factor, i.e. in the scaled units of the Jacobian columns of the last linearisation:
//
//   r = 1 - p (a Cx a'),  p = 1 / sigma^2          redundancy number (sum r = n - u + d)
//   w = v / (sigma sqrt(r))                         standardised residual; r < 1e-10: not checkable, w = 0
//
// The row of an observation is a = [E | F]: E its 2 x (6 + cw) image-and-camera part, F its 2 x 3
// tie-point part (F = 0 for a control observation).  The tie points are eliminated, so with the point's
// row groups G (its m images, 6 rows each, and its camera(s), cw rows each), T~ = [T_1; ...; T_m; Tc]
// (T = W V^-1, fba_cov.hip) and Cx_cp = -C T~, Cx_pp = V^-1 + T~' C T~:
//
//   a Cx a' = E C_EE E' - 2 E (C_GG T~)_{rows of E} F' + F (V^-1 + T~' C_GG T~) F'
//
// C = Q - Z' Wz with the inner-constraint border (nz = 14), C = Q without, exactly cget's; Q is the
// selected inverse launch_selinv leaves in S.  Only the diagonal (q_x, q_y) of the 2 x 2 is formed.
//
// Kernels
//   k_rel_pts     regular tie points, ONE WORKGROUP (4 waves) per point.  A point seen by m images has
//                 n = 6 m + cw rows and X = C_GG T~ is n x 3: up to 36.3 KiB at m = CHUNK_OBS, which four
//                 wave-per-point workgroups could not hold in LDS side by side, and a single code path
//                 for every m is worth more here than the last factor of occupancy (the kernel runs once
//                 per adjustment).  The n row indices are staged in LDS once (6 KiB more), so the entry
//                 loops do no division by cw and no gimg / gcam load.  Step 1: X, every row owned by 4 adjacent lanes which walk the row's n
//                 entries of C_GG in column order (stride 4) and are summed by a fixed xor butterfly --
//                 the square pattern is traversed once, cross-block entries through the rr / cc swap of
//                 k_cov_pts, and no sum needs an atomic.  Step 2: the border, X -= Z_G' (Wz_G T~).  Step 3:
//                 the 3 x 3 T~' X, plus V^-1.  Step 4: one wave per observation deals the (6 + cw)^2 entries
//                 of E C_EE E' to its lanes, lanes < nz add the border term, one lane the two F terms.
//   k_rel_gen     the general points of fba_general.hip (several cameras, more than CHUNK_OBS images,
//                 repeated measurements in an image): the same four steps over GenPlan's gimg / gpc
//                 groups; n has no bound there, so X lives in a global scratch ([6 n_gi + cw n_gc][3]).
//                 cw is a run-time argument in all of these kernels (they keep no per-nK register arrays),
//                 so there is one instance instead of one per nK.
//   k_rel_ctl     control observations (F = 0): one wave per observation, step 4's first two terms.
//   k_rel_finish  r, w from q, sigma and fba_residuals' v, scattered to PHO order.
// Every sum runs in a fixed order, no float atomics: results are bitwise reproducible.
#include "fba_internal.h"

#include <algorithm>

namespace fba {

constexpr int RB = NB;
constexpr int REL_ROWS = 6 * CHUNK_OBS + 5 + FBA_NK_MAX;  // rows of a regular point's groups, at most

__device__ __forceinline__ double rel_wave_sum(double v) {
#pragma unroll
    for (int w = 32; w > 0; w >>= 1) v += __shfl_xor(v, w, 64);
    return v;
}
__device__ __forceinline__ double rel_quad_sum(double v) {  // the 4 lanes of a row, every lane gets the sum
    v += __shfl_xor(v, 1, 64);
    v += __shfl_xor(v, 2, 64);
    return v;
}

// Q(r, c) from the selected inverse in S (lower blocks; diagonal blocks full)
__device__ __forceinline__ double qget(const double* __restrict__ S, int64_t ld, int64_t r, int64_t c) {
    const int64_t rr = (r / RB >= c / RB) ? r : c, cc = (r / RB >= c / RB) ? c : r;
    return S[rr * ld + cc];
}

// the row groups of one point: ni image groups (6 rows of image slot gimg[g], T at Ti + g ti_stride), then
// nc camera groups (cw rows of camera gcam[x], Tc at Tc + x tc_stride); row j of the n = 6 ni + cw nc
struct RelRows {
    int ni, nc, cw, n;
    const int32_t* gimg;
    const int32_t* gcam;
    const double* Ti;
    int64_t ti_stride;
    const double* Tc;
    int64_t tc_stride;
    int64_t cam_base;  // 6 n_img
    __device__ __forceinline__ int64_t row(int j) const {
        if (j < 6 * ni) return 6 * (int64_t)gimg[j / 6] + j % 6;
        const int e = j - 6 * ni;
        return cam_base + (int64_t)gcam[e / cw] * cw + e % cw;
    }
    __device__ __forceinline__ const double* trow(int j) const {
        if (j < 6 * ni) return Ti + (j / 6) * ti_stride + 3 * (j % 6);
        const int e = j - 6 * ni;
        return Tc + (e / cw) * tc_stride + 3 * (e % cw);
    }
};

struct RelMat {  // the camera-side cofactor: selected inverse and the border's low-rank term
    const double* S;
    int64_t ld;
    const double* Z;
    const double* Wz;
    int nz;
    int64_t n_pad;
};

// steps 1-3 for one point by a workgroup of 256: X [n][3] (LDS or global), cpp [9] = V^-1 + T~' X (LDS),
// wt [42] LDS scratch.  vinv: 00 01 02 11 12 22.
//
// STAGED (regular points, n <= REL_ROWS): the n row indices are computed once into rows (LDS) instead of once per
// entry (a division by the run-time cw and a gimg / gcam load each), and T~'s rows are read where they lie: the
// images' T are contiguous (18 per observation = 3 per row) and there is one camera.  General points have no
// bound on n and keep R.row / R.trow.  The values and the order of every sum are the same either way.
template <bool STAGED>
__device__ __forceinline__ void rel_point(const RelRows& R, const RelMat& M, const double* __restrict__ vinv,
                                          double* X, double* cpp, double* wt, int32_t* rows) {
    const int t = threadIdx.x, sub = t & 3, n = R.n;
    if (STAGED) {
        for (int j = t; j < n; j += 256) rows[j] = (int32_t)R.row(j);  // < n_pad, far below 2^31
        __syncthreads();
    }
    auto rowof = [&](int j) -> int64_t { return STAGED ? (int64_t)rows[j] : R.row(j); };
    auto trowof = [&](int j) -> const double* {
        if (!STAGED) return R.trow(j);
        return j < 6 * R.ni ? R.Ti + 3 * j : R.Tc + 3 * (j - 6 * R.ni);
    };
    for (int j0 = 0; j0 < n; j0 += 64) {
        const int j = j0 + (t >> 2);
        double s0 = 0.0, s1 = 0.0, s2 = 0.0;
        if (j < n) {
            const int64_t r = rowof(j);
            for (int i = sub; i < n; i += 4) {
                const double v = qget(M.S, M.ld, r, rowof(i));
                const double* T = trowof(i);
                s0 += v * T[0]; s1 += v * T[1]; s2 += v * T[2];
            }
        }
        s0 = rel_quad_sum(s0); s1 = rel_quad_sum(s1); s2 = rel_quad_sum(s2);
        if (j < n && sub == 0) { X[3 * j] = s0; X[3 * j + 1] = s1; X[3 * j + 2] = s2; }
    }
    if (M.nz) {  // wt[a][k] = sum_j Wz[a][row j] T~[j][k], then X[j][k] -= sum_a Z[a][row j] wt[a][k]
        const int a = t / 12, k = (t >> 2) % 3;
        double s = 0.0;
        if (a < M.nz)
            for (int i = sub; i < n; i += 4) s += M.Wz[a * M.n_pad + rowof(i)] * trowof(i)[k];
        s = rel_quad_sum(s);
        if (a < M.nz && sub == 0) wt[3 * a + k] = s;
        __syncthreads();  // wt, and step 1's X
        for (int j = t; j < n; j += 256) {
            const int64_t r = rowof(j);
            double d0 = 0.0, d1 = 0.0, d2 = 0.0;
            for (int b = 0; b < M.nz; ++b) {
                const double z = M.Z[b * M.n_pad + r];
                d0 += z * wt[3 * b]; d1 += z * wt[3 * b + 1]; d2 += z * wt[3 * b + 2];
            }
            X[3 * j] -= d0; X[3 * j + 1] -= d1; X[3 * j + 2] -= d2;
        }
    }
    __syncthreads();
    {  // cpp[k][l] = V^-1[k][l] + sum_j T~[j][k] X[j][l]
        const int e = t >> 2, k = e / 3, l = e % 3;
        double s = 0.0;
        if (e < 9)
            for (int i = sub; i < n; i += 4) s += trowof(i)[k] * X[3 * i + l];
        s = rel_quad_sum(s);
        if (e < 9 && sub == 0) {
            const int lo = k < l ? k : l, hi = k < l ? l : k;
            cpp[e] = vinv[lo == 0 ? hi : lo + hi + 1] + s;  // 00 01 02 11 12 22
        }
    }
    __syncthreads();
}

// step 4 for one observation by one wave: q_x, q_y of its Jacobian rows Jo (x at 0, y at nj: 6 EOP | cw
// camera | 3 XYZ) with image rows r_img.., camera rows r_cam..; Xi / Xc: the X rows of its image / camera
// group (nullptr: a control observation, F = 0)
__device__ __forceinline__ void rel_obs(int lane, const double* __restrict__ Jo, int nj, int cw, int64_t r_img,
                                        int64_t r_cam, const RelMat& M, const double* Xi, const double* Xc,
                                        const double* cpp, double* __restrict__ qout) {
    const int ne = 6 + cw;
    double qx = 0.0, qy = 0.0;
    for (int idx = lane; idx < ne * ne; idx += 64) {
        const int a = idx / ne, b = idx - ne * a;
        const int64_t ra = a < 6 ? r_img + a : r_cam + (a - 6), rb = b < 6 ? r_img + b : r_cam + (b - 6);
        const double v = qget(M.S, M.ld, ra, rb);
        qx += Jo[a] * v * Jo[b];
        qy += Jo[nj + a] * v * Jo[nj + b];
    }
    if (lane < M.nz) {
        double zx = 0.0, wx = 0.0, zy = 0.0, wy = 0.0;
        for (int a = 0; a < ne; ++a) {
            const int64_t ra = a < 6 ? r_img + a : r_cam + (a - 6);
            const double zv = M.Z[lane * M.n_pad + ra], wv = M.Wz[lane * M.n_pad + ra];
            zx += zv * Jo[a]; wx += wv * Jo[a];
            zy += zv * Jo[nj + a]; wy += wv * Jo[nj + a];
        }
        qx -= zx * wx;
        qy -= zy * wy;
    }
    if (Xi && lane == 32) {
#pragma unroll
        for (int row = 0; row < 2; ++row) {
            const double* e = Jo + row * nj;
            const double* f = e + 6 + cw;
            double t0 = 0.0, t1 = 0.0, t2 = 0.0;
            for (int a = 0; a < 6; ++a) { t0 += e[a] * Xi[3 * a]; t1 += e[a] * Xi[3 * a + 1]; t2 += e[a] * Xi[3 * a + 2]; }
            for (int c = 0; c < cw; ++c) {
                t0 += e[6 + c] * Xc[3 * c]; t1 += e[6 + c] * Xc[3 * c + 1]; t2 += e[6 + c] * Xc[3 * c + 2];
            }
            double pp = 0.0;
            for (int k = 0; k < 3; ++k) pp += f[k] * (cpp[3 * k] * f[0] + cpp[3 * k + 1] * f[1] + cpp[3 * k + 2] * f[2]);
            const double s = pp - 2.0 * (t0 * f[0] + t1 * f[1] + t2 * f[2]);
            if (row == 0) qx += s;
            else qy += s;
        }
    }
    qx = rel_wave_sum(qx);
    qy = rel_wave_sum(qy);
    if (lane == 0) { qout[0] = qx; qout[1] = qy; }
}

// regular tie points: one workgroup per local point p (observations lp_start[p] .. lp_start[p + 1], one per
// image, one camera)
__global__ __launch_bounds__(256) void k_rel_pts(RelMat M, const double* __restrict__ J, int js,
                                                 const double* __restrict__ WT, const double* __restrict__ PT, int ps,
                                                 const int32_t* __restrict__ lp_start, const int32_t* __restrict__ lp_cam,
                                                 const int32_t* __restrict__ img, int n_img, int cw,
                                                 double* __restrict__ q) {
    __shared__ double X[3 * REL_ROWS];
    __shared__ double cpp[9], wt[42];
    __shared__ int32_t rows[REL_ROWS];
    const int64_t p = blockIdx.x;
    const int o0 = lp_start[p], m = lp_start[p + 1] - o0;
    if (m <= 0 || m > CHUNK_OBS) return;  // (the chunking admits no such point)
    const double* P = PT + p * ps;
    RelRows R;
    R.ni = m; R.nc = 1; R.cw = cw; R.n = 6 * m + cw;
    R.gimg = img + o0; R.gcam = lp_cam + p;
    R.Ti = WT + (int64_t)o0 * T_ROW; R.ti_stride = T_ROW;
    R.Tc = P + pt_tc(cw); R.tc_stride = 0;
    R.cam_base = 6 * (int64_t)n_img;
    rel_point<true>(R, M, P, X, cpp, wt, rows);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, nj = 9 + cw;
    const int64_t r_cam = R.cam_base + (int64_t)lp_cam[p] * cw;
    for (int g = wave; g < m; g += 4)
        rel_obs(lane, J + (int64_t)(o0 + g) * js, nj, cw, 6 * (int64_t)img[o0 + g], r_cam, M, X + 18 * g, X + 18 * m, cpp,
                q + 2 * (int64_t)(o0 + g));
}

// general points: one workgroup per point; X in the global scratch Xg, the rows of gimg i at 6 i, of gpc
// x at 6 n_gi + cw x (a point's gimgs and gpcs are contiguous)
__global__ __launch_bounds__(256) void k_rel_gen(RelMat M, const double* __restrict__ J, int js,
                                                 const int32_t* __restrict__ A, const GenPlan g,
                                                 const double* __restrict__ gpt, const double* __restrict__ gcu,
                                                 const double* __restrict__ gug, int n_img, int cw,
                                                 double* __restrict__ Xg, double* __restrict__ q) {
    __shared__ double cpp[9], wt[42];
    const int64_t pq = blockIdx.x;
    const int i0 = A[g.g_gi + pq], ni = A[g.g_gi + pq + 1] - i0;
    const int c0 = A[g.g_gc + pq], nc = A[g.g_gc + pq + 1] - c0;
    RelRows R;
    R.ni = ni; R.nc = nc; R.cw = cw; R.n = 6 * ni + cw * nc;
    R.gimg = A + g.gi_img + i0; R.gcam = A + g.gc_cam + c0;
    R.Ti = gug + (int64_t)i0 * GUG + GUG_T; R.ti_stride = GUG;
    R.Tc = gcu + (int64_t)c0 * 6 * cw + 3 * cw; R.tc_stride = gpc_tab(cw);  // (row c0 of gpc_tab(cw), its Tc half)
    R.cam_base = 6 * (int64_t)n_img;
    // this point's X: [6 ni rows of its gimgs | cw nc rows of its gpcs], at the offset of all earlier points'
    double* X = Xg + 3 * (6 * (int64_t)i0 + (int64_t)cw * c0);
    rel_point<false>(R, M, gpt + pq * GPT, X, cpp, wt, nullptr);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, nj = 9 + cw;
    for (int gi = wave; gi < ni; gi += 4) {
        const int xc = A[g.gi_gc + i0 + gi] - c0;  // the gpc of the image's camera
        const int64_t r_img = 6 * (int64_t)A[g.gi_img + i0 + gi];
        const int64_t r_cam = R.cam_base + (int64_t)A[g.gc_cam + c0 + xc] * cw;
        for (int o = A[g.gi_obs + i0 + gi]; o < A[g.gi_obs + i0 + gi + 1]; ++o)
            rel_obs(lane, J + (int64_t)o * js, nj, cw, r_img, r_cam, M, X + 18 * gi, X + 18 * ni + 3 * cw * xc, cpp,
                    q + 2 * (int64_t)o);
    }
}

// control observations: one wave per local observation o0 + i with pt < 0
__global__ __launch_bounds__(256) void k_rel_ctl(RelMat M, const double* __restrict__ J, int js,
                                                 const int32_t* __restrict__ img, const int32_t* __restrict__ cam,
                                                 const int32_t* __restrict__ pt, int64_t o0, int64_t o1, int n_img, int cw,
                                                 double* __restrict__ q) {
    const int64_t o = o0 + (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (o >= o1 || pt[o] >= 0) return;
    rel_obs(threadIdx.x & 63, J + o * js, 9 + cw, cw, 6 * (int64_t)img[o], 6 * (int64_t)n_img + (int64_t)cam[o] * cw, M,
            nullptr, nullptr, nullptr, q + 2 * o);
}

// r = 1 - p q, w = v / (sigma sqrt(r)) (0 where r < 1e-10), local observation o -> PHO row obs_pho[o].  With
// per-observation weights / a robust loss (seff: k_lin_point's s, else nullptr) q comes from whitened rows, so
// r needs nothing, and the standardised residual is that of the whitened v: w = v s / (sigma sqrt(r)) (v is raw)
__global__ __launch_bounds__(256) void k_rel_finish(const double* __restrict__ q, const double* __restrict__ v,
                                                    const int64_t* __restrict__ obs_pho, int64_t n_obs, double sx,
                                                    double sy, const double* __restrict__ seff,
                                                    double* __restrict__ red, double* __restrict__ wst) {
    const int64_t o = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (o >= n_obs) return;
    const int64_t i = obs_pho[o];
#pragma unroll
    for (int m = 0; m < 2; ++m) {
        const double s = m ? sy : sx;
        const double r = 1.0 - q[2 * o + m] / (s * s);
        red[2 * i + m] = r;
        const double vm = seff ? v[2 * o + m] * seff[2 * o + m] : v[2 * o + m];
        wst[2 * i + m] = r < 1e-10 ? 0.0 : vm / (s * sqrt(r));
    }
}

int launch_obs_T(Ctx& c, double* T);

// after launch_selinv (and launch_cov_outputs, which shares d_T): v of the last linearisation into c.d_res and
// q = a Cx a' per local observation into d_q [2 n_obs] (local order) -- the part of the reliability outputs that
// fba_vce shares.  Runs launch_residuals for v, so c.d_res / c.d_part are overwritten (fba_residuals recomputes both).
int launch_rel_q(Ctx& c, SelInv& si, double* d_q) {
    const Layout& L = c.L;
    const GenPlan& g = c.gen;
    int rc;
    const RelMat M{c.d_S, L.ld, si.d_Z, si.d_Wz, si.nz, L.n_pad};
    if (c.n_obs == 0) return FBA_OK;
    if ((rc = launch_residuals(c))) return rc;  // v of the last linearisation (d_J) and correction, as fba_residuals
    if (c.n_lp > 0) {
        if (!si.d_T && ((rc = ws_get(c, WS_OBS_T, (size_t)T_ROW * std::max<int64_t>(c.n_obs_tie, 1), &si.d_T)) || (rc = launch_obs_T(c, si.d_T))))
            return rc;
        k_rel_pts<<<(unsigned)c.n_lp, 256, 0, c.stream>>>(M, c.d_J, c.ncomp, si.d_T, c.d_pt_tab, c.pt_comp, c.d_lp_start,
                                                         c.d_lp_cam, c.d_img, L.n_img, L.cw, d_q);
    }
    // the control observations follow the regular points' (the general points' come last: pt >= 0, skipped)
    if (c.n_obs > c.n_obs_tie)
        k_rel_ctl<<<(unsigned)((c.n_obs - c.n_obs_tie + 3) / 4), 256, 0, c.stream>>>(M, c.d_J, c.ncomp, c.d_img, c.d_cam, c.d_pt,
                                                                                  c.n_obs_tie, c.n_obs, L.n_img, L.cw, d_q);
    if (g.n_gp > 0) {
        double* d_Xg = nullptr;
        if ((rc = ws_get(c, WS_REL_XG, (size_t)3 * (6 * (size_t)g.n_gi + (size_t)L.cw * g.n_gc), &d_Xg))) return rc;
        k_rel_gen<<<(unsigned)g.n_gp, 256, 0, c.stream>>>(M, c.d_J, c.ncomp, c.d_acc, g, c.d_gpt, c.d_gcu, c.d_gug, L.n_img,
                                                         L.cw, d_Xg, d_q);
    }
    FBA_HIP(hipGetLastError());
    return FBA_OK;
}

// launch_rel_q, then r and w in PHO order into d_red / d_wst [2 n_pts] (zeroed first: another rank's rows)
int launch_rel_outputs(Ctx& c, SelInv& si, double* d_q, double* d_red, double* d_wst) {
    int rc;
    FBA_HIP(hipMemsetAsync(d_red, 0, sizeof(double) * 2 * std::max<int64_t>(c.n_pts, 1), c.stream));
    FBA_HIP(hipMemsetAsync(d_wst, 0, sizeof(double) * 2 * std::max<int64_t>(c.n_pts, 1), c.stream));
    if (c.n_obs == 0) return FBA_OK;
    if ((rc = launch_rel_q(c, si, d_q))) return rc;
    k_rel_finish<<<(unsigned)((c.n_obs + 255) / 256), 256, 0, c.stream>>>(d_q, c.d_res, c.d_obs_pho, c.n_obs,
                                                                         c.set.meas_std_x, c.set.meas_std_y,
                                                                         c.whiten_on() ? c.d_seff : nullptr, d_red, d_wst);
    FBA_HIP(hipGetLastError());
    return FBA_OK;
}

}  // namespace fba
