// fba_api_postfit.cpp -- the C API of the post-fit outputs: fba_covariance, fba_reliability and fba_postfit_outputs
// on one selected inverse of the last solve's factor (include/fba.h; the kernels in fba_cov.hip and fba_rel.hip).
#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

#include "fba_api.h"

using namespace fba;

// fba_covariance, and with rel fba_reliability: the same launches and host code for cx_diag / corr, then the
// reliability kernels on the same selected inverse (redundancy / wstat [2 n_pts], either may be NULL)
// fba_postfit_outputs: besides those four, the tie points' full blocks (cx_tie [TIE_BLK n_tie], TIE order) and their
// ellipsoids (ellipsoid [ELL_OUT n_tie]); either may be NULL, the ellipsoids alone keep the blocks in workspace
static int covariance_impl(Ctx* c, const char* who, double sigma02, double* cx_diag, double* corr, bool rel,
                           double* redundancy, double* wstat, double* cx_tie = nullptr, double* ellipsoid = nullptr) {
    if (!c) { set_error("NULL context"); return FBA_ERR_ARG; }
    if (rel && c->sched.split) {
        set_error(std::string(who) + ": redundancy / wstat are not implemented for the subtree split (fba_solve_mode 1); "
                  "use the replicated solve");
        return FBA_ERR_UNSUPPORTED;
    }
    if (!c->have_factor || !c->have_delta) {
        set_error(std::string(who) + " needs the factor of the last solve (call it once, right after the iterations)");
        return FBA_ERR_ARG;
    }
    const Layout& L = c->L;
    const bool split = c->sched.split;
    const int m = 6 + L.cw;
    double *d_cdiag = nullptr, *d_pdiag = nullptr, *d_iblk = nullptr;
    int32_t *d_islot = nullptr, *d_icam = nullptr;
    std::vector<int32_t> islot(std::max(L.n_img_ref, 1), 0), icam(std::max(L.n_img_ref, 1), 0);
    for (int e = 0; e < L.n_img_ref; ++e) {
        islot[e] = c->img_new[e];
        icam[e] = std::max(c->ref_img_cam[e], 0);
    }
    int rc;  // (all device scratch is the context's workspace, kept for the next call)
    if ((rc = ws_get(*c, WS_CDIAG, (size_t)L.u_c, &d_cdiag)) ||
        (rc = ws_get(*c, WS_PDIAG, 3 * (size_t)std::max(L.n_tie, 1), &d_pdiag)) ||
        (corr && (rc = ws_get(*c, WS_IBLK, (size_t)std::max(L.n_img_ref, 1) * m * m, &d_iblk))) ||
        (rc = ws_get(*c, WS_ISLOT, islot.size(), &d_islot)) || (rc = ws_get(*c, WS_ICAM, icam.size(), &d_icam)))
        return rc;
    if (hipMemcpyAsync(d_islot, islot.data(), sizeof(int32_t) * islot.size(), hipMemcpyHostToDevice, c->stream) != hipSuccess ||
        hipMemcpyAsync(d_icam, icam.data(), sizeof(int32_t) * icam.size(), hipMemcpyHostToDevice, c->stream) != hipSuccess) {
        set_error("hipMemcpyAsync failed");
        return FBA_ERR_HIP;
    }
    if (hipMemsetAsync(d_pdiag, 0, sizeof(double) * 3 * std::max(L.n_tie, 1), c->stream) != hipSuccess) {
        set_error("hipMemsetAsync failed");
        return FBA_ERR_HIP;
    }
    double *d_q = nullptr, *d_red = nullptr, *d_wst = nullptr;
    if (rel && ((rc = ws_get(*c, WS_REL_Q, 2 * (size_t)std::max<int64_t>(c->n_obs, 1), &d_q)) ||
                (rc = ws_get(*c, WS_REL_RED, 2 * (size_t)std::max<int64_t>(c->n_pts, 1), &d_red)) ||
                (rc = ws_get(*c, WS_REL_WST, 2 * (size_t)std::max<int64_t>(c->n_pts, 1), &d_wst))))
        return rc;
    double *d_blk = nullptr, *d_ell = nullptr;
    const size_t nt = (size_t)std::max(L.n_tie, 1);
    if (((cx_tie || ellipsoid) && (rc = ws_get(*c, WS_TIE_BLK, TIE_BLK * nt, &d_blk))) ||
        (ellipsoid && (rc = ws_get(*c, WS_ELLIPSOID, ELL_OUT * nt, &d_ell))))
        return rc;
    if ((rc = launch_postfit(*c, d_cdiag, d_pdiag, d_iblk, d_islot, d_icam, corr ? L.n_img_ref : 0, d_q, d_red, d_wst, sigma02,
                             d_blk, d_ell)))
        return rc;
    if (L.n_tie > 0 && (cx_tie || ellipsoid)) {
        if ((cx_tie && hipMemcpy(cx_tie, d_blk, sizeof(double) * TIE_BLK * (size_t)L.n_tie, hipMemcpyDeviceToHost) != hipSuccess) ||
            (ellipsoid && hipMemcpy(ellipsoid, d_ell, sizeof(double) * ELL_OUT * (size_t)L.n_tie, hipMemcpyDeviceToHost) != hipSuccess)) {
            set_error("HIP error copying the tie points' blocks back");
            return FBA_ERR_HIP;
        }
        // (another rank's points: zeros, so that the ranks' outputs sum; their blocks are zero already)
        if (ellipsoid)
            for (int t = 0; t < L.n_tie; ++t)
                if (!c->full_owned[L.u_c + 3 * (int64_t)t]) std::fill(ellipsoid + ELL_OUT * (size_t)t, ellipsoid + ELL_OUT * (size_t)t + ELL_OUT, 0.0);
    }
    if (rel && c->n_pts > 0) {
        const size_t nb = sizeof(double) * 2 * (size_t)c->n_pts;
        if ((redundancy && hipMemcpy(redundancy, d_red, nb, hipMemcpyDeviceToHost) != hipSuccess) ||
            (wstat && hipMemcpy(wstat, d_wst, nb, hipMemcpyDeviceToHost) != hipSuccess)) {
            set_error("HIP error copying the reliability back");
            return FBA_ERR_HIP;
        }
    }
    std::vector<double> cd(L.u_c), pd(3 * (size_t)L.n_tie), ib(corr ? (size_t)L.n_img_ref * m * m : 0);
    const hipError_t e1 = hipMemcpy(cd.data(), d_cdiag, sizeof(double) * cd.size(), hipMemcpyDeviceToHost);
    const hipError_t e2 = pd.empty() ? hipSuccess : hipMemcpy(pd.data(), d_pdiag, sizeof(double) * pd.size(), hipMemcpyDeviceToHost);
    const hipError_t e3 = ib.empty() ? hipSuccess : hipMemcpy(ib.data(), d_iblk, sizeof(double) * ib.size(), hipMemcpyDeviceToHost);
    if (e1 != hipSuccess || e2 != hipSuccess || e3 != hipSuccess) {
        set_error("HIP error copying the covariance back");
        return FBA_ERR_HIP;
    }
    if (cx_diag) {
        std::fill(cx_diag, cx_diag + L.u_ref, 0.0);
        for (int64_t i = 0; i < L.u_full; ++i) {
            const int64_t r = c->full_to_ref[i];
            // (tie entries: this rank's points; camera-side entries: every rank, or with the subtree split
            // this rank's rows -- its subtrees', and the top's on rank 0 -- so that the ranks' outputs sum)
            if (r < 0 || ((i >= L.u_c || split) && !c->full_owned[i])) continue;
            cx_diag[r] = sigma02 * (i < L.u_c ? cd[i] : pd[i - L.u_c]);  // main.m:602: Cx = sigma02 .* Cx
        }
    }
    if (corr) {
        // the reference's Correlation (main.m:446-456, before the distortion de-scaling) over
        // [the image's estimated EOPs, its camera's estimated IOPs] (main.m:831-840), in xhat order
        const int mu = L.u_img + L.u_cam;
        std::vector<int> sel;
        const int ee[6] = {c->set.est_Xc, c->set.est_Yc, c->set.est_Zc, c->set.est_omega, c->set.est_phi, c->set.est_kappa};
        for (int a = 0; a < 6; ++a)
            if (ee[a]) sel.push_back(a);
        const int64_t cb = 6 * (int64_t)L.n_img;
        for (int q = 0; q < L.cw; ++q)
            if (L.n_cam > 0 && c->full_to_ref[cb + q] >= 0) sel.push_back(6 + q);
        for (int e = 0; e < L.n_img_ref; ++e) {
            const double* b = ib.data() + (size_t)e * m * m;
            double* out = corr + (size_t)e * mu * mu;
            // (subtree split: an image's block on the rank that owns its first row -- its subtree's rank, even
            // when the image straddles into a top block; a wholly-top image on rank 0 -- zeros elsewhere)
            if (split && !c->full_owned[6 * (int64_t)c->img_new[e]]) {
                std::fill(out, out + (size_t)mu * mu, 0.0);
                continue;
            }
            for (int a = 0; a < (int)sel.size(); ++a)
                for (int q = 0; q < (int)sel.size(); ++q) {
                    const int ra = sel[a], rq = sel[q];
                    out[a * mu + q] = c->ref_img_cam[e] < 0
                                          ? 0.0
                                          : b[ra * m + rq] / (std::sqrt(b[ra * m + ra]) * std::sqrt(b[rq * m + rq]));
                }
        }
    }
    return FBA_OK;
}

extern "C" {

int fba_covariance(fba_ctx* ctx, double sigma02, double* cx_diag, double* corr) {
    return covariance_impl(reinterpret_cast<Ctx*>(ctx), "fba_covariance", sigma02, cx_diag, corr, false, nullptr, nullptr);
}

int fba_reliability(fba_ctx* ctx, double sigma02, double* cx_diag, double* corr, double* redundancy, double* wstat) {
    return covariance_impl(reinterpret_cast<Ctx*>(ctx), "fba_reliability", sigma02, cx_diag, corr, true, redundancy, wstat);
}

int fba_postfit_outputs(fba_ctx* ctx, double sigma02, const fba_postfit* out) {
    if (!out) { set_error("fba_postfit_outputs: NULL output structure"); return FBA_ERR_ARG; }
    return covariance_impl(reinterpret_cast<Ctx*>(ctx), "fba_postfit_outputs", sigma02, out->cx_diag, out->corr,
                           out->redundancy || out->wstat, out->redundancy, out->wstat, out->cx_tie, out->ellipsoid);
}

}  // extern "C"
