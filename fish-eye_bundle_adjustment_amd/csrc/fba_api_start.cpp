// fba_api_start.cpp -- the C API of the starting values: the image rays, the forward intersection of the tie points
// and the space resection of the images (include/fba.h; no reference counterpart; kernels in fba_intersect.hip and
// fba_resect.hip, the per-image routines in fba_resect.h).
#include <algorithm>
#include <cmath>
#include <vector>

#include "fba_api.h"

namespace fba {

// the rays of this rank's observations at d_xfull into workspace (local order): ray [RAY_REC n_obs], rst [n_obs], xu [2 n_obs]
static int rays_to_ws(Ctx* c, double** d_ray, int32_t** d_rst, double** d_xu) {
    const size_t n = (size_t)std::max<int64_t>(c->n_obs, 1);
    int rc;
    if ((rc = ws_get(*c, WS_RAY, RAY_REC * n, d_ray)) || (rc = ws_get(*c, WS_RAY_ST, n, d_rst)) ||
        (rc = ws_get(*c, WS_RAY_XU, 2 * n, d_xu)))
        return rc;
    // the image / camera tables at d_xfull: functions of xhat alone, so between fba_accumulate and fba_solve_update
    // they are rewritten with the values they hold (launch_cost's argument)
    if ((rc = launch_params(*c)) || (rc = launch_rays(*c, *d_ray, *d_rst, *d_xu))) return rc;
    return FBA_OK;
}

// the image list on first use: d_img downloaded once, sorted on the host (build_image_list), kept by the context
int image_list_once(Ctx* c) {
    if (c->have_img_list) return FBA_OK;
    std::vector<int32_t> img((size_t)c->n_obs), start, list;
    if (c->n_obs > 0) FBA_HIP(hipMemcpy(img.data(), c->d_img, sizeof(int32_t) * img.size(), hipMemcpyDeviceToHost));
    build_image_list(img, c->L.n_img, start, list);
    if ((int64_t)list.size() != c->n_obs) { set_error("fba_resect: an observation's image slot is out of range"); return FBA_ERR_ARG; }
    int rc;
    if ((rc = upload(*c, &c->d_il_start, start)) || (rc = upload(*c, &c->d_il_obs, list)) ||
        (rc = upload(*c, &c->d_il_ext, c->img_ord)))
        return rc;
    c->have_img_list = true;
    return FBA_OK;
}

}  // namespace fba

using namespace fba;

extern "C" {

int fba_image_rays(fba_ctx* ctx, double* ray, int32_t* status) {
    int rc;
    Ctx* c = enter(ctx, "fba_image_rays", REQ_IDLE, rc);
    if (!c) return rc;
    double *d_ray = nullptr, *d_xu = nullptr;
    int32_t* d_rst = nullptr;
    if ((rc = rays_to_ws(c, &d_ray, &d_rst, &d_xu))) return rc;
    const int64_t n = c->n_obs;
    std::vector<double> hr(RAY_REC * (size_t)n);
    std::vector<int32_t> hs((size_t)n);
    if (n > 0) {
        FBA_HIP(hipMemcpyAsync(hr.data(), d_ray, sizeof(double) * hr.size(), hipMemcpyDeviceToHost, c->stream));
        FBA_HIP(hipMemcpyAsync(hs.data(), d_rst, sizeof(int32_t) * hs.size(), hipMemcpyDeviceToHost, c->stream));
    }
    FBA_HIP(hipStreamSynchronize(c->stream));
    if (ray) std::fill(ray, ray + RAY_REC * c->n_pts, 0.0);
    if (status) std::fill(status, status + c->n_pts, 0);
    for (int64_t o = 0; o < n; ++o) {  // local order -> PHO order; another rank's rows stay 0
        const int64_t i = c->obs_pho[o];
        if (ray) std::copy(hr.begin() + RAY_REC * o, hr.begin() + RAY_REC * o + RAY_REC, ray + RAY_REC * i);
        if (status) status[i] = hs[o];
    }
    return FBA_OK;
}

int fba_intersect(fba_ctx* ctx, const fba_intersect_options* o, double* xyz, double* quality, int32_t* status,
                  int64_t* n_not_ok) {
    int rc;
    Ctx* c = enter(ctx, "fba_intersect", REQ_IDLE, rc);
    if (!c) return rc;
    const fba_intersect_options& op = o ? *o : kIntersectDefaults;
    if (op.refine_iters < 0 || !std::isfinite(op.min_ratio) || op.min_ratio < 0.0 || !std::isfinite(op.refine_tol) ||
        op.refine_tol < 0.0) {
        set_error("fba_intersect: refine_iters >= 0, min_ratio and refine_tol finite and >= 0");
        return FBA_ERR_ARG;
    }
    const size_t nt = (size_t)std::max<int32_t>(c->L.n_tie, 1);
    double *d_ray = nullptr, *d_xu = nullptr, *d_out = nullptr;
    int32_t *d_rst = nullptr, *d_st = nullptr;
    if ((rc = ws_get(*c, WS_ISECT_OUT, 7 * nt, &d_out)) || (rc = ws_get(*c, WS_ISECT_ST, nt, &d_st)))
        return rc;
    // another rank's tie points stay 0 (the ranks' outputs sum to the whole)
    FBA_HIP(hipMemsetAsync(d_out, 0, sizeof(double) * 7 * nt, c->stream));
    FBA_HIP(hipMemsetAsync(d_st, 0, sizeof(int32_t) * nt, c->stream));
    CallTimer timer;
    if ((rc = timer.init(c, "fba_intersect"))) return rc;
    timer.start(c->stream);
    if ((rc = rays_to_ws(c, &d_ray, &d_rst, &d_xu)) ||
        (rc = launch_intersect(*c, d_ray, d_rst, d_xu, op.refine_iters, op.min_ratio, op.refine_tol, op.write_xhat != 0, d_out,
                               d_out + 3 * nt, d_st)))
        return rc;
    timer.stop(c->stream);
    if (op.write_xhat) c->xhat_changed();  // as fba_set_xhat
    const int64_t n_tie = c->L.n_tie;
    std::vector<int32_t> hs;
    if (n_tie > 0) {
        if (xyz) FBA_HIP(hipMemcpyAsync(xyz, d_out, sizeof(double) * 3 * n_tie, hipMemcpyDeviceToHost, c->stream));
        if (quality) FBA_HIP(hipMemcpyAsync(quality, d_out + 3 * nt, sizeof(double) * 4 * n_tie, hipMemcpyDeviceToHost, c->stream));
        if (status || n_not_ok) {
            hs.resize((size_t)n_tie);
            FBA_HIP(hipMemcpyAsync(hs.data(), d_st, sizeof(int32_t) * n_tie, hipMemcpyDeviceToHost, c->stream));
        }
    }
    FBA_HIP(hipStreamSynchronize(c->stream));
    if (status) std::copy(hs.begin(), hs.end(), status);
    if (n_not_ok) *n_not_ok = (int64_t)std::count_if(hs.begin(), hs.end(), [](int32_t s) { return s != FBA_ISECT_OK; });
    if ((rc = timer.lap())) return rc;
    timer.publish(c);
    return FBA_OK;
}

int fba_resect(fba_ctx* ctx, const fba_resect_options* o, double* eop, double* quality, int32_t* status, int64_t* n_not_ok) {
    int rc;
    Ctx* c = enter(ctx, "fba_resect", REQ_IDLE, rc);
    if (!c) return rc;
    const fba_resect_options& op = o ? *o : kResectDefaults;
    if ((rc = check_resect_options("fba_resect", op)) ||
        (rc = require(c, "fba_resect", REQ_SINGLE_GPU, ": an image's observations are spread over the ranks")))
        return rc;
    const fba_settings& s = c->set;
    if (op.write_xhat && !(s.est_Xc && s.est_Yc && s.est_Zc && s.est_omega && s.est_phi && s.est_kappa)) {
        set_error("fba_resect: write_xhat with a fixed exterior orientation (an Estimate_Xc .. Estimate_Kappa flag is off)");
        return FBA_ERR_UNSUPPORTED;
    }
    if ((int)c->img_ord.size() != c->L.n_img) { set_error("fba_resect: image order and layout disagree"); return FBA_ERR_ARG; }
    if ((rc = image_list_once(c))) return rc;
    const int64_t ni = c->L.n_img_ref;
    const size_t no = (size_t)std::max<int64_t>(c->n_obs, 1), nio = (size_t)std::max<int64_t>(ni, 1);
    double *d_rec = nullptr, *d_out = nullptr;
    int32_t *d_use = nullptr, *d_st = nullptr;
    if ((rc = ws_get(*c, WS_RESECT_REC, RESECT_REC * no, &d_rec)) || (rc = ws_get(*c, WS_RESECT_USE, no, &d_use)) ||
        (rc = ws_get(*c, WS_RESECT_OUT, 11 * nio, &d_out)) || (rc = ws_get(*c, WS_RESECT_ST, nio, &d_st)))
        return rc;
    CallTimer timer;
    if ((rc = timer.init(c, "fba_resect"))) return rc;
    timer.start(c->stream);
    // the camera table at d_xfull: a function of xhat alone, so between fba_accumulate and fba_solve_update it is
    // rewritten with the values it holds (fba_intersect's argument)
    if ((rc = launch_params(*c)) || (rc = launch_resect_gather(*c, op.use == FBA_RESECT_USE_ALL, d_rec, d_use)) ||
        (rc = launch_resect(*c, d_rec, d_use, op.refine_iters, op.min_ratio, op.refine_tol, op.write_xhat != 0, d_out,
                            d_out + 6 * nio, d_st)))
        return rc;
    timer.stop(c->stream);
    if (op.write_xhat) c->xhat_changed();  // as fba_set_xhat
    std::vector<int32_t> hs;
    if (ni > 0) {
        if (eop) FBA_HIP(hipMemcpyAsync(eop, d_out, sizeof(double) * 6 * ni, hipMemcpyDeviceToHost, c->stream));
        if (quality) FBA_HIP(hipMemcpyAsync(quality, d_out + 6 * nio, sizeof(double) * 5 * ni, hipMemcpyDeviceToHost, c->stream));
        if (status || n_not_ok) {
            hs.resize((size_t)ni);
            FBA_HIP(hipMemcpyAsync(hs.data(), d_st, sizeof(int32_t) * ni, hipMemcpyDeviceToHost, c->stream));
        }
    }
    FBA_HIP(hipStreamSynchronize(c->stream));
    if (status) std::copy(hs.begin(), hs.end(), status);
    if (n_not_ok) *n_not_ok = (int64_t)std::count_if(hs.begin(), hs.end(), [](int32_t v) { return v != FBA_RESECT_OK; });
    if ((rc = timer.lap())) return rc;
    timer.publish(c);
    return FBA_OK;
}

}  // extern "C"
