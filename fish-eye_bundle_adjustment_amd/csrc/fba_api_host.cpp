// fba_api_host.cpp -- the part of the C API (include/fba.h) that touches no device: the error text, the entry checks,
// the option defaults and their checks, and every entry point that runs on the host alone.
//
// No HIP call: with fba_plan.cpp and fba_order.cpp it links into a stand-alone host program (tests/*_check.cpp).
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <string>
#include <vector>

#include "fba_api.h"
#include "fba_eig3.h"
#include "fba_ray.h"
#include "fba_resect.h"
#include "fba_vce.h"
#include "fba_snoop.h"

namespace fba {

static thread_local std::string g_err;
void set_error(const std::string& msg) { g_err = msg; }

int require(const Ctx* c, const char* who, unsigned req, const char* tail) {
    const std::string w(who);
    if ((req & REQ_IDLE) && c->pending) {
        set_error(w + " between fba_solve_update_async and fba_solve_finish");
        return FBA_ERR_ARG;
    }
    if ((req & REQ_SINGLE_GPU) && c->opt.world != 1) {
        set_error(w + " is single-GPU (world == 1)" + ((req & REQ_NO_LOSS) ? "" : tail));
        return FBA_ERR_UNSUPPORTED;
    }
    if ((req & REQ_NO_LOSS) && c->loss != FBA_LOSS_NONE) {
        set_error(w + " with a robust loss set: " + tail);
        return FBA_ERR_UNSUPPORTED;
    }
    if ((req & REQ_NO_DAMPING) && c->damp_on()) {
        set_error(w + " with damping > 0: the factor of a damped solve is not that of N");
        return FBA_ERR_UNSUPPORTED;
    }
    return FBA_OK;
}

Ctx* enter(fba_ctx* ctx, const char* who, unsigned req, int& rc, const char* tail) {
    Ctx* c = reinterpret_cast<Ctx*>(ctx);
    if (!c) {
        set_error(std::string(who) + ": NULL context");
        rc = FBA_ERR_ARG;
        return nullptr;
    }
    return (rc = require(c, who, req, tail)) ? nullptr : c;
}

const fba_lm_options kLmDefaults{1e-3, 10.0, 10.0, 1e-12, 1e8, 1e-9};
const fba_intersect_options kIntersectDefaults{10, 0, 0.5 * (1.0 - std::cos(std::acos(-1.0) / 180.0)), 1e-10};
const fba_resect_options kResectDefaults{FBA_RESECT_USE_CONTROL, 10, 0, 0, 1e-6, 1e-10};
const fba_vce_options kVceDefaults{10, 0, 1e-3, 1.0, 100.0};
const fba_snoop_options kSnoopDefaults{20, 2, 6, 0, 3.29, 0.05};

int check_resect_options(const char* who, const fba_resect_options& op) {
    if ((op.use != FBA_RESECT_USE_CONTROL && op.use != FBA_RESECT_USE_ALL) || op.refine_iters < 0 ||
        !std::isfinite(op.min_ratio) || op.min_ratio < 0.0 || !std::isfinite(op.refine_tol) || op.refine_tol < 0.0) {
        set_error(std::string(who) + ": use CONTROL or ALL, refine_iters >= 0, min_ratio and refine_tol finite and >= 0");
        return FBA_ERR_ARG;
    }
    return FBA_OK;
}

int check_vce_args(const char* who, int64_t n_rows, int32_t n_groups, const int32_t* group, const fba_vce_options& op) {
    char buf[200];
    if (n_groups < 1 || n_groups > FBA_VCE_MAX_GROUPS) {
        snprintf(buf, sizeof buf, "%s: n_groups = %d outside [1, %d]", who, (int)n_groups, FBA_VCE_MAX_GROUPS);
        set_error(buf);
        return FBA_ERR_ARG;
    }
    if (op.max_rounds < 1 || !std::isfinite(op.tol) || op.tol < 0.0 || !std::isfinite(op.min_redundancy) ||
        op.min_redundancy < 0.0 || !std::isfinite(op.clip) || op.clip < 1.0) {
        set_error(std::string(who) + ": max_rounds >= 1; tol >= 0, min_redundancy >= 0 and clip >= 1, all finite");
        return FBA_ERR_ARG;
    }
    if (n_rows < 0 || (n_rows > 0 && !group)) { set_error(std::string(who) + ": NULL group array"); return FBA_ERR_ARG; }
    for (int64_t i = 0; i < n_rows; ++i)
        if (group[i] < -1 || group[i] >= n_groups) {
            snprintf(buf, sizeof buf, "%s: group[%ld] = %d outside [-1, %d)", who, (long)i, (int)group[i], (int)n_groups);
            set_error(buf);
            return FBA_ERR_ARG;
        }
    return FBA_OK;
}

int check_snoop_options(const char* who, const fba_snoop_options& op) {
    if (op.max_rounds < 1 || op.min_rays < 1 || op.min_img_points < 1 || !std::isfinite(op.crit) || !(op.crit > 0.0) ||
        !std::isfinite(op.max_share) || !(op.max_share > 0.0) || op.max_share > 1.0) {
        set_error(std::string(who) + ": max_rounds, min_rays and min_img_points >= 1; crit > 0 and 0 < max_share <= 1, both finite");
        return FBA_ERR_ARG;
    }
    return FBA_OK;
}

}  // namespace fba

using namespace fba;

extern "C" {

const char* fba_last_error(void) { return g_err.c_str(); }
int fba_abi_version(void) { return FBA_ABI_VERSION; }

int fba_count_unknowns(const fba_problem* p, const fba_settings* s, int64_t* u_out) {
    if (!p || !s || !u_out) { set_error("NULL argument"); return FBA_ERR_ARG; }
    *u_out = count_unknowns(p, s);
    return FBA_OK;
}

int fba_partition(const fba_problem* p, int32_t world, int32_t* tie_owner, int32_t* ctl_owner) {
    if (!p || world < 1) { set_error("bad argument"); return FBA_ERR_ARG; }
    std::vector<int32_t> t, q;
    partition(p, world, t, q);
    if (tie_owner) std::copy(t.begin(), t.end(), tie_owner);
    if (ctl_owner) std::copy(q.begin(), q.end(), ctl_owner);
    return FBA_OK;
}

int fba_image_order(const fba_problem* p, int32_t* order, int32_t* n_slots) {
    if (!p || !n_slots) { set_error("NULL argument"); return FBA_ERR_ARG; }
    std::vector<int32_t> ord;
    const int rc = image_order(p, ord);
    if (rc) return rc;
    *n_slots = (int32_t)ord.size();
    if (order) std::copy(ord.begin(), ord.end(), order);
    return FBA_OK;
}

int fba_finish_stats(const fba_problem* p, const fba_settings* s, const double* sums, double vtpv, double* stats) {
    if (!p || !s || !sums || !stats) { set_error("NULL argument"); return FBA_ERR_ARG; }
    int64_t u = 0;
    fba_count_unknowns(p, s, &u);
    const double n = (double)p->n_pts;
    const double rx = std::sqrt(sums[0] / n), ry = std::sqrt(sums[1] / n);
    const double nu = (double)(2 * p->n_pts - u);
    stats[0] = rx; stats[1] = ry; stats[2] = std::sqrt(rx * rx + ry * ry);
    stats[3] = vtpv / nu; stats[4] = vtpv; stats[5] = nu;
    return FBA_OK;
}

int fba_eig3_host(int64_t n, const double* blk, double* ell) {
    if (n < 0 || (n > 0 && (!blk || !ell))) { set_error("fba_eig3_host: NULL argument"); return FBA_ERR_ARG; }
    for (int64_t i = 0; i < n; ++i) eig3_block(blk + TIE_BLK * i, ell + ELL_OUT * i);
    return FBA_OK;
}

// ---- forward intersection: the inverse projection model of fba_ray.h ----
int fba_unproject_host(int32_t type, int32_t nk, int64_t n, const double* xy, const double* camtab, double* out,
                       int32_t* status) {
    if (type < FBA_TYPE_FISHEYE || type > FBA_TYPE_STEREOGRAPHIC) { set_error("fba_unproject_host: invalid type"); return FBA_ERR_TYPE; }
    if (nk < 1 || nk > FBA_NK_MAX || n < 0 || !camtab || (n > 0 && !xy)) {
        set_error("fba_unproject_host: nk in 1..FBA_NK_MAX, n >= 0, xy and camtab not NULL");
        return FBA_ERR_ARG;
    }
    for (int64_t i = 0; i < n; ++i) {
        double v[5];
        const int st = ray_unproject<0>(xy[2 * i], xy[2 * i + 1], camtab[0], camtab[1], camtab[2], camtab[3], camtab[4],
                                        camtab[5], camtab + 6, nk, type, v[0], v[1], v[2], v[3], v[4]);
        if (out) std::copy(v, v + 5, out + 5 * i);
        if (status) status[i] = st;
    }
    return FBA_OK;
}

// ---- space resection: the per-image routines of fba_resect.h ----
int fba_resect_host(int32_t type, int64_t n, const double* xyz, const double* ray, const int32_t* ray_status, double cc,
                    double ydir, double std_x, double std_y, const fba_resect_options* o, double* eop, double* quality,
                    int32_t* status) {
    if (type < FBA_TYPE_FISHEYE || type > FBA_TYPE_STEREOGRAPHIC) { set_error("fba_resect_host: invalid type"); return FBA_ERR_TYPE; }
    if (n < 0 || (n > 0 && (!xyz || !ray)) || !(std_x > 0.0) || !(std_y > 0.0)) {
        set_error("fba_resect_host: n >= 0, xyz and ray not NULL, the standard deviations > 0");
        return FBA_ERR_ARG;
    }
    const fba_resect_options& op = o ? *o : kResectDefaults;
    int rc;
    if ((rc = check_resect_options("fba_resect_host", op))) return rc;
    std::vector<double> rec(RESECT_REC * (size_t)n);
    std::vector<int32_t> use((size_t)n);
    for (int64_t i = 0; i < n; ++i) {
        std::copy(ray + 5 * i, ray + 5 * i + 5, rec.begin() + RESECT_REC * i);
        std::copy(xyz + 3 * i, xyz + 3 * i + 3, rec.begin() + RESECT_REC * i + 5);
        use[(size_t)i] = (!ray_status || ray_status[i] == FBA_RAY_OK) ? 1 : 0;
    }
    const ResectHostSrc src{rec.data(), use.data(), n, cc, ydir};
    double A[144], V[144], e[6], q[5];
    const double zero[6] = {0, 0, 0, 0, 0, 0};
    int st;
    resect_solve(src, type, 1.0 / (std_x * std_x), 1.0 / (std_y * std_y), op.refine_iters, op.min_ratio, op.refine_tol, A, V,
                 zero, e, q, st);
    if (eop) std::copy(e, e + 6, eop);
    if (quality) std::copy(q, q + 5, quality);
    if (status) *status = st;
    return FBA_OK;
}

// ---- variance component estimation: the group arithmetic of fba_vce.h ----
int fba_vce_host(int64_t n_rows, int32_t n_groups, const int32_t* group, const double* r, const double* t,
                 const fba_vce_options* o, double* sums, double* sigma2, double* factor, int32_t* status) {
    const fba_vce_options& op = o ? *o : kVceDefaults;
    int rc;
    if ((rc = check_vce_args("fba_vce_host", n_rows, n_groups, group, op))) return rc;
    if (n_rows > 0 && (!r || !t)) { set_error("fba_vce_host: NULL r or t"); return FBA_ERR_ARG; }
    std::vector<double> s((size_t)(n_groups + 1) * VCE_SUMS, 0.0);
    vce_sum_rows(n_rows, n_groups, group, r, t, s.data());
    if (sums) std::copy(s.begin(), s.end(), sums);
    bool finite = true;
    for (int g = 0; g <= n_groups; ++g) {
        finite = finite && std::isfinite(s[(size_t)VCE_SUMS * g]) && std::isfinite(s[(size_t)VCE_SUMS * g + 1]);
        if (g == n_groups) break;
        double e, f;
        int st;
        vce_group(s[(size_t)VCE_SUMS * g], s[(size_t)VCE_SUMS * g + 1], s[(size_t)VCE_SUMS * g + 2], op.min_redundancy, op.clip, e, f, st);
        if (sigma2) sigma2[g] = e;
        if (factor) factor[g] = f;
        if (status) status[g] = st;
    }
    if (!finite) { set_error("fba_vce_host: a non-finite group sum"); return FBA_ERR_NONFINITE; }
    return FBA_OK;
}

// ---- Baarda data snooping: one round's selection of fba_snoop.h ----
int fba_snoop_host(int64_t n, const double* W, const uint8_t* state, const int32_t* tie, const int32_t* img, int32_t n_tie,
                   int32_t n_img, const fba_snoop_options* o, uint8_t* pick, uint8_t* readmit, int32_t* status_bits) {
    const fba_snoop_options& op = o ? *o : kSnoopDefaults;
    int rc;
    if ((rc = check_snoop_options("fba_snoop_host", op))) return rc;
    if (n < 0 || n_tie < 0 || n_img < 0 || (n > 0 && (!W || !state || !tie || !img || !pick || !readmit))) {
        set_error("fba_snoop_host: n, n_tie, n_img >= 0 and no NULL array");
        return FBA_ERR_ARG;
    }
    int64_t n_excl = 0;
    for (int64_t i = 0; i < n; ++i) {
        if (tie[i] >= n_tie || img[i] < 0 || img[i] >= n_img || state[i] > SNOOP_READMITTED) {
            char buf[160];
            snprintf(buf, sizeof buf, "fba_snoop_host: point %ld: tie %d (< %d), img %d (in [0, %d)), state %d (0, 1 or 2)", (long)i,
                     (int)tie[i], (int)n_tie, (int)img[i], (int)n_img, (int)state[i]);
            set_error(buf);
            return FBA_ERR_ARG;
        }
        n_excl += state[i] == SNOOP_EXCLUDED;
    }
    int64_t n_pick = 0, n_back = 0;
    snoop_select(n, W, state, tie, img, nullptr, n_tie, n_img, op.min_rays, op.min_img_points, op.crit, pick, readmit, n_pick, n_back);
    int bits = 0;
    if (n_pick > 0 && snoop_share_stop(n_excl, n_pick, n, op.max_share)) {
        bits |= 2;
        std::fill(pick, pick + n, (uint8_t)0);
    }
    if (status_bits) *status_bits = bits;
    return FBA_OK;
}

}  // extern "C"
