// fba_api_rounds.cpp -- the C API of the loops of adjustment rounds: variance component estimation over observation
// groups (fba_vce) and Baarda data snooping over the image points (fba_snoop) (include/fba.h; no reference
// counterpart; kernels in fba_vce.hip and fba_snoop.hip).  Both re-weight on the device between two adjustments.
#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

#include "fba_api.h"
#include "fba_vce.h"
#include "fba_snoop.h"

namespace fba {

int solve_round(fba_ctx* ctx, const char* who, int& n_iter) {
    const Ctx* c = reinterpret_cast<const Ctx*>(ctx);
    int32_t it = 0;
    const int rc = fba_adjust(ctx, &it, nullptr);
    n_iter += it;
    if (rc) return rc;
    if (!c->have_factor || !c->have_delta) { set_error(std::string(who) + ": the last solve left no factor"); return FBA_ERR_ARG; }
    return FBA_OK;
}

// the point list on first use: d_pt downloaded once, sorted on the host (build_point_list), kept by the context
static int point_list_once(Ctx* c) {
    if (c->have_pt_list) return FBA_OK;
    std::vector<int32_t> pt((size_t)c->n_obs), start, list;
    if (c->n_obs > 0) FBA_HIP(hipMemcpy(pt.data(), c->d_pt, sizeof(int32_t) * pt.size(), hipMemcpyDeviceToHost));
    const int64_t n_pl = c->n_lp + c->gen.n_gp;  // d_pt counts the general points after the regular ones
    for (int32_t p : pt)
        if (p >= n_pl) { set_error("fba_snoop: an observation's local point is out of range"); return FBA_ERR_ARG; }
    build_point_list(pt, (int)n_pl, start, list);
    int rc;
    if ((rc = upload(*c, &c->d_pl_start, start)) || (rc = upload(*c, &c->d_pl_obs, list))) return rc;
    c->n_pl = n_pl;
    c->have_pt_list = true;
    return FBA_OK;
}

}  // namespace fba

using namespace fba;

extern "C" {

// ---- variance component estimation over observation groups ----
int fba_vce(fba_ctx* ctx, int32_t n_groups, const int32_t* group, const fba_vce_options* o, double* component, double* table,
            int32_t* status, int32_t* rounds, int32_t* iterations, int32_t* converged) {
    int rc;
    Ctx* c = enter(ctx, "fba_vce", REQ_IDLE, rc);
    if (!c) return rc;
    const fba_vce_options& op = o ? *o : kVceDefaults;
    if ((rc = check_vce_args("fba_vce", 2 * c->n_pts, n_groups, group, op)) ||
        (rc = require(c, "fba_vce", REQ_SINGLE_GPU | REQ_NO_LOSS | REQ_NO_DAMPING,
                      "its IRLS factor and a variance component would fight over the same residuals")))
        return rc;

    const Layout& L = c->L;
    const int ng = n_groups, ng1 = ng + 1, ng2 = ng + 2;
    const int64_t n_blocks = (c->n_obs + 255) / 256;
    // the group ids in local order, once per call
    std::vector<int32_t> gl(2 * (size_t)std::max<int64_t>(c->n_obs, 1), -1);
    for (int64_t i = 0; i < c->n_obs; ++i) {
        gl[2 * i] = group[2 * c->obs_pho[i]];
        gl[2 * i + 1] = group[2 * c->obs_pho[i] + 1];
    }
    int32_t* d_grp = nullptr;
    double *d_slab = nullptr, *d_out = nullptr, *d_q = nullptr, *d_cdiag = nullptr, *d_pdiag = nullptr;
    if ((rc = ws_get(*c, WS_VCE_GROUP, gl.size(), &d_grp)) ||
        (rc = ws_get(*c, WS_VCE_SLAB, (size_t)std::max<int64_t>(n_blocks, 1) * ng1 * VCE_SUMS, &d_slab)) ||
        (rc = ws_get(*c, WS_VCE_OUT, (size_t)ng1 * VCE_OUT, &d_out)) ||
        (rc = ws_get(*c, WS_REL_Q, 2 * (size_t)std::max<int64_t>(c->n_obs, 1), &d_q)))
        return rc;
    std::vector<int64_t> pr_idx;
    std::vector<double> pr_val, cd, pd;
    if (c->n_prior > 0) {  // (world == 1: this rank adds every prior)
        if ((rc = ws_get(*c, WS_CDIAG, (size_t)L.u_c, &d_cdiag)) || (rc = ws_get(*c, WS_PDIAG, 3 * (size_t)std::max(L.n_tie, 1), &d_pdiag)))
            return rc;
        pr_idx.resize(2 * (size_t)c->n_pres);
        pr_val.resize(2 * (size_t)c->n_pres);
        cd.resize((size_t)L.u_c);
        pd.resize(3 * (size_t)L.n_tie);
        if (c->n_pres > 0) {
            FBA_HIP(hipMemcpy(pr_idx.data(), c->d_pr_idx, sizeof(int64_t) * pr_idx.size(), hipMemcpyDeviceToHost));
            FBA_HIP(hipMemcpy(pr_val.data(), c->d_pr_val, sizeof(double) * pr_val.size(), hipMemcpyDeviceToHost));
        }
    }
    FBA_HIP(hipMemcpyAsync(d_grp, gl.data(), sizeof(int32_t) * gl.size(), hipMemcpyHostToDevice, c->stream));
    FBA_HIP(hipStreamSynchronize(c->stream));  // (gl is pageable memory of this call)

    CallTimer timer;
    if ((rc = timer.init(c, "fba_vce"))) return rc;
    std::vector<double> comp((size_t)ng2, 1.0), out((size_t)ng1 * VCE_OUT);
    std::vector<int32_t> st((size_t)ng2, FBA_VCE_EMPTY);
    int n_rounds = 0, n_iter = 0, conv = 0;
    auto publish = [&]() {
        if (component) std::copy(comp.begin(), comp.end(), component);
        if (status) std::copy(st.begin(), st.end(), status);
        if (rounds) *rounds = n_rounds;
        if (iterations) *iterations = n_iter;
        if (converged) *converged = conv;
        timer.publish(c);
    };
    for (int k = 0; k < op.max_rounds; ++k) {
        if ((rc = solve_round(ctx, "fba_vce", n_iter))) { publish(); return rc; }
        timer.start(c->stream);
        if ((rc = launch_vce_q(*c, d_cdiag, d_pdiag, d_q)) ||
            (rc = launch_vce_sums(*c, d_q, d_grp, ng, op.min_redundancy, op.clip, d_slab, d_out))) {
            publish();
            return rc;
        }
        timer.stop(c->stream);
        FBA_HIP(hipMemcpyAsync(out.data(), d_out, sizeof(double) * out.size(), hipMemcpyDeviceToHost, c->stream));
        if (c->n_prior > 0) {
            FBA_HIP(hipMemcpyAsync(cd.data(), d_cdiag, sizeof(double) * cd.size(), hipMemcpyDeviceToHost, c->stream));
            if (!pd.empty()) FBA_HIP(hipMemcpyAsync(pd.data(), d_pdiag, sizeof(double) * pd.size(), hipMemcpyDeviceToHost, c->stream));
        }
        FBA_HIP(hipStreamSynchronize(c->stream));
        if ((rc = timer.lap())) return rc;
        n_rounds = k + 1;
        // the round's rows: the groups and the rows of no group from the device, the priors on the host
        double* trow = table ? table + (size_t)k * ng2 * 4 : nullptr;
        bool finite = true, clipped = false, within = true;
        for (int g = 0; g < ng1; ++g) {
            const double* r = out.data() + (size_t)VCE_OUT * g;
            st[g] = (int32_t)r[5];
            if (trow) { trow[4 * g] = r[0]; trow[4 * g + 1] = r[1]; trow[4 * g + 2] = r[2]; trow[4 * g + 3] = r[3]; }
            finite = finite && std::isfinite(r[0]) && std::isfinite(r[1]);
            if (g < ng) {
                clipped = clipped || st[g] == FBA_VCE_CLIPPED;
                if (st[g] == FBA_VCE_OK && !(std::fabs(r[3] - 1.0) <= op.tol)) within = false;
            }
        }
        double pR = 0.0, pT = 0.0;
        if (c->n_prior > 0) {
            for (int64_t j = 0; j < c->n_pres; ++j) {
                const int64_t i = pr_idx[2 * j];
                pR += 1.0 - pr_val[2 * j] * (i < L.u_c ? cd[(size_t)i] : pd[(size_t)(i - L.u_c)]);
            }
            if ((rc = fba_get_priors(ctx, nullptr, nullptr, &pT))) { publish(); return rc; }
            finite = finite && std::isfinite(pR) && std::isfinite(pT);
        }
        st[ng1] = c->n_prior > 0 ? FBA_VCE_OK : FBA_VCE_EMPTY;
        if (trow) {
            trow[4 * ng1] = pR; trow[4 * ng1 + 1] = pT; trow[4 * ng1 + 2] = (double)c->n_prior;
            trow[4 * ng1 + 3] = (c->n_prior > 0 && pR > 0.0) ? pT / pR : 1.0;
        }
        if (!finite) {
            publish();
            set_error("fba_vce: a non-finite group sum in round " + std::to_string(k + 1));
            return FBA_ERR_NONFINITE;
        }
        conv = (within && !clipped) ? 1 : 0;
        if (conv || k == op.max_rounds - 1) break;
        // re-weight: the first rescale of an unweighted context switches the weighted kernels on
        const bool first = !c->weights_on;
        if ((rc = reweight_begin(c)) || (rc = launch_vce_rescale(*c, d_grp, d_out, ng, first)) || (rc = reweight_end(c))) {
            publish();
            return rc;
        }
        for (int g = 0; g < ng; ++g) comp[g] *= out[(size_t)VCE_OUT * g + 3];
    }
    // one plain step: the context as the loop leaves one with these weights (lin, delta, factor)
    double dsum = 0.0;
    rc = fba_step(ctx, &dsum);
    ++n_iter;
    publish();
    return rc;
}

// ---- Baarda data snooping over the image points ----
int fba_snoop(fba_ctx* ctx, const fba_snoop_options* o, uint8_t* excluded, double* stat, double* table, int32_t* rounds,
              int32_t* iterations, int32_t* converged, int32_t* status_bits) {
    int rc;
    Ctx* c = enter(ctx, "fba_snoop", REQ_IDLE, rc);
    if (!c) return rc;
    const fba_snoop_options& op = o ? *o : kSnoopDefaults;
    if ((rc = check_snoop_options("fba_snoop", op)) ||
        (rc = require(c, "fba_snoop", REQ_SINGLE_GPU | REQ_NO_LOSS | REQ_NO_DAMPING,
                      "the w-test wants the residuals of a plain L2 adjustment")))
        return rc;
    if ((int)c->img_ord.size() != c->L.n_img) { set_error("fba_snoop: image order and layout disagree"); return FBA_ERR_ARG; }
    if ((rc = image_list_once(c)) || (rc = point_list_once(c))) return rc;

    const int64_t n = c->n_obs;
    const size_t no = (size_t)std::max<int64_t>(n, 1), nseg = (size_t)std::max<int64_t>(c->n_pl + c->L.n_img, 1);
    const int64_t n_blocks = (n + 255) / 256;
    SnoopBufs b;
    double* d_q = nullptr;
    if ((rc = ws_get(*c, WS_SNOOP_S0, 2 * no, &b.s0)) || (rc = ws_get(*c, WS_SNOOP_W, no, &b.W)) ||
        (rc = ws_get(*c, WS_SNOOP_STATE, no, &b.state)) || (rc = ws_get(*c, WS_SNOOP_CAND, no, &b.cand)) ||
        (rc = ws_get(*c, WS_SNOOP_BACK, no, &b.back)) || (rc = ws_get(*c, WS_SNOOP_WIN, nseg, &b.win)) ||
        (rc = ws_get(*c, WS_SNOOP_CNT, nseg, &b.cnt)) || (rc = ws_get(*c, WS_SNOOP_PICK, (size_t)std::max(c->L.n_img, 1), &b.pick)) ||
        (rc = ws_get(*c, WS_SNOOP_PART, (size_t)std::max<int64_t>(n_blocks, 1) * SNOOP_PART, &b.part)) ||
        (rc = ws_get(*c, WS_SNOOP_OUT, (size_t)SNOOP_OUT, &b.out)) || (rc = ws_get(*c, WS_REL_Q, 2 * no, &d_q)))
        return rc;
    // the starting state in local order
    std::vector<uint8_t> st(no, SNOOP_ACTIVE);
    int64_t n_excl = 0;
    if (excluded)
        for (int64_t i = 0; i < n; ++i) {
            st[(size_t)i] = excluded[c->obs_pho[i]] ? SNOOP_EXCLUDED : SNOOP_ACTIVE;
            n_excl += st[(size_t)i] == SNOOP_EXCLUDED;
        }
    FBA_HIP(hipMemcpyAsync(b.state, st.data(), st.size(), hipMemcpyHostToDevice, c->stream));
    if ((rc = launch_snoop_init(*c, b))) return rc;
    FBA_HIP(hipStreamSynchronize(c->stream));  // (st is pageable memory of this call)
    // a change of the weights: the first one of an unweighted context switches the weighted kernels on
    auto apply = [&](int mode) -> int {
        int r;
        if ((r = reweight_begin(c)) || (r = launch_snoop_apply(*c, b, mode))) return r;
        return reweight_end(c);
    };
    if (n_excl > 0 && (rc = apply(0))) return rc;

    CallTimer timer;
    if ((rc = timer.init(c, "fba_snoop"))) return rc;
    int n_rounds = 0, n_iter = 0, conv = 0, bits = 0;
    auto publish = [&]() -> int {
        if (rounds) *rounds = n_rounds;
        if (iterations) *iterations = n_iter;
        if (converged) *converged = conv;
        if (status_bits) *status_bits = bits;
        timer.publish(c);
        if (n > 0 && (excluded || stat)) {
            std::vector<double> w((size_t)n, 0.0);
            if (n_rounds > 0) FBA_HIP(hipMemcpyAsync(w.data(), b.W, sizeof(double) * n, hipMemcpyDeviceToHost, c->stream));
            FBA_HIP(hipMemcpyAsync(st.data(), b.state, (size_t)n, hipMemcpyDeviceToHost, c->stream));
            FBA_HIP(hipStreamSynchronize(c->stream));
            for (int64_t i = 0; i < n; ++i) {
                if (excluded) excluded[c->obs_pho[i]] = st[(size_t)i];
                if (stat) stat[c->obs_pho[i]] = w[(size_t)i];
            }
        }
        return FBA_OK;
    };
    double out[SNOOP_OUT] = {0, 0, 0, 0};
    for (int k = 0; k < op.max_rounds; ++k) {
        if ((rc = solve_round(ctx, "fba_snoop", n_iter))) { (void)publish(); return rc; }
        timer.start(c->stream);
        if ((rc = launch_vce_q(*c, nullptr, nullptr, d_q)) ||
            (rc = launch_snoop_round(*c, b, d_q, op.min_rays, op.min_img_points, op.crit))) {
            (void)publish();
            return rc;
        }
        timer.stop(c->stream);
        FBA_HIP(hipMemcpyAsync(out, b.out, sizeof out, hipMemcpyDeviceToHost, c->stream));
        FBA_HIP(hipStreamSynchronize(c->stream));
        if ((rc = timer.lap())) return rc;
        n_rounds = k + 1;
        const int64_t n_pick = (int64_t)out[0], n_back = n_pick ? 0 : (int64_t)out[1];
        n_excl = (int64_t)out[2];
        const bool last = k == op.max_rounds - 1;
        const bool stop = n_pick > 0 && snoop_share_stop(n_excl, n_pick, c->n_pts, op.max_share);
        const bool change = (n_pick > 0 || n_back > 0) && !last && !stop;
        if (table) {
            double* t = table + 4 * (size_t)k;
            t[0] = (double)n_pick; t[1] = (double)n_back; t[3] = out[3];
            t[2] = (double)(change ? n_excl + n_pick - n_back : n_excl);
        }
        if (n_pick == 0 && n_back == 0) { conv = 1; break; }
        if (stop) bits |= 2;
        if (!change) break;
        if ((rc = apply(n_pick > 0 ? 1 : 2))) { (void)publish(); return rc; }
    }
    return publish();
}

}  // extern "C"
