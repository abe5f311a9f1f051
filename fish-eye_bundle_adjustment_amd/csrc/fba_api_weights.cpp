// fba_api_weights.cpp -- the C API of the weighting: per-observation weights and robust loss, Levenberg-Marquardt
// damping, the cost and the damped loop (include/fba.h; no reference counterpart).
#include <algorithm>
#include <cmath>
#include <cstdio>

#include "fba_api.h"

namespace fba {

int weight_buffers(Ctx* c) {
    if (c->d_sw) return FBA_OK;
    const size_t n = 2 * (size_t)std::max<int64_t>(c->n_obs, 1);
    int rc;
    if ((rc = dalloc(*c, &c->d_sw, n)) || (rc = dalloc(*c, &c->d_seff, n)) || (rc = dalloc(*c, &c->d_weff, n))) return rc;
    return FBA_OK;
}

// a change of the weighting: the captured accumulation holds the old kernel arguments, and neither the
// linearisation nor the factor of the last solve belongs to the new weights
int weighting_changed(Ctx* c) {
    FBA_HIP(hipStreamSynchronize(c->stream));
    if (c->graph[0]) {
        (void)hipGraphExecDestroy(c->graph[0]);
        c->graph[0] = nullptr;
    }
    c->weights_changed();
    return FBA_OK;
}

int reweight_begin(Ctx* c) {
    int rc;
    if (!c->weights_on && ((rc = weight_buffers(c)) || (rc = weighting_changed(c)))) return rc;
    return FBA_OK;
}

int reweight_end(Ctx* c) {
    FBA_HIP(hipStreamSynchronize(c->stream));
    c->weights_on = true;
    c->weights_changed();
    return FBA_OK;
}

}  // namespace fba

using namespace fba;

extern "C" {

int fba_set_weights(fba_ctx* ctx, const double* weight) {
    int rc;
    Ctx* c = enter(ctx, "fba_set_weights", REQ_IDLE, rc);
    if (!c) return rc;
    const int64_t n = 2 * c->n_pts;
    bool all_one = true;  // all 1 is NULL: the unweighted kernels, whose arithmetic the weighted ones match
                          // only to rounding (s = 1 is exact, the compiler's contraction around it is not the same)
    if (weight)
        for (int64_t i = 0; i < n; ++i) {
            all_one = all_one && weight[i] == 1.0;
            if (!std::isfinite(weight[i]) || !(weight[i] > 0.0)) {
                char buf[160];
                snprintf(buf, sizeof buf, "fba_set_weights: weight[%ld] = %g (PHO row %ld, %c) must be finite and > 0",
                         (long)i, weight[i], (long)(i / 2), i % 2 ? 'y' : 'x');
                set_error(buf);
                return FBA_ERR_ARG;
            }
        }
    if ((rc = weighting_changed(c))) return rc;
    if (!weight || all_one) {
        c->weights_on = false;
        return FBA_OK;
    }
    if ((rc = weight_buffers(c))) return rc;
    double* d_w = nullptr;
    if ((rc = ws_get(*c, WS_WEIGHTS, (size_t)n, &d_w))) return rc;
    if (n > 0) FBA_HIP(hipMemcpyAsync(d_w, weight, sizeof(double) * n, hipMemcpyHostToDevice, c->stream));
    if ((rc = launch_set_weights(*c, d_w))) return rc;
    return reweight_end(c);
}

int fba_set_loss(fba_ctx* ctx, int32_t loss, double k) {
    if (loss != FBA_LOSS_NONE && loss != FBA_LOSS_HUBER && loss != FBA_LOSS_CAUCHY) {
        set_error("fba_set_loss: unknown loss (FBA_LOSS_NONE, FBA_LOSS_HUBER or FBA_LOSS_CAUCHY)");
        return FBA_ERR_ARG;
    }
    if (loss != FBA_LOSS_NONE && (!std::isfinite(k) || !(k > 0.0))) {
        set_error("fba_set_loss: k (in units of sigma) must be finite and > 0");
        return FBA_ERR_ARG;
    }
    int rc;
    Ctx* c = enter(ctx, "fba_set_loss", REQ_IDLE, rc);
    if (!c) return rc;
    if ((rc = weighting_changed(c)) || (loss != FBA_LOSS_NONE && (rc = weight_buffers(c)))) return rc;
    c->loss = loss;
    c->loss_k = loss == FBA_LOSS_NONE ? 0.0 : k;
    return FBA_OK;
}

int fba_get_weights(fba_ctx* ctx, double* weight) {
    Ctx* c = reinterpret_cast<Ctx*>(ctx);
    if (!c || !weight) { set_error("fba_get_weights: NULL argument"); return FBA_ERR_ARG; }
    if (!c->have_lin || !c->have_delta) { set_error("fba_get_weights needs at least one iteration"); return FBA_ERR_ARG; }
    const int64_t n = 2 * c->n_pts;
    if (!c->whiten_on()) {  // neither weights nor a loss (the kernels write none): 1 for this rank's observations
        std::fill(weight, weight + n, 0.0);
        for (int64_t o = 0; o < c->n_obs; ++o) weight[2 * c->obs_pho[o]] = weight[2 * c->obs_pho[o] + 1] = 1.0;
        return FBA_OK;
    }
    // the weights of the last linearisation: its rows again, as fba_residuals (k_residuals writes s^2)
    int rc;
    if ((rc = launch_params(*c, c->d_xlin)) || (rc = launch_linearize(*c, c->d_xlin)) || (rc = launch_residuals(*c)))
        return rc;
    double* d_w = nullptr;
    if ((rc = ws_get(*c, WS_WEIGHTS, (size_t)n, &d_w))) return rc;
    if (n > 0) FBA_HIP(hipMemsetAsync(d_w, 0, sizeof(double) * n, c->stream));
    if ((rc = launch_get_weights(*c, d_w))) return rc;
    if (n > 0) FBA_HIP(hipMemcpyAsync(weight, d_w, sizeof(double) * n, hipMemcpyDeviceToHost, c->stream));
    FBA_HIP(hipStreamSynchronize(c->stream));
    return FBA_OK;
}

// ---- Levenberg-Marquardt damping, the cost and the damped loop ----
int fba_set_damping(fba_ctx* ctx, double lambda) {
    int rc;
    Ctx* c = enter(ctx, "fba_set_damping", 0, rc);
    if (!c) return rc;
    if (!std::isfinite(lambda) || lambda < 0.0) { set_error("fba_set_damping: lambda must be finite and >= 0"); return FBA_ERR_ARG; }
    if ((rc = require(c, "fba_set_damping", REQ_IDLE))) return rc;
    if (lambda > 0.0 && c->sched.split) {
        set_error("fba_set_damping: not implemented for the subtree split (fba_solve_mode 1); use the replicated solve");
        return FBA_ERR_UNSUPPORTED;
    }
    if (lambda == c->damping) return FBA_OK;
    if ((lambda > 0.0) != c->damp_on()) {
        // on / off: other kernels and launches in both halves (the WH instantiations, k_damp_diag, the border
        // weights' own launch), so both captured graphs go; lambda itself is a device scalar, and a change of
        // its value re-captures nothing
        if ((rc = weighting_changed(c))) return rc;
        if (c->graph[1]) {
            (void)hipGraphExecDestroy(c->graph[1]);
            c->graph[1] = nullptr;
        }
    } else {
        // lambda1 -> lambda2: the tie points of a held linearisation were eliminated with V + lambda1 diag(V), and
        // k_damp_diag would scale S' with lambda2 -- a system of neither; fba_solve_update asks for a new fba_accumulate
        FBA_HIP(hipStreamSynchronize(c->stream));
        c->weights_changed();
    }
    FBA_HIP(hipMemcpy(c->d_scal + SCAL_DAMP, &lambda, sizeof lambda, hipMemcpyHostToDevice));
    c->damping = lambda;
    return FBA_OK;
}

int fba_cost(fba_ctx* ctx, double* cost) {
    Ctx* c = reinterpret_cast<Ctx*>(ctx);
    if (!c || !cost) { set_error("fba_cost: NULL argument"); return FBA_ERR_ARG; }
    int rc;
    if ((rc = require(c, "fba_cost", REQ_IDLE))) return rc;
    const size_t nblk = (size_t)((c->n_obs + 255) / 256);
    double* d_w = nullptr;
    if ((rc = ws_get(*c, WS_COST, nblk + 4, &d_w)) || (rc = launch_cost(*c, d_w + 4, d_w))) return rc;
    FBA_HIP(hipMemcpyAsync(cost, d_w, sizeof(double) * 3, hipMemcpyDeviceToHost, c->stream));
    FBA_HIP(hipStreamSynchronize(c->stream));
    return FBA_OK;
}

int fba_adjust_lm(fba_ctx* ctx, const fba_lm_options* o, int32_t* trials, int32_t* polish, double* hist) {
    int rc;
    Ctx* c = enter(ctx, "fba_adjust_lm", REQ_SINGLE_GPU, rc);
    if (!c) return rc;
    const fba_lm_options q = o ? *o : kLmDefaults;
    if (!(q.lambda0 > 0.0) || !(q.up > 1.0) || !(q.down > 1.0) || !(q.lambda_min > 0.0) || !(q.lambda_max >= q.lambda0) ||
        !(q.ftol >= 0.0) || !std::isfinite(q.lambda_max) || !std::isfinite(q.up) || !std::isfinite(q.down)) {
        set_error("fba_adjust_lm: options need lambda0 > 0, up > 1, down > 1, lambda_min > 0, lambda0 <= lambda_max < inf, ftol >= 0");
        return FBA_ERR_ARG;
    }
    if (trials) *trials = 0;
    if (polish) *polish = 0;
    const int cap = std::max(c->set.iteration_cap, 1);
    const size_t xbytes = sizeof(double) * (size_t)c->L.u_full;
    double* d_save = nullptr;
    int n = 0, nt = 0;
    if ((rc = ws_get(*c, WS_LM_SAVE, (size_t)c->L.u_full, &d_save))) return rc;
    auto record = [&](double lambda, double cost, double dsum, int acc) {
        if (hist) { hist[4 * n] = lambda; hist[4 * n + 1] = cost; hist[4 * n + 2] = dsum; hist[4 * n + 3] = acc; }
        ++n;
    };
    auto restore = [&]() -> int {  // xhat as before the trial; its linearisation and correction are not this xhat's
        FBA_HIP(hipMemcpyAsync(c->d_xfull, d_save, xbytes, hipMemcpyDeviceToDevice, c->stream));
        c->xhat_changed();
        return FBA_OK;
    };
    // every exit leaves the context undamped: the damped phase's failures through fail(), the not-converged exit by
    // its own call, and the polish phase runs with damping already 0.  fba_set_damping(0) cannot fail here except on a
    // HIP error, which the failure being returned already reports, so its result is dropped
    auto fail = [&](int code) { (void)fba_set_damping(ctx, 0.0); return code; };  // (keeps the failure's message)
    double f3[3], F, lambda = q.lambda0;
    if ((rc = fba_cost(ctx, f3))) return rc;
    F = f3[0];
    // damped phase: at most cap - 1 trials, so that one polish pass always fits under Iteration_Cap
    while (n < cap - 1) {
        FBA_HIP(hipMemcpyAsync(d_save, c->d_xfull, xbytes, hipMemcpyDeviceToDevice, c->stream));
        if ((rc = fba_set_damping(ctx, lambda))) return fail(rc);
        double dsum = 0.0, Fn = HUGE_VAL;
        rc = fba_step(ctx, &dsum);
        if (rc != FBA_OK && rc != FBA_ERR_NOT_SPD) return fail(rc);
        if (rc == FBA_OK) {
            if ((rc = fba_cost(ctx, f3))) return fail(rc);
            Fn = f3[0];
        }
        ++nt;
        if (trials) *trials = nt;
        if (std::isfinite(Fn) && std::fabs(Fn - F) <= q.ftol * F) {  // the differences have reached rounding: stop here
            const int keep = Fn <= F;
            if (!keep && (rc = restore())) return fail(rc);
            record(lambda, Fn, dsum, keep);
            if (keep) F = Fn;
            break;
        }
        if (std::isfinite(Fn) && Fn < F) {
            record(lambda, Fn, dsum, 1);
            F = Fn;
            lambda = std::max(lambda / q.down, q.lambda_min);
            if (dsum <= c->set.threshold) break;
            continue;
        }
        if ((rc = restore())) return fail(rc);
        record(lambda, Fn, dsum, 0);
        lambda *= q.up;
        if (lambda > q.lambda_max) {
            (void)fba_set_damping(ctx, 0.0);
            set_error("fba_adjust_lm: not converged, no damped step lowers the cost up to lambda_max");
            return FBA_ERR_NONFINITE;
        }
    }
    // polish: plain Gauss-Newton passes to the reference's stop rule (main.m:412, :490-493), at least one, so
    // that v, sigma02, Cx and the reliability numbers come from an undamped last pass as after fba_adjust
    if ((rc = fba_set_damping(ctx, 0.0))) return rc;
    double dsum = 100.0;
    int np = 0;
    while (dsum > c->set.threshold && n < cap) {
        if ((rc = fba_step(ctx, &dsum))) return rc;
        if ((rc = fba_cost(ctx, f3))) return rc;
        record(0.0, f3[0], dsum, 1);
        ++np;
        if (polish) *polish = np;
    }
    return FBA_OK;
}

}  // extern "C"
