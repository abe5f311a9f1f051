// fba_api.h -- what the files of the C API (fba_capi.cpp, fba_api_*.cpp) share (not part of the ABI).
#pragma once
#include "fba_internal.h"

namespace fba {

// ---- entry checks ----
// What an entry point requires of its context; require() tests them in this order.
enum Req : unsigned {
    REQ_IDLE = 1,        // no fba_solve_update_async waiting for its fba_solve_finish (FBA_ERR_ARG)
    REQ_SINGLE_GPU = 2,  // world == 1 (FBA_ERR_UNSUPPORTED)
    REQ_NO_LOSS = 4,     // no robust loss set (FBA_ERR_UNSUPPORTED)
    REQ_NO_DAMPING = 8,  // damping == 0 (FBA_ERR_UNSUPPORTED)
};
// FBA_OK, or the error set and its code.  tail: the function's own reason after the common part of a refusal --
// of the robust-loss refusal when REQ_NO_LOSS is asked for, else of the single-GPU one
int require(const Ctx* c, const char* who, unsigned req, const char* tail = "");
// the context of an entry point after "<who>: NULL context" and require(); nullptr with rc set
Ctx* enter(fba_ctx* ctx, const char* who, unsigned req, int& rc, const char* tail = "");

// ---- option defaults and checks (fba_api_host.cpp: the *_host entry points need them too) ----
extern const fba_lm_options kLmDefaults;
extern const fba_intersect_options kIntersectDefaults;
extern const fba_resect_options kResectDefaults;
extern const fba_vce_options kVceDefaults;
extern const fba_snoop_options kSnoopDefaults;
int check_resect_options(const char* who, const fba_resect_options& op);
int check_vce_args(const char* who, int64_t n_rows, int32_t n_groups, const int32_t* group, const fba_vce_options& op);
int check_snoop_options(const char* who, const fba_snoop_options& op);

// ---- weights (fba_api_weights.cpp) ----
int weight_buffers(Ctx* c);     // the three [2 n_obs] buffers, on first use
int weighting_changed(Ctx* c);  // the stream drained, the captured accumulation dropped, Ctx::weights_changed()
// A kernel of the caller's rewrites d_sw between the two: begin switches the weighted kernels on when the context
// was unweighted (weight_buffers, weighting_changed), end waits for the kernel and marks the new weights
int reweight_begin(Ctx* c);
int reweight_end(Ctx* c);

// ---- the image list of fba_resect and fba_snoop (fba_api_start.cpp) ----
int image_list_once(Ctx* c);

// ---- the round head of fba_vce and fba_snoop (fba_api_rounds.cpp) ----
// fba_adjust with its iterations added to n_iter, then "<who>: the last solve left no factor"
int solve_round(fba_ctx* ctx, const char* who, int& n_iter);

// ---- the time of a call's own launches ----
// An event pair of the call's own (the steps in between use the context's): start / stop around the launches, lap()
// after the stream was synchronised adds the pair's time, publish() writes fba_last_timings' slots -- zeros, the sum
// in slot 7.  With timing off it creates and records nothing.
struct CallTimer {
    hipEvent_t e0 = nullptr, e1 = nullptr;
    double ms = 0.0;
    CallTimer() = default;
    CallTimer(const CallTimer&) = delete;
    CallTimer& operator=(const CallTimer&) = delete;
    ~CallTimer() {
        if (e0) (void)hipEventDestroy(e0);
        if (e1) (void)hipEventDestroy(e1);
    }
    int init(const Ctx* c, const char* who) {
        if (!c->timing) return FBA_OK;
        if (hipEventCreate(&e0) != hipSuccess || hipEventCreate(&e1) != hipSuccess) {
            set_error(std::string(who) + ": hipEventCreate failed");
            return FBA_ERR_HIP;
        }
        return FBA_OK;
    }
    void start(hipStream_t s) { if (e1) (void)hipEventRecord(e0, s); }
    void stop(hipStream_t s) { if (e1) (void)hipEventRecord(e1, s); }
    int lap() {
        if (!e1) return FBA_OK;
        float t = 0.f;
        FBA_HIP(hipEventElapsedTime(&t, e0, e1));
        ms += t;
        return FBA_OK;
    }
    void publish(Ctx* c) const {
        if (!e1) return;
        for (double& v : c->last_ms) v = 0.0;
        c->last_ms[7] = ms;
    }
};

}  // namespace fba
