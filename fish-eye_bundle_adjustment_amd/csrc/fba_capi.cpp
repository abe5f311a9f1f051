// fba_capi.cpp -- the core of the extern "C" boundary of libfba.so (include/fba.h): the context and the step.
//
// Host side of the device-resident Gauss-Newton loop: has the packed problem validated and planned
// (fba_plan.cpp: observation orderings, chunks, accumulation plan; fba_order.cpp: the factorisation
// schedule), uploads that plan, allocates device memory once, and drives the kernels of
// fba_kernels.hip / fba_chol.hip.  Also xhat, the dense A / w / G, the residuals, the priors' read-back and the
// timing, probe and test hooks.
// The loop semantics are the reference's main.m:407-494; the unknown layout is Buildxhat.m:6-134.
// The rest of the API, by subsystem: fba_api_host.cpp (everything that touches no device, the error text, the
// entry checks and option defaults), fba_api_weights.cpp (weights, loss, damping, cost, the damped loop),
// fba_api_postfit.cpp (covariance, reliability, post-fit outputs), fba_api_start.cpp (rays, intersection,
// resection), fba_api_rounds.cpp (variance components, data snooping); what they share is in fba_api.h.
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <string>
#include <thread>

#include "fba_api.h"

namespace fba {

static void destroy(Ctx* c) {
    if (!c) return;
    for (auto& q : c->owned) mem_free(q.first, q.second);
    for (auto& w : c->ws) mem_free(w.first);
    for (auto& e : c->ev)
        if (e) (void)hipEventDestroy(e);
    for (auto e : c->probe_ev)
        if (e) (void)hipEventDestroy(e);
    for (auto g : c->graph)
        if (g) (void)hipGraphExecDestroy(g);

    if (c->own_stream && c->stream) (void)hipStreamDestroy(c->stream);
    delete c;
}

struct CtxDeleter {
    void operator()(Ctx* c) const { destroy(c); }
};

// stage 3 of create(): the plan's arrays, uploaded as they are
static int upload_plan(Ctx& c, const HostPlan& hp) {
    const bool split = c.sched.split;
    int rc = FBA_OK;
    if (c.n_prior > 0 &&
        ((c.n_pcam > 0 && ((rc = upload(c, &c.d_pc_idx, hp.pc_idx)) || (rc = upload(c, &c.d_pc_val, hp.pc_val)))) ||
         (!hp.gprior.empty() && (rc = upload(c, &c.d_gprior, hp.gprior))) ||
         (c.n_pres > 0 && ((rc = upload(c, &c.d_pr_idx, hp.pr_idx)) || (rc = upload(c, &c.d_pr_val, hp.pr_val))))))
        return rc;
    if ((rc = upload(c, &c.d_xoff, hp.xoff)) || (rc = upload(c, &c.d_xy, hp.xy)) || (rc = upload(c, &c.d_img, hp.img)) ||
        (rc = upload(c, &c.d_cam, hp.cam)) || (rc = upload(c, &c.d_pt, hp.pt)) || (rc = upload(c, &c.d_ctl, hp.ctl)) ||
        (rc = upload(c, &c.d_lp_tie, hp.lp_tie)) || (rc = upload(c, &c.d_lp_start, hp.lp_start)) ||
        (rc = upload(c, &c.d_lp_cam, hp.lp_cam)) || (rc = upload(c, &c.d_acc, hp.acc)) || (rc = upload(c, &c.d_xfull, c.xfull0)) ||
        (rc = upload(c, &c.d_caminfo, hp.caminfo)) || (rc = upload(c, &c.d_active, hp.active)) ||
        (rc = upload(c, &c.d_counted, hp.counted)) || (rc = upload(c, &c.d_obs_pho, c.obs_pho)) ||
        (rc = upload(c, &c.d_chunk_obs, hp.chunk_obs)) || (rc = upload(c, &c.d_chunk_pt, hp.chunk_pt)) ||
        (rc = upload(c, &c.d_sched, c.sched.buf)) ||
        (c.opt.world > 1 && !split && (rc = upload(c, &c.d_gpairs, hp.gpairs))) ||
        (split && ((rc = upload(c, &c.d_bown, hp.bown)) || (rc = upload(c, &c.d_rown, hp.rown)) || (rc = upload(c, &c.d_topdiag, hp.topdiag)))))
        return rc;
    return FBA_OK;
}

// stage 4 of create(): the work buffers, their initial contents, the kernels' one-time setup
static int alloc_work(Ctx& c) {
    const Layout& L = c.L;
    const AccPlan& A = c.acc;
    const GenPlan& G = c.gen;
    c.ncomp = jac_stride(L.cw);
    c.pt_comp = pt_stride(L.cw);
    const int npk = cam_part(L.cw);
    c.n_part = (int)std::max<int64_t>((L.u_full + 255) / 256, (c.n_obs + 255) / 256 * 3) + 8;
    int rc;
    if ((c.n_prior > 0 && ((rc = dalloc(c, &c.d_pr_out, (size_t)c.n_prior + 1)) || (rc = dalloc(c, &c.d_pr_part, (size_t)(c.n_pres + 255) / 256)))) ||
        (rc = dalloc(c, &c.d_lrt, 2)) || ((c.opt.world > 1 || c.sched.split) && (rc = dalloc(c, &c.d_red, (size_t)c.n_red))) ||
        (rc = dalloc(c, &c.d_delta, L.u_full)) || (rc = dalloc(c, &c.d_xlin, L.u_full)) || (rc = dalloc(c, &c.d_img_tab, (size_t)L.n_img * IMG_TAB)) ||
        (rc = dalloc(c, &c.d_cam_tab, (size_t)L.n_cam * c.cam_tab_stride)) ||
        (rc = dalloc(c, &c.d_G, (size_t)std::max(L.n_img, 1) * G_BLK)) ||
        (rc = dalloc(c, &c.d_J, (size_t)c.ncomp * c.n_obs_pad)) || (rc = dalloc(c, &c.d_WT, (size_t)OBS_REC * c.n_obs_pad)) ||
        (rc = dalloc(c, &c.d_pt_tab, (size_t)c.pt_comp * c.n_lp_pad)) ||
        (rc = dalloc(c, &c.d_ppart, (size_t)A.n_pk * PAIR_BLK)) ||
        (rc = dalloc(c, &c.d_U, A.n_tt > 0 ? (size_t)T_ROW * c.n_obs_pad : 1)) ||
        (rc = dalloc(c, &c.d_ipart, (size_t)A.n_ik * img_part(L.cw))) ||
        (rc = dalloc(c, &c.d_cpart, (size_t)(c.n_chunks_lr + G.n_gc) * npk)) ||
        (rc = dalloc(c, &c.d_gpt, (size_t)G.n_gp * GPT)) || (rc = dalloc(c, &c.d_gcu, (size_t)G.n_gc * gpc_tab(L.cw))) ||
        (rc = dalloc(c, &c.d_gug, (size_t)G.n_gi * GUG)) || (rc = dalloc(c, &c.d_xpart, (size_t)G.n_gx * xcam_part(L.cw))) ||
        (rc = dalloc(c, &c.d_kpart, (size_t)G.n_gkk * campair_part(L.cw))) ||
        (rc = dalloc(c, &c.d_cseg, (size_t)std::max(L.n_cam, 1) * CAM_SEG * npk)) ||
        (rc = dalloc(c, &c.d_bscr, (size_t)BSC_TOTAL)) ||
        (rc = dalloc(c, &c.d_gblk, (size_t)(L.n_pad / NB) * GRAM_BLK)) ||
        (rc = dalloc(c, &c.d_S, (size_t)(L.n_pad + NB) * L.ld)) ||
        (rc = dalloc(c, &c.d_P, (size_t)std::max(c.sched.n_scratch, 1) * 4096)) || (rc = dalloc(c, &c.d_X, (size_t)L.n_pad)) ||
        (rc = dalloc(c, &c.d_dinv, (size_t)(L.n_pad / NB) * 8 * 256)) ||
        (rc = dalloc(c, &c.d_linv, (size_t)(L.n_pad / NB) * NB * NB)) ||
        (rc = dalloc(c, &c.d_scal, (size_t)SCAL_TOTAL)) || (rc = dalloc(c, &c.d_part, (size_t)c.n_part)) ||
        (rc = dalloc(c, &c.d_res, (size_t)RES_ROW * std::max<int64_t>(c.n_obs, 1))))
        return rc;
    FBA_HIP(hipMemset(c.d_lrt, 0, 2 * sizeof(unsigned)));
    FBA_HIP(hipMemset(c.d_scal, 0, sizeof(double) * SCAL_ZEROED));  // (chol_setup then sets scal[SCAL_SPINS])
    if ((rc = chol_setup(c)) || (rc = acc_setup(c))) return rc;
    if (getenv("FBA_LR_PROFILE") && c.n_chunks_lr > 0 && (rc = dalloc(c, &c.d_lrprof, (size_t)LR_PROF * c.n_chunks_lr))) return rc;
    if (getenv("FBA_PANEL_TRACE") && c.sched.n_waves > 0) {
        const size_t nt = std::max<size_t>((size_t)PTRACE_WG * c.sched.n_waves, (size_t)c.sched.flow_n * FTRACE / 8);
        if ((rc = dalloc(c, &c.d_ptrace, 8 * nt))) return rc;
        FBA_HIP(hipMemset(c.d_ptrace, 0, sizeof(uint64_t) * 8 * nt));
    }
    FBA_HIP(hipMemset(c.d_delta, 0, sizeof(double) * L.u_full));
    // outside the factor's block pattern S stays zero; the pattern itself is zeroed per accumulation
    FBA_HIP(hipMemsetAsync(c.d_S, 0, sizeof(double) * (size_t)(L.n_pad + NB) * L.ld, c.stream));
    FBA_HIP(hipStreamSynchronize(c.stream));
    if ((rc = dalloc(c, &c.h_pinned, (size_t)HPIN_TOTAL, true))) return rc;
    FBA_HIP(hipHostGetDevicePointer((void**)&c.d_hpinned, c.h_pinned, 0));
    std::fill(c.h_pinned, c.h_pinned + HPIN_TOTAL, 0.0);
    for (auto& e : c.ev) FBA_HIP(hipEventCreate(&e));
    return FBA_OK;
}

// validate -> plan (fba_plan.cpp, host only) -> upload the plan -> allocate the work buffers.  The context is
// owned here until it is handed out, so every early return frees what it holds.
// pr: prior observations of unknowns, or nullptr (fba_create)
static int create(const fba_problem* p, const fba_settings* s, const fba_options* o, const fba_priors* pr, Ctx** out) {
    fba_options opt{};
    int rc = check_inputs(p, s, o, &pr, opt);
    if (rc) return rc;

    std::unique_ptr<Ctx, CtxDeleter> ctx(new Ctx());
    Ctx& c = *ctx;
    c.force_sync = getenv("FBA_SYNC") && atoi(getenv("FBA_SYNC")) != 0;  // (read per context)
    // the order of k_lin_reduce's (D) task queue: 1 camera-image-pair, 2 image-pair-camera, 3 image-camera-pair;
    // anything else the default.  The results do not depend on it (tests/test_gpu_lr_queue.py)
    c.lr_order = getenv("FBA_LR_ORDER") ? atoi(getenv("FBA_LR_ORDER")) : 0;
    if (c.lr_order < 0 || c.lr_order > 3) c.lr_order = 0;
    PlanKnobs knobs;
    if (getenv("FBA_PAIR_TERMS")) knobs.pair_terms = atof(getenv("FBA_PAIR_TERMS"));
    HostPlan hp;
    if ((rc = build_plan(p, s, opt, pr, knobs, c, hp))) return rc;

    FBA_HIP(hipSetDevice(opt.device));
    c.device = opt.device;
    if (opt.stream) {
        c.stream = (hipStream_t)opt.stream;
    } else {
        FBA_HIP(hipStreamCreateWithFlags(&c.stream, hipStreamNonBlocking));
        c.own_stream = true;
    }
    if ((rc = upload_plan(c, hp)) || (rc = alloc_work(c))) return rc;
    if (opt.verbose)
        fprintf(stderr, "[fba] rank %d/%d: n_obs %ld (tie %ld), points %ld, pairs %ld (%ld terms), u_c %ld, n_pad %ld; "
                "chunks %ld, pair keys %ld, U-row pair terms %ld, image keys %ld (%d lanes each); general points %ld\n",
                opt.rank, opt.world, (long)c.n_obs, (long)c.n_obs_tie, (long)c.n_lp, (long)c.n_pairs,
                (long)c.n_pair_terms, (long)c.L.u_c, (long)c.L.n_pad, (long)c.n_chunks_lr, (long)c.acc.n_pk, (long)c.acc.n_tt,
                (long)c.acc.n_ik, c.ik_lanes, (long)c.gen.n_gp);
    *out = ctx.release();
    return FBA_OK;
}

static int set_xhat_ref(Ctx* c, const double* xhat) {
    std::vector<double> xf = c->xfull0;
    for (int64_t i = 0; i < c->L.u_full; ++i)
        if (c->full_to_ref[i] >= 0) xf[i] = xhat[c->full_to_ref[i]];
    FBA_HIP(hipMemcpyAsync(c->d_xfull, xf.data(), sizeof(double) * xf.size(), hipMemcpyHostToDevice, c->stream));
    FBA_HIP(hipStreamSynchronize(c->stream));
    c->xhat_changed();
    return FBA_OK;
}

static inline void mark(Ctx* c, int i) {
    if (c->timing) (void)hipEventRecord(c->ev[i], c->stream);
}

static bool graph_eligible(const Ctx* c) {
    return c->graphs_ok && c->stream && !c->timing && !c->probe && !c->d_lrprof && !c->d_ptrace;
}

// run body() on the context's stream, through a graph captured from its first run when eligible
template <class F>
static int run_graph(Ctx* c, int which, F&& body) {
    if (!graph_eligible(c)) return body();
    if (!c->graph[which]) {
        if (hipStreamBeginCapture(c->stream, hipStreamCaptureModeThreadLocal) != hipSuccess) {
            (void)hipGetLastError();  // e.g. a stream that cannot be captured: launch eagerly from now on
            c->graphs_ok = false;
            return body();
        }
        const int rc = body();
        hipGraph_t g = nullptr;
        const hipError_t e = hipStreamEndCapture(c->stream, &g);
        if (rc != FBA_OK || e != hipSuccess || !g) {
            if (g) (void)hipGraphDestroy(g);
            (void)hipGetLastError();  // do not leave the capture's error to the next call's checks
            if (rc != FBA_OK) return rc;
            c->graphs_ok = false;  // capture unsupported here: run eagerly from now on
            return body();
        }
        const hipError_t ei = hipGraphInstantiate(&c->graph[which], g, nullptr, nullptr, 0);
        (void)hipGraphDestroy(g);
        if (ei != hipSuccess) {
            c->graph[which] = nullptr;
            c->graphs_ok = false;
            return body();
        }
    }
    FBA_HIP(hipGraphLaunch(c->graph[which], c->stream));
    return FBA_OK;
}

static int accumulate_body(Ctx* c) {
    int rc;
    mark(c, 0);
    // tables + the linearisation point; S's pattern is zeroed by k_lin_reduce's tail workgroups
    if ((rc = launch_params(*c, nullptr, c->d_xlin))) return rc;
    mark(c, 1);
    // general tie points: their Jacobian rows, point tables and partials (ahead of the reductions)
    if ((rc = launch_gen_tables(*c, nullptr, c->damp_on())) || (rc = launch_gen_keys(*c))) return rc;
    mark(c, 2);
    // the camera-side priors behind the reductions' stores of the summed partials, ahead of the pack and the border
    if ((rc = launch_accumulate(*c)) || (rc = launch_gen_reduce(*c)) || (rc = launch_prior_cam(*c))) return rc;
    if (c->d_lrprof) {  // FBA_LR_PROFILE: per-phase averages of k_lin_reduce (us)
        std::vector<uint64_t> tp(LR_PROF * c->n_chunks_lr);
        FBA_HIP(hipMemcpyAsync(tp.data(), c->d_lrprof, sizeof(uint64_t) * tp.size(), hipMemcpyDeviceToHost, c->stream));
        FBA_HIP(hipStreamSynchronize(c->stream));
        // stamps (wave 0's): 0 start, 1 model done, 2 points done, 3 couplings done: the queues start, 5 the queues and
        // the camera sum done; 4, 6, 7 the finish of the last camera (points' part), image-key and pair-key task of (D)'s
        // queue, 8 of the last early task (camera observation sums; 0: the chunk had none); 9 the early tasks
        // waves 4-7 had finished at stamp 3, under the point phases
        double ph[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
        uint64_t lo = UINT64_MAX, hi = 0;
        const double nch = (double)c->n_chunks_lr;
        for (int64_t ch = 0; ch < c->n_chunks_lr; ++ch) {
            const uint64_t* q = &tp[LR_PROF * ch];
            for (int i = 0; i < 3; ++i) ph[i] += (double)(q[i + 1] - q[i]) * 0.01 / nch;
            ph[3] += (double)(q[5] - q[3]) * 0.01 / nch;  // (D)
            const int last[4] = {4, 6, 7, 8};
            for (int k = 0; k < 4; ++k) ph[4 + k] += (double)(std::max(q[last[k]], q[3]) - q[3]) * 0.01 / nch;
            ph[8] += (double)q[9] / nch;
            lo = std::min(lo, q[0]);
            hi = std::max(hi, q[5]);
        }
        fprintf(stderr, "[fba] k_lin_reduce per chunk (us): model %.2f points %.2f couplings %.2f queue %.2f "
                "(last task done at: early camera %.2f camera %.2f image keys %.2f pair keys %.2f; order %d; "
                "early tasks done under the point phases %.2f); span %.1f\n", ph[0], ph[1], ph[2], ph[3], ph[7], ph[4],
                ph[5], ph[6], c->lr_order, ph[8], (double)(hi - lo) * 0.01);
    }
    if (c->sched.split) {
        // subtree split: the top rows' accumulated diagonal (before k_border_rhs writes unit rows), the
        // border rows, this rank's subtree columns (flow A: their factor, forward solve and Schur updates of
        // the top blocks), then the buffer
        if ((rc = launch_pack_split(*c, 2)) || (rc = launch_border(*c)) || (rc = launch_cholesky(*c, 0)) ||
            (rc = launch_pack_split(*c, 0)))
            return rc;
    } else if (c->opt.world > 1 && (rc = launch_pack(*c, 0))) {
        return rc;
    }
    mark(c, 3);
    return FBA_OK;
}

static int accumulate(Ctx* c) {
    c->have_factor = false;
    const int rc = run_graph(c, 0, [&] { return accumulate_body(c); });
    if (rc == FBA_OK) {
        c->have_lin = true;
        c->solved = false;
    }
    return rc;
}

static int solve_body(Ctx* c) {
    int rc;
    const Layout& L = c->L;
    if (c->sched.split) {  // the summed top blocks (+ the B rows' weights), then the top columns (flow B)
        if ((rc = launch_pack_split(*c, 1))) return rc;
        mark(c, 4);
        if ((rc = launch_cholesky(*c, 1))) return rc;
    } else {
        if (c->opt.world > 1 && (rc = launch_pack(*c, 1))) return rc;
        // damping: S' + lambda diag(S') on the summed system, ahead of the border (its weights read the diagonal)
        if ((rc = launch_damp_diag(*c)) || (rc = launch_border(*c))) return rc;
        mark(c, 4);
        if ((rc = launch_cholesky(*c))) return rc;
    }
    mark(c, 5);
    // tie-point corrections of other ranks' points stay zero (a single rank writes every one of them in
    // k_backsub; a zero-byte memset is not a valid graph node)
    if (L.u_full > L.u_c && c->opt.world > 1)
        FBA_HIP(hipMemsetAsync(c->d_delta + L.u_c, 0, sizeof(double) * (L.u_full - L.u_c), c->stream));
    if ((rc = launch_backward(*c))) return rc;
    mark(c, 6);
    if ((rc = launch_backsub_update(*c))) return rc;
    mark(c, 7);
    // the mirrored d_scal slots reach h_pinned from k_sum_parts itself (host-mapped stores, no copy node)
    return FBA_OK;
}

static int solve_enqueue(Ctx* c) {
    if (!c->have_lin) { set_error("fba_solve_update before fba_accumulate"); return FBA_ERR_ARG; }
    // the solve factors S in place (and with the subtree split, flow A's sync words are not re-zeroed by
    // the solve: flow B's tickets would be past its grid), so a second solve of one accumulation would
    // factor a factor -- refused; accumulate again
    if (c->solved) {
        set_error("one fba_solve_update per fba_accumulate (the solve factors the accumulated system in place)");
        return FBA_ERR_ARG;
    }
    // marked before the launches: a solve that fails part way may already have factored S in place, so a
    // retry must accumulate again too (accumulate() clears the mark)
    c->solved = true;
    const int rc = run_graph(c, 1, [&] { return solve_body(c); });
    if (rc == FBA_OK) ++c->solves_enqueued;  // k_sum_parts' count once this solve is done
    return rc;
}

// wait for the solve, read scal (again from the device when `recopy`: a caller may have all-reduced
// the deltasum share in place after the graph's own copy), check the failure flags
// FBA_PANEL_TRACE: one line per elimination-tree level, times in us from the first k_panel's start:
// launch span, the gap after the previous launch, and per workgroup role the last end (diagonal-block
// updates, potrf start / after its waits / end, panel solves, inverses, other updates)
// k_chol_flow (FBA_PANEL_TRACE=1): per diagonal-block record, times in us from the launch's first start:
// start, waits done, fused panel solve + diagonal update done, late partials added, end (potrf done);
// then per role the record count and the last end
static void print_flow_trace(Ctx* c) {
    const Sched& s = c->sched;
    std::vector<uint64_t> t((size_t)FTRACE * s.flow_n);
    if (hipMemcpy(t.data(), c->d_ptrace, t.size() * sizeof(uint64_t), hipMemcpyDeviceToHost) != hipSuccess) return;
    uint64_t t0 = UINT64_MAX;
    for (int b = 0; b < s.flow_n; ++b)
        if (t[FTRACE * (size_t)b]) t0 = std::min(t0, t[FTRACE * (size_t)b]);
    const uint64_t M = (1ull << 63) - 1;
    auto us = [&](uint64_t v) { return (v & M) ? (double)((v & M) - t0) * 0.01 : -1.0; };
    uint64_t rend[5] = {0, 0, 0, 0, 0};
    int rn[5] = {0, 0, 0, 0, 0};
    const int32_t* recs = s.buf.data() + s.flow_rec;
    const bool detail = getenv("FBA_PANEL_TRACE")[0] == '2';
    if (getenv("FBA_PANEL_TRACE")[0] == '3')  // every record in dispatch order: role, ids, start, waits done, end
        for (int b = 0; b < s.flow_n; ++b) {
            const uint64_t* r = &t[FTRACE * (size_t)b];
            const int32_t* rec = recs + (size_t)Sched::FLOW_REC * b;
            fprintf(stderr, "[fba] rec %d %d %d %d %d %.2f %.2f %.2f %.2f %.2f\n", b, rec[0], rec[1], rec[2], rec[3], us(r[0]),
                    us(r[1]), us(r[2]), us(r[48]), us(r[49]));
        }
    for (int b = 0; b < s.flow_n; ++b) {
        const uint64_t* r = &t[FTRACE * (size_t)b];
        const int32_t* rec = recs + (size_t)Sched::FLOW_REC * b;
        const int role = rec[0];
        rend[role] = std::max(rend[role], r[2]);
        rn[role]++;
        if (role != 0) continue;
        fprintf(stderr, "[fba]   diag wg %5d block %3d (fused %3d%s): start %7.1f  waits %7.1f  fused %7.1f  late %7.1f  end %7.1f\n",
                b, rec[1], rec[2], rec[6] > 0 ? ", late" : "", us(r[0]), us(r[1]), rec[2] >= 0 ? us(r[4]) : -1.0,
                rec[2] >= 0 ? us(r[5]) : -1.0, us(r[2]));
        if (!detail) continue;
        fprintf(stderr, "[fba]       potrf leaf 0 %.1f, barrier %.1f, panel tile (2, 0) %.1f; column solved / published:",
                us(r[3]), us(r[6]), us(r[7]));
        for (int q = 0; q < 8; ++q) fprintf(stderr, " %.1f/%.1f", us(r[24 + q]), us(r[32 + q]));
        fprintf(stderr, "\n");
        if (rec[2] < 0) continue;
        fprintf(stderr, "[fba]       block in LDS / applied:");
        for (int q = 0; q < 8; ++q) fprintf(stderr, " %.1f/%.1f%s", us(r[8 + q]), us(r[16 + q]), (r[16 + q] >> 63) ? "p" : "");
        fprintf(stderr, "\n");
        fprintf(stderr, "[fba]       loading group's share stored:");
        for (int q = 0; q < 8; ++q) fprintf(stderr, " %.1f", us(r[40 + q]));
        fprintf(stderr, "\n");
        for (int x = 0; x < s.flow_n; ++x) {  // the panel halves of its fused rows
            const int32_t* rx = recs + (size_t)Sched::FLOW_REC * x;
            const uint64_t* q = &t[FTRACE * (size_t)x];
            if (!(rx[0] == 1 && rx[1] == rec[2] && (rx[2] >> 1) == rec[1])) continue;
            fprintf(stderr, "[fba]       half %d wg %5d: start %.1f waits %.1f column in / published:", rx[2] & 1, x, us(q[0]),
                    us(q[1]));
            for (int u = 0; u < 8; ++u) fprintf(stderr, " %.1f/%.1f", us(q[8 + u]), us(q[16 + u]));
            fprintf(stderr, "  end %.1f\n", us(q[2]));
        }
        for (int x = 0; x < s.flow_n && rec[9] >= 0; ++x) {  // its split helper
            const int32_t* rx = recs + (size_t)Sched::FLOW_REC * x;
            const uint64_t* q = &t[FTRACE * (size_t)x];
            if (!(rx[0] == 4 && rx[1] == rec[1])) continue;
            fprintf(stderr, "[fba]       split helper wg %5d: start %.1f block in LDS / applied:", x, us(q[0]));
            for (int u = 0; u < 8; ++u) fprintf(stderr, " %.1f/%.1f", us(q[8 + u]), us(q[16 + u]));
            fprintf(stderr, "  end %.1f\n", us(q[2]));
        }
    }
    fprintf(stderr, "[fba] flow: diag %d (last end %.1f), panel halves %d (%.1f), updates %d (%.1f), inverses %d (%.1f), "
            "split helpers %d (%.1f)\n", rn[0], us(rend[0]), rn[1], us(rend[1]), rn[2], us(rend[2]), rn[3], us(rend[3]),
            rn[4], us(rend[4]));
    (void)hipMemset(c->d_ptrace, 0, t.size() * sizeof(uint64_t));
}

static void print_panel_trace(Ctx* c) {
    if (c->chol_flow && c->sched.flow_ok && c->sched.flow_n > 0) { print_flow_trace(c); return; }
    const int nw = c->sched.n_waves;
    std::vector<uint64_t> t((size_t)8 * PTRACE_WG * nw);
    if (hipMemcpy(t.data(), c->d_ptrace, t.size() * sizeof(uint64_t), hipMemcpyDeviceToHost) != hipSuccess) return;
    uint64_t t0 = UINT64_MAX, prev_end = 0;
    for (int w = 0; w < nw; ++w)
        for (int b = 0; b < PTRACE_WG; ++b)
            if (t[(size_t)8 * (w * PTRACE_WG + b)] != 0) t0 = std::min(t0, t[(size_t)8 * (w * PTRACE_WG + b)]);
    auto us = [&](uint64_t v) { return v ? (double)(v - t0) * 0.01 : -1.0; };
    auto hi_trsm_end = [&](int w) {
        uint64_t m = 0;
        for (int b = 0; b < PTRACE_WG; ++b) {
            const uint64_t* r = &t[(size_t)8 * (w * PTRACE_WG + b)];
            if (r[0] != 0 && r[3] == 3) m = std::max(m, r[2]);
        }
        return m;
    };
    for (int w = 0; w < nw; ++w) {
        uint64_t lo = UINT64_MAX, hi = 0, rend[6] = {0, 0, 0, 0, 0, 0}, pst = 0, prd = 0, tfirst = UINT64_MAX, tseen = 0;
        int n = 0;
        for (int b = 0; b < PTRACE_WG; ++b) {
            const uint64_t* r = &t[(size_t)8 * (w * PTRACE_WG + b)];
            if (r[0] == 0) continue;
            ++n;
            lo = std::min(lo, r[0]);
            hi = std::max(hi, r[2]);
            const int role = (int)r[3];
            if (role >= 0 && role < 6) rend[role] = std::max(rend[role], r[2]);
            if (role == 1) { pst = std::max(pst, r[0]); prd = std::max(prd, r[1]); }
            if (role == 3) { tfirst = std::min(tfirst, r[0]); tseen = std::max(tseen, r[1]); }
            if (role == 3 && getenv("FBA_PANEL_TRACE")[0] == '3' && r[2] == hi_trsm_end(w))
                fprintf(stderr, "[fba]   level %2d last panel solve wg %4d: start %6.1f  step 6 done %6.1f  factor seen %6.1f  "
                        "step 7 done %6.1f  end %6.1f  batches %llx\n", w, b, us(r[0]), us(r[5]), us(r[1]), us(r[6]), us(r[2]),
                        (unsigned long long)r[4]);
            if (role == 0 && getenv("FBA_PANEL_TRACE")[0] == '2')
                fprintf(stderr, "[fba]   level %2d diag-update wg %3d: %2d sources%s  %6.1f .. %6.1f (%4.1f us)\n", w, b,
                        (int)(r[1] & 0xff), (r[1] & 0x100) ? " (split group)" : "", us(r[0]), us(r[2]), (double)(r[2] - r[0]) * 0.01);
            if (role == 0 && getenv("FBA_PANEL_TRACE")[0] == '2')
                fprintf(stderr, "[fba]       loaded +%.1f  products +%.1f  published +%.1f\n", (double)(r[4] - r[0]) * 0.01,
                        (double)(r[5] - r[0]) * 0.01, (double)(r[2] - r[0]) * 0.01);
        }
        if (n == 0) { fprintf(stderr, "[fba] level %2d: own k_potrf128/k_trsm128 launches (no trace)\n", w); continue; }
        fprintf(stderr, "[fba] level %2d: %4d wg  span %7.1f .. %7.1f (%5.1f)  gap %5.1f | diag-upd end %7.1f | potrf %7.1f wait-end %7.1f "
                "end %7.1f | panel-upd end %7.1f | trsm %7.1f .. (factor seen %7.1f) %7.1f | trtri end %7.1f | other-upd end %7.1f\n",
                w, n, us(lo), us(hi), (double)(hi - lo) * 0.01, prev_end ? (double)(lo - prev_end) * 0.01 : 0.0, us(rend[0]),
                us(pst), us(prd), us(rend[1]), us(rend[2]), tfirst == UINT64_MAX ? -1.0 : us(tfirst), us(tseen), us(rend[3]),
                us(rend[4]), us(rend[5]));
        prev_end = hi;
    }
    (void)hipMemset(c->d_ptrace, 0, t.size() * sizeof(uint64_t));
}

// Completion of a solve: k_sum_parts, the last kernel of every solve, writes its results to host-mapped
// memory and then the device's count of finished solves; fba_step polls that count until it reaches the
// number of solves enqueued on the context (a spin on coherent host memory returns a few us after the
// GPU's write, where hipStreamSynchronize's wake-up is slower) -- later work on the stream is ordered after
// the solve anyway.  The poll spins briefly, then yields the core between reads; once the count is there,
// hipStreamQuery surfaces an asynchronous error of the stream at once.  The stream is synchronised instead
// when a caller re-copies scal (the multi-GPU path), with tracing or timing on, with FBA_SYNC=1, and after
// ~5 s without the count (a faulted launch: the synchronisation reports it).
static bool wait_solve_seq(Ctx* c) {
    if (c->force_sync || c->timing || c->d_ptrace || c->d_lrprof) return false;
    const double want = (double)c->solves_enqueued;
    volatile const double* seq = c->h_pinned + HPIN_SEQ;
    const auto t0 = std::chrono::steady_clock::now();
    for (unsigned it = 0; *seq < want; ++it) {
        if (it < 4096) continue;  // ~the first 10-20 us: spin
        std::this_thread::yield();
        if ((it & 255) == 0 && std::chrono::steady_clock::now() - t0 > std::chrono::seconds(5)) return false;
    }
    std::atomic_thread_fence(std::memory_order_acquire);
    return true;
}

static int solve_finish(Ctx* c, double* dsum, bool recopy) {
    if (recopy) FBA_HIP(hipMemcpyAsync(c->h_pinned, c->d_scal, sizeof(double) * SCAL_MIRROR, hipMemcpyDeviceToHost, c->stream));
    if (recopy || !wait_solve_seq(c)) {
        FBA_HIP(hipStreamSynchronize(c->stream));
    } else {
        const hipError_t q = hipStreamQuery(c->stream);  // (hipErrorNotReady: later work queued, no error)
        if (q != hipSuccess && q != hipErrorNotReady) FBA_HIP(q);
    }
    c->solve_seq = c->h_pinned[HPIN_SEQ];
    if (c->d_ptrace && !c->sched.split) print_panel_trace(c);
    if (c->timing) {
        float ms;
        for (int i = 0; i < 7; ++i) {
            (void)hipEventElapsedTime(&ms, c->ev[i], c->ev[i + 1]);
            c->last_ms[i] = ms;
        }
        (void)hipEventElapsedTime(&ms, c->ev[0], c->ev[7]);
        c->last_ms[7] = ms;
    }
    c->iterations++;
    const double info = c->h_pinned[HPIN_FAIL];
    *dsum = c->h_pinned[HPIN_DSUM];
    if (info < 0.0) {
        // k_update left xhat as it was (fba_chol.hip, bounded polls): the context stays usable
        set_error("device hand-off timeout in the block Cholesky / backward solve (a workgroup of k_chol_flow, "
                  "k_panel or k_bwd_flow was not resident); xhat left unchanged");
        c->have_delta = false;
        c->have_factor = false;
        return FBA_ERR_HIP;
    }
    c->have_delta = true;
    c->have_factor = !c->damp_on();  // a damped solve's factor is not that of N: no covariance from it
    if (info != 0.0) {
        char buf[160];
        snprintf(buf, sizeof buf, "reduced normal matrix not positive definite (pivot %ld): singular / unconstrained network",
                 (long)info);
        set_error(buf);
        return FBA_ERR_NOT_SPD;
    }
    if (!std::isfinite(*dsum)) { set_error("non-finite correction vector"); return FBA_ERR_NONFINITE; }
    return FBA_OK;
}

static int solve_update(Ctx* c, double* dsum) {
    int rc;
    if ((rc = solve_enqueue(c))) return rc;
    return solve_finish(c, dsum, false);
}

}  // namespace fba

using namespace fba;

extern "C" {

int fba_set_spin_bound(fba_ctx* ctx, int64_t spins) {
    if (!ctx || spins < 0) { set_error("fba_set_spin_bound: bad argument"); return FBA_ERR_ARG; }
    Ctx* c = reinterpret_cast<Ctx*>(ctx);
    const double v = spin_bound_value(spins);
    FBA_HIP(hipStreamSynchronize(c->stream));
    FBA_HIP(hipMemcpy(c->d_scal + SCAL_SPINS, &v, sizeof v, hipMemcpyHostToDevice));
    return FBA_OK;
}

int fba_solve_mode(fba_ctx* ctx, int32_t* split) {
    if (!ctx || !split) { set_error("fba_solve_mode: null argument"); return FBA_ERR_ARG; }
    *split = reinterpret_cast<Ctx*>(ctx)->sched.split ? 1 : 0;
    return FBA_OK;
}

int fba_create(const fba_problem* p, const fba_settings* s, const fba_options* o, fba_ctx** out) {
    if (!out) { set_error("out is NULL"); return FBA_ERR_ARG; }
    *out = nullptr;
    Ctx* c = nullptr;
    int rc = create(p, s, o, nullptr, &c);
    if (rc) return rc;
    *out = reinterpret_cast<fba_ctx*>(c);
    return FBA_OK;
}

int fba_create_priors(const fba_problem* p, const fba_settings* s, const fba_options* o, const fba_priors* pr,
                      fba_ctx** out) {
    if (!out) { set_error("out is NULL"); return FBA_ERR_ARG; }
    *out = nullptr;
    Ctx* c = nullptr;
    int rc = create(p, s, o, pr, &c);
    if (rc) return rc;
    *out = reinterpret_cast<fba_ctx*>(c);
    return FBA_OK;
}

int fba_get_priors(fba_ctx* ctx, int64_t* n, double* resid, double* vtpv) {
    int rc;
    Ctx* c = enter(ctx, "fba_get_priors", 0, rc);
    if (!c) return rc;
    if (n) *n = c->n_prior;
    if (vtpv) *vtpv = 0.0;
    if (c->n_prior == 0 || (!resid && !vtpv)) return FBA_OK;
    if ((rc = launch_prior_resid(*c))) return rc;
    std::vector<double> out((size_t)c->n_prior + 1);
    FBA_HIP(hipMemcpyAsync(out.data(), c->d_pr_out, sizeof(double) * out.size(), hipMemcpyDeviceToHost, c->stream));
    FBA_HIP(hipStreamSynchronize(c->stream));
    if (resid) std::copy(out.begin(), out.end() - 1, resid);
    if (vtpv) *vtpv = out.back();
    return FBA_OK;
}

void fba_destroy(fba_ctx* ctx) { destroy(reinterpret_cast<Ctx*>(ctx)); }

int fba_buildxhat(fba_ctx* ctx, double* xhat, int64_t* u_out) {
    Ctx* c = reinterpret_cast<Ctx*>(ctx);
    if (!c) { set_error("NULL context"); return FBA_ERR_ARG; }
    if (u_out) *u_out = c->L.u_ref;
    if (xhat)
        for (int64_t i = 0; i < c->L.u_full; ++i)
            if (c->full_to_ref[i] >= 0) xhat[c->full_to_ref[i]] = c->xfull0[i];
    return FBA_OK;
}

int fba_set_xhat(fba_ctx* ctx, const double* xhat) {
    Ctx* c = reinterpret_cast<Ctx*>(ctx);
    if (!c || !xhat) { set_error("NULL argument"); return FBA_ERR_ARG; }
    return set_xhat_ref(c, xhat);
}

int fba_get_xhat(fba_ctx* ctx, double* xhat, int32_t owned_only) {
    Ctx* c = reinterpret_cast<Ctx*>(ctx);
    if (!c || !xhat) { set_error("NULL argument"); return FBA_ERR_ARG; }
    std::vector<double> xf(c->L.u_full);
    FBA_HIP(hipMemcpyAsync(xf.data(), c->d_xfull, sizeof(double) * xf.size(), hipMemcpyDeviceToHost, c->stream));
    FBA_HIP(hipStreamSynchronize(c->stream));
    for (int64_t i = 0; i < c->L.u_full; ++i)
        if (c->full_to_ref[i] >= 0) xhat[c->full_to_ref[i]] = (owned_only && !c->full_owned[i]) ? 0.0 : xf[i];
    return FBA_OK;
}

int fba_build_awg(fba_ctx* ctx, const double* xhat, double* A, double* w, double* G, double* dist_scaling) {
    Ctx* c = reinterpret_cast<Ctx*>(ctx);
    if (!c) { set_error("NULL context"); return FBA_ERR_ARG; }
    int rc;
    if (xhat && (rc = set_xhat_ref(c, xhat))) return rc;
    // the reference's raw A, w whatever weights / loss are set; every reader of d_J linearises again first
    // (fba_residuals, fba_covariance), and have_lin is cleared below, so the raw rows are never read as whitened
    if ((rc = launch_params(*c)) || (rc = launch_linearize(*c, nullptr, true))) return rc;
    const Layout& L = c->L;
    const int64_t n = 2 * c->n_pts, u = L.u_ref;
    DevBuf<double> dA, dW;  // (freed on every return)
    DevBuf<int64_t> dmap;
    if ((rc = dA.alloc((size_t)n * u)) || (rc = dW.alloc((size_t)n)) || (rc = dmap.upload(c->full_to_ref))) return rc;
    FBA_HIP(hipMemsetAsync(dA.get(), 0, sizeof(double) * n * u, c->stream));
    FBA_HIP(hipMemsetAsync(dW.get(), 0, sizeof(double) * n, c->stream));
    if ((rc = launch_dense_awg(*c, dA.get(), dW.get(), dmap.get(), n, u))) return rc;
    if (A) FBA_HIP(hipMemcpyAsync(A, dA.get(), sizeof(double) * n * u, hipMemcpyDeviceToHost, c->stream));
    if (w) FBA_HIP(hipMemcpyAsync(w, dW.get(), sizeof(double) * n, hipMemcpyDeviceToHost, c->stream));
    std::vector<double> g((size_t)std::max(L.n_img, 1) * G_BLK), ct((size_t)L.n_cam * c->cam_tab_stride);
    FBA_HIP(hipMemcpyAsync(g.data(), c->d_G, sizeof(double) * g.size(), hipMemcpyDeviceToHost, c->stream));
    FBA_HIP(hipMemcpyAsync(ct.data(), c->d_cam_tab, sizeof(double) * ct.size(), hipMemcpyDeviceToHost, c->stream));
    FBA_HIP(hipStreamSynchronize(c->stream));
    if (G && c->set.inner_constraints) {
        std::fill(G, G + u * G_ROW, 0.0);
        for (int e = 0; e < L.n_img; ++e)
            for (int a = 0; a < 6; ++a) {
                const int64_t r = c->full_to_ref[6 * (int64_t)e + a];
                if (r < 0) continue;  // padding slot
                for (int m = 0; m < G_ROW; ++m) G[r + m * u] = g[(size_t)e * G_BLK + a * G_ROW + m];
            }
    }
    if (dist_scaling) {
        const int nc = L.n_cam, ncol = 2 + L.nk;
        std::fill(dist_scaling, dist_scaling + (size_t)nc * ncol, 0.0);
        for (int k = 0; k < nc; ++k) {
            // the reference stores 1-based xhat indices (BuildAwG.m:138, :150)
            const int64_t base = 6 * (int64_t)L.n_img + (int64_t)k * L.cw;
            if (c->set.est_radial) dist_scaling[k + 0 * nc] = (double)(c->full_to_ref[base + 3] + 1);
            if (c->set.est_decent) dist_scaling[k + 1 * nc] = (double)(c->full_to_ref[base + 3 + L.nk] + 1);
            for (int j = 0; j < L.nk; ++j)
                dist_scaling[k + (2 + j) * nc] = ct[(size_t)k * c->cam_tab_stride + CAM_TAB_HDR + L.nk + j];
        }
    }
    c->have_lin = false;
    return FBA_OK;
}

int fba_accumulate(fba_ctx* ctx) {
    Ctx* c = reinterpret_cast<Ctx*>(ctx);
    if (!c) { set_error("NULL context"); return FBA_ERR_ARG; }
    return accumulate(c);
}

int fba_reduce_buffer(fba_ctx* ctx, void** dev_ptr, int64_t* n_doubles) {
    Ctx* c = reinterpret_cast<Ctx*>(ctx);
    if (!c || !dev_ptr || !n_doubles) { set_error("NULL argument"); return FBA_ERR_ARG; }
    if (c->opt.world > 1) {  // compact: only the entries any rank writes (~6 MB at config 4)
        *dev_ptr = c->d_red;
        *n_doubles = c->n_red;
    } else {
        *dev_ptr = c->d_S;
        *n_doubles = (c->L.n_pad + 1) * c->L.ld;  // lower normal matrix + RHS row 0
    }
    return FBA_OK;
}

int fba_synchronize(fba_ctx* ctx) {
    Ctx* c = reinterpret_cast<Ctx*>(ctx);
    if (!c) { set_error("NULL context"); return FBA_ERR_ARG; }
    FBA_HIP(hipStreamSynchronize(c->stream));
    return FBA_OK;
}

int fba_solve_update(fba_ctx* ctx, double* deltasum_part) {
    Ctx* c = reinterpret_cast<Ctx*>(ctx);
    if (!c) { set_error("NULL context"); return FBA_ERR_ARG; }
    double d = 0.0;
    int rc = solve_update(c, &d);
    if (deltasum_part) *deltasum_part = d;
    return rc;
}

int fba_solve_update_async(fba_ctx* ctx) {
    Ctx* c = reinterpret_cast<Ctx*>(ctx);
    if (!c) { set_error("NULL context"); return FBA_ERR_ARG; }
    const int rc = solve_enqueue(c);
    if (rc == FBA_OK) c->pending = true;
    return rc;
}

int fba_deltasum_device(fba_ctx* ctx, void** dev_ptr) {
    Ctx* c = reinterpret_cast<Ctx*>(ctx);
    if (!c || !dev_ptr) { set_error("NULL argument"); return FBA_ERR_ARG; }
    *dev_ptr = c->d_scal + SCAL_DSUM;
    return FBA_OK;
}

int fba_solve_finish(fba_ctx* ctx, double* deltasum) {
    Ctx* c = reinterpret_cast<Ctx*>(ctx);
    if (!c) { set_error("NULL context"); return FBA_ERR_ARG; }
    if (!c->pending) { set_error("fba_solve_finish without fba_solve_update_async"); return FBA_ERR_ARG; }
    c->pending = false;
    double d = 0.0;
    const int rc = solve_finish(c, &d, true);
    if (deltasum) *deltasum = d;
    return rc;
}

int fba_step(fba_ctx* ctx, double* deltasum) {
    Ctx* c = reinterpret_cast<Ctx*>(ctx);
    if (!c) { set_error("NULL context"); return FBA_ERR_ARG; }
    if (c->opt.world != 1) { set_error("fba_step is single-GPU; use fba_accumulate/fba_solve_update"); return FBA_ERR_ARG; }
    int rc = accumulate(c);
    if (rc) return rc;
    double d = 0.0;
    rc = solve_update(c, &d);
    if (deltasum) *deltasum = d;
    return rc;
}

int fba_adjust(fba_ctx* ctx, int32_t* iterations, double* deltasum_hist) {
    Ctx* c = reinterpret_cast<Ctx*>(ctx);
    if (!c) { set_error("NULL context"); return FBA_ERR_ARG; }
    double deltasum = 100.0;  // main.m:407
    int count = 0;
    while (deltasum > c->set.threshold) {  // main.m:412
        ++count;
        int rc = fba_step(ctx, &deltasum);
        if (deltasum_hist) deltasum_hist[count - 1] = deltasum;
        if (iterations) *iterations = count;
        if (rc) return rc;
        if (count >= c->set.iteration_cap) break;  // main.m:490-493
    }
    if (iterations) *iterations = count;
    return FBA_OK;
}

int fba_residuals(fba_ctx* ctx, double* v, double* rsd, double* stats) {
    Ctx* c = reinterpret_cast<Ctx*>(ctx);
    if (!c) { set_error("NULL context"); return FBA_ERR_ARG; }
    if (!c->have_lin || !c->have_delta) { set_error("fba_residuals needs at least one iteration"); return FBA_ERR_ARG; }
    // v = A delta + w with A, w of the last linearisation (main.m:569): its Jacobian rows again, at
    // the parameters it was taken at
    int rc;
    if ((rc = launch_params(*c, c->d_xlin)) || (rc = launch_linearize(*c, c->d_xlin)) || (rc = launch_residuals(*c)))
        return rc;
    const int64_t n = c->n_obs;
    const int nblk = (int)((n + 255) / 256);
    std::vector<double> res(RES_ROW * (size_t)n), part(3 * (size_t)nblk);
    if (n > 0) {
        FBA_HIP(hipMemcpyAsync(res.data(), c->d_res, sizeof(double) * res.size(), hipMemcpyDeviceToHost, c->stream));
        FBA_HIP(hipMemcpyAsync(part.data(), c->d_part, sizeof(double) * part.size(), hipMemcpyDeviceToHost, c->stream));
    }
    FBA_HIP(hipStreamSynchronize(c->stream));
    if (v) std::fill(v, v + 2 * c->n_pts, 0.0);
    if (rsd) std::fill(rsd, rsd + RSD_ROW * c->n_pts, 0.0);
    for (int64_t o = 0; o < n; ++o) {
        const int64_t i = c->obs_pho[o];
        if (v) { v[2 * i] = res[2 * o]; v[2 * i + 1] = res[2 * o + 1]; }
        if (rsd)
            for (int m = 0; m < RSD_ROW; ++m) rsd[RSD_ROW * i + m] = res[2 * n + RSD_ROW * o + m];
    }
    double sx = 0, sy = 0, sp = 0;
    for (int b = 0; b < nblk; ++b) { sx += part[3 * b]; sy += part[3 * b + 1]; sp += part[3 * b + 2]; }
    if (stats && c->n_prior > 0) {  // the priors' rows: v'Pv gains sum p v^2, the divisor their count
        double pv = 0.0;
        if ((rc = fba_get_priors(ctx, nullptr, nullptr, &pv))) return rc;
        sp += pv;
    }
    if (stats) {
        const double nu = (double)(2 * c->n_pts + c->n_prior - c->L.u_ref);
        if (c->opt.world == 1) {
            const double rx = std::sqrt(sx / (double)c->n_pts), ry = std::sqrt(sy / (double)c->n_pts);
            stats[0] = rx; stats[1] = ry; stats[2] = std::sqrt(rx * rx + ry * ry);
            stats[3] = sp / nu;  // main.m:601: v'Pv / (n - u)
        } else {
            stats[0] = sx; stats[1] = sy; stats[2] = 0; stats[3] = 0;
        }
        stats[4] = sp;
        stats[5] = nu;
    }
    return FBA_OK;
}

int fba_build_rsd(fba_ctx* ctx, const double* v, const double* xhat, double* rsd) {
    Ctx* c = reinterpret_cast<Ctx*>(ctx);
    if (!c || !v || !xhat || !rsd) { set_error("NULL argument"); return FBA_ERR_ARG; }
    const Layout& L = c->L;
    // xp, yp per camera: from xhat when estimated, else the INT values (BuildRSD.m:12-26)
    std::vector<double> xpyp(2 * (size_t)std::max(L.n_cam, 1));
    for (int k = 0; k < L.n_cam; ++k)
        for (int a = 0; a < 2; ++a) {
            const int64_t f = 6 * (int64_t)L.n_img + (int64_t)k * L.cw + a;
            xpyp[2 * k + a] = c->full_to_ref[f] >= 0 ? xhat[c->full_to_ref[f]] : c->xfull0[f];
        }
    const int64_t n = c->n_pts;
    DevBuf<double> dv, dx, dr;  // (freed on every return)
    int rc;
    if ((rc = dv.alloc(2 * (size_t)n)) || (rc = dx.upload(xpyp)) || (rc = dr.alloc(RSD_ROW * (size_t)n))) return rc;
    FBA_HIP(hipMemcpyAsync(dv.get(), v, sizeof(double) * 2 * n, hipMemcpyHostToDevice, c->stream));
    FBA_HIP(hipMemsetAsync(dr.get(), 0, sizeof(double) * RSD_ROW * n, c->stream));
    if ((rc = launch_build_rsd(*c, dv.get(), dx.get(), dr.get()))) return rc;
    FBA_HIP(hipMemcpyAsync(rsd, dr.get(), sizeof(double) * RSD_ROW * n, hipMemcpyDeviceToHost, c->stream));
    FBA_HIP(hipStreamSynchronize(c->stream));
    return FBA_OK;
}

int fba_last_timings(fba_ctx* ctx, double* ms) {
    Ctx* c = reinterpret_cast<Ctx*>(ctx);
    if (!c || !ms) { set_error("NULL argument"); return FBA_ERR_ARG; }
    for (int i = 0; i < 8; ++i) ms[i] = c->last_ms[i];
    return FBA_OK;
}

int fba_set_probe(fba_ctx* ctx, int32_t enabled) {
    Ctx* c = reinterpret_cast<Ctx*>(ctx);
    if (!c) { set_error("NULL context"); return FBA_ERR_ARG; }
    if (enabled < 0 || enabled > 2) { set_error("fba_set_probe: 0 (off), 1 (k_syrk_multi) or 2 (k_panel)"); return FBA_ERR_ARG; }
    c->probe = enabled;
    c->probe_n = 0;
    c->probe_flops = 0.0;
    return FBA_OK;
}

int fba_probe_stats(fba_ctx* ctx, double* out) {
    Ctx* c = reinterpret_cast<Ctx*>(ctx);
    if (!c || !out) { set_error("NULL argument"); return FBA_ERR_ARG; }
    FBA_HIP(hipStreamSynchronize(c->stream));
    double ms = 0.0;
    for (int i = 0; i < c->probe_n; ++i) {
        float t = 0.f;
        FBA_HIP(hipEventElapsedTime(&t, c->probe_ev[2 * i], c->probe_ev[2 * i + 1]));
        ms += t;
    }
    out[0] = c->probe_n;
    out[1] = ms;
    out[2] = c->probe_flops;
    out[3] = 0.0;
    return FBA_OK;
}

int fba_test_live_allocations(int64_t* n) {
    if (!n) { set_error("NULL argument"); return FBA_ERR_ARG; }
    *n = g_live_allocations.load(std::memory_order_relaxed);
    return FBA_OK;
}

int fba_test_border_solve(int32_t device, const double* gram, double* coef) {
    if (!gram || !coef) { set_error("NULL argument"); return FBA_ERR_ARG; }
    return border_solve_selftest(device, gram, coef);
}

int fba_set_timing(fba_ctx* ctx, int32_t enabled) {
    Ctx* c = reinterpret_cast<Ctx*>(ctx);
    if (!c) { set_error("NULL context"); return FBA_ERR_ARG; }
    c->timing = enabled != 0;
    return FBA_OK;
}

}  // extern "C"
