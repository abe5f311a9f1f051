// fba_capi.cpp -- the extern "C" boundary of libfba.so (include/fba.h).
//
// Host side of the device-resident Gauss-Newton loop: has the packed problem validated and planned
// (fba_plan.cpp: observation orderings, chunks, accumulation plan; fba_order.cpp: the factorisation
// schedule), uploads that plan, allocates device memory once, and drives the kernels of
// fba_kernels.hip / fba_chol.hip.
// The loop semantics are the reference's main.m:407-494; the unknown layout is Buildxhat.m:6-134.
#include <algorithm>
#include <array>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <thread>
#include <map>
#include <memory>
#include <numeric>
#include <tuple>

#include "fba_internal.h"
#include "fba_eig3.h"
#include "fba_ray.h"
#include "fba_resect.h"
#include "fba_vce.h"
#include "fba_snoop.h"

namespace fba {

static thread_local std::string g_err;
void set_error(const std::string& msg) { g_err = msg; }

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
    c->have_lin = false;
    c->have_delta = false;
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

const char* fba_last_error(void) { return g_err.c_str(); }
int fba_abi_version(void) { return FBA_ABI_VERSION; }

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
    Ctx* c = reinterpret_cast<Ctx*>(ctx);
    if (!c) { set_error("fba_get_priors: NULL context"); return FBA_ERR_ARG; }
    if (n) *n = c->n_prior;
    if (vtpv) *vtpv = 0.0;
    if (c->n_prior == 0 || (!resid && !vtpv)) return FBA_OK;
    int rc;
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

// ---- per-observation weights and robust loss (no reference counterpart) ----
namespace fba {
// the three [2 n_obs] buffers, on first use
static int weight_buffers(Ctx* c) {
    if (c->d_sw) return FBA_OK;
    const size_t n = 2 * (size_t)std::max<int64_t>(c->n_obs, 1);
    int rc;
    if ((rc = dalloc(*c, &c->d_sw, n)) || (rc = dalloc(*c, &c->d_seff, n)) || (rc = dalloc(*c, &c->d_weff, n))) return rc;
    return FBA_OK;
}
// a change of the weighting: the captured accumulation holds the old kernel arguments, and neither the
// linearisation nor the factor of the last solve belongs to the new weights
static int weighting_changed(Ctx* c) {
    FBA_HIP(hipStreamSynchronize(c->stream));
    if (c->graph[0]) {
        (void)hipGraphExecDestroy(c->graph[0]);
        c->graph[0] = nullptr;
    }
    c->have_lin = false;
    c->have_factor = false;
    return FBA_OK;
}
}  // namespace fba

int fba_set_weights(fba_ctx* ctx, const double* weight) {
    Ctx* c = reinterpret_cast<Ctx*>(ctx);
    if (!c) { set_error("fba_set_weights: NULL context"); return FBA_ERR_ARG; }
    if (c->pending) { set_error("fba_set_weights between fba_solve_update_async and fba_solve_finish"); return FBA_ERR_ARG; }
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
    int rc;
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
    FBA_HIP(hipStreamSynchronize(c->stream));
    c->weights_on = true;
    return FBA_OK;
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
    Ctx* c = reinterpret_cast<Ctx*>(ctx);
    if (!c) { set_error("fba_set_loss: NULL context"); return FBA_ERR_ARG; }
    if (c->pending) { set_error("fba_set_loss between fba_solve_update_async and fba_solve_finish"); return FBA_ERR_ARG; }
    int rc;
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

// ---- Levenberg-Marquardt damping, the cost and the damped loop (no reference counterpart) ----
int fba_set_damping(fba_ctx* ctx, double lambda) {
    Ctx* c = reinterpret_cast<Ctx*>(ctx);
    if (!c) { set_error("fba_set_damping: NULL context"); return FBA_ERR_ARG; }
    if (!std::isfinite(lambda) || lambda < 0.0) { set_error("fba_set_damping: lambda must be finite and >= 0"); return FBA_ERR_ARG; }
    if (c->pending) { set_error("fba_set_damping between fba_solve_update_async and fba_solve_finish"); return FBA_ERR_ARG; }
    if (lambda > 0.0 && c->sched.split) {
        set_error("fba_set_damping: not implemented for the subtree split (fba_solve_mode 1); use the replicated solve");
        return FBA_ERR_UNSUPPORTED;
    }
    if (lambda == c->damping) return FBA_OK;
    int rc;
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
        c->have_lin = false;
    }
    FBA_HIP(hipMemcpy(c->d_scal + SCAL_DAMP, &lambda, sizeof lambda, hipMemcpyHostToDevice));
    c->damping = lambda;
    c->have_factor = false;
    return FBA_OK;
}

int fba_cost(fba_ctx* ctx, double* cost) {
    Ctx* c = reinterpret_cast<Ctx*>(ctx);
    if (!c || !cost) { set_error("fba_cost: NULL argument"); return FBA_ERR_ARG; }
    if (c->pending) { set_error("fba_cost between fba_solve_update_async and fba_solve_finish"); return FBA_ERR_ARG; }
    const size_t nblk = (size_t)((c->n_obs + 255) / 256);
    double* d_w = nullptr;
    int rc;
    if ((rc = ws_get(*c, WS_COST, nblk + 4, &d_w)) || (rc = launch_cost(*c, d_w + 4, d_w))) return rc;
    FBA_HIP(hipMemcpyAsync(cost, d_w, sizeof(double) * 3, hipMemcpyDeviceToHost, c->stream));
    FBA_HIP(hipStreamSynchronize(c->stream));
    return FBA_OK;
}

int fba_adjust_lm(fba_ctx* ctx, const fba_lm_options* o, int32_t* trials, int32_t* polish, double* hist) {
    Ctx* c = reinterpret_cast<Ctx*>(ctx);
    if (!c) { set_error("fba_adjust_lm: NULL context"); return FBA_ERR_ARG; }
    if (c->opt.world != 1) { set_error("fba_adjust_lm is single-GPU (world == 1)"); return FBA_ERR_UNSUPPORTED; }
    const fba_lm_options def{1e-3, 10.0, 10.0, 1e-12, 1e8, 1e-9};
    const fba_lm_options q = o ? *o : def;
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
    int rc, n = 0, nt = 0;
    if ((rc = ws_get(*c, WS_LM_SAVE, (size_t)c->L.u_full, &d_save))) return rc;
    auto record = [&](double lambda, double cost, double dsum, int acc) {
        if (hist) { hist[4 * n] = lambda; hist[4 * n + 1] = cost; hist[4 * n + 2] = dsum; hist[4 * n + 3] = acc; }
        ++n;
    };
    auto restore = [&]() -> int {  // xhat as before the trial; its linearisation and correction are not this xhat's
        FBA_HIP(hipMemcpyAsync(c->d_xfull, d_save, xbytes, hipMemcpyDeviceToDevice, c->stream));
        c->have_lin = false;
        c->have_delta = false;
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

int fba_eig3_host(int64_t n, const double* blk, double* ell) {
    if (n < 0 || (n > 0 && (!blk || !ell))) { set_error("fba_eig3_host: NULL argument"); return FBA_ERR_ARG; }
    for (int64_t i = 0; i < n; ++i) eig3_block(blk + TIE_BLK * i, ell + ELL_OUT * i);
    return FBA_OK;
}

// ---- forward intersection (no reference counterpart; kernels in fba_intersect.hip) ----
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
}  // namespace fba

int fba_image_rays(fba_ctx* ctx, double* ray, int32_t* status) {
    Ctx* c = reinterpret_cast<Ctx*>(ctx);
    if (!c) { set_error("fba_image_rays: NULL context"); return FBA_ERR_ARG; }
    if (c->pending) { set_error("fba_image_rays between fba_solve_update_async and fba_solve_finish"); return FBA_ERR_ARG; }
    double *d_ray = nullptr, *d_xu = nullptr;
    int32_t* d_rst = nullptr;
    int rc;
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
    Ctx* c = reinterpret_cast<Ctx*>(ctx);
    if (!c) { set_error("fba_intersect: NULL context"); return FBA_ERR_ARG; }
    if (c->pending) { set_error("fba_intersect between fba_solve_update_async and fba_solve_finish"); return FBA_ERR_ARG; }
    const fba_intersect_options def{10, 0, 0.5 * (1.0 - std::cos(std::acos(-1.0) / 180.0)), 1e-10};
    const fba_intersect_options& op = o ? *o : def;
    if (op.refine_iters < 0 || !std::isfinite(op.min_ratio) || op.min_ratio < 0.0 || !std::isfinite(op.refine_tol) ||
        op.refine_tol < 0.0) {
        set_error("fba_intersect: refine_iters >= 0, min_ratio and refine_tol finite and >= 0");
        return FBA_ERR_ARG;
    }
    const size_t nt = (size_t)std::max<int32_t>(c->L.n_tie, 1);
    double *d_ray = nullptr, *d_xu = nullptr, *d_out = nullptr;
    int32_t *d_rst = nullptr, *d_st = nullptr;
    int rc;
    if ((rc = ws_get(*c, WS_ISECT_OUT, 7 * nt, &d_out)) || (rc = ws_get(*c, WS_ISECT_ST, nt, &d_st)))
        return rc;
    // another rank's tie points stay 0 (the ranks' outputs sum to the whole)
    FBA_HIP(hipMemsetAsync(d_out, 0, sizeof(double) * 7 * nt, c->stream));
    FBA_HIP(hipMemsetAsync(d_st, 0, sizeof(int32_t) * nt, c->stream));
    hipEvent_t e0 = c->ev[0], e1 = c->ev[1];
    if (c->timing) (void)hipEventRecord(e0, c->stream);
    if ((rc = rays_to_ws(c, &d_ray, &d_rst, &d_xu)) ||
        (rc = launch_intersect(*c, d_ray, d_rst, d_xu, op.refine_iters, op.min_ratio, op.refine_tol, op.write_xhat != 0, d_out,
                               d_out + 3 * nt, d_st)))
        return rc;
    if (c->timing) (void)hipEventRecord(e1, c->stream);
    if (op.write_xhat) {  // as fba_set_xhat: neither the linearisation nor the factor belongs to the new xhat
        c->have_lin = false;
        c->have_delta = false;
        c->have_factor = false;
    }
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
    if (c->timing) {
        float ms = 0.f;
        FBA_HIP(hipEventElapsedTime(&ms, e0, e1));
        std::fill(c->last_ms, c->last_ms + 8, 0.0);
        c->last_ms[7] = ms;
    }
    return FBA_OK;
}

// ---- space resection (no reference counterpart; kernels in fba_resect.hip, per-image routines in fba_resect.h) ----
namespace fba {
static const fba_resect_options kResectDefaults{FBA_RESECT_USE_CONTROL, 10, 0, 0, 1e-6, 1e-10};
static int check_resect_options(const char* who, const fba_resect_options& op) {
    if ((op.use != FBA_RESECT_USE_CONTROL && op.use != FBA_RESECT_USE_ALL) || op.refine_iters < 0 ||
        !std::isfinite(op.min_ratio) || op.min_ratio < 0.0 || !std::isfinite(op.refine_tol) || op.refine_tol < 0.0) {
        set_error(std::string(who) + ": use CONTROL or ALL, refine_iters >= 0, min_ratio and refine_tol finite and >= 0");
        return FBA_ERR_ARG;
    }
    return FBA_OK;
}
// the image list on first use: d_img downloaded once, sorted on the host (build_image_list), kept by the context
static int image_list_once(Ctx* c) {
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

int fba_resect(fba_ctx* ctx, const fba_resect_options* o, double* eop, double* quality, int32_t* status, int64_t* n_not_ok) {
    Ctx* c = reinterpret_cast<Ctx*>(ctx);
    if (!c) { set_error("fba_resect: NULL context"); return FBA_ERR_ARG; }
    if (c->pending) { set_error("fba_resect between fba_solve_update_async and fba_solve_finish"); return FBA_ERR_ARG; }
    const fba_resect_options& op = o ? *o : kResectDefaults;
    int rc;
    if ((rc = check_resect_options("fba_resect", op))) return rc;
    if (c->opt.world != 1) {
        set_error("fba_resect is single-GPU (world == 1): an image's observations are spread over the ranks");
        return FBA_ERR_UNSUPPORTED;
    }
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
    hipEvent_t e0 = c->ev[0], e1 = c->ev[1];
    if (c->timing) (void)hipEventRecord(e0, c->stream);
    // the camera table at d_xfull: a function of xhat alone, so between fba_accumulate and fba_solve_update it is
    // rewritten with the values it holds (fba_intersect's argument)
    if ((rc = launch_params(*c)) || (rc = launch_resect_gather(*c, op.use == FBA_RESECT_USE_ALL, d_rec, d_use)) ||
        (rc = launch_resect(*c, d_rec, d_use, op.refine_iters, op.min_ratio, op.refine_tol, op.write_xhat != 0, d_out,
                            d_out + 6 * nio, d_st)))
        return rc;
    if (c->timing) (void)hipEventRecord(e1, c->stream);
    if (op.write_xhat) {  // as fba_set_xhat: neither the linearisation nor the factor belongs to the new xhat
        c->have_lin = false;
        c->have_delta = false;
        c->have_factor = false;
    }
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
    if (c->timing) {
        float ms = 0.f;
        FBA_HIP(hipEventElapsedTime(&ms, e0, e1));
        std::fill(c->last_ms, c->last_ms + 8, 0.0);
        c->last_ms[7] = ms;
    }
    return FBA_OK;
}

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

// ---- variance component estimation over observation groups (no reference counterpart) ----
namespace fba {
static const fba_vce_options kVceDefaults{10, 0, 1e-3, 1.0, 100.0};
static int check_vce_args(const char* who, int64_t n_rows, int32_t n_groups, const int32_t* group, const fba_vce_options& op) {
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
}  // namespace fba

int fba_vce(fba_ctx* ctx, int32_t n_groups, const int32_t* group, const fba_vce_options* o, double* component, double* table,
            int32_t* status, int32_t* rounds, int32_t* iterations, int32_t* converged) {
    Ctx* c = reinterpret_cast<Ctx*>(ctx);
    if (!c) { set_error("fba_vce: NULL context"); return FBA_ERR_ARG; }
    if (c->pending) { set_error("fba_vce between fba_solve_update_async and fba_solve_finish"); return FBA_ERR_ARG; }
    const fba_vce_options& op = o ? *o : kVceDefaults;
    int rc;
    if ((rc = check_vce_args("fba_vce", 2 * c->n_pts, n_groups, group, op))) return rc;
    if (c->opt.world != 1) { set_error("fba_vce is single-GPU (world == 1)"); return FBA_ERR_UNSUPPORTED; }
    if (c->loss != FBA_LOSS_NONE) {
        set_error("fba_vce with a robust loss set: its IRLS factor and a variance component would fight over the same residuals");
        return FBA_ERR_UNSUPPORTED;
    }
    if (c->damp_on()) { set_error("fba_vce with damping > 0: the factor of a damped solve is not that of N"); return FBA_ERR_UNSUPPORTED; }

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

    hipEvent_t e0 = nullptr, e1 = nullptr;  // events of the call's own: the steps in between use the context's
    if (c->timing) {
        FBA_HIP(hipEventCreate(&e0));
        if (hipEventCreate(&e1) != hipSuccess) { (void)hipEventDestroy(e0); set_error("fba_vce: hipEventCreate failed"); return FBA_ERR_HIP; }
    }
    struct EvGuard {
        hipEvent_t a, b;
        ~EvGuard() { if (a) (void)hipEventDestroy(a); if (b) (void)hipEventDestroy(b); }
    } guard{e0, e1};

    std::vector<double> comp((size_t)ng2, 1.0), out((size_t)ng1 * VCE_OUT);
    std::vector<int32_t> st((size_t)ng2, FBA_VCE_EMPTY);
    int n_rounds = 0, n_iter = 0, conv = 0;
    double own_ms = 0.0;
    auto publish = [&]() {
        if (component) std::copy(comp.begin(), comp.end(), component);
        if (status) std::copy(st.begin(), st.end(), status);
        if (rounds) *rounds = n_rounds;
        if (iterations) *iterations = n_iter;
        if (converged) *converged = conv;
        if (c->timing) {
            std::fill(c->last_ms, c->last_ms + 8, 0.0);
            c->last_ms[7] = own_ms;
        }
    };
    for (int k = 0; k < op.max_rounds; ++k) {
        int32_t it = 0;
        rc = fba_adjust(ctx, &it, nullptr);
        n_iter += it;
        if (rc) { publish(); return rc; }
        if (!c->have_factor || !c->have_delta) { publish(); set_error("fba_vce: the last solve left no factor"); return FBA_ERR_ARG; }
        if (c->timing) (void)hipEventRecord(e0, c->stream);
        if ((rc = launch_vce_q(*c, d_cdiag, d_pdiag, d_q)) ||
            (rc = launch_vce_sums(*c, d_q, d_grp, ng, op.min_redundancy, op.clip, d_slab, d_out))) {
            publish();
            return rc;
        }
        if (c->timing) (void)hipEventRecord(e1, c->stream);
        FBA_HIP(hipMemcpyAsync(out.data(), d_out, sizeof(double) * out.size(), hipMemcpyDeviceToHost, c->stream));
        if (c->n_prior > 0) {
            FBA_HIP(hipMemcpyAsync(cd.data(), d_cdiag, sizeof(double) * cd.size(), hipMemcpyDeviceToHost, c->stream));
            if (!pd.empty()) FBA_HIP(hipMemcpyAsync(pd.data(), d_pdiag, sizeof(double) * pd.size(), hipMemcpyDeviceToHost, c->stream));
        }
        FBA_HIP(hipStreamSynchronize(c->stream));
        if (c->timing) {
            float ms = 0.f;
            FBA_HIP(hipEventElapsedTime(&ms, e0, e1));
            own_ms += ms;
        }
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
        if (first) {
            if ((rc = weight_buffers(c)) || (rc = weighting_changed(c))) { publish(); return rc; }
        }
        if ((rc = launch_vce_rescale(*c, d_grp, d_out, ng, first))) { publish(); return rc; }
        FBA_HIP(hipStreamSynchronize(c->stream));
        c->weights_on = true;
        c->have_lin = false;  // neither the linearisation nor the factor belongs to the new weights
        c->have_factor = false;
        for (int g = 0; g < ng; ++g) comp[g] *= out[(size_t)VCE_OUT * g + 3];
    }
    // one plain step: the context as the loop leaves one with these weights (lin, delta, factor)
    double dsum = 0.0;
    rc = fba_step(ctx, &dsum);
    ++n_iter;
    publish();
    return rc;
}

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

// ---- Baarda data snooping over the image points (no reference counterpart) ----
namespace fba {
static const fba_snoop_options kSnoopDefaults{20, 2, 6, 0, 3.29, 0.05};
static int check_snoop_options(const char* who, const fba_snoop_options& op) {
    if (op.max_rounds < 1 || op.min_rays < 1 || op.min_img_points < 1 || !std::isfinite(op.crit) || !(op.crit > 0.0) ||
        !std::isfinite(op.max_share) || !(op.max_share > 0.0) || op.max_share > 1.0) {
        set_error(std::string(who) + ": max_rounds, min_rays and min_img_points >= 1; crit > 0 and 0 < max_share <= 1, both finite");
        return FBA_ERR_ARG;
    }
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

int fba_snoop(fba_ctx* ctx, const fba_snoop_options* o, uint8_t* excluded, double* stat, double* table, int32_t* rounds,
              int32_t* iterations, int32_t* converged, int32_t* status_bits) {
    Ctx* c = reinterpret_cast<Ctx*>(ctx);
    if (!c) { set_error("fba_snoop: NULL context"); return FBA_ERR_ARG; }
    if (c->pending) { set_error("fba_snoop between fba_solve_update_async and fba_solve_finish"); return FBA_ERR_ARG; }
    const fba_snoop_options& op = o ? *o : kSnoopDefaults;
    int rc;
    if ((rc = check_snoop_options("fba_snoop", op))) return rc;
    if (c->opt.world != 1) { set_error("fba_snoop is single-GPU (world == 1)"); return FBA_ERR_UNSUPPORTED; }
    if (c->loss != FBA_LOSS_NONE) {
        set_error("fba_snoop with a robust loss set: the w-test wants the residuals of a plain L2 adjustment");
        return FBA_ERR_UNSUPPORTED;
    }
    if (c->damp_on()) { set_error("fba_snoop with damping > 0: the factor of a damped solve is not that of N"); return FBA_ERR_UNSUPPORTED; }
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
        if (!c->weights_on && ((r = weight_buffers(c)) || (r = weighting_changed(c)))) return r;
        if ((r = launch_snoop_apply(*c, b, mode))) return r;
        FBA_HIP(hipStreamSynchronize(c->stream));
        c->weights_on = true;
        c->have_lin = false;  // neither the linearisation nor the factor belongs to the new weights
        c->have_factor = false;
        return FBA_OK;
    };
    if (n_excl > 0 && (rc = apply(0))) return rc;

    hipEvent_t e0 = nullptr, e1 = nullptr;  // events of the call's own: the steps in between use the context's
    if (c->timing) {
        FBA_HIP(hipEventCreate(&e0));
        if (hipEventCreate(&e1) != hipSuccess) { (void)hipEventDestroy(e0); set_error("fba_snoop: hipEventCreate failed"); return FBA_ERR_HIP; }
    }
    struct EvGuard {
        hipEvent_t a, b;
        ~EvGuard() { if (a) (void)hipEventDestroy(a); if (b) (void)hipEventDestroy(b); }
    } guard{e0, e1};

    int n_rounds = 0, n_iter = 0, conv = 0, bits = 0;
    double own_ms = 0.0;
    auto publish = [&]() -> int {
        if (rounds) *rounds = n_rounds;
        if (iterations) *iterations = n_iter;
        if (converged) *converged = conv;
        if (status_bits) *status_bits = bits;
        if (c->timing) {
            std::fill(c->last_ms, c->last_ms + 8, 0.0);
            c->last_ms[7] = own_ms;
        }
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
        int32_t it = 0;
        rc = fba_adjust(ctx, &it, nullptr);
        n_iter += it;
        if (rc) { (void)publish(); return rc; }
        if (!c->have_factor || !c->have_delta) { (void)publish(); set_error("fba_snoop: the last solve left no factor"); return FBA_ERR_ARG; }
        if (c->timing) (void)hipEventRecord(e0, c->stream);
        if ((rc = launch_vce_q(*c, nullptr, nullptr, d_q)) ||
            (rc = launch_snoop_round(*c, b, d_q, op.min_rays, op.min_img_points, op.crit))) {
            (void)publish();
            return rc;
        }
        if (c->timing) (void)hipEventRecord(e1, c->stream);
        FBA_HIP(hipMemcpyAsync(out, b.out, sizeof out, hipMemcpyDeviceToHost, c->stream));
        FBA_HIP(hipStreamSynchronize(c->stream));
        if (c->timing) {
            float ms = 0.f;
            FBA_HIP(hipEventElapsedTime(&ms, e0, e1));
            own_ms += ms;
        }
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
