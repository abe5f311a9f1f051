// fba_plan.cpp -- the host planning of fba_create: everything the kernels later take on trust.
//
// Validates the packed problem, then decides which rank owns which point, which tie points take the
// chunked fast path (k_lin_reduce) and which the general one (fba_general.hip), the order of the local
// points and observations, the chunk cuts, the accumulation plan (AccPlan: per chunk its pair keys,
// U-row terms and image keys; per pair / image / camera its partial slots, in chunk order -- the fixed
// summation order that makes S bit-reproducible), the general points' plan (GenPlan), the reduce-buffer
// layout of the multi-rank solves, the ownership masks and the prior tables.  Like fba_order.cpp this
// file makes no HIP call and links without the HIP runtime; fba_capi.cpp uploads the HostPlan it fills.
// tests/plan_check.cpp checks the plan against brute force on the CPU.
#include <algorithm>
#include <array>
#include <cmath>
#include <cstdio>
#include <map>
#include <tuple>

#include "fba_internal.h"

namespace fba {

static int64_t round_up(int64_t a, int64_t b) { return (a + b - 1) / b * b; }

static int check_settings(const fba_settings* s) {
    if (!s) { set_error("settings is NULL"); return FBA_ERR_ARG; }
    if (s->type < 0 || s->type > 4) { set_error("BuildAwG, invalid type in data.settings.type"); return FBA_ERR_TYPE; }
    if (s->num_radial < 1) {
        // BuildAwG.m:18-20 clamps a local copy to 1 but Buildxhat.m:13 does not: with 0 the reference
        // indexes an empty K (radial not estimated) or misaligns columns (estimated).
        set_error("Num_Radial_Distortions must be >= 1");
        return FBA_ERR_UNSUPPORTED;
    }
    if (s->num_radial > FBA_NK_MAX) { set_error("Num_Radial_Distortions > FBA_NK_MAX"); return FBA_ERR_UNSUPPORTED; }
    if (!(s->meas_std_x > 0) || !(s->meas_std_y > 0)) { set_error("Meas_std must be > 0"); return FBA_ERR_ARG; }
    if (s->inner_constraints &&
        !(s->est_Xc && s->est_Yc && s->est_Zc && s->est_omega && s->est_phi && s->est_kappa)) {
        // BuildAwG.m:525 writes 6 rows per image: the reference assumes all EOPs are estimated
        set_error("Inner_Constraints requires all six EOPs to be estimated (BuildAwG.m:525)");
        return FBA_ERR_UNSUPPORTED;
    }
    return FBA_OK;
}

// n_slots: internal image slots (the EXT images in camera order plus padding slots, fba_order.cpp)
static void compute_layout(const fba_problem* p, const fba_settings* s, Layout& L, int n_slots) {
    L.n_img = n_slots;
    L.n_img_ref = p->n_img;
    L.n_cam = p->n_cam;
    L.n_tie = p->n_tie;
    L.nk = s->num_radial;
    L.cw = 5 + L.nk;
    L.u_c = 6 * (int64_t)L.n_img + (int64_t)L.cw * L.n_cam;
    L.u_full = L.u_c + 3 * (int64_t)L.n_tie;
    L.n_pad = round_up(std::max<int64_t>(L.u_c, 1), NB);
    L.ld = L.n_pad;
    L.nrhs = s->inner_constraints ? 15 : 1;
    L.u_img = s->est_Xc + s->est_Yc + s->est_Zc + s->est_omega + s->est_phi + s->est_kappa;
    L.u_cam = s->est_c + s->est_xp + s->est_yp + s->est_radial * s->num_radial + s->est_decent * 2;
    L.u_ref = (int64_t)L.u_img * L.n_img_ref + (int64_t)L.u_cam * L.n_cam + 3 * (int64_t)L.n_tie;
}

int64_t count_unknowns(const fba_problem* p, const fba_settings* s) {
    return (int64_t)(s->est_Xc + s->est_Yc + s->est_Zc + s->est_omega + s->est_phi + s->est_kappa) * p->n_img +
           (int64_t)(s->est_c + s->est_xp + s->est_yp + s->est_radial * s->num_radial + s->est_decent * 2) * p->n_cam +
           3 * (int64_t)p->n_tie;
}

// full (internal) index -> the reference's xhat index.  Internal image slot e is EXT row img_ord[e]
// (-1: a padding slot, no reference unknowns).
static void full_to_ref_map(const fba_settings* s, const Layout& L, const std::vector<int32_t>& img_ord,
                            std::vector<int64_t>& map) {
    map.assign(L.u_full, -1);
    const int ee[6] = {s->est_Xc, s->est_Yc, s->est_Zc, s->est_omega, s->est_phi, s->est_kappa};
    for (int e = 0; e < L.n_img; ++e) {
        if (img_ord[e] < 0) continue;
        int cnt = 0;
        for (int a = 0; a < 6; ++a)
            if (ee[a]) map[6 * (int64_t)e + a] = (int64_t)img_ord[e] * L.u_img + cnt++;
    }
    std::vector<int> ce(L.cw, 0);
    ce[0] = s->est_xp;
    ce[1] = s->est_yp;
    ce[2] = s->est_c;
    for (int j = 0; j < L.nk; ++j) ce[3 + j] = s->est_radial;
    ce[3 + L.nk] = ce[4 + L.nk] = s->est_decent;
    for (int k = 0; k < L.n_cam; ++k) {
        int cnt = 0;
        for (int c = 0; c < L.cw; ++c)
            if (ce[c]) map[6 * (int64_t)L.n_img + (int64_t)k * L.cw + c] = (int64_t)L.u_img * L.n_img_ref + (int64_t)k * L.u_cam + cnt++;
    }
    const int64_t tb = (int64_t)L.u_img * L.n_img_ref + (int64_t)L.u_cam * L.n_cam;
    for (int64_t t = 0; t < 3 * (int64_t)L.n_tie; ++t) map[L.u_c + t] = tb + t;
}

static int check_problem(const fba_problem* p) {
    if (!p) { set_error("problem is NULL"); return FBA_ERR_ARG; }
    if (p->n_pts < 0 || p->n_img < 0 || p->n_cam < 0 || p->n_tie < 0) { set_error("negative size"); return FBA_ERR_ARG; }
    if (p->n_pts > 0 && (!p->xy || !p->img || !p->cam || !p->tie || !p->xyz_fixed)) {
        set_error("NULL observation array");
        return FBA_ERR_ARG;
    }
    if ((p->n_img > 0 && !p->eop0) || (p->n_cam > 0 && (!p->iop0 || !p->cam_info)) || (p->n_tie > 0 && !p->tie0)) {
        set_error("NULL parameter array");
        return FBA_ERR_ARG;
    }
    for (int k = 0; k < p->n_cam; ++k) {
        const double yd = p->cam_info[5 * k];
        if (yd != 1.0 && yd != -1.0) { set_error("y_dir should be +-1 only (main.m:334-337)"); return FBA_ERR_ARG; }
    }
    std::vector<int32_t> img_cam(p->n_img, -1);
    for (int64_t i = 0; i < p->n_pts; ++i) {
        const int e = p->img[i], k = p->cam[i], t = p->tie[i];
        if (e < 0 || e >= p->n_img) { set_error("image index out of range (EXT must list the images of .pho in order)"); return FBA_ERR_ARG; }
        if (k < 0 || k >= p->n_cam) { set_error("camera index out of range"); return FBA_ERR_ARG; }
        if (t < -1 || t >= p->n_tie) { set_error("tie index out of range"); return FBA_ERR_ARG; }
        // an image's camera is its EXT row's (main.m:323): every observation of it goes through that camera
        if (img_cam[e] < 0) img_cam[e] = k;
        else if (img_cam[e] != k) { set_error("observations of one image with different cameras"); return FBA_ERR_ARG; }
    }
    return FBA_OK;
}

// contiguous tie ranges balanced by observation count; control observations by contiguous ranges
void partition(const fba_problem* p, int world, std::vector<int32_t>& tie_owner, std::vector<int32_t>& ctl_owner) {
    tie_owner.assign(p->n_tie, 0);
    ctl_owner.assign(p->n_pts, -1);
    std::vector<int64_t> cnt(p->n_tie, 0);
    int64_t n_ctl = 0;
    for (int64_t i = 0; i < p->n_pts; ++i) {
        if (p->tie[i] >= 0) cnt[p->tie[i]]++;
        else n_ctl++;
    }
    const int64_t n_tie_obs = p->n_pts - n_ctl;
    int64_t acc = 0;
    for (int t = 0; t < p->n_tie; ++t) {
        // owner = floor(world * (obs before the middle of this point) / total)
        const int64_t mid2 = 2 * acc + cnt[t];
        int r = n_tie_obs > 0 ? (int)((mid2 * world) / (2 * n_tie_obs)) : 0;
        tie_owner[t] = std::min(std::max(r, 0), world - 1);
        acc += cnt[t];
    }
    int64_t q = 0;
    for (int64_t i = 0; i < p->n_pts; ++i) {
        if (p->tie[i] >= 0) continue;
        ctl_owner[i] = n_ctl > 0 ? (int32_t)std::min<int64_t>((q * world) / n_ctl, world - 1) : 0;
        ++q;
    }
}

int image_order(const fba_problem* p, std::vector<int32_t>& order) {
    if (p->n_img < 0 || (p->n_pts > 0 && (!p->img || !p->tie))) { set_error("bad problem"); return FBA_ERR_ARG; }
    for (int64_t i = 0; i < p->n_pts; ++i)
        if (p->img[i] < 0 || p->img[i] >= p->n_img || p->tie[i] < -1 || p->tie[i] >= p->n_tie) {
            set_error("image / tie index out of range");
            return FBA_ERR_ARG;
        }
    order = camera_order(p);
    return FBA_OK;
}

// fba_create_priors' list against the u unknowns of the reference layout
static int check_priors(const fba_priors* pr, int64_t u) {
    if (pr->n < 0 || !pr->index || !pr->value || !pr->sigma) { set_error("fba_create_priors: negative n or NULL array"); return FBA_ERR_ARG; }
    char buf[200];
    std::vector<int64_t> seen(pr->index, pr->index + pr->n);
    for (int64_t j = 0; j < pr->n; ++j) {
        if (pr->index[j] < 0 || pr->index[j] >= u) {
            snprintf(buf, sizeof buf, "fba_create_priors: index[%ld] = %ld is outside [0, %ld)", (long)j, (long)pr->index[j], (long)u);
            set_error(buf);
            return FBA_ERR_ARG;
        }
        if (!std::isfinite(pr->value[j])) {
            snprintf(buf, sizeof buf, "fba_create_priors: value[%ld] = %g must be finite", (long)j, pr->value[j]);
            set_error(buf);
            return FBA_ERR_ARG;
        }
        if (!std::isfinite(pr->sigma[j]) || !(pr->sigma[j] > 0.0)) {
            snprintf(buf, sizeof buf, "fba_create_priors: sigma[%ld] = %g must be finite and > 0", (long)j, pr->sigma[j]);
            set_error(buf);
            return FBA_ERR_ARG;
        }
    }
    std::sort(seen.begin(), seen.end());
    const auto dup = std::adjacent_find(seen.begin(), seen.end());
    if (dup != seen.end()) {
        snprintf(buf, sizeof buf, "fba_create_priors: duplicate index %ld (one prior per unknown)", (long)*dup);
        set_error(buf);
        return FBA_ERR_ARG;
    }
    return FBA_OK;
}

int check_inputs(const fba_problem* p, const fba_settings* s, const fba_options* o, const fba_priors** pr, fba_options& opt) {
    int rc = check_settings(s);
    if (rc) return rc;
    if ((rc = check_problem(p))) return rc;
    opt = fba_options{};
    opt.world = 1;
    if (o) opt = *o;
    if (opt.world < 1 || opt.rank < 0 || opt.rank >= opt.world) { set_error("bad rank/world"); return FBA_ERR_ARG; }
    if (*pr && (*pr)->n == 0) *pr = nullptr;
    if (*pr) {
        if ((rc = check_priors(*pr, count_unknowns(p, s)))) return rc;
        if (opt.world > 1 && opt.split) {
            set_error("fba_create_priors: priors are not implemented for the subtree split (fba_options.split); use the replicated solve");
            return FBA_ERR_UNSUPPORTED;
        }
    }
    return FBA_OK;
}

namespace {

// what the planning steps hand to one another (host only, dropped when build_plan returns)
struct Work {
    const fba_problem* p = nullptr;
    const fba_priors* pr = nullptr;
    std::vector<std::pair<int32_t, int32_t>> gp;  // the co-visible image pairs of ALL tie points (slots, e1 > e2)
    std::vector<int32_t> ctl_owner;               // [n_pts] rank of each control observation, -1: a tie observation
    std::vector<std::vector<int64_t>> tie_obs;    // [n_tie] PHO rows of each tie point, ascending
    std::vector<int32_t> tie_cam;                 // [n_tie] camera of its last observation
    std::vector<int32_t> lps, gps;                // this rank's regular / general tie points, local order
    int64_t o_gen0 = 0;                           // first general observation
    // the accumulation plan's lists, in the order they are keyed (chunks, then general points)
    std::vector<int32_t> ck_cam, ck_pk{0}, pk_t{0}, pk_term, ck_ik{0}, ik_o{0}, ik_obs, ck_tm, ik_img;
    std::vector<std::pair<int32_t, int32_t>> pk_key;
    std::vector<std::array<int32_t, 4>> tterm;    // (e1, e2, a, b) of the U-row chunks' terms, chunk order
    // the general points' lists (GenPlan)
    std::vector<int32_t> g_obs, g_gi{0}, g_gc{0}, gi_obs, gi_img, gi_gp, gi_gc, gc_cam, gc_gp, gc_o{0}, gc_list, gpk, gx, gkk;
    std::vector<int32_t> xt_start{0}, xt_list, xt_key, kt_start{0}, kt_list, kt_key;
};

int plan_bug(const char* what) {
    set_error(std::string("internal error in the accumulation plan: ") + what);
    return FBA_ERR_UNSUPPORTED;
}

// image order, unknown layout, initial parameters, and the factorisation schedule (fba_order.cpp)
void plan_layout(Ctx& c, Work& w) {
    const fba_problem* p = w.p;
    const fba_settings* s = &c.set;
    Layout& L = c.L;
    // camera-side order of the images: nested dissection with padding slots (fba_order.cpp)
    c.img_ord = camera_order(p);
    compute_layout(p, s, L, (int)c.img_ord.size());
    c.cam_tab_stride = cam_tab_row(L.cw);  // header | K_j | rmax^(2j) | rmax^-(2j)
    c.img_new.assign(L.n_img_ref, 0);
    for (int e = 0; e < L.n_img; ++e)
        if (c.img_ord[e] >= 0) c.img_new[c.img_ord[e]] = e;
    full_to_ref_map(s, L, c.img_ord, c.full_to_ref);
    c.ref_img_cam.assign(L.n_img_ref, -1);
    for (int64_t i = 0; i < p->n_pts; ++i) c.ref_img_cam[p->img[i]] = p->cam[i];

    // initial full-space parameters
    c.xfull0.assign(L.u_full, 0.0);
    for (int e = 0; e < L.n_img; ++e)
        if (c.img_ord[e] >= 0)
            for (int a = 0; a < 6; ++a) c.xfull0[6 * (int64_t)e + a] = p->eop0[6 * (int64_t)c.img_ord[e] + a];
    for (int64_t i = 0; i < (int64_t)L.cw * L.n_cam; ++i) c.xfull0[6 * (int64_t)L.n_img + i] = p->iop0[i];
    for (int64_t i = 0; i < 3 * (int64_t)L.n_tie; ++i) c.xfull0[L.u_c + i] = p->tie0[i];

    // the co-visible image pairs of ALL tie points (identical on every rank): the compact reduce
    // buffer of ranks > 1 and the block envelope of the reduced system
    std::vector<std::pair<int32_t, int32_t>>& gp = w.gp;
    std::vector<std::pair<int32_t, int32_t>> pi;  // (tie, internal image)
    for (int64_t i = 0; i < p->n_pts; ++i)
        if (p->tie[i] >= 0) pi.emplace_back(p->tie[i], c.img_new[p->img[i]]);
    std::sort(pi.begin(), pi.end());
    for (size_t a = 0; a < pi.size();) {
        size_t b = a;
        while (b < pi.size() && pi[b].first == pi[a].first) ++b;
        for (size_t x = a; x < b; ++x)
            for (size_t y = a; y < b; ++y)
                if (pi[x].second > pi[y].second) gp.emplace_back(pi[x].second, pi[y].second);
        a = b;
    }
    std::sort(gp.begin(), gp.end());
    gp.erase(std::unique(gp.begin(), gp.end()), gp.end());
    // inner constraints: the border is applied on the first n_loc image slots only (local
    // border), so M keeps the sparsity of S
    c.n_loc = s->inner_constraints ? std::min<int>(L.n_img, (int)(NB / 6)) : 0;
    build_schedule(c, gp);
}

// subtree split: a point's images lie on one root path of the elimination tree (every two of them
// share a block of S), so at most one rank's subtree: the point goes to that rank; points of top
// images only (and control observations of top images) go to the least loaded rank
void shard_split(Ctx& c, Work& w) {
    const fba_problem* p = w.p;
    const Layout& L = c.L;
    const std::vector<int32_t>& br = c.sched.blk_rank;
    auto img_rank = [&](int64_t e) {  // EXT image -> rank of its rows' subtree, or -1
        const int64_t slot = c.img_new[e];
        int r = -1;
        for (int64_t blk = 6 * slot / NB; blk <= (6 * slot + 5) / NB; ++blk) r = std::max(r, (int)br[blk]);
        return r;
    };
    std::vector<int64_t> load(c.opt.world, 0);
    std::vector<int32_t> tr(L.n_tie, -1);
    std::vector<int64_t> tcnt(L.n_tie, 0);
    for (int64_t i = 0; i < p->n_pts; ++i)
        if (p->tie[i] >= 0) {
            tr[p->tie[i]] = std::max(tr[p->tie[i]], img_rank(p->img[i]));
            tcnt[p->tie[i]]++;
        }
    c.tie_owner.assign(L.n_tie, 0);
    for (int t = 0; t < L.n_tie; ++t)
        if (tr[t] >= 0) { c.tie_owner[t] = tr[t]; load[tr[t]] += tcnt[t]; }
    for (int t = 0; t < L.n_tie; ++t)
        if (tr[t] < 0) {
            const int r = (int)(std::min_element(load.begin(), load.end()) - load.begin());
            c.tie_owner[t] = r;
            load[r] += tcnt[t];
        }
    w.ctl_owner.assign(p->n_pts, -1);
    for (int64_t i = 0; i < p->n_pts; ++i)
        if (p->tie[i] < 0) {
            int r = img_rank(p->img[i]);
            if (r < 0) r = (int)(std::min_element(load.begin(), load.end()) - load.begin());
            w.ctl_owner[i] = r;
            load[r]++;
        }
}

// this rank's tie points: regular (lps, in their final order) and general (gps)
int classify_points(Ctx& c, Work& w) {
    const fba_problem* p = w.p;
    const fba_priors* pr = w.pr;
    const Layout& L = c.L;
    std::vector<std::vector<int64_t>>& tie_obs = w.tie_obs;
    std::vector<int32_t>&tie_cam = w.tie_cam, &lps = w.lps, &gps = w.gps;
    // local tie points sorted by camera; their observations in PHO order
    tie_obs.assign(L.n_tie, {});
    tie_cam.assign(L.n_tie, 0);
    for (int64_t i = 0; i < p->n_pts; ++i)
        if (p->tie[i] >= 0) {
            tie_obs[p->tie[i]].push_back(i);
            tie_cam[p->tie[i]] = p->cam[i];
        }
    // regular tie points (k_lin_reduce's chunks): one camera, <= CHUNK_OBS observations, at most one per
    // image; the others are "general" points (fba_general.hip) -- the reference accepts all of them
    // a tie point that carries a prior is a general point too: its V and b take the prior's terms in
    // k_gen_point (k_lin_reduce forms and factors V per chunk and knows no priors)
    const int64_t ref_tie0 = (int64_t)L.u_img * L.n_img_ref + (int64_t)L.u_cam * L.n_cam;  // xhat index of the first tie unknown
    std::vector<uint8_t> has_prior(L.n_tie, 0);
    for (int64_t j = 0; pr && j < pr->n; ++j)
        if (pr->index[j] >= ref_tie0) {
            const int t = (int)((pr->index[j] - ref_tie0) / 3);
            if (tie_obs[t].empty()) {
                set_error("fba_create_priors: a prior on a tie point without observations");
                return FBA_ERR_UNSUPPORTED;
            }
            has_prior[t] = 1;
        }
    auto is_general = [&](int t) {
        const std::vector<int64_t>& ob = tie_obs[t];
        if (has_prior[t]) return true;
        if ((int64_t)ob.size() > CHUNK_OBS) return true;
        std::vector<int32_t> im;
        for (int64_t i : ob) {
            if (p->cam[i] != p->cam[ob[0]]) return true;
            im.push_back(p->img[i]);
        }
        std::sort(im.begin(), im.end());
        return std::adjacent_find(im.begin(), im.end()) != im.end();
    };
    for (int t = 0; t < L.n_tie; ++t)
        if (c.tie_owner[t] == c.opt.rank && !tie_obs[t].empty()) (is_general(t) ? gps : lps).push_back(t);
    // within a camera, points in Morton (Z-curve) order of their initial coordinates: the points two
    // co-visible images share -- and so the W/T and Jacobian rows a pair or an image gathers -- sit
    // close together in memory
    std::vector<uint64_t> zkey(L.n_tie, 0);
    {
        double lo[3] = {1e300, 1e300, 1e300}, hi[3] = {-1e300, -1e300, -1e300};
        for (int32_t t : lps)
            for (int d = 0; d < 3; ++d) {
                lo[d] = std::min(lo[d], p->tie0[3 * (int64_t)t + d]);
                hi[d] = std::max(hi[d], p->tie0[3 * (int64_t)t + d]);
            }
        auto spread = [](uint64_t v) {  // 21 bits -> every third bit
            v &= 0x1fffff;
            v = (v | v << 32) & 0x1f00000000ffffULL;
            v = (v | v << 16) & 0x1f0000ff0000ffULL;
            v = (v | v << 8) & 0x100f00f00f00f00fULL;
            v = (v | v << 4) & 0x10c30c30c30c30c3ULL;
            v = (v | v << 2) & 0x1249249249249249ULL;
            return v;
        };
        for (int32_t t : lps) {
            uint64_t k = 0;
            for (int d = 0; d < 3; ++d) {
                const double span = hi[d] > lo[d] ? hi[d] - lo[d] : 1.0;
                double f = (p->tie0[3 * (int64_t)t + d] - lo[d]) / span;
                f = std::isfinite(f) ? std::min(std::max(f, 0.0), 1.0) : 0.0;
                k |= spread((uint64_t)(f * 2097151.0)) << d;
            }
            zkey[t] = k;
        }
    }
    // default: lexicographic order of the points' (sorted) image sets -- consecutive points share most
    // of their co-visible pairs, so the rows k_pairs gathers for one pair sit close together
    std::vector<std::vector<int32_t>> iset(L.n_tie);
    for (int32_t t : lps) {
        for (int64_t i : tie_obs[t]) iset[t].push_back(c.img_new[p->img[i]]);
        std::sort(iset[t].begin(), iset[t].end());
    }
    std::stable_sort(lps.begin(), lps.end(), [&](int32_t a, int32_t b) {
        if (tie_cam[a] != tie_cam[b]) return tie_cam[a] < tie_cam[b];
        if (iset[a] != iset[b]) return iset[a] < iset[b];
        return zkey[a] < zkey[b];
    });
    c.n_lp = (int64_t)lps.size();
    return FBA_OK;
}

// the local observation order: [regular tie points | control | general points]
int order_observations(Ctx& c, Work& w, HostPlan& hp) {
    const fba_problem* p = w.p;
    std::vector<int64_t>& pho = c.obs_pho;
    pho.reserve(p->n_pts);  // (an upper bound: the rank's share of the PHO rows)
    hp.xy.reserve(2 * p->n_pts);
    hp.img.reserve(p->n_pts);
    hp.cam.reserve(p->n_pts);
    hp.pt.reserve(p->n_pts);
    auto add = [&](int64_t i, int32_t point) {
        pho.push_back(i);
        hp.xy.push_back(p->xy[2 * i]);
        hp.xy.push_back(p->xy[2 * i + 1]);
        hp.img.push_back(c.img_new[p->img[i]]);
        hp.cam.push_back(p->cam[i]);
        hp.pt.push_back(point);
    };
    hp.lp_start.push_back(0);
    for (int64_t lp = 0; lp < c.n_lp; ++lp) {
        const int t = w.lps[lp];
        for (int64_t i : w.tie_obs[t]) add(i, (int32_t)lp);
        hp.lp_start.push_back((int32_t)pho.size());
        hp.lp_cam.push_back(w.tie_cam[t]);
    }
    c.n_obs_tie = (int64_t)pho.size();
    // control observations of this rank, sorted by camera (stable in PHO order)
    std::vector<int64_t> ctls;
    for (int64_t i = 0; i < p->n_pts; ++i)
        if (p->tie[i] < 0 && w.ctl_owner[i] == c.opt.rank) ctls.push_back(i);
    std::stable_sort(ctls.begin(), ctls.end(), [&](int64_t a, int64_t b) { return p->cam[a] < p->cam[b]; });
    for (size_t q = 0; q < ctls.size(); ++q) {
        const int64_t i = ctls[q];
        add(i, -1 - (int32_t)q);
        for (int m = 0; m < 3; ++m) hp.ctl.push_back(p->xyz_fixed[3 * i + m]);
    }
    // the general points' observations, after the control observations: each point's contiguous,
    // sorted by image slot (then PHO row)
    w.o_gen0 = (int64_t)pho.size();
    w.g_obs.push_back((int32_t)w.o_gen0);
    for (size_t q = 0; q < w.gps.size(); ++q) {
        std::vector<int64_t> ob = w.tie_obs[w.gps[q]];
        std::stable_sort(ob.begin(), ob.end(), [&](int64_t a, int64_t b) { return c.img_new[p->img[a]] < c.img_new[p->img[b]]; });
        for (int64_t i : ob) add(i, (int32_t)(c.n_lp + (int64_t)q));
        w.g_obs.push_back((int32_t)pho.size());
    }
    c.n_obs = (int64_t)pho.size();
    if (c.n_obs >= (int64_t)1 << 31) { set_error("too many observations per rank"); return FBA_ERR_UNSUPPORTED; }
    c.n_obs_pad = round_up(std::max<int64_t>(c.n_obs, 1), 64);
    c.n_lp_pad = round_up(std::max<int64_t>(c.n_lp, 1), 64);
    return FBA_OK;
}

// chunks (one k_lin_reduce / k_lin_point workgroup each): consecutive whole tie points of one
// camera, <= CHUNK_OBS observations and <= chunk_pts(nK) points, then control observations of one
// camera, <= CHUNK_OBS at a time
void cut_chunks(Ctx& c, const Work& w, HostPlan& hp) {
    const Layout& L = c.L;
    const std::vector<int32_t>&lp_start = hp.lp_start, &lp_cam = hp.lp_cam, &cam = hp.cam;
    std::vector<int32_t>&chunk_obs = hp.chunk_obs, &chunk_pt = hp.chunk_pt;
    chunk_obs.assign(1, 0);
    chunk_pt.assign(1, 0);
    int64_t cur_terms = 0;
    for (int64_t lp = 0; lp < c.n_lp; ++lp) {
        const int64_t n_lp_obs = lp_start[lp + 1] - lp_start[lp];
        const int64_t lp_terms = n_lp_obs * (n_lp_obs - 1) / 2;
        const bool split = lp > chunk_pt.back() &&
                           (lp_start[lp + 1] - chunk_obs.back() > CHUNK_OBS || lp - chunk_pt.back() >= chunk_pts(L.nk) ||
                            lp_cam[lp] != lp_cam[lp - 1] || cur_terms + lp_terms > chunk_terms(L.nk));
        if (split) {
            chunk_obs.push_back(lp_start[lp]);
            chunk_pt.push_back((int32_t)lp);
            cur_terms = 0;
        }
        cur_terms += lp_terms;
    }
    if (c.n_lp > 0) {
        chunk_obs.push_back(lp_start[c.n_lp]);
        chunk_pt.push_back((int32_t)c.n_lp);
    }
    for (int64_t o = c.n_obs_tie; o < w.o_gen0;) {
        int64_t e = o + 1;
        while (e < w.o_gen0 && e - o < CHUNK_OBS && cam[e] == cam[o]) ++e;
        chunk_obs.push_back((int32_t)e);
        chunk_pt.push_back((int32_t)c.n_lp);
        o = e;
    }
    c.n_chunks_lr = (int64_t)chunk_obs.size() - 1;
    // the general observations: linearised by k_lin_point only (empty point range), CHUNK_OBS at a time
    for (int64_t o = w.o_gen0; o < c.n_obs;) {
        const int64_t e = std::min<int64_t>(o + CHUNK_OBS, c.n_obs);
        chunk_obs.push_back((int32_t)e);
        chunk_pt.push_back((int32_t)c.n_lp);
        o = e;
    }
    c.n_chunks = (int64_t)chunk_obs.size() - 1;
}

// accumulation plan (k_lin_reduce), per chunk: its co-visible pair keys with their (i, j) observation
// terms -- or its U-row terms -- and its image keys with their observations.
// A chunk's pair terms take the U-row path (AccPlan::ck_tm) when its pair keys hold at most tm_ratio
// terms each on average: a partial row costs 288 B written and read back per key, the U-row path
// one 144-B U row per observation plus two cached U-row reads per term (PlanKnobs::pair_terms: the
// ratio; 0 = never, tested both ways in tests/test_gpu_parity.py)
int plan_chunk_keys(Ctx& c, Work& w, const HostPlan& hp, double tm_ratio) {
    const std::vector<int32_t>&img = hp.img, &cam = hp.cam, &lp_start = hp.lp_start;
    for (int64_t ch = 0; ch < c.n_chunks_lr; ++ch) {
        const int o0 = hp.chunk_obs[ch], o1 = hp.chunk_obs[ch + 1];
        w.ck_cam.push_back(cam[o0]);
        std::vector<std::tuple<int32_t, int32_t, int32_t>> tk;  // (e1, e2, term), e1 > e2, point order
        for (int32_t lp = hp.chunk_pt[ch]; lp < hp.chunk_pt[ch + 1]; ++lp)
            for (int i = lp_start[lp]; i < lp_start[lp + 1]; ++i)
                for (int j = lp_start[lp]; j < lp_start[lp + 1]; ++j) {
                    if (img[i] == img[j]) {
                        if (i != j) return plan_bug("a regular point holds two observations of one image");
                        continue;
                    }
                    if (img[i] > img[j]) tk.emplace_back(img[i], img[j], (i - o0) | ((j - o0) << 16));
                }
        std::stable_sort(tk.begin(), tk.end(), [](const auto& x, const auto& y) {
            return std::get<0>(x) != std::get<0>(y) ? std::get<0>(x) < std::get<0>(y) : std::get<1>(x) < std::get<1>(y);
        });
        // the chunk's pair keys, most terms first: the threads of a wave then run similar trip counts
        std::vector<std::pair<size_t, size_t>> kr;  // [begin, end) in tk
        for (size_t q = 0; q < tk.size(); ++q)
            if (q == 0 || std::get<0>(tk[q]) != std::get<0>(tk[q - 1]) || std::get<1>(tk[q]) != std::get<1>(tk[q - 1]))
                kr.emplace_back(q, q + 1);
            else
                kr.back().second = q + 1;
        std::stable_sort(kr.begin(), kr.end(), [](const auto& x, const auto& y) { return x.second - x.first > y.second - y.first; });
        const bool tmode = !kr.empty() && (double)tk.size() <= tm_ratio * (double)kr.size();
        w.ck_tm.push_back(tmode ? 1 : 0);
        if (tmode) {
            for (size_t q = 0; q < tk.size(); ++q) {  // (e1, e2) ascending, point order within a key
                const int32_t tm = std::get<2>(tk[q]);
                w.tterm.push_back({std::get<0>(tk[q]), std::get<1>(tk[q]), o0 + (tm & 0xffff), o0 + (tm >> 16)});
            }
        } else {
            for (auto& r : kr) {
                w.pk_key.emplace_back(std::get<0>(tk[r.first]), std::get<1>(tk[r.first]));
                for (size_t q = r.first; q < r.second; ++q) w.pk_term.push_back(std::get<2>(tk[q]));
                w.pk_t.push_back((int32_t)w.pk_term.size());
            }
        }
        w.ck_pk.push_back((int32_t)w.pk_key.size());
        std::vector<std::pair<int32_t, int32_t>> io;  // (image, local obs)
        for (int o = o0; o < o1; ++o) io.emplace_back(img[o], o - o0);
        std::sort(io.begin(), io.end());
        for (size_t q = 0; q < io.size(); ++q) {
            if (q == 0 || io[q].first != io[q - 1].first) {
                if (q > 0) w.ik_o.push_back((int32_t)w.ik_obs.size());
                w.ik_img.push_back(io[q].first);
            }
            w.ik_obs.push_back(io[q].second);
        }
        if (!io.empty()) w.ik_o.push_back((int32_t)w.ik_obs.size());
        w.ck_ik.push_back((int32_t)w.ik_img.size());
    }
    // image-key lanes of k_lin_reduce: 4 when the chunks' image keys hold <= 2 observations on average
    c.ik_lanes = (w.ck_ik.back() > 0 && w.ik_obs.size() <= 2 * (size_t)w.ck_ik.back()) ? 4 : 8;
    return FBA_OK;
}

// general points: gimg / gpc groups and their keys, appended after the chunks' keys
void plan_general(Ctx& c, Work& w, const HostPlan& hp) {
    const std::vector<int32_t>&img = hp.img, &cam = hp.cam;
    GenPlan& G = c.gen;
    G.n_gp = (int64_t)w.gps.size();
    G.lp0 = c.n_lp;
    G.pk0 = (int64_t)w.pk_key.size();
    G.ik0 = (int64_t)w.ik_img.size();
    G.ck0 = c.n_chunks_lr;
    std::vector<int32_t>&gi_obs = w.gi_obs, &gi_img = w.gi_img, &gc_cam = w.gc_cam, &gc_list = w.gc_list, &gx = w.gx, &gkk = w.gkk;
    std::map<std::pair<int32_t, int32_t>, std::vector<int32_t>> xt, kt;  // target block -> slots, ascending
    for (int64_t q = 0; q < G.n_gp; ++q) {
        const int a = w.g_obs[q], b = w.g_obs[q + 1];
        const int gi0 = (int)gi_img.size(), gc0 = (int)gc_cam.size();
        for (int o = a; o < b; ++o)
            if (o == a || img[o] != img[o - 1]) {
                gi_obs.push_back(o);
                gi_img.push_back(img[o]);
                w.gi_gp.push_back((int32_t)q);
            }
        std::vector<int32_t> cams;
        for (int o = a; o < b; ++o) cams.push_back(cam[o]);
        std::sort(cams.begin(), cams.end());
        cams.erase(std::unique(cams.begin(), cams.end()), cams.end());
        for (int32_t k : cams) {
            gc_cam.push_back(k);
            w.gc_gp.push_back((int32_t)q);
            for (int o = a; o < b; ++o)
                if (cam[o] == k) gc_list.push_back(o);
            w.gc_o.push_back((int32_t)gc_list.size());
        }
        const int gi1 = (int)gi_img.size(), gc1 = (int)gc_cam.size();
        for (int i = gi0; i < gi1; ++i) {
            const int32_t own = cam[gi_obs[i]];
            for (int k = gc0; k < gc1; ++k) {
                if (gc_cam[k] == own) w.gi_gc.push_back(k);
                else {  // image i x another camera of the point
                    xt[{gi_img[i], gc_cam[k]}].push_back((int32_t)(gx.size() / 2));
                    gx.push_back(i);
                    gx.push_back(k);
                }
            }
            for (int j = gi0; j < i; ++j) {  // images ascending: gimg i is the higher image
                w.gpk.push_back(i);
                w.gpk.push_back(j);
                w.pk_key.emplace_back(gi_img[i], gi_img[j]);
            }
            w.ik_img.push_back(gi_img[i]);
        }
        for (int k1 = gc0; k1 < gc1; ++k1) {
            w.ck_cam.push_back(gc_cam[k1]);  // camera partial slot ck0 + gpc
            for (int k2 = gc0; k2 < k1; ++k2) {  // cameras ascending: k1 the higher camera
                kt[{gc_cam[k1], gc_cam[k2]}].push_back((int32_t)(gkk.size() / 2));
                gkk.push_back(k1);
                gkk.push_back(k2);
            }
        }
        w.g_gi.push_back(gi1);
        w.g_gc.push_back(gc1);
    }
    gi_obs.push_back((int32_t)c.n_obs);
    G.n_gi = (int64_t)gi_img.size();
    G.n_gc = (int64_t)gc_cam.size();
    G.n_gpk = (int64_t)w.gpk.size() / 2;
    G.n_gx = (int64_t)gx.size() / 2;
    G.n_gkk = (int64_t)gkk.size() / 2;
    for (auto& e : xt) {
        w.xt_key.push_back(e.first.first);
        w.xt_key.push_back(e.first.second);
        w.xt_list.insert(w.xt_list.end(), e.second.begin(), e.second.end());
        w.xt_start.push_back((int32_t)w.xt_list.size());
    }
    for (auto& e : kt) {
        w.kt_key.push_back(e.first.first);
        w.kt_key.push_back(e.first.second);
        w.kt_list.insert(w.kt_list.end(), e.second.begin(), e.second.end());
        w.kt_start.push_back((int32_t)w.kt_list.size());
    }
    G.n_xt = (int64_t)xt.size();
    G.n_kt = (int64_t)kt.size();
}

// per pair / image / camera the partial slots the reduce kernels add up, in chunk order; then every
// list of both plans packed into HostPlan::acc (the offsets in Ctx::acc / Ctx::gen)
void plan_slots(Ctx& c, const Work& w, HostPlan& hp) {
    const Layout& L = c.L;
    AccPlan& A = c.acc;
    GenPlan& G = c.gen;
    const std::vector<std::pair<int32_t, int32_t>>& pk_key = w.pk_key;
    const std::vector<std::array<int32_t, 4>>& tterm = w.tterm;
    // the local co-visible pairs and, per pair, its partial slots
    std::vector<std::pair<int32_t, int32_t>> lpairs(pk_key);
    for (auto& t : tterm) lpairs.emplace_back(t[0], t[1]);
    std::sort(lpairs.begin(), lpairs.end());
    lpairs.erase(std::unique(lpairs.begin(), lpairs.end()), lpairs.end());
    c.n_pairs = (int64_t)lpairs.size();
    c.n_pair_terms = (int64_t)(w.pk_term.size() + tterm.size());
    // the U-row terms per pair (counting sort by pair: chunk order kept)
    std::vector<int32_t> tp_start(c.n_pairs + 1, 0), tp_ab(2 * tterm.size());
    {
        std::vector<int32_t> pid(tterm.size());
        for (size_t q = 0; q < tterm.size(); ++q) {
            pid[q] = (int32_t)(std::lower_bound(lpairs.begin(), lpairs.end(), std::make_pair(tterm[q][0], tterm[q][1])) -
                               lpairs.begin());
            tp_start[pid[q] + 1]++;
        }
        for (int64_t q = 0; q < c.n_pairs; ++q) tp_start[q + 1] += tp_start[q];
        std::vector<int32_t> fill(tp_start.begin(), tp_start.end() - 1);
        for (size_t q = 0; q < tterm.size(); ++q) {
            const int32_t x = fill[pid[q]]++;
            tp_ab[2 * x] = tterm[q][2];
            tp_ab[2 * x + 1] = tterm[q][3];
        }
    }
    std::vector<int32_t> rp_start(c.n_pairs + 1, 0), rp_list(pk_key.size()), rp_e;
    {
        std::vector<int32_t> pid(pk_key.size());
        for (size_t q = 0; q < pk_key.size(); ++q) {
            pid[q] = (int32_t)(std::lower_bound(lpairs.begin(), lpairs.end(), pk_key[q]) - lpairs.begin());
            rp_start[pid[q] + 1]++;
        }
        for (int64_t q = 0; q < c.n_pairs; ++q) rp_start[q + 1] += rp_start[q];
        std::vector<int32_t> fill(rp_start.begin(), rp_start.end() - 1);
        for (size_t q = 0; q < pk_key.size(); ++q) rp_list[fill[pid[q]]++] = (int32_t)q;
        for (auto& q : lpairs) { rp_e.push_back(q.first); rp_e.push_back(q.second); }
    }
    std::vector<int32_t> ri_start(L.n_img + 1, 0), ri_list(w.ik_img.size()), img_cam(L.n_img, -1);
    {
        for (int32_t e : w.ik_img) ri_start[e + 1]++;
        for (int e = 0; e < L.n_img; ++e) ri_start[e + 1] += ri_start[e];
        std::vector<int32_t> fill(ri_start.begin(), ri_start.end() - 1);
        for (size_t q = 0; q < w.ik_img.size(); ++q) ri_list[fill[w.ik_img[q]]++] = (int32_t)q;
        for (int64_t o = 0; o < c.n_obs; ++o) img_cam[hp.img[o]] = hp.cam[o];
    }
    // camera partial slots: the chunks', then one per general point-camera group (ck_cam covers both)
    std::vector<int32_t> rc_start(L.n_cam + 1, 0), rc_list(w.ck_cam.size());
    {
        for (int32_t k : w.ck_cam) rc_start[k + 1]++;
        for (int k = 0; k < L.n_cam; ++k) rc_start[k + 1] += rc_start[k];
        std::vector<int32_t> fill(rc_start.begin(), rc_start.end() - 1);
        for (size_t ch = 0; ch < w.ck_cam.size(); ++ch) rc_list[fill[w.ck_cam[ch]]++] = (int32_t)ch;
    }
    A.n_pk = (int64_t)pk_key.size();
    A.n_ik = (int64_t)w.ik_img.size();
    A.n_tt = (int64_t)tterm.size();
    // every list, in the order the offsets have always had
    std::vector<int32_t> pk_slot(rp_list.size()), ik_slot(ri_list.size());
    for (size_t x = 0; x < rp_list.size(); ++x) pk_slot[rp_list[x]] = (int32_t)x;
    for (size_t x = 0; x < ri_list.size(); ++x) ik_slot[ri_list[x]] = (int32_t)x;
    const std::pair<int64_t*, const std::vector<int32_t>*> lists[] = {
        {&A.ck_cam, &w.ck_cam}, {&A.ck_pk, &w.ck_pk}, {&A.pk_t, &w.pk_t}, {&A.pk_term, &w.pk_term}, {&A.ck_ik, &w.ck_ik},
        {&A.ik_o, &w.ik_o}, {&A.ik_obs, &w.ik_obs}, {&A.rp_start, &rp_start}, {&A.rp_e, &rp_e}, {&A.rp_list, &rp_list},
        {&A.ri_start, &ri_start}, {&A.ri_list, &ri_list}, {&A.pk_slot, &pk_slot}, {&A.ik_slot, &ik_slot}, {&A.img_cam, &img_cam},
        {&A.rc_start, &rc_start}, {&A.rc_list, &rc_list}, {&A.ck_tm, &w.ck_tm}, {&A.tp_start, &tp_start}, {&A.tp_ab, &tp_ab},
        {&G.g_obs, &w.g_obs}, {&G.g_gi, &w.g_gi}, {&G.g_gc, &w.g_gc}, {&G.gi_obs, &w.gi_obs}, {&G.gi_img, &w.gi_img},
        {&G.gi_gp, &w.gi_gp}, {&G.gi_gc, &w.gi_gc}, {&G.gc_cam, &w.gc_cam}, {&G.gc_gp, &w.gc_gp}, {&G.gc_o, &w.gc_o},
        {&G.gc_list, &w.gc_list}, {&G.gpk, &w.gpk}, {&G.gx, &w.gx}, {&G.gkk, &w.gkk}, {&G.xt_start, &w.xt_start},
        {&G.xt_list, &w.xt_list}, {&G.xt_key, &w.xt_key}, {&G.kt_start, &w.kt_start}, {&G.kt_list, &w.kt_list}, {&G.kt_key, &w.kt_key}};
    std::vector<int32_t>& abuf = hp.acc;
    size_t total = 0;
    for (auto& l : lists) total += l.second->size();
    abuf.reserve(total);
    for (auto& l : lists) {
        *l.first = (int64_t)abuf.size();
        abuf.insert(abuf.end(), l.second->begin(), l.second->end());
    }
    G.pk_slot = A.pk_slot;
    G.ik_slot = A.ik_slot;
}

// the reduce buffer of the multi-rank solves, and which full-space entries are estimated / owned / counted
void plan_ranks(Ctx& c, const Work& w, HostPlan& hp) {
    const Layout& L = c.L;
    const int rank = c.opt.rank;
    const bool split = c.sched.split;
    if (c.opt.world > 1 && !split) {
        for (auto& q : w.gp) { hp.gpairs.push_back(q.first); hp.gpairs.push_back(q.second); }
        c.n_gpairs = (int64_t)w.gp.size();
        c.n_red = 36 * (c.n_gpairs + L.n_img) + (int64_t)L.cw * L.n_cam * L.n_pad + L.n_pad;
    }
    // subtree split: the reduce buffer's layout (k_pack_split) and the per-block roles
    std::vector<int8_t>&bown = hp.bown, &rown = hp.rown;
    if (split) {
        const Sched& sc = c.sched;
        const int64_t nb = L.n_pad / NB;
        bown.assign(nb, 0);
        for (int64_t k = 0; k < nb; ++k) bown[k] = sc.blk_rank[k] < 0 ? 2 : (sc.blk_rank[k] == rank ? 1 : 0);
        rown.assign(L.n_pad, 0);
        for (int64_t i = 0; i < L.n_pad; ++i) {
            rown[i] = bown[i / NB];
            if (i < 6 * (int64_t)L.n_img && c.img_ord[i / 6] >= 0) {
                int r = -1;  // the rank of the image's subtree (any of its rows in one), -1 wholly top
                for (int64_t blk = 6 * (i / 6) / NB; blk <= (6 * (i / 6) + 5) / NB; ++blk) r = std::max(r, (int)sc.blk_rank[blk]);
                rown[i] = r < 0 ? 2 : (r == rank ? 1 : 0);
            }
        }
        int64_t n = 0, ng = 0;
        for (int q = 0; q < sc.n_top_blocks; ++q) n += (int64_t)(sc.buf[sc.top_blocks + 2 * q] == nb ? L.nrhs : NB) * NB;
        for (int64_t i = 0; i < 6 * (int64_t)L.n_img; ++i)
            if (rown[i] == 2) hp.topdiag.push_back((int32_t)i);
        for (int64_t k = 0; k < nb; ++k) ng += bown[k] != 2;
        c.n_topdiag = (int64_t)hp.topdiag.size();
        c.red_diag = n;
        c.red_gblk = c.red_diag + c.n_topdiag;
        c.red_w = c.red_gblk + 256 * ng;
        c.n_red = c.red_w + 9;  // 7 weight sums, the abort flag, the pivot-failure row
    }
    hp.active.assign(L.n_pad, 0);
    hp.counted.assign(L.u_full, 0);
    c.full_owned.assign(L.u_full, 0);
    for (int64_t i = 0; i < L.u_c; ++i) {
        hp.active[i] = c.full_to_ref[i] >= 0 ? 1 : 0;
        // (split: this rank's subtree rows, and the top rows on rank 0)
        const bool mine = split ? (bown[i / NB] == 1 || (bown[i / NB] == 2 && rank == 0)) : rank == 0;
        hp.counted[i] = (mine && hp.active[i]) ? 1 : 0;
        c.full_owned[i] = mine ? 1 : 0;
    }
    for (int t = 0; t < L.n_tie; ++t)
        for (int m = 0; m < 3; ++m) {
            const int64_t i = L.u_c + 3 * (int64_t)t + m;
            hp.counted[i] = c.tie_owner[t] == rank ? 1 : 0;
            c.full_owned[i] = hp.counted[i];
        }
}

// priors: the tables of the ones this rank adds -- camera-side on rank 0 (k_prior_cam), a tie point's on
// its owner (k_gen_point's per-point table), all of them for the residuals (k_prior_resid)
void plan_priors(Ctx& c, const Work& w, HostPlan& hp) {
    const fba_priors* pr = w.pr;
    const Layout& L = c.L;
    c.n_prior = pr->n;
    std::vector<int64_t> ref_to_full(L.u_ref, -1);
    for (int64_t i = 0; i < L.u_full; ++i)
        if (c.full_to_ref[i] >= 0) ref_to_full[c.full_to_ref[i]] = i;
    std::vector<int32_t> gp_of(L.n_tie, -1);
    for (size_t q = 0; q < w.gps.size(); ++q) gp_of[w.gps[q]] = (int32_t)q;
    const int64_t cb = 6 * (int64_t)L.n_img;
    const int stride = c.cam_tab_stride;
    for (int64_t j = 0; j < pr->n; ++j) {
        const int64_t i = ref_to_full[pr->index[j]];
        const double pw = 1.0 / (pr->sigma[j] * pr->sigma[j]);
        if (i < L.u_c) {
            if (c.opt.rank != 0) continue;
            int so = -1;  // the distortion unknowns' scale in the camera table: rmax^(2j) for K_j, rmax^2 for P
            if (i >= cb) {
                const int k = (int)((i - cb) / L.cw), q = (int)((i - cb) % L.cw);
                if (q >= 3 && q < 3 + L.nk) so = k * stride + CAM_TAB_HDR + L.nk + (q - 3);
                else if (q >= 3 + L.nk) so = k * stride + 6;
            }
            hp.pc_idx.push_back((int32_t)i);
            hp.pc_idx.push_back(so);
            hp.pc_val.push_back(pw);
            hp.pc_val.push_back(pr->value[j]);
        } else {
            const int t = (int)((i - L.u_c) / 3), d = (int)((i - L.u_c) % 3);
            if (gp_of[t] < 0) continue;  // another rank's point
            if (hp.gprior.empty()) hp.gprior.assign(6 * w.gps.size(), 0.0);
            hp.gprior[6 * (size_t)gp_of[t] + d] = pw;
            hp.gprior[6 * (size_t)gp_of[t] + 3 + d] = pr->value[j];
        }
        hp.pr_idx.push_back(i);
        hp.pr_idx.push_back(j);
        hp.pr_val.push_back(pw);
        hp.pr_val.push_back(pr->value[j]);
    }
    c.n_pcam = (int64_t)hp.pc_idx.size() / 2;
    c.n_pres = (int64_t)hp.pr_idx.size() / 2;
}

}  // namespace

void build_image_list(const std::vector<int32_t>& img, int n_img, std::vector<int32_t>& start, std::vector<int32_t>& list) {
    const int32_t ni = std::max(n_img, 0);
    start.assign((size_t)ni + 1, 0);
    for (int32_t e : img)
        if (e >= 0 && e < ni) ++start[(size_t)e + 1];
    for (int32_t e = 0; e < ni; ++e) start[(size_t)e + 1] += start[e];
    list.assign((size_t)start[ni], 0);
    std::vector<int32_t> next(start.begin(), start.end() - 1);
    for (size_t o = 0; o < img.size(); ++o)
        if (img[o] >= 0 && img[o] < ni) list[(size_t)next[img[o]]++] = (int32_t)o;
}

// the same stable counting sort, keyed by the local tie point: a control observation (pt < 0) is in no list
void build_point_list(const std::vector<int32_t>& pt, int n_lp, std::vector<int32_t>& start, std::vector<int32_t>& list) {
    build_image_list(pt, n_lp, start, list);
}

int build_plan(const fba_problem* p, const fba_settings* s, const fba_options& opt, const fba_priors* pr,
               const PlanKnobs& knobs, Ctx& c, HostPlan& hp) {
    c.prob = *p;
    c.set = *s;
    c.opt = opt;
    c.n_pts = p->n_pts;
    Work w;
    w.p = p;
    w.pr = pr;
    plan_layout(c, w);
    if (c.sched.split) shard_split(c, w);
    else partition(p, opt.world, c.tie_owner, w.ctl_owner);
    int rc;
    if ((rc = classify_points(c, w)) || (rc = order_observations(c, w, hp))) return rc;
    cut_chunks(c, w, hp);
    if ((rc = plan_chunk_keys(c, w, hp, knobs.pair_terms))) return rc;
    plan_general(c, w, hp);
    plan_slots(c, w, hp);
    plan_ranks(c, w, hp);
    hp.lp_tie.assign(w.lps.begin(), w.lps.end());
    hp.lp_tie.insert(hp.lp_tie.end(), w.gps.begin(), w.gps.end());
    hp.caminfo.assign(p->cam_info, p->cam_info + 5 * (size_t)c.L.n_cam);
    // k_lin_reduce reads the observation's point coordinates at xfull[xoff] (one gather level fewer than
    // pt -> lp_tie -> xfull, so the next chunk's inputs can be in flight behind the current chunk)
    hp.xoff.assign(hp.pt.size(), 0);
    for (size_t o = 0; o < hp.pt.size(); ++o)
        if (hp.pt[o] >= 0) hp.xoff[o] = (int32_t)(c.L.u_c + 3 * (int64_t)hp.lp_tie[hp.pt[o]]);
    if (pr) plan_priors(c, w, hp);
    return FBA_OK;
}

}  // namespace fba
