// plan_check.cpp -- host-only check of fba_create's planning (fish-eye_bundle_adjustment_amd/csrc/fba_plan.cpp),
// built and run by tests/test_plan.py (no GPU needed).
//
// Small scenes are built here, build_plan() runs on them for every rank, and what it hands to the kernels
// -- the observation order, the chunk cuts, the accumulation plan (AccPlan), the general points' plan
// (GenPlan), the reduce-buffer layout and the ownership masks -- is verified against brute force computed
// from the problem arrays alone.  The lists are read the way the kernels read them: through the offsets of
// Ctx::acc / Ctx::gen into HostPlan::acc.
//
//   plan_check            every scene; prints one "ok <scene> ..." line each, or "FAIL <scene>: <what>"
//   plan_check <scene>    that scene only
#include <algorithm>
#include <array>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <random>
#include <set>

#include "../fish-eye_bundle_adjustment_amd/csrc/fba_internal.h"

using namespace fba;

static int fail_at(const char* what, int line) {
    printf("FAIL line %d: %s\n", line, what);
    return 1;
}
#define CHECK(cond)                                    \
    do {                                               \
        if (!(cond)) return fail_at(#cond, __LINE__); \
    } while (0)

typedef std::array<int32_t, 4> Term;  // (e1, e2, obs in e1, obs in e2), observations in the rank's local order

struct Scene {
    int n_img = 0, n_cam = 1, n_tie = 0, nk = 3;
    std::vector<int32_t> img, cam, tie, img_cam;
    std::vector<double> xy, xyzf, eop, tie0;
    std::vector<int64_t> pr_index;  // priors (reference xhat indices), sigma 0.5 each
    std::mt19937_64 rng{7};
    void images(int n, int cams = 1) {  // the first half of the images through camera 0, the rest through camera 1
        n_img = n;
        n_cam = cams;
        for (int e = 0; e < n; ++e) {
            img_cam.push_back(cams == 1 ? 0 : (e < n / 2 ? 0 : 1));
            const double v[6] = {100.0 * (e % 20), 100.0 * (e / 20), 500.0, 0.0, 0.0, 0.0};
            eop.insert(eop.end(), v, v + 6);
        }
    }
    void obs(int e, int t) {  // t < 0: a control observation
        img.push_back(e);
        cam.push_back(img_cam[e]);
        tie.push_back(t);
        std::uniform_real_distribution<double> U(-1.0, 1.0);
        xy.push_back(1000.0 * U(rng));
        xy.push_back(1000.0 * U(rng));
        for (int m = 0; m < 3; ++m) xyzf.push_back(t < 0 ? 50.0 * U(rng) : 0.0);
    }
    int point() {
        std::uniform_real_distribution<double> U(0.0, 2000.0);
        for (int m = 0; m < 3; ++m) tie0.push_back(U(rng));
        return n_tie++;
    }
};

// what the ranks' plans must add up to
struct Sums {
    std::vector<int> seen_pho;         // [n_pts] ranks holding each observation
    std::vector<int> counted, owned;   // [u_full] ranks counting / owning each full-space entry
    std::vector<uint8_t> active;       // [n_pad]
    int64_t u_c = -1;
};

// one rank's plan against brute force
static int check_rank(const Scene& sc, int world, int rank, int split, double ratio, Sums& sums, std::string& line) {
    fba_settings set{};
    set.est_Xc = set.est_Yc = set.est_Zc = set.est_omega = set.est_phi = set.est_kappa = 1;
    set.est_c = set.est_radial = 1;  // (xp, yp, decentering fixed: inactive unknowns)
    set.num_radial = sc.nk;
    set.type = FBA_TYPE_FISHEYE;
    set.meas_std_x = set.meas_std_y = 0.5;
    std::vector<double> iop((size_t)sc.n_cam * (5 + sc.nk), 0.0), caminfo;
    for (int k = 0; k < sc.n_cam; ++k) {
        const double v[5] = {1.0, -1000.0, -1000.0, 1000.0, 1000.0};
        caminfo.insert(caminfo.end(), v, v + 5);
    }
    fba_problem p{};
    p.n_pts = (int64_t)sc.img.size();
    p.n_img = sc.n_img;
    p.n_cam = sc.n_cam;
    p.n_tie = sc.n_tie;
    p.xy = sc.xy.data();
    p.img = sc.img.data();
    p.cam = sc.cam.data();
    p.tie = sc.tie.data();
    p.xyz_fixed = sc.xyzf.data();
    p.eop0 = sc.eop.data();
    p.iop0 = iop.data();
    p.cam_info = caminfo.data();
    p.tie0 = sc.tie0.data();
    fba_options o{};
    o.rank = rank;
    o.world = world;
    o.split = split;
    std::vector<double> pval(sc.pr_index.size(), 1.0), psig(sc.pr_index.size(), 0.5);
    fba_priors prs{(int64_t)sc.pr_index.size(), sc.pr_index.data(), pval.data(), psig.data()};
    const fba_priors* pr = &prs;
    fba_options opt{};
    if (check_inputs(&p, &set, &o, &pr, opt)) return fail_at(fba_last_error(), __LINE__);
    Ctx c;
    HostPlan hp;
    PlanKnobs knobs;
    knobs.pair_terms = ratio;
    if (build_plan(&p, &set, opt, pr, knobs, c, hp)) return fail_at(fba_last_error(), __LINE__);
    CHECK(c.sched.split == (split != 0));

    const Layout& L = c.L;
    const AccPlan& A = c.acc;
    const GenPlan& G = c.gen;
    const int32_t* B = hp.acc.data();
    const int64_t n_obs = c.n_obs, n_lp = c.n_lp, n_pts = p.n_pts;
    auto in_buf = [&](int64_t off, int64_t n) { return off >= 0 && n >= 0 && off + n <= (int64_t)hp.acc.size(); };
    CHECK((int64_t)c.obs_pho.size() == n_obs && (int64_t)hp.img.size() == n_obs && (int64_t)hp.cam.size() == n_obs &&
          (int64_t)hp.pt.size() == n_obs && (int64_t)hp.xy.size() == 2 * n_obs && (int64_t)hp.xoff.size() == n_obs);
    CHECK((int64_t)hp.lp_start.size() == n_lp + 1 && (int64_t)hp.lp_cam.size() == n_lp && (int64_t)hp.lp_tie.size() == n_lp + G.n_gp);
    CHECK(G.lp0 == n_lp && in_buf(G.g_obs, G.n_gp + 1));
    CHECK((int)c.tie_owner.size() == sc.n_tie && (int)c.img_new.size() == sc.n_img);
    const int64_t o_gen0 = B[G.g_obs];

    // ---- the observations: every one of the rank once; tie | control | general; a point's contiguous ----
    std::vector<std::vector<int64_t>> tie_rows(sc.n_tie);
    for (int64_t i = 0; i < n_pts; ++i)
        if (sc.tie[i] >= 0) tie_rows[sc.tie[i]].push_back(i);
    std::set<int64_t> prior_ties;
    const int64_t ref_tie0 = L.u_ref - 3 * (int64_t)sc.n_tie;
    for (int64_t x : sc.pr_index)
        if (x >= ref_tie0) prior_ties.insert((x - ref_tie0) / 3);
    auto is_general = [&](int t) {  // from the problem arrays alone
        std::set<int32_t> ims, cams;
        for (int64_t i : tie_rows[t]) { ims.insert(sc.img[i]); cams.insert(sc.cam[i]); }
        return cams.size() > 1 || ims.size() < tie_rows[t].size() || tie_rows[t].size() > (size_t)CHUNK_OBS || prior_ties.count(t) > 0;
    };
    CHECK(0 <= c.n_obs_tie && c.n_obs_tie <= o_gen0 && o_gen0 <= n_obs && hp.lp_start[0] == 0 && hp.lp_start[n_lp] == c.n_obs_tie);
    CHECK((int64_t)hp.ctl.size() == 3 * (o_gen0 - c.n_obs_tie));
    std::vector<int> local_seen(n_pts, 0);
    for (int64_t o = 0; o < n_obs; ++o) {
        const int64_t i = c.obs_pho[o];
        CHECK(i >= 0 && i < n_pts && !local_seen[i]++);
        sums.seen_pho[i]++;
        CHECK(hp.img[o] == c.img_new[sc.img[i]] && hp.cam[o] == sc.cam[i] && hp.xy[2 * o] == sc.xy[2 * i] && hp.xy[2 * o + 1] == sc.xy[2 * i + 1]);
        if (o >= c.n_obs_tie && o < o_gen0) {  // control: numbered in order, its fixed coordinates
            const int64_t q = o - c.n_obs_tie;
            CHECK(sc.tie[i] < 0 && hp.pt[o] == -1 - (int32_t)q && hp.xoff[o] == 0);
            for (int m = 0; m < 3; ++m) CHECK(hp.ctl[3 * q + m] == sc.xyzf[3 * i + m]);
            CHECK(q == 0 || hp.cam[o - 1] <= hp.cam[o]);
        } else {
            CHECK(sc.tie[i] >= 0 && c.tie_owner[sc.tie[i]] == rank);
            CHECK(hp.pt[o] >= 0 && hp.pt[o] < n_lp + G.n_gp && hp.lp_tie[hp.pt[o]] == sc.tie[i]);
            CHECK((o < c.n_obs_tie) == (hp.pt[o] < n_lp) && (o < c.n_obs_tie) == !is_general(sc.tie[i]));
            CHECK(hp.xoff[o] == L.u_c + 3 * sc.tie[i]);
        }
    }
    for (int t = 0; t < sc.n_tie; ++t) {
        CHECK(c.tie_owner[t] >= 0 && c.tie_owner[t] < world);
        for (int64_t i : tie_rows[t]) CHECK(local_seen[i] == (c.tie_owner[t] == rank));
    }
    for (int64_t lp = 0; lp < n_lp + G.n_gp; ++lp) {  // a point's observations: one range, all of them
        const int64_t a = lp < n_lp ? hp.lp_start[lp] : B[G.g_obs + lp - n_lp], b = lp < n_lp ? hp.lp_start[lp + 1] : B[G.g_obs + lp - n_lp + 1];
        CHECK(a < b && b <= n_obs && b - a == (int64_t)tie_rows[hp.lp_tie[lp]].size());
        for (int64_t o = a; o < b; ++o) CHECK(hp.pt[o] == lp);
        if (lp < n_lp) {
            CHECK(hp.lp_cam[lp] == hp.cam[a] && (lp == 0 || hp.lp_cam[lp - 1] <= hp.lp_cam[lp]));
            if (lp > 0 && hp.lp_cam[lp - 1] == hp.lp_cam[lp]) {  // within a camera: by (sorted) image set
                std::vector<int32_t> s0(hp.img.begin() + hp.lp_start[lp - 1], hp.img.begin() + a), s1(hp.img.begin() + a, hp.img.begin() + b);
                std::sort(s0.begin(), s0.end());
                std::sort(s1.begin(), s1.end());
                CHECK(s0 <= s1);
            }
        }
    }

    // ---- the chunks: legal, and cut exactly where a condition first fails ----
    const std::vector<int32_t>&co = hp.chunk_obs, &cp = hp.chunk_pt;
    const int64_t n_ch = c.n_chunks, n_lr = c.n_chunks_lr;
    CHECK((int64_t)co.size() == n_ch + 1 && (int64_t)cp.size() == n_ch + 1 && co[0] == 0 && cp[0] == 0 && co[n_ch] == n_obs && n_lr <= n_ch);
    auto pt_terms = [&](int64_t lp) { const int64_t n = hp.lp_start[lp + 1] - hp.lp_start[lp]; return n * (n - 1) / 2; };
    std::vector<int32_t> chunk_of(n_obs, -1);
    int64_t n_tie_chunks = 0;
    for (int64_t ch = 0; ch < n_ch; ++ch) {
        const int64_t o0 = co[ch], o1 = co[ch + 1], p0 = cp[ch], p1 = cp[ch + 1];
        CHECK(o0 < o1 && p0 <= p1 && p1 <= n_lp);
        for (int64_t o = o0; o < o1; ++o) chunk_of[o] = (int32_t)ch;
        if (ch >= n_lr) {  // general observations, CHUNK_OBS at a time
            CHECK(o0 >= o_gen0 && p0 == n_lp && (o1 - o0 == CHUNK_OBS || o1 == n_obs));
            continue;
        }
        for (int64_t o = o0; o < o1; ++o) CHECK(hp.cam[o] == hp.cam[o0]);
        if (o0 < c.n_obs_tie) {
            ++n_tie_chunks;
            CHECK(p0 < p1 && o0 == hp.lp_start[p0] && o1 == hp.lp_start[p1]);
            int64_t terms = 0;
            for (int64_t lp = p0; lp < p1; ++lp) terms += pt_terms(lp);
            CHECK(p1 - p0 == 1 || (o1 - o0 <= CHUNK_OBS && p1 - p0 <= chunk_pts(L.nk) && terms <= chunk_terms(L.nk)));
            if (p1 < n_lp)  // the next point would not have fitted
                CHECK(hp.lp_start[p1 + 1] - o0 > CHUNK_OBS || p1 - p0 >= chunk_pts(L.nk) || hp.lp_cam[p1] != hp.lp_cam[p1 - 1] ||
                      terms + pt_terms(p1) > chunk_terms(L.nk));
        } else {
            CHECK(o1 <= o_gen0 && p0 == n_lp && o1 - o0 <= CHUNK_OBS);
            CHECK(o1 == o_gen0 || o1 - o0 == CHUNK_OBS || hp.cam[o1] != hp.cam[o0]);
        }
    }
    CHECK(n_lp == 0 || cp[n_tie_chunks] == n_lp);

    // ---- partial slot lists: permutations, grouped, ascending within a group; the slots their inverses ----
    const int64_t n_pk = A.n_pk, n_ik = A.n_ik, n_ck = n_lr + G.n_gc, n_pairs = c.n_pairs;
    CHECK(in_buf(A.ck_cam, n_ck) && in_buf(A.ck_pk, n_lr + 1) && in_buf(A.pk_t, n_pk - G.n_gpk + 1) && in_buf(A.ck_ik, n_lr + 1) &&
          in_buf(A.rp_start, n_pairs + 1) && in_buf(A.rp_e, 2 * n_pairs) && in_buf(A.rp_list, n_pk) && in_buf(A.pk_slot, n_pk) &&
          in_buf(A.ri_start, L.n_img + 1) && in_buf(A.ri_list, n_ik) && in_buf(A.ik_slot, n_ik) && in_buf(A.img_cam, L.n_img) &&
          in_buf(A.rc_start, L.n_cam + 1) && in_buf(A.rc_list, n_ck) && in_buf(A.ck_tm, n_lr) && in_buf(A.tp_start, n_pairs + 1) &&
          in_buf(A.tp_ab, 2 * A.n_tt));
    CHECK(G.pk0 + G.n_gpk == n_pk && G.ik0 + G.n_gi == n_ik && G.ck0 == n_lr && G.pk_slot == A.pk_slot && G.ik_slot == A.ik_slot);
    CHECK(B[A.ck_pk] == 0 && B[A.ck_pk + n_lr] == G.pk0 && B[A.ck_ik] == 0 && B[A.ck_ik + n_lr] == G.ik0 && B[A.pk_t] == 0);
    CHECK(in_buf(A.ik_o, G.ik0 + 1) && B[A.ik_o] == 0 && in_buf(A.pk_term, B[A.pk_t + G.pk0]) && in_buf(A.ik_obs, B[A.ik_o + G.ik0]));
    // group g of list[start[g] .. start[g+1]): a permutation of [0, n), ascending within each group; group_of = the inverse
    auto check_groups = [&](int64_t start, int64_t list, int64_t ngroups, int64_t n, std::vector<int32_t>& group_of) -> int {
        group_of.assign(n, -1);
        CHECK(B[start] == 0 && B[start + ngroups] == n);
        for (int64_t g = 0; g < ngroups; ++g) {
            CHECK(B[start + g] <= B[start + g + 1]);
            for (int64_t x = B[start + g]; x < B[start + g + 1]; ++x) {
                const int32_t K = B[list + x];
                CHECK(K >= 0 && K < n && group_of[K] < 0);
                CHECK(x == B[start + g] || B[list + x - 1] < K);  // the fixed summation order
                group_of[K] = (int32_t)g;
            }
        }
        return 0;
    };
    std::vector<int32_t> pk_pair, ik_image, ck_camera;
    if (check_groups(A.rp_start, A.rp_list, n_pairs, n_pk, pk_pair)) return 1;
    if (check_groups(A.ri_start, A.ri_list, L.n_img, n_ik, ik_image)) return 1;
    if (check_groups(A.rc_start, A.rc_list, L.n_cam, n_ck, ck_camera)) return 1;
    for (int64_t x = 0; x < n_pk; ++x) CHECK(B[A.pk_slot + B[A.rp_list + x]] == x);
    for (int64_t x = 0; x < n_ik; ++x) CHECK(B[A.ik_slot + B[A.ri_list + x]] == x);
    for (int64_t q = 0; q < n_pairs; ++q) {
        const int32_t* e = B + A.rp_e + 2 * q;
        CHECK(e[0] > e[1] && e[1] >= 0 && e[0] < L.n_img);
        CHECK(q == 0 || std::make_pair(e[-2], e[-1]) < std::make_pair(e[0], e[1]));
        CHECK(B[A.rp_start + q] < B[A.rp_start + q + 1] || B[A.tp_start + q] < B[A.tp_start + q + 1]);  // no pair without a term
    }
    for (int64_t k = 0; k < n_ck; ++k) CHECK(B[A.ck_cam + k] == ck_camera[k]);
    for (int64_t ch = 0; ch < n_lr; ++ch) CHECK(B[A.ck_cam + ch] == hp.cam[co[ch]]);
    {
        std::vector<int32_t> ic(L.n_img, -1);
        for (int64_t o = 0; o < n_obs; ++o) ic[hp.img[o]] = hp.cam[o];
        for (int e = 0; e < L.n_img; ++e) CHECK(B[A.img_cam + e] == ic[e]);
    }

    // ---- per chunk: the pair terms against the co-observing pairs of its points; the image keys ----
    std::vector<std::vector<Term>> got(n_lr);
    CHECK(B[A.tp_start] == 0 && B[A.tp_start + n_pairs] == A.n_tt);
    for (int64_t q = 0; q < n_pairs; ++q)  // U-row terms: per pair in chunk order, filed under the chunk of their observations
        for (int64_t x = B[A.tp_start + q]; x < B[A.tp_start + q + 1]; ++x) {
            const int32_t a = B[A.tp_ab + 2 * x], b = B[A.tp_ab + 2 * x + 1];
            CHECK(a >= 0 && a < c.n_obs_tie && b >= 0 && b < c.n_obs_tie && chunk_of[a] == chunk_of[b] && B[A.ck_tm + chunk_of[a]] == 1);
            CHECK(x == B[A.tp_start + q] || chunk_of[B[A.tp_ab + 2 * x - 2]] <= chunk_of[a]);
            got[chunk_of[a]].push_back({B[A.rp_e + 2 * q], B[A.rp_e + 2 * q + 1], a, b});
        }
    int64_t n_terms = 0, n_tm_chunks = 0;
    for (int64_t ch = 0; ch < n_lr; ++ch) {
        const int64_t o0 = co[ch], o1 = co[ch + 1];
        std::vector<Term> want;
        std::set<std::pair<int32_t, int32_t>> want_keys;
        for (int64_t lp = cp[ch]; lp < cp[ch + 1]; ++lp)
            for (int64_t i = hp.lp_start[lp]; i < hp.lp_start[lp + 1]; ++i)
                for (int64_t j = hp.lp_start[lp]; j < hp.lp_start[lp + 1]; ++j)
                    if (hp.img[i] > hp.img[j]) {
                        want.push_back({hp.img[i], hp.img[j], (int32_t)i, (int32_t)j});
                        want_keys.insert({hp.img[i], hp.img[j]});
                    }
        const bool tm = B[A.ck_tm + ch] != 0;
        CHECK(tm == (!want_keys.empty() && (double)want.size() <= ratio * (double)want_keys.size()));
        const int64_t k0 = B[A.ck_pk + ch], k1 = B[A.ck_pk + ch + 1];
        CHECK(k0 <= k1 && (!tm || k0 == k1) && (tm || k1 - k0 == (int64_t)want_keys.size()));
        n_tm_chunks += tm;
        for (int64_t K = k0; K < k1; ++K) {
            const int64_t t0 = B[A.pk_t + K], t1 = B[A.pk_t + K + 1];
            CHECK(t0 < t1 && (K == k0 || t1 - t0 <= B[A.pk_t + K] - B[A.pk_t + K - 1]));  // most terms first
            for (int64_t x = t0; x < t1; ++x) {
                const int32_t tm2 = B[A.pk_term + x], i = tm2 & 0xffff, j = tm2 >> 16;
                CHECK(i < o1 - o0 && j < o1 - o0 && j >= 0);
                got[ch].push_back({B[A.rp_e + 2 * pk_pair[K]], B[A.rp_e + 2 * pk_pair[K] + 1], (int32_t)(o0 + i), (int32_t)(o0 + j)});
            }
        }
        std::sort(want.begin(), want.end());
        std::sort(got[ch].begin(), got[ch].end());
        CHECK(want == got[ch]);
        n_terms += (int64_t)want.size();
        // image keys: a partition of the chunk's observations by image
        const int64_t i0 = B[A.ck_ik + ch], i1 = B[A.ck_ik + ch + 1];
        std::vector<int> hit(o1 - o0, 0);
        std::set<int32_t> imgs;
        for (int64_t K = i0; K < i1; ++K) {
            CHECK(B[A.ik_o + K] < B[A.ik_o + K + 1] && imgs.insert(ik_image[K]).second);
            for (int64_t x = B[A.ik_o + K]; x < B[A.ik_o + K + 1]; ++x) {
                const int32_t lo = B[A.ik_obs + x];
                CHECK(lo >= 0 && lo < o1 - o0 && !hit[lo]++ && hp.img[o0 + lo] == ik_image[K]);
            }
        }
        for (int h : hit) CHECK(h == 1);
    }
    CHECK(n_terms == c.n_pair_terms);
    CHECK(c.ik_lanes == ((G.ik0 > 0 && B[A.ik_o + G.ik0] <= 2 * G.ik0) ? 4 : 8));

    // ---- general points ----
    CHECK(in_buf(G.g_gi, G.n_gp + 1) && in_buf(G.g_gc, G.n_gp + 1) && in_buf(G.gi_obs, G.n_gi + 1) && in_buf(G.gi_img, G.n_gi) &&
          in_buf(G.gi_gp, G.n_gi) && in_buf(G.gi_gc, G.n_gi) && in_buf(G.gc_cam, G.n_gc) && in_buf(G.gc_gp, G.n_gc) &&
          in_buf(G.gc_o, G.n_gc + 1) && in_buf(G.gpk, 2 * G.n_gpk) && in_buf(G.gx, 2 * G.n_gx) && in_buf(G.gkk, 2 * G.n_gkk) &&
          in_buf(G.xt_start, G.n_xt + 1) && in_buf(G.xt_key, 2 * G.n_xt) && in_buf(G.xt_list, G.n_gx) &&
          in_buf(G.kt_start, G.n_kt + 1) && in_buf(G.kt_key, 2 * G.n_kt) && in_buf(G.kt_list, G.n_gkk));
    CHECK(B[G.g_gi] == 0 && B[G.g_gc] == 0 && B[G.g_gi + G.n_gp] == G.n_gi && B[G.g_gc + G.n_gp] == G.n_gc && B[G.gc_o] == 0 &&
          B[G.g_obs + G.n_gp] == n_obs && B[G.gi_obs + G.n_gi] == n_obs && in_buf(G.gc_list, B[G.gc_o + G.n_gc]));
    std::set<std::pair<int32_t, int32_t>> want_gpk, want_gx, want_gkk;
    for (int64_t q = 0; q < G.n_gp; ++q) {
        const int32_t a = B[G.g_obs + q], b = B[G.g_obs + q + 1], gi0 = B[G.g_gi + q], gi1 = B[G.g_gi + q + 1], gc0 = B[G.g_gc + q],
                      gc1 = B[G.g_gc + q + 1];
        CHECK(gi0 < gi1 && gc0 < gc1 && B[G.gi_obs + gi0] == a);
        for (int32_t o = a + 1; o < b; ++o) CHECK(hp.img[o - 1] <= hp.img[o]);
        for (int32_t i = gi0; i < gi1; ++i) {  // gimg: the point's observations in one image
            const int32_t oa = B[G.gi_obs + i], ob = i + 1 < gi1 ? B[G.gi_obs + i + 1] : b;
            CHECK(oa < ob && ob <= b && B[G.gi_gp + i] == q && (i == gi0 || B[G.gi_img + i - 1] < B[G.gi_img + i]));
            for (int32_t o = oa; o < ob; ++o) CHECK(hp.img[o] == B[G.gi_img + i]);
            const int32_t own = B[G.gi_gc + i];
            CHECK(own >= gc0 && own < gc1 && B[G.gc_cam + own] == hp.cam[oa]);  // the observation's own camera
            CHECK(ik_image[G.ik0 + i] == B[G.gi_img + i]);                        // its appended image key
            for (int32_t j = gi0; j < i; ++j) want_gpk.insert({i, j});
            for (int32_t k = gc0; k < gc1; ++k)
                if (k != own) want_gx.insert({i, k});
        }
        for (int32_t k = gc0; k < gc1; ++k) {  // gpc: the point's observations through one camera
            CHECK(B[G.gc_gp + k] == q && (k == gc0 || B[G.gc_cam + k - 1] < B[G.gc_cam + k]) && B[A.ck_cam + G.ck0 + k] == B[G.gc_cam + k]);
            std::vector<int32_t> lst(B + G.gc_list + B[G.gc_o + k], B + G.gc_list + B[G.gc_o + k + 1]), w;
            for (int32_t o = a; o < b; ++o)
                if (hp.cam[o] == B[G.gc_cam + k]) w.push_back(o);
            CHECK(!w.empty() && lst == w);
            for (int32_t k2 = gc0; k2 < k; ++k2) want_gkk.insert({k, k2});
        }
        std::set<int32_t> cams(hp.cam.begin() + a, hp.cam.begin() + b);
        CHECK((int32_t)cams.size() == gc1 - gc0);
    }
    // keys listed once each: pair keys with their pair, foreign-camera and camera-pair keys filed under their target block
    auto check_keys = [&](int64_t keys, int64_t n, const std::set<std::pair<int32_t, int32_t>>& want) -> int {
        std::set<std::pair<int32_t, int32_t>> have;
        for (int64_t m = 0; m < n; ++m) CHECK(have.insert({B[keys + 2 * m], B[keys + 2 * m + 1]}).second);
        CHECK(have == want);
        return 0;
    };
    if (check_keys(G.gpk, G.n_gpk, want_gpk) || check_keys(G.gx, G.n_gx, want_gx) || check_keys(G.gkk, G.n_gkk, want_gkk)) return 1;
    for (int64_t m = 0; m < G.n_gpk; ++m) {
        const int32_t* e = B + A.rp_e + 2 * pk_pair[G.pk0 + m];
        CHECK(e[0] == B[G.gi_img + B[G.gpk + 2 * m]] && e[1] == B[G.gi_img + B[G.gpk + 2 * m + 1]]);
    }
    auto check_targets = [&](int64_t start, int64_t list, int64_t key, int64_t nblocks, int64_t keys, int64_t nkeys, int64_t tab0,
                             int64_t tab1) -> int {
        std::vector<int32_t> blk;
        if (check_groups(start, list, nblocks, nkeys, blk)) return 1;
        for (int64_t b = 0; b < nblocks; ++b) {
            CHECK(B[start + b] < B[start + b + 1]);
            CHECK(b == 0 || std::make_pair(B[key + 2 * b - 2], B[key + 2 * b - 1]) < std::make_pair(B[key + 2 * b], B[key + 2 * b + 1]));
        }
        for (int64_t m = 0; m < nkeys; ++m)
            CHECK(B[tab0 + B[keys + 2 * m]] == B[key + 2 * blk[m]] && B[tab1 + B[keys + 2 * m + 1]] == B[key + 2 * blk[m] + 1]);
        return 0;
    };
    if (check_targets(G.xt_start, G.xt_list, G.xt_key, G.n_xt, G.gx, G.n_gx, G.gi_img, G.gc_cam)) return 1;
    if (check_targets(G.kt_start, G.kt_list, G.kt_key, G.n_kt, G.gkk, G.n_gkk, G.gc_cam, G.gc_cam)) return 1;

    // ---- masks and ownership ----
    CHECK((int64_t)hp.active.size() == L.n_pad && (int64_t)hp.counted.size() == L.u_full && (int64_t)c.full_owned.size() == L.u_full);
    {
        std::vector<int> ref_hit(L.u_ref, 0);
        for (int64_t i = 0; i < L.u_full; ++i)
            if (c.full_to_ref[i] >= 0) { CHECK(c.full_to_ref[i] < L.u_ref); ref_hit[c.full_to_ref[i]]++; }
        for (int h : ref_hit) CHECK(h == 1);
    }
    for (int64_t i = 0; i < L.n_pad; ++i) CHECK(hp.active[i] == (i < L.u_c && c.full_to_ref[i] >= 0));
    if (sums.u_c < 0) {
        sums.u_c = L.u_c;
        sums.active = hp.active;
        sums.counted.assign(L.u_full, 0);
        sums.owned.assign(L.u_full, 0);
    }
    CHECK(sums.u_c == L.u_c && sums.active == hp.active && (int64_t)sums.counted.size() == L.u_full);  // the same on every rank
    for (int64_t i = 0; i < L.u_full; ++i) {
        if (i >= L.u_c) CHECK(hp.counted[i] == (c.tie_owner[(i - L.u_c) / 3] == rank) && c.full_owned[i] == hp.counted[i]);
        else if (!split) CHECK(c.full_owned[i] == (rank == 0) && hp.counted[i] == (rank == 0 && hp.active[i]));
        else CHECK(hp.counted[i] == (c.full_owned[i] && hp.active[i]));
        sums.counted[i] += hp.counted[i];
        sums.owned[i] += c.full_owned[i];
    }

    // ---- multi-rank reduce buffers ----
    if (world > 1 && !split) {
        std::set<std::pair<int32_t, int32_t>> all;
        for (int t = 0; t < sc.n_tie; ++t)
            for (int64_t i : tie_rows[t])
                for (int64_t j : tie_rows[t])
                    if (c.img_new[sc.img[i]] > c.img_new[sc.img[j]]) all.insert({c.img_new[sc.img[i]], c.img_new[sc.img[j]]});
        std::vector<int32_t> flat;
        for (auto& q : all) { flat.push_back(q.first); flat.push_back(q.second); }
        CHECK(flat == hp.gpairs && c.n_gpairs == (int64_t)all.size());
        CHECK(c.n_red == 36 * (c.n_gpairs + L.n_img) + (int64_t)L.cw * L.n_cam * L.n_pad + L.n_pad);
    }
    int64_t n_top = 0;
    if (split) {
        const std::vector<int32_t>& br = c.sched.blk_rank;
        const int64_t nb = L.n_pad / NB;
        CHECK((int64_t)br.size() == nb && (int64_t)hp.bown.size() == nb && (int64_t)hp.rown.size() == L.n_pad);
        auto role = [&](int r) { return r < 0 ? 2 : (r == rank ? 1 : 0); };
        auto slot_rank = [&](int64_t e) { return std::max(br[6 * e / NB], br[(6 * e + 5) / NB]); };  // an image's subtree, -1: top
        std::vector<int32_t> td;
        int64_t ng = 0;
        for (int64_t k = 0; k < nb; ++k) {
            CHECK(br[k] >= -1 && br[k] < world && hp.bown[k] == role(br[k]));
            ng += br[k] >= 0;
            n_top += br[k] < 0;
        }
        for (int64_t i = 0; i < L.n_pad; ++i) {
            const bool image_row = i < 6 * (int64_t)L.n_img && c.img_ord[i / 6] >= 0;
            CHECK(hp.rown[i] == (image_row ? role(slot_rank(i / 6)) : hp.bown[i / NB]));
            if (i < 6 * (int64_t)L.n_img && hp.rown[i] == 2) td.push_back((int32_t)i);
            if (i < L.u_c) CHECK(c.full_owned[i] == (hp.bown[i / NB] == 1 || (hp.bown[i / NB] == 2 && rank == 0)));
        }
        CHECK(td == hp.topdiag && c.n_topdiag == (int64_t)td.size());
        int64_t n = 0;
        for (int64_t a = 0; a <= nb; ++a)  // the top blocks (a, b), b <= a, the RHS block row's included
            for (int64_t b = 0; b <= std::min(a, nb - 1); ++b)
                if ((a == nb || br[a] < 0) && br[b] < 0) n += (a == nb ? L.nrhs : NB) * NB;
        CHECK(n >= c.red_diag);  // (the schedule lists the nonzero ones of them)
        int64_t listed = 0;
        for (int q = 0; q < c.sched.n_top_blocks; ++q) {
            const int32_t a = c.sched.buf[c.sched.top_blocks + 2 * q], b = c.sched.buf[c.sched.top_blocks + 2 * q + 1];
            CHECK(b >= 0 && b < nb && a >= b && a <= nb && (a == nb || br[a] < 0) && br[b] < 0);
            listed += (a == nb ? L.nrhs : NB) * NB;
        }
        CHECK(c.red_diag == listed && c.red_gblk == c.red_diag + c.n_topdiag && c.red_w == c.red_gblk + 256 * ng && c.n_red == c.red_w + 9);
        for (int64_t i = 0; i < n_pts; ++i)  // a tie point's images: its owner's subtree or the top
            if (sc.tie[i] >= 0) {
                const int r = slot_rank(c.img_new[sc.img[i]]);
                CHECK(r < 0 || r == c.tie_owner[sc.tie[i]]);
            }
    }

    // ---- priors ----
    if (pr) {
        CHECK(c.n_prior == pr->n && c.cam_tab_stride == CAM_TAB_HDR + 3 * L.nk);
        int64_t n_cam_side = 0, n_own_tie = 0;
        for (int64_t j = 0; j < pr->n; ++j) {
            if (pr->index[j] < ref_tie0) { n_cam_side += rank == 0; continue; }
            const int t = (int)((pr->index[j] - ref_tie0) / 3), d = (int)((pr->index[j] - ref_tie0) % 3);
            if (c.tie_owner[t] != rank) continue;
            ++n_own_tie;
            const int64_t q = std::find(hp.lp_tie.begin() + n_lp, hp.lp_tie.end(), t) - (hp.lp_tie.begin() + n_lp);
            CHECK(q < G.n_gp && (int64_t)hp.gprior.size() == 6 * G.n_gp && hp.gprior[6 * q + d] == 4.0 && hp.gprior[6 * q + 3 + d] == 1.0);
        }
        CHECK(c.n_pcam == n_cam_side && c.n_pres == n_cam_side + n_own_tie && (int64_t)hp.pr_idx.size() == 2 * c.n_pres);
        for (int64_t x = 0; x < c.n_pres; ++x) CHECK(c.full_to_ref[hp.pr_idx[2 * x]] == pr->index[hp.pr_idx[2 * x + 1]]);
    }

    char buf[300];
    snprintf(buf, sizeof buf, " r%d:obs=%ld,points=%ld,chunks=%ld,pair_keys=%ld,urow_chunks=%ld,urow_terms=%ld,image_keys=%ld,general=%ld,top=%ld",
             rank, (long)n_obs, (long)n_lp, (long)n_lr, (long)n_pk, (long)n_tm_chunks, (long)A.n_tt, (long)n_ik, (long)G.n_gp, (long)n_top);
    line += buf;
    return 0;
}

// every rank of one scene, and what the ranks must add up to
static int check_scene(const char* name, const Scene& sc, int world = 1, int split = 0, double ratio = 2.0) {
    Sums sums;
    sums.seen_pho.assign(sc.img.size(), 0);
    std::string line;
    for (int r = 0; r < world; ++r)
        if (check_rank(sc, world, r, split, ratio, sums, line)) { printf("FAIL %s (rank %d of %d)\n", name, r, world); return 1; }
    for (int s : sums.seen_pho)
        if (s != 1) { printf("FAIL %s: an observation on %d ranks\n", name, s); return 1; }
    // every full-space entry is owned by one rank; every estimated one (and no other) is counted once
    for (int64_t i = 0; i < (int64_t)sums.owned.size(); ++i) {
        const int want = i < sums.u_c ? sums.active[i] : 1;
        if (sums.owned[i] != 1 || sums.counted[i] != want) {
            printf("FAIL %s: full entry %ld owned %d / counted %d times\n", name, (long)i, sums.owned[i], sums.counted[i]);
            return 1;
        }
    }
    printf("ok %s%s\n", name, line.c_str());
    return 0;
}

// 12 images in two rows, points seen by 3 or 4 neighbouring images
static Scene strip_scene(int n_points, int cams, int nk) {
    Scene s;
    s.nk = nk;
    s.images(12, cams);
    for (int q = 0; q < n_points; ++q) {
        const int t = s.point();
        const int half = cams == 2 ? 6 : 12, base = cams == 2 && (q & 1) ? 6 : 0, e0 = (q * 5) % (half - 3);
        for (int k = 0; k < 3 + (q % 2); ++k) s.obs(base + e0 + k, t);
    }
    return s;
}

int main(int argc, char** argv) {
    const char* only = argc > 1 ? argv[1] : nullptr;
    auto want = [&](const char* n) { return !only || !strcmp(only, n); };
    int bad = 0, ran = 0;
    auto run = [&](int rc) { bad += rc; ++ran; };
    if (want("points")) run(check_scene("points", strip_scene(150, 1, 3)));       // cuts by point count (64)
    if (want("points_nk6")) run(check_scene("points_nk6", strip_scene(150, 1, 6)));  // 32-point chunks
    if (want("two_cameras")) run(check_scene("two_cameras", strip_scene(150, 2, 3)));
    if (want("cut_obs") || want("cut_terms")) {  // points of 12 images: 21 fill CHUNK_OBS; of 20 images: 10 fill chunk_terms
        for (int per : {12, 20}) {
            Scene s;
            s.images(24);
            for (int q = 0; q < (per == 12 ? 40 : 30); ++q) {
                const int t = s.point();
                for (int k = 0; k < per; ++k) s.obs((q % (25 - per)) + k, t);
            }
            if (want(per == 12 ? "cut_obs" : "cut_terms")) run(check_scene(per == 12 ? "cut_obs" : "cut_terms", s));
        }
    }
    if (want("own_pairs") || want("own_pairs_ratio0")) {  // every point seen by an image pair of its own: one term per key
        Scene s;
        s.images(30);
        for (int a = 1; a < 30; ++a)
            for (int b = 0; b < a && s.n_tie < 300; ++b) {
                const int t = s.point();
                s.obs(a, t);
                s.obs(b, t);
            }
        if (want("own_pairs")) run(check_scene("own_pairs", s));
        if (want("own_pairs_ratio0")) run(check_scene("own_pairs_ratio0", s, 1, 0, 0.0));
    }
    if (want("general") || want("general_world2")) {  // each kind of general point among regular ones
        Scene s = strip_scene(40, 2, 3);
        Scene big;
        big.nk = 3;
        big.images(520, 2);  // 260 images per camera
        big.img = s.img; big.cam = s.cam; big.tie = s.tie; big.xy = s.xy; big.xyzf = s.xyzf; big.tie0 = s.tie0; big.n_tie = s.n_tie;
        for (size_t q = 0; q < big.img.size(); ++q)  // the strip's camera 1 images 6-11 -> this scene's camera 1
            if (big.cam[q] == 1) big.img[q] += 260 - 6;
        const int two_cam = big.point(), twice = big.point(), wide = big.point(), prior = big.point(), both = big.point();
        for (int e : {3, 4, 270, 271, 272}) big.obs(e, two_cam);
        for (int e : {7, 8, 8, 9}) big.obs(e, twice);
        for (int e = 0; e < 257; ++e) big.obs(e, wide);  // > CHUNK_OBS images, all of camera 0
        for (int e : {20, 21, 22}) big.obs(e, prior);
        for (int e : {30, 30, 31, 280, 280, 281}) big.obs(e, both);  // twice in an image and two cameras
        for (int e : {2, 265}) big.obs(e, -1);
        // priors: the prior point's X and Z, one image unknown, one camera's K2
        const int64_t u_img = 6, u_cam = 1 + big.nk, tb = u_img * 520 + u_cam * 2;
        big.pr_index = {tb + 3 * prior, tb + 3 * prior + 2, 6 * 17 + 4, u_img * 520 + u_cam * 1 + 2};
        if (want("general")) run(check_scene("general", big));
        if (want("general_world2")) run(check_scene("general_world2", big, 2));
    }
    if (want("control")) {  // control observations of two cameras, 300 of one: chunks of 256 + 44, then the other camera's
        Scene s = strip_scene(20, 2, 3);
        for (int q = 0; q < 300; ++q) s.obs(q % 6, -1);
        for (int q = 0; q < 10; ++q) s.obs(6 + q % 6, -1);
        for (int q = 0; q < 5; ++q) s.obs(q, -1);  // (camera 0 again, later in PHO order)
        run(check_scene("control", s));
    }
    if (want("replicated")) {  // world 2 and 3, replicated solve, every rank
        Scene s = strip_scene(150, 2, 3);
        for (int q = 0; q < 40; ++q) s.obs(q % 12, -1);
        run(check_scene("replicated", s, 2));
        run(check_scene("replicated", s, 3));
    }
    if (want("split")) {  // world 2, subtree split: sched_check's 420-image scene with leaves of 60
        setenv("FBA_ND_LEAF", "60", 1);
        Scene s;
        const int n = 420, gw = std::max(1, (int)std::sqrt(n * 0.6));
        s.n_img = n;
        for (int e = 0; e < n; ++e) {
            s.img_cam.push_back(0);
            const double v[6] = {1000.0 * (e % gw), 1000.0 * (e / gw), 800.0, 0.0, 0.0, 0.0};
            s.eop.insert(s.eop.end(), v, v + 6);
        }
        std::mt19937_64 rng(3);
        std::uniform_real_distribution<double> U(0.0, 1.0);
        for (int q = 0; q < 20 * n; ++q) {
            const double px = U(rng) * gw, py = U(rng) * ((n + gw - 1) / gw);
            const int t = s.point();
            for (int e = 0; e < n; ++e)
                if (std::hypot(e % gw - px, e / gw - py) < 1.6) s.obs(e, t);
        }
        for (int q = 0; q < 50; ++q) s.obs((q * 37) % n, -1);
        run(check_scene("split", s, 2, 1));
        unsetenv("FBA_ND_LEAF");
    }
    if (!ran) { printf("FAIL no scene named %s\n", only); return 2; }
    return bad ? 1 : 0;
}
