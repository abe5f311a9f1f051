// fba_snoop.h -- Baarda data snooping over the image points, fp64: the per-row and per-point arithmetic and the
// selection rule of k_snoop_stat / k_snoop_seg / k_snoop_pick (fba_snoop.hip) and, the same routines, of the host
// (fba_snoop_host).  No reference counterpart: main.m never tests a measurement.
//
// State per image point (a PHO row, its x and y rows together): SNOOP_ACTIVE, SNOOP_EXCLUDED (both sqrt weights
// SNOOP_EPS s0, s0 the point's starting sqrt weights) or SNOOP_READMITTED (active again, never a candidate again).
// With q = a Cx a' of the whitened row (launch_vce_q), the raw residual v, the a-priori sigma of the axis:
//   active    r = 1 - q / sigma^2,  w = s v / (sigma sqrt(r)), 0 where r < 1e-10 (k_rel_finish);  W = max |w_x|, |w_y|
//   excluded  the statistic of the predicted residual: |s0 v| / sqrt(sigma^2 + q / EPS^2) per row -- q / EPS^2 is the
//             unscaled s0^2 a Cx a', a division, no difference is taken;  W~ = the larger of the two rows
// A candidate is an ACTIVE point with W > crit whose removal leaves its tie point min_rays active observations
// (control observations have no tie point) and its image min_img_points.  A candidate is eliminated when it is the
// best of the candidates of its tie point and of its image: the larger W, the lower PHO row between equal W.  A round
// that eliminates nothing re-admits every excluded point with W~ <= crit.
//
// The device (one xor tree per segment) and the host (index order) pick the same points: the order (W, -row) is total.
#pragma once
#include <cmath>
#include <cstdint>
#include <vector>

#include "../../include/fba.h"

#ifndef FBA_HD
#if defined(__HIPCC__) || defined(__CUDACC__)
#define FBA_HD __host__ __device__
#else
#define FBA_HD
#endif
#endif

namespace fba {

constexpr double SNOOP_EPS = 1e-6;  // an excluded point's sqrt weight factor: weight 1e-12 (fba_set_weights' advice)
enum : uint8_t { SNOOP_ACTIVE = 0, SNOOP_EXCLUDED = 1, SNOOP_READMITTED = 2 };
constexpr int SNOOP_PART = 3;  // per block of k_snoop_pick: verdicts of the back-check, excluded points, largest active W
constexpr int SNOOP_OUT = 4;   // k_snoop_counts: picks, back-check verdicts, excluded points, largest active W

// |w| of one active row, k_rel_finish's arithmetic; s the current sqrt weight (1 without weights)
FBA_HD inline double snoop_w_active(double q, double v, double s, double sigma) {
    const double r = 1.0 - q / (sigma * sigma);
    return r < 1e-10 ? 0.0 : fabs((v * s) / (sigma * sqrt(r)));
}

// the statistic of the predicted residual of one excluded row, carried at the sqrt weight SNOOP_EPS s0
FBA_HD inline double snoop_w_excluded(double q, double v, double s0, double sigma) {
    return fabs(s0 * v) / sqrt(sigma * sigma + q / (SNOOP_EPS * SNOOP_EPS));
}

// W or W~ of a point from its two rows
FBA_HD inline double snoop_point_stat(uint8_t state, double qx, double qy, double vx, double vy, double swx, double swy,
                                      double s0x, double s0y, double sx, double sy) {
    const double a = state == SNOOP_EXCLUDED ? snoop_w_excluded(qx, vx, s0x, sx) : snoop_w_active(qx, vx, swx, sx);
    const double b = state == SNOOP_EXCLUDED ? snoop_w_excluded(qy, vy, s0y, sy) : snoop_w_active(qy, vy, swy, sy);
    return b > a ? b : a;
}

// tie_count: the active observations of the point's tie point, or < 0 for a control observation
FBA_HD inline bool snoop_candidate(uint8_t state, double W, double crit, int tie_count, int img_count, int min_rays,
                                   int min_img_points) {
    return state == SNOOP_ACTIVE && W > crit && (tie_count < 0 || tie_count - 1 >= min_rays) && img_count - 1 >= min_img_points;
}

// the back-check's verdict: an excluded point whose predicted residual passes the test (a NaN does not)
FBA_HD inline bool snoop_readmit(uint8_t state, double W, double crit) { return state == SNOOP_EXCLUDED && W <= crit; }

// candidate (Wa, row a) beats candidate (Wb, row b): the larger W, the lower PHO row between equal W
FBA_HD inline bool snoop_better(double Wa, int64_t ra, double Wb, int64_t rb) { return Wa > Wb || (Wa == Wb && ra < rb); }

// the excluded share after n_pick further eliminations would pass max_share of n_pts
FBA_HD inline bool snoop_share_stop(int64_t n_excluded, int64_t n_pick, int64_t n_pts, double max_share) {
    return (double)(n_excluded + n_pick) > max_share * (double)n_pts;
}

// One round's selection on the host, in index order.  n points with W (or W~), state, tie (< 0: a control observation),
// img and the PHO row of each (row == nullptr: the index); tie in [.., n_tie), img in [0, n_img) (the caller checked).
// pick / back [n]: 1 where the point is eliminated / re-admitted by this round -- the back-check runs only where
// nothing is eliminated.  Returns the number of picks through n_pick, of re-admissions through n_back.
inline void snoop_select(int64_t n, const double* W, const uint8_t* state, const int32_t* tie, const int32_t* img,
                         const int64_t* row, int32_t n_tie, int32_t n_img, int min_rays, int min_img_points, double crit,
                         uint8_t* pick, uint8_t* back, int64_t& n_pick, int64_t& n_back) {
    std::vector<int32_t> ct((size_t)(n_tie > 0 ? n_tie : 0), 0), ci((size_t)(n_img > 0 ? n_img : 0), 0);
    std::vector<int64_t> wt(ct.size(), -1), wi(ci.size(), -1);
    std::vector<uint8_t> cand((size_t)n, 0);
    for (int64_t i = 0; i < n; ++i)
        if (state[i] != SNOOP_EXCLUDED) {
            if (tie[i] >= 0) ++ct[(size_t)tie[i]];
            ++ci[(size_t)img[i]];
        }
    auto rw = [&](int64_t i) { return row ? row[i] : i; };
    for (int64_t i = 0; i < n; ++i) {
        cand[(size_t)i] = snoop_candidate(state[i], W[i], crit, tie[i] >= 0 ? ct[(size_t)tie[i]] : -1, ci[(size_t)img[i]],
                                          min_rays, min_img_points);
        if (!cand[(size_t)i]) continue;
        if (tie[i] >= 0) {
            int64_t& b = wt[(size_t)tie[i]];
            if (b < 0 || snoop_better(W[i], rw(i), W[b], rw(b))) b = i;
        }
        int64_t& b = wi[(size_t)img[i]];
        if (b < 0 || snoop_better(W[i], rw(i), W[b], rw(b))) b = i;
    }
    n_pick = n_back = 0;
    for (int64_t i = 0; i < n; ++i) {
        pick[i] = cand[(size_t)i] && (tie[i] < 0 || wt[(size_t)tie[i]] == i) && wi[(size_t)img[i]] == i;
        n_pick += pick[i];
    }
    for (int64_t i = 0; i < n; ++i) {
        back[i] = n_pick == 0 && snoop_readmit(state[i], W[i], crit);
        n_back += back[i];
    }
}

}  // namespace fba
