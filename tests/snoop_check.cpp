// snoop_check.cpp -- stand-alone checker of the data-snooping arithmetic and selection the device and the host share,
// and of the point list builder (tests/test_snoop_host.py builds it with -Xarch_host -fsanitize=address,undefined --
// the host compilation only -- together with fba_plan.cpp / fba_order.cpp and runs it directly; no GPU, no HIP call).
//
// Drives csrc/fba_snoop.h's routines over the edge cases: the two statistics, no candidates, equal W (the lower row
// wins), a two-ray tie point, an image at min_img_points, the local-maximum rule, the back-check, a re-admitted
// point, the max_share stop, empty lists; and build_point_list over a tie point without observations, control
// observations and an empty problem.  One "ok <case>" line per case; any failure prints "FAIL ..." and exits 1.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <string>
#include <vector>

#include "../fish-eye_bundle_adjustment_amd/csrc/fba_internal.h"
#include "../fish-eye_bundle_adjustment_amd/csrc/fba_snoop.h"

namespace fba {
void set_error(const std::string&) {}
}  // namespace fba

using namespace fba;

#define CHECK(cond)                                                     \
    do {                                                                \
        if (!(cond)) {                                                  \
            std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); \
            std::exit(1);                                               \
        }                                                               \
    } while (0)

struct Sel {
    std::vector<uint8_t> pick, back;
    int64_t n_pick = 0, n_back = 0;
};

static Sel run(const std::vector<double>& W, const std::vector<uint8_t>& st, const std::vector<int32_t>& tie,
               const std::vector<int32_t>& img, int n_tie, int n_img, int min_rays = 2, int min_img = 2, double crit = 3.29,
               const std::vector<int64_t>* row = nullptr) {
    Sel s;
    s.pick.resize(W.size());  // exactly the documented sizes: the sanitizer sees an overrun
    s.back.resize(W.size());
    snoop_select((int64_t)W.size(), W.data(), st.data(), tie.data(), img.data(), row ? row->data() : nullptr, n_tie, n_img,
                 min_rays, min_img, crit, s.pick.data(), s.back.data(), s.n_pick, s.n_back);
    return s;
}

int main() {
    {  // the statistics: r = 0.5 -> w = s v / (sigma sqrt(r)); r < 1e-10 -> 0; the excluded row by division
        CHECK(std::fabs(snoop_w_active(0.045, -0.6, 1.0, 0.3) - 2.0 * std::sqrt(2.0)) < 1e-14);
        CHECK(snoop_w_active(0.09, 5.0, 1.0, 0.3) == 0.0);
        const double q = (SNOOP_EPS * 2.0) * (SNOOP_EPS * 2.0) * 0.04;  // (EPS s0)^2 a Cx a', s0 = 2
        CHECK(std::fabs(snoop_w_excluded(q, 1.5, 2.0, 0.3) - 3.0 / std::sqrt(0.09 + 0.16)) < 1e-13);
        CHECK(snoop_point_stat(SNOOP_ACTIVE, 0.045, 0.0, 0.6, -0.9, 1, 1, 1, 1, 0.3, 0.3) == 3.0);
        CHECK(std::fabs(snoop_point_stat(SNOOP_EXCLUDED, q, q, 1.5, 0.1, 9, 9, 2, 2, 0.3, 0.3) - 6.0) < 1e-12);
        std::printf("ok statistics\n");
    }
    // six points: tie points 0 0 0 1 1 1, images 0 1 2 0 1 2
    const std::vector<int32_t> tie{0, 0, 0, 1, 1, 1}, img{0, 1, 2, 0, 1, 2};
    const std::vector<uint8_t> act(6, SNOOP_ACTIVE);
    {  // no candidates: nothing picked, nothing to re-admit
        const Sel s = run({1, 2, 3, 1, 2, 3}, act, tie, img, 2, 3);
        CHECK(s.n_pick == 0 && s.n_back == 0);
        std::printf("ok none\n");
    }
    {  // the local-maximum rule: 0 (tie 0, image 0) wins; 1 shares its tie point, 3 its image, and 5 loses its tie
       // point to 3: all three wait for the next round
        const Sel s = run({9, 5, 1, 8, 1, 4}, act, tie, img, 2, 3, 2, 1);
        CHECK(s.pick[0] && !s.pick[1] && !s.pick[3] && !s.pick[5] && s.n_pick == 1 && s.n_back == 0);
        std::printf("ok local maximum\n");
    }
    {  // equal W: the lower row wins -- by index, and by the PHO rows given
        const Sel s = run({7, 7, 1, 1, 1, 1}, act, tie, img, 2, 3, 2, 1);
        CHECK(s.pick[0] && !s.pick[1] && s.n_pick == 1);
        const std::vector<int64_t> row{5, 4, 3, 2, 1, 0};
        const Sel t = run({7, 7, 1, 1, 1, 1}, act, tie, img, 2, 3, 2, 1, 3.29, &row);
        CHECK(!t.pick[0] && t.pick[1] && t.n_pick == 1);
        std::printf("ok equal\n");
    }
    {  // a two-ray tie point is never eligible; a control observation (tie -1) skips the condition
        const Sel s = run({9, 1, 9, 9}, std::vector<uint8_t>(4, SNOOP_ACTIVE), {0, 0, -1, -2}, {0, 1, 1, 1}, 1, 2, 2, 1);
        CHECK(!s.pick[0] && s.pick[2] && !s.pick[3] && s.n_pick == 1);
        std::printf("ok two rays\n");
    }
    {  // an image at min_img_points keeps its points; one above it gives one
        const Sel s = run({9, 5, 1, 8, 1, 4}, act, tie, img, 2, 3, 2, 2);
        CHECK(s.n_pick == 0);
        const Sel t = run({9, 5, 1, 8, 1, 4}, act, tie, img, 2, 3, 2, 1);
        CHECK(t.pick[0] && t.n_pick == 1);
        // an excluded point does not count: image 0 holds rows 0, 3; with 3 excluded it is at 1 = min + 0
        const Sel u = run({9, 5, 1, 8, 1, 4}, {0, 0, 0, 1, 0, 0}, tie, img, 2, 3, 2, 1);
        CHECK(!u.pick[0] && u.pick[1] && u.n_back == 0);
        std::printf("ok image minimum\n");
    }
    {  // the back-check: only where nothing is picked; W~ <= crit comes back, a NaN does not; a re-admitted point is
       // no candidate
        const double nan = std::numeric_limits<double>::quiet_NaN();
        const Sel s = run({1, 2, 9, nan, 3.29, 9}, {0, 0, 1, 1, 1, 2}, tie, img, 2, 3, 1, 1);
        CHECK(s.n_pick == 0 && s.n_back == 1 && s.back[4] && !s.back[2] && !s.back[3] && !s.pick[5]);
        const Sel t = run({9, 2, 9, 1, 1, 1}, {0, 0, 1, 0, 1, 0}, tie, img, 2, 3, 1, 1);
        CHECK(t.n_pick == 1 && t.pick[0] && t.n_back == 0 && !t.back[4]);
        std::printf("ok back-check\n");
    }
    {  // the max_share stop and empty lists
        CHECK(!snoop_share_stop(0, 1, 20, 0.05) && snoop_share_stop(1, 1, 20, 0.05) && snoop_share_stop(0, 1, 0, 1.0));
        const Sel s = run({}, {}, {}, {}, 0, 0);
        CHECK(s.n_pick == 0 && s.n_back == 0);
        const Sel t = run({}, {}, {}, {}, 3, 2);
        CHECK(t.n_pick == 0 && t.n_back == 0);
        std::printf("ok stop and empty\n");
    }
    {  // build_point_list: stable, a tie point without observations, control observations left out, an empty problem
        std::vector<int32_t> start, list;
        build_point_list({2, 0, -1, 2, 0, -3, 3}, 4, start, list);
        CHECK((start == std::vector<int32_t>{0, 2, 2, 4, 5}) && (list == std::vector<int32_t>{1, 4, 0, 3, 6}));
        build_point_list({}, 0, start, list);
        CHECK(start == std::vector<int32_t>{0} && list.empty());
        build_point_list({-1, -2}, 3, start, list);
        CHECK((start == std::vector<int32_t>{0, 0, 0, 0}) && list.empty());
        build_point_list({0, 7}, 2, start, list);  // an index past n_lp is left out (fba_snoop refuses it before)
        CHECK((start == std::vector<int32_t>{0, 1, 1}) && (list == std::vector<int32_t>{0}));
        std::printf("ok point list\n");
    }
    return 0;
}
