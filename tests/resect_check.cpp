// resect_check.cpp -- stand-alone checker of the space resection's host-visible routines (tests/test_resect_host.py
// builds it with -Xarch_host -fsanitize=address,undefined -- the host compilation only -- together with
// fba_api_host.cpp / fba_plan.cpp / fba_order.cpp and runs it directly; no GPU, no HIP call).
//
// Drives csrc/fba_resect.h's per-image routines through the host's source of sums over the edge cases -- exact data of
// every Type and both sides of W, 0 / 5 / 6 points, coplanar points, a NaN point, every usable flag off, phi at a right
// angle, a singular 6 x 6 system -- and fba_plan.cpp's image-list builder: an image without observations, an empty
// problem, no images, slots out of range.  Every case also goes through the exported fba_resect_host, which must give
// the same numbers; then one refusal per argument check of it.  One "ok <case>" line per case; any failure prints
// "FAIL ..." and exits 1.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <random>
#include <vector>

#include "../fish-eye_bundle_adjustment_amd/csrc/fba_internal.h"
#include "../fish-eye_bundle_adjustment_amd/csrc/fba_resect.h"

using namespace fba;

#define CHECK(cond)                                                     \
    do {                                                                \
        if (!(cond)) {                                                  \
            std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); \
            std::exit(1);                                               \
        }                                                               \
    } while (0)

struct Scene {
    std::vector<double> rec;
    double eop[6];
    double c = 650.0, ydir = -1.0;
};

// n points in front of (side < 0: W < 0) the camera at eop, exact rays and corrected coordinates
static Scene make_scene(int type, int n, const double* eop, double side, bool coplanar, unsigned seed) {
    Scene s;
    for (int q = 0; q < 6; ++q) s.eop[q] = eop[q];
    ResectPose P;
    resect_pose(eop, P);
    std::mt19937 rng(seed);
    std::uniform_real_distribution<double> uv(-800.0, 800.0), w(900.0, 2500.0);
    for (int i = 0; i < n; ++i) {
        const double U = uv(rng), V = uv(rng), W = side * (coplanar ? 1500.0 + 0.01 * U : w(rng));
        double X[3];
        for (int q = 0; q < 3; ++q) X[q] = eop[q] + P.M[q] * U + P.M[3 + q] * V + P.M[6 + q] * W;  // X = C + M'(U V W)
        double px, py, jp[6];
        ray_project(type, P.M, X[0] - eop[0], X[1] - eop[1], X[2] - eop[2], s.c, s.ydir, px, py, jp);
        const double nrm = std::sqrt(U * U + V * V + W * W), sg = W < 0.0 ? -1.0 : 1.0;  // ray_unproject's d has d2 >= 0
        const double r[RESECT_REC] = {px, py, sg * U / nrm, sg * V / nrm, sg * W / nrm, X[0], X[1], X[2]};
        s.rec.insert(s.rec.end(), r, r + RESECT_REC);
    }
    return s;
}

struct Result {
    double eop[6], qual[5];
    int status;
};
static Result solve(int type, const Scene& s, int64_t n, const int32_t* use, int iters) {
    const ResectHostSrc src{s.rec.data(), use, n, s.c, s.ydir};
    std::vector<double> A(144), V(144);  // on the heap: the sanitizer watches their bounds
    const double cur[6] = {1, 2, 3, 4, 5, 6};
    Result r;
    resect_solve(src, type, 1.0 / 0.09, 1.0 / 0.09, iters, 1e-6, 1e-10, A.data(), V.data(), cur, r.eop, r.qual, r.status);
    // the exported entry point on the same records, from and into arrays of exactly the documented sizes: the same
    // status and quality, and the same pose where there is one (FEW and WEAK: zeros, where the routine keeps `cur`)
    std::vector<double> xyz(3 * (size_t)n), ray(5 * (size_t)n), eop(6), qual(5);
    std::vector<int32_t> rst((size_t)n);
    for (int64_t i = 0; i < n; ++i) {
        for (int q = 0; q < 5; ++q) ray[5 * i + q] = s.rec[RESECT_REC * i + q];
        for (int q = 0; q < 3; ++q) xyz[3 * i + q] = s.rec[RESECT_REC * i + 5 + q];
        rst[(size_t)i] = (!use || use[i]) ? FBA_RAY_OK : FBA_RAY_DOMAIN;
    }
    const fba_resect_options op{FBA_RESECT_USE_CONTROL, iters, 0, 0, 1e-6, 1e-10};
    int32_t st = -1;
    CHECK(fba_resect_host(type, n, xyz.data(), ray.data(), use ? rst.data() : nullptr, s.c, s.ydir, 0.3, 0.3, &op, eop.data(),
                          qual.data(), &st) == FBA_OK);
    const bool pose = r.status == FBA_RESECT_OK || r.status == FBA_RESECT_REFINE;
    CHECK(st == r.status && !std::memcmp(qual.data(), r.qual, sizeof r.qual));
    for (int q = 0; q < 6; ++q) CHECK(pose ? eop[q] == r.eop[q] : eop[q] == 0.0);
    return r;
}

static bool refused(int rc, int code, const char* text) { return rc == code && !std::strcmp(fba_last_error(), text); }

static double centre_error(const Result& r, const Scene& s) {
    double e = 0.0;
    for (int q = 0; q < 3; ++q) e = std::fmax(e, std::fabs(r.eop[q] - s.eop[q]));
    return e;
}
static double rotation_error(const Result& r, const Scene& s) {
    ResectPose a, b;
    resect_pose(r.eop, a);
    resect_pose(s.eop, b);
    double e = 0.0;
    for (int q = 0; q < 9; ++q) e = std::fmax(e, std::fabs(a.M[q] - b.M[q]));
    return e;
}

int main() {
    const double eop[6] = {100.0, -200.0, 3000.0, 0.1, -0.15, 2.0};
    for (int type = FBA_TYPE_FISHEYE; type <= FBA_TYPE_STEREOGRAPHIC; ++type)
        for (double side : {-1.0, 1.0}) {
            const Scene s = make_scene(type, 30, eop, side, false, 7u + (unsigned)type);
            for (int iters : {0, 10}) {
                const Result r = solve(type, s, 30, nullptr, iters);
                CHECK(r.status == FBA_RESECT_OK || (iters > 0 && r.status == FBA_RESECT_REFINE));
                CHECK(r.qual[0] == 30.0 && r.qual[1] > 1e-4 && r.qual[3] <= 1e-8);
                CHECK(centre_error(r, s) <= 1e-8 && rotation_error(r, s) <= 1e-11);
                CHECK(r.qual[4] == (side > 0.0 ? 1.0 : 0.0));
            }
        }
    std::printf("ok exact\n");
    {
        const Scene s = make_scene(FBA_TYPE_FISHEYE, 30, eop, -1.0, false, 3u);
        Result r = solve(FBA_TYPE_FISHEYE, s, 0, nullptr, 10);  // no record is read
        CHECK(r.status == FBA_RESECT_FEW && r.qual[0] == 0.0 && r.eop[0] == 1.0 && r.eop[5] == 6.0);
        r = solve(FBA_TYPE_FISHEYE, s, 5, nullptr, 10);
        CHECK(r.status == FBA_RESECT_FEW && r.qual[0] == 5.0 && r.qual[1] == 0.0 && r.eop[3] == 4.0);
        r = solve(FBA_TYPE_FISHEYE, s, 6, nullptr, 0);
        CHECK(r.status == FBA_RESECT_OK && r.qual[0] == 6.0);
        std::vector<int32_t> use(30, 0);
        r = solve(FBA_TYPE_FISHEYE, s, 30, use.data(), 10);
        CHECK(r.status == FBA_RESECT_FEW && r.qual[0] == 0.0);
        for (int i = 0; i < 30; i += 2) use[i] = 1;  // every other record
        r = solve(FBA_TYPE_FISHEYE, s, 30, use.data(), 10);
        CHECK(r.status != FBA_RESECT_FEW && r.qual[0] == 15.0 && centre_error(r, s) <= 1e-7);
    }
    std::printf("ok few\n");
    {
        const Scene s = make_scene(FBA_TYPE_FISHEYE, 30, eop, -1.0, true, 5u);
        const Result r = solve(FBA_TYPE_FISHEYE, s, 30, nullptr, 10);
        CHECK(r.status == FBA_RESECT_WEAK && r.qual[1] <= 1e-12 && r.qual[2] == 0.0 && r.qual[3] == 0.0 && r.eop[0] == 1.0);
    }
    std::printf("ok coplanar\n");
    {
        Scene s = make_scene(FBA_TYPE_PINHOLE, 12, eop, -1.0, false, 9u);
        s.rec[RESECT_REC * 4 + 6] = std::numeric_limits<double>::quiet_NaN();
        Result r = solve(FBA_TYPE_PINHOLE, s, 12, nullptr, 10);
        CHECK(r.status == FBA_RESECT_WEAK && r.eop[0] == 1.0 && r.qual[2] == 0.0);
        for (double& v : s.rec) v = 0.0;  // every point at the origin, every direction zero
        r = solve(FBA_TYPE_PINHOLE, s, 12, nullptr, 10);
        CHECK(r.status == FBA_RESECT_WEAK && r.eop[0] == 1.0);
    }
    std::printf("ok nan\n");
    for (double sign : {1.0, -1.0}) {
        const double g[6] = {100.0, -200.0, 50.0, 0.3, sign * std::acos(-1.0) / 2, -0.7};
        const Scene s = make_scene(FBA_TYPE_FISHEYE, 30, g, -1.0, false, 11u);
        const Result r = solve(FBA_TYPE_FISHEYE, s, 30, nullptr, 10);
        CHECK(r.status == FBA_RESECT_OK || r.status == FBA_RESECT_REFINE);
        CHECK(rotation_error(r, s) <= 1e-6 && centre_error(r, s) <= 1e-3);
    }
    std::printf("ok gimbal\n");
    {
        double N[21] = {0}, g[6] = {1, 1, 1, 1, 1, 1}, x[6];
        for (int a = 0; a < 6; ++a) N[a * (a + 1) / 2 + a] = 2.0 + a;
        CHECK(resect_chol6(N, g, x) && std::fabs(x[0] - 0.5) <= 1e-15 && std::fabs(x[5] - 1.0 / 7.0) <= 1e-15);
        N[5] = 0.0;  // a zero pivot
        CHECK(!resect_chol6(N, g, x));
        N[5] = std::numeric_limits<double>::quiet_NaN();
        CHECK(!resect_chol6(N, g, x));
    }
    std::printf("ok cholesky\n");
    {
        std::vector<int32_t> start, list;
        build_image_list({2, 0, 2, 4, 0, 2}, 5, start, list);  // images 1 and 3 without observations
        CHECK((start == std::vector<int32_t>{0, 2, 2, 5, 5, 6}) && (list == std::vector<int32_t>{1, 4, 0, 2, 5, 3}));
        build_image_list({}, 3, start, list);  // an empty problem
        CHECK((start == std::vector<int32_t>{0, 0, 0, 0}) && list.empty());
        build_image_list({}, 0, start, list);
        CHECK(start == std::vector<int32_t>{0} && list.empty());
        build_image_list({0, 7, -1, 1}, 2, start, list);  // slots out of range are left out
        CHECK((start == std::vector<int32_t>{0, 1, 2}) && (list == std::vector<int32_t>{0, 3}));
        std::mt19937 rng(1);
        std::vector<int32_t> img(1000);
        for (auto& e : img) e = (int32_t)(rng() % 37);
        build_image_list(img, 40, start, list);
        CHECK(start.size() == 41 && list.size() == 1000 && start[40] == 1000 && start[38] == start[37]);
        for (int e = 0; e < 40; ++e)
            for (int i = start[e]; i < start[e + 1]; ++i) {
                CHECK(img[list[i]] == e);
                CHECK(i == start[e] || list[i - 1] < list[i]);  // ascending inside an image
            }
    }
    std::printf("ok image_list\n");
    {
        // the rows of an image read through the list, as k_resect_gather lays them out: the last image's records end
        // at the buffer's end
        const Scene s = make_scene(FBA_TYPE_EQUISOLID, 8, eop, 1.0, false, 13u);
        Scene tail = s;
        tail.rec.assign(s.rec.end() - RESECT_REC * 7, s.rec.end());
        tail.rec.shrink_to_fit();
        const Result r = solve(FBA_TYPE_EQUISOLID, tail, 7, nullptr, 10);
        CHECK(r.status != FBA_RESECT_FEW && r.qual[0] == 7.0);
    }
    std::printf("ok tail\n");
    {  // fba_resect_host: one refusal per argument check; every output optional, the defaults of a NULL options pointer
        const Scene s = make_scene(FBA_TYPE_FISHEYE, 6, eop, -1.0, false, 17u);
        std::vector<double> xyz(18), ray(30);
        for (int i = 0; i < 6; ++i) {
            for (int q = 0; q < 5; ++q) ray[5 * i + q] = s.rec[RESECT_REC * i + q];
            for (int q = 0; q < 3; ++q) xyz[3 * i + q] = s.rec[RESECT_REC * i + 5 + q];
        }
        auto call = [&](int type, int64_t n, const double* X, double sx, const fba_resect_options* o) {
            return fba_resect_host(type, n, X, ray.data(), nullptr, s.c, s.ydir, sx, 0.3, o, nullptr, nullptr, nullptr);
        };
        CHECK(refused(call(9, 6, xyz.data(), 0.3, nullptr), FBA_ERR_TYPE, "fba_resect_host: invalid type"));
        const char* args = "fba_resect_host: n >= 0, xyz and ray not NULL, the standard deviations > 0";
        CHECK(refused(call(FBA_TYPE_FISHEYE, -1, xyz.data(), 0.3, nullptr), FBA_ERR_ARG, args));
        CHECK(refused(call(FBA_TYPE_FISHEYE, 6, nullptr, 0.3, nullptr), FBA_ERR_ARG, args));
        CHECK(refused(call(FBA_TYPE_FISHEYE, 6, xyz.data(), 0.0, nullptr), FBA_ERR_ARG, args));
        const fba_resect_options bad{FBA_RESECT_USE_CONTROL, -1, 0, 0, 1e-6, 1e-10};
        CHECK(refused(call(FBA_TYPE_FISHEYE, 6, xyz.data(), 0.3, &bad), FBA_ERR_ARG,
                      "fba_resect_host: use CONTROL or ALL, refine_iters >= 0, min_ratio and refine_tol finite and >= 0"));
        CHECK(call(FBA_TYPE_FISHEYE, 6, xyz.data(), 0.3, nullptr) == FBA_OK);
        CHECK(call(FBA_TYPE_FISHEYE, 0, nullptr, 0.3, nullptr) == FBA_OK);
    }
    std::printf("ok entry point\n");
    return 0;
}
