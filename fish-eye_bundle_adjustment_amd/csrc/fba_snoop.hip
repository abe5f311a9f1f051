// fba_snoop.hip -- Baarda data snooping over the image points on the device (gfx950 / MI355X).
// No reference counterpart: main.m never tests a measurement.
//
// After launch_vce_q (fba_cov.hip) has left q = a Cx a' and the residuals v per local observation, one round runs:
//   k_snoop_seg     one wave64 per segment -- the local tie points (d_pl_*), then the image slots (d_il_*).  Lane l takes
//                   the entries l, l + 64, ... of the segment's list in ascending order: the count of its points that
//                   are not excluded, and (with the candidate flags given) the best candidate by snoop_better, both
//                   through one fixed xor tree (32 .. 1).  Launched twice: the counts before k_snoop_stat, which needs
//                   them for the candidate flag, and the winners after it.
//   k_snoop_stat    one thread per local observation: W or W~ (snoop_point_stat, fba_snoop.h), the candidate flag
//                   (snoop_candidate, with the two counts) and the back-check's verdict (snoop_readmit).
//   k_snoop_pick    one thread per observation: a candidate that won both its segments writes itself into
//                   pick[image slot] (-1 before: at most one per image, so no two threads meet); the block's number of
//                   back-check verdicts and of excluded points and its largest active W go to its row of a partial slab.
//   k_snoop_counts  one workgroup: the picks over the image slots and the block rows in ascending order -> out
//                   [SNOOP_OUT] picks, verdicts, excluded, largest active W (counts and a maximum: any order gives the
//                   same value, the order is fixed all the same).
//   k_snoop_apply   one thread per observation: the picks become EXCLUDED (mode 1) or the verdicts READMITTED (mode 2),
//                   then both sqrt weights as one double2: SNOOP_EPS s0 for an excluded point, s0 -- bit for bit the
//                   starting value -- for every other.
// The host (fba_snoop, fba_capi.cpp) reads out between k_snoop_counts and k_snoop_apply: it decides the stops
// (max_rounds, max_share) and switches the weights on before the first apply of an unweighted context.
// No atomics, no communication between workgroups: two calls are bitwise equal.
#include "fba_internal.h"
#include "fba_snoop.h"

#include <algorithm>

namespace fba {

// the best candidate of a wave by snoop_better; lanes without one carry idx -1
__device__ __forceinline__ void snoop_wave_best(double& W, long long& row, int& idx) {
#pragma unroll
    for (int w = 32; w > 0; w >>= 1) {
        const double W2 = __shfl_xor(W, w, 64);
        const long long r2 = __shfl_xor(row, w, 64);
        const int i2 = __shfl_xor(idx, w, 64);
        if (i2 >= 0 && (idx < 0 || snoop_better(W2, r2, W, row))) { W = W2; row = r2; idx = i2; }
    }
}
__device__ __forceinline__ int snoop_wave_isum(int v) {
#pragma unroll
    for (int w = 32; w > 0; w >>= 1) v += __shfl_xor(v, w, 64);
    return v;
}
__device__ __forceinline__ double snoop_wave_max(double v) {
#pragma unroll
    for (int w = 32; w > 0; w >>= 1) v = fmax(v, __shfl_xor(v, w, 64));
    return v;
}

__global__ __launch_bounds__(256) void k_snoop_seg(const int32_t* __restrict__ pl_start, const int32_t* __restrict__ pl_obs,
                                                   const int32_t* __restrict__ il_start, const int32_t* __restrict__ il_obs,
                                                   int n_lp, int n_seg, const uint8_t* __restrict__ state,
                                                   const uint8_t* __restrict__ cand, const double* __restrict__ W,
                                                   const int64_t* __restrict__ obs_pho, int32_t* __restrict__ win,
                                                   int32_t* __restrict__ cnt) {
    const int seg = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (seg >= n_seg) return;  // (whole waves leave: the shuffles below see full waves)
    const bool tie = seg < n_lp;
    const int32_t* start = tie ? pl_start + seg : il_start + (seg - n_lp);
    const int32_t* list = tie ? pl_obs : il_obs;
    const int e0 = start[0], e1 = start[1];
    int n = 0, idx = -1;
    double bw = 0.0;
    long long br = 0;
    for (int e = e0 + lane; e < e1; e += 64) {
        const int o = list[e];
        n += state[o] != SNOOP_EXCLUDED;
        if (cand && cand[o]) {
            const long long r = obs_pho[o];
            if (idx < 0 || snoop_better(W[o], r, bw, br)) { bw = W[o]; br = r; idx = o; }
        }
    }
    n = snoop_wave_isum(n);
    if (cand) {
        snoop_wave_best(bw, br, idx);
        if (lane == 0) win[seg] = idx;
    } else if (lane == 0) {
        cnt[seg] = n;
    }
}

__global__ __launch_bounds__(256) void k_snoop_stat(const double* __restrict__ q, const double* __restrict__ v,
                                                    const double* __restrict__ sw, const double* __restrict__ s0,
                                                    const uint8_t* __restrict__ state, const int32_t* __restrict__ pt,
                                                    const int32_t* __restrict__ img, const int32_t* __restrict__ cnt,
                                                    int64_t n_obs, int n_lp, int n_img, double sx, double sy, double crit,
                                                    int min_rays, int min_img_points, double* __restrict__ W,
                                                    uint8_t* __restrict__ cand, uint8_t* __restrict__ back) {
    const int64_t o = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (o >= n_obs) return;
    const double2 qq = *reinterpret_cast<const double2*>(q + 2 * o);
    const double2 vv = *reinterpret_cast<const double2*>(v + 2 * o);
    const double2 ss = sw ? *reinterpret_cast<const double2*>(sw + 2 * o) : double2{1.0, 1.0};
    const double2 s00 = *reinterpret_cast<const double2*>(s0 + 2 * o);
    const uint8_t st = state[o];
    const double w = snoop_point_stat(st, qq.x, qq.y, vv.x, vv.y, ss.x, ss.y, s00.x, s00.y, sx, sy);
    const int p = pt[o], e = img[o];
    const int ct = ((unsigned)p < (unsigned)n_lp) ? cnt[p] : -1;
    const int ci = ((unsigned)e < (unsigned)n_img) ? cnt[n_lp + e] : 0;
    W[o] = w;
    cand[o] = snoop_candidate(st, w, crit, ct, ci, min_rays, min_img_points) ? 1 : 0;
    back[o] = snoop_readmit(st, w, crit) ? 1 : 0;
}

__global__ __launch_bounds__(256) void k_snoop_pick(const uint8_t* __restrict__ cand, const uint8_t* __restrict__ back,
                                                    const uint8_t* __restrict__ state, const double* __restrict__ W,
                                                    const int32_t* __restrict__ pt, const int32_t* __restrict__ img,
                                                    const int32_t* __restrict__ win, int64_t n_obs, int n_lp, int n_img,
                                                    int32_t* __restrict__ pick, double* __restrict__ part) {
    __shared__ double sh[4][SNOOP_PART];
    const int64_t o = (int64_t)blockIdx.x * 256 + threadIdx.x;
    int nb = 0, nx = 0;
    double mw = 0.0;
    if (o < n_obs) {
        const int p = pt[o], e = img[o];
        if (cand[o] && (unsigned)e < (unsigned)n_img && win[n_lp + e] == (int)o &&
            (!((unsigned)p < (unsigned)n_lp) || win[p] == (int)o))
            pick[e] = (int32_t)o;
        nb = back[o];
        nx = state[o] == SNOOP_EXCLUDED;
        if (!nx) mw = W[o];  // (fmax drops a NaN)
    }
    nb = snoop_wave_isum(nb);
    nx = snoop_wave_isum(nx);
    mw = snoop_wave_max(mw);
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { sh[wave][0] = nb; sh[wave][1] = nx; sh[wave][2] = mw; }
    __syncthreads();
    if (threadIdx.x == 0) {
        double* r = part + (int64_t)blockIdx.x * SNOOP_PART;
        r[0] = ((sh[0][0] + sh[1][0]) + sh[2][0]) + sh[3][0];
        r[1] = ((sh[0][1] + sh[1][1]) + sh[2][1]) + sh[3][1];
        r[2] = fmax(fmax(sh[0][2], sh[1][2]), fmax(sh[2][2], sh[3][2]));
    }
}

__global__ __launch_bounds__(256) void k_snoop_counts(const int32_t* __restrict__ pick, int n_img,
                                                      const double* __restrict__ part, int64_t n_blocks,
                                                      double* __restrict__ out) {
    __shared__ double sh[4][SNOOP_OUT];
    int np = 0;
    for (int e = threadIdx.x; e < n_img; e += 256) np += pick[e] >= 0;
    double nb = 0.0, nx = 0.0, mw = 0.0;
    for (int64_t b = threadIdx.x; b < n_blocks; b += 256) {
        nb += part[b * SNOOP_PART];
        nx += part[b * SNOOP_PART + 1];
        mw = fmax(mw, part[b * SNOOP_PART + 2]);
    }
    np = snoop_wave_isum(np);
    const int inb = snoop_wave_isum((int)nb), inx = snoop_wave_isum((int)nx);  // (counts: exact in either type)
    mw = snoop_wave_max(mw);
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { sh[wave][0] = np; sh[wave][1] = inb; sh[wave][2] = inx; sh[wave][3] = mw; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int k = 0; k < 3; ++k) out[k] = ((sh[0][k] + sh[1][k]) + sh[2][k]) + sh[3][k];
        out[3] = fmax(fmax(sh[0][3], sh[1][3]), fmax(sh[2][3], sh[3][3]));
    }
}

__global__ __launch_bounds__(256) void k_snoop_init(const double* __restrict__ sw, double* __restrict__ s0, int64_t n_obs) {
    const int64_t o = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (o >= n_obs) return;
    *reinterpret_cast<double2*>(s0 + 2 * o) = sw ? *reinterpret_cast<const double2*>(sw + 2 * o) : double2{1.0, 1.0};
}

__global__ __launch_bounds__(256) void k_snoop_apply(const int32_t* __restrict__ pick, const uint8_t* __restrict__ back,
                                                     const int32_t* __restrict__ img, const double* __restrict__ s0,
                                                     int64_t n_obs, int n_img, int mode, uint8_t* __restrict__ state,
                                                     double* __restrict__ sw) {
    const int64_t o = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (o >= n_obs) return;
    uint8_t st = state[o];
    const int e = img[o];
    if (mode == 1 && (unsigned)e < (unsigned)n_img && pick[e] == (int)o) st = SNOOP_EXCLUDED;
    if (mode == 2 && back[o]) st = SNOOP_READMITTED;
    state[o] = st;
    const double2 s = *reinterpret_cast<const double2*>(s0 + 2 * o);
    *reinterpret_cast<double2*>(sw + 2 * o) = st == SNOOP_EXCLUDED ? double2{SNOOP_EPS * s.x, SNOOP_EPS * s.y} : s;
}

int launch_snoop_init(Ctx& c, const SnoopBufs& b) {
    if (c.n_obs == 0) return FBA_OK;
    k_snoop_init<<<(unsigned)((c.n_obs + 255) / 256), 256, 0, c.stream>>>(c.weights_on ? c.d_sw : nullptr, b.s0, c.n_obs);
    FBA_HIP(hipGetLastError());
    return FBA_OK;
}

int launch_snoop_round(Ctx& c, const SnoopBufs& b, const double* d_q, int min_rays, int min_img_points, double crit) {
    const int n_lp = (int)c.n_pl, n_img = c.L.n_img, n_seg = n_lp + n_img;  // (n_lp: every point of the list)
    const int64_t n_blocks = (c.n_obs + 255) / 256;
    const unsigned seg_blocks = (unsigned)((n_seg + 3) / 4);
    FBA_HIP(hipMemsetAsync(b.pick, 0xFF, sizeof(int32_t) * std::max(n_img, 1), c.stream));
    if (c.n_obs > 0 && n_seg > 0) {
        k_snoop_seg<<<seg_blocks, 256, 0, c.stream>>>(c.d_pl_start, c.d_pl_obs, c.d_il_start, c.d_il_obs, n_lp, n_seg, b.state,
                                                      nullptr, nullptr, c.d_obs_pho, b.win, b.cnt);
        FBA_HIP(hipGetLastError());
        k_snoop_stat<<<(unsigned)n_blocks, 256, 0, c.stream>>>(d_q, c.d_res, c.weights_on ? c.d_sw : nullptr, b.s0, b.state,
                                                               c.d_pt, c.d_img, b.cnt, c.n_obs, n_lp, n_img, c.set.meas_std_x,
                                                               c.set.meas_std_y, crit, min_rays, min_img_points, b.W, b.cand,
                                                               b.back);
        FBA_HIP(hipGetLastError());
        k_snoop_seg<<<seg_blocks, 256, 0, c.stream>>>(c.d_pl_start, c.d_pl_obs, c.d_il_start, c.d_il_obs, n_lp, n_seg, b.state,
                                                      b.cand, b.W, c.d_obs_pho, b.win, b.cnt);
        FBA_HIP(hipGetLastError());
        k_snoop_pick<<<(unsigned)n_blocks, 256, 0, c.stream>>>(b.cand, b.back, b.state, b.W, c.d_pt, c.d_img, b.win, c.n_obs,
                                                               n_lp, n_img, b.pick, b.part);
        FBA_HIP(hipGetLastError());
    }
    k_snoop_counts<<<1, 256, 0, c.stream>>>(b.pick, n_img, b.part, c.n_obs > 0 && n_seg > 0 ? n_blocks : 0, b.out);
    FBA_HIP(hipGetLastError());
    return FBA_OK;
}

int launch_snoop_apply(Ctx& c, const SnoopBufs& b, int mode) {
    if (c.n_obs == 0) return FBA_OK;
    k_snoop_apply<<<(unsigned)((c.n_obs + 255) / 256), 256, 0, c.stream>>>(b.pick, b.back, c.d_img, b.s0, c.n_obs, c.L.n_img,
                                                                          mode, b.state, c.d_sw);
    FBA_HIP(hipGetLastError());
    return FBA_OK;
}

}  // namespace fba
