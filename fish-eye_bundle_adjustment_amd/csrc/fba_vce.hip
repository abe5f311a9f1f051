// fba_vce.hip -- variance component estimation over observation groups on the device (gfx950 / MI355X).
// No reference counterpart: main.m:397-402 fixes the weights 1 / Meas_std^2 before the loop.
//
// After the reliability part (launch_rel_q, fba_rel.hip) has left q = a Cx a' and the residuals v per local
// observation, the per-observation arrays stay on the device:
//   k_vce_sums     one thread per local observation, its x and y row: r = 1 - q / sigma^2, t = (s v / sigma)^2
//                  (vce_row, fba_vce.h) and the group id of either row (local order, -1 -> slot n_groups).  A wave
//                  loops over the groups PRESENT in it: the id of the first lane with a row left, every lane's
//                  contribution to that group (0 from non-members) through one fixed xor tree (32 .. 1) for r, t and
//                  the count, the members' rows cleared -- as many rounds as the wave holds distinct groups, whatever
//                  n_groups is.  Lane 0 stores the three sums in the wave's row of an LDS slab [4][n_groups + 1][3]
//                  (zeroed first); after a barrier the four rows are added in wave order into the block's row of the
//                  global slab [n_blocks][n_groups + 1][3].  Every entry of the global slab is written.
//   k_vce_finish   one workgroup: per (group, quantity) lane l adds the blocks l, l + 64, ... in ascending order and
//                  the 64 partial sums go through the same xor tree; then one thread per group applies vce_group (the
//                  estimate, the clamp, the factor, the status) and writes [n_groups + 1][6]: R T n sigma2 factor status.
//   k_vce_rescale  sw[row] *= factor[group[row]] (or = factor on the first switch-on), one double2 per observation.
// No atomics, no communication between workgroups: every sum has one fixed order, two calls are bitwise equal.
#include "fba_internal.h"
#include "fba_vce.h"

namespace fba {

constexpr int VCE_WAVES = 4;

__device__ __forceinline__ double vce_wave_sum(double v) {
    v += __shfl_xor(v, 32, 64);
    v += __shfl_xor(v, 16, 64);
    v += __shfl_xor(v, 8, 64);
    v += __shfl_xor(v, 4, 64);
    v += __shfl_xor(v, 2, 64);
    v += __shfl_xor(v, 1, 64);
    return v;
}

// a row's slot in [0, n_groups]: its group, or n_groups for -1 (the host checked the range; anything else counts as -1)
__device__ __forceinline__ int vce_slot(int id, int n_groups) { return (unsigned)id < (unsigned)n_groups ? id : n_groups; }

__global__ __launch_bounds__(256) void k_vce_sums(const double* __restrict__ q, const double* __restrict__ v,
                                                  const double* __restrict__ sw, const int32_t* __restrict__ grp,
                                                  int64_t n_obs, int n_groups, double sx, double sy,
                                                  double* __restrict__ slab) {
    extern __shared__ double wsum[];  // [VCE_WAVES][n_groups + 1][VCE_SUMS]
    const int row = (n_groups + 1) * VCE_SUMS;
    for (int i = threadIdx.x; i < VCE_WAVES * row; i += 256) wsum[i] = 0.0;
    __syncthreads();
    const int64_t o = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    int a0 = 0, a1 = 0;
    bool p0 = false, p1 = false;  // the row is still to be summed
    double r0 = 0.0, t0 = 0.0, r1 = 0.0, t1 = 0.0;
    if (o < n_obs) {
        const double2 qq = *reinterpret_cast<const double2*>(q + 2 * o);
        const double2 vv = *reinterpret_cast<const double2*>(v + 2 * o);
        const double2 ss = sw ? *reinterpret_cast<const double2*>(sw + 2 * o) : double2{1.0, 1.0};
        const int2 g = *reinterpret_cast<const int2*>(grp + 2 * o);
        a0 = vce_slot(g.x, n_groups);
        a1 = vce_slot(g.y, n_groups);
        vce_row(qq.x, vv.x, ss.x, sx, r0, t0);
        vce_row(qq.y, vv.y, ss.y, sy, r1, t1);
        p0 = p1 = true;
    }
    double* W = wsum + wave * row;
    for (;;) {
        const unsigned long long left = __ballot(p0 || p1);
        if (!left) break;
        const int g = __shfl(p0 ? a0 : a1, __ffsll(left) - 1, 64);  // the first remaining lane's group
        const bool m0 = p0 && a0 == g, m1 = p1 && a1 == g;
        const double sr = vce_wave_sum((m0 ? r0 : 0.0) + (m1 ? r1 : 0.0));
        const double st = vce_wave_sum((m0 ? t0 : 0.0) + (m1 ? t1 : 0.0));
        const double sn = vce_wave_sum((m0 ? 1.0 : 0.0) + (m1 ? 1.0 : 0.0));
        if (lane == 0) {  // g is visited once per wave
            W[VCE_SUMS * g] = sr;
            W[VCE_SUMS * g + 1] = st;
            W[VCE_SUMS * g + 2] = sn;
        }
        p0 = p0 && !m0;
        p1 = p1 && !m1;
    }
    __syncthreads();
    double* out = slab + (int64_t)blockIdx.x * row;
    for (int i = threadIdx.x; i < row; i += 256)
        out[i] = ((wsum[i] + wsum[row + i]) + wsum[2 * row + i]) + wsum[3 * row + i];
}

__global__ __launch_bounds__(256) void k_vce_finish(const double* __restrict__ slab, int64_t n_blocks, int n_groups,
                                                    double min_redundancy, double clip, double* __restrict__ out) {
    extern __shared__ double tot[];  // [n_groups + 1][VCE_SUMS]
    const int row = (n_groups + 1) * VCE_SUMS;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int i = wave; i < row; i += VCE_WAVES) {
        double s = 0.0;
        for (int64_t b = lane; b < n_blocks; b += 64) s += slab[b * row + i];
        s = vce_wave_sum(s);
        if (lane == 0) tot[i] = s;
    }
    __syncthreads();
    for (int g = threadIdx.x; g <= n_groups; g += 256) {
        const double R = tot[VCE_SUMS * g], T = tot[VCE_SUMS * g + 1], n = tot[VCE_SUMS * g + 2];
        double sigma2, factor;
        int status;
        if (g < n_groups) vce_group(R, T, n, min_redundancy, clip, sigma2, factor, status);
        else vce_rest(R, T, n, sigma2, factor, status);
        double* o = out + VCE_OUT * g;
        o[0] = R; o[1] = T; o[2] = n; o[3] = sigma2; o[4] = factor; o[5] = (double)status;
    }
}

__global__ __launch_bounds__(256) void k_vce_rescale(double* __restrict__ sw, const int32_t* __restrict__ grp,
                                                     const double* __restrict__ out, int64_t n_obs, int n_groups,
                                                     int first) {
    const int64_t o = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (o >= n_obs) return;
    const int2 g = *reinterpret_cast<const int2*>(grp + 2 * o);
    const double f0 = out[VCE_OUT * vce_slot(g.x, n_groups) + 4], f1 = out[VCE_OUT * vce_slot(g.y, n_groups) + 4];
    double2* s = reinterpret_cast<double2*>(sw + 2 * o);
    if (first) {
        *s = double2{f0, f1};
    } else {
        const double2 c = *s;
        *s = double2{c.x * f0, c.y * f1};
    }
}

// after launch_rel_q: the group sums of this rank's rows and the groups' rows [n_groups + 1][VCE_OUT] into d_out;
// d_slab: [ceil(n_obs / 256)][n_groups + 1][VCE_SUMS]
int launch_vce_sums(Ctx& c, const double* d_q, const int32_t* d_grp, int n_groups, double min_redundancy, double clip,
                    double* d_slab, double* d_out) {
    const int64_t n_blocks = (c.n_obs + 255) / 256;
    const size_t row = (size_t)(n_groups + 1) * VCE_SUMS * sizeof(double);
    if (n_blocks > 0) {
        k_vce_sums<<<(unsigned)n_blocks, 256, VCE_WAVES * row, c.stream>>>(d_q, c.d_res, c.weights_on ? c.d_sw : nullptr, d_grp,
                                                                          c.n_obs, n_groups, c.set.meas_std_x,
                                                                          c.set.meas_std_y, d_slab);
        FBA_HIP(hipGetLastError());
    }
    k_vce_finish<<<1, 256, row, c.stream>>>(d_slab, n_blocks, n_groups, min_redundancy, clip, d_out);
    FBA_HIP(hipGetLastError());
    return FBA_OK;
}

// d_sw *= the factors of d_out (first: d_sw = the factors, the context had no weights)
int launch_vce_rescale(Ctx& c, const int32_t* d_grp, const double* d_out, int n_groups, bool first) {
    if (c.n_obs == 0) return FBA_OK;
    k_vce_rescale<<<(unsigned)((c.n_obs + 255) / 256), 256, 0, c.stream>>>(c.d_sw, d_grp, d_out, c.n_obs, n_groups, first ? 1 : 0);
    FBA_HIP(hipGetLastError());
    return FBA_OK;
}

}  // namespace fba
