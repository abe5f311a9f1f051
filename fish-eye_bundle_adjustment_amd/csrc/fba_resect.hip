// fba_resect.hip -- space resection of the images from object points and the measured image rays, for gfx950 (MI355X).
// No reference counterpart: Buildxhat.m:22-63 copies the exterior orientation's starting values from the .ext file.
//
//   k_resect_gather  one thread per entry of the image list (Ctx::d_il_obs: the local observations by image slot,
//                    ascending inside an image): the closed-form image ray of the measurement in the CAMERA frame
//                    (ray_unproject, fba_ray.h) from k_params' camera table, the object point from d_ctl (control) or
//                    from d_xfull at d_xoff (tie); stores the record [xu yu d0 d1 d2 X Y Z] (64 B) and the usable flag
//                    (status OK and of the `use` class) in LIST order, so an image's records are contiguous
//   k_resect         one wave64 per image slot, 4 per workgroup: resect_solve (fba_resect.h) over the image's records.
//                    Lane l takes the records l, l + 64, ... in ascending order; every sum -- the count and the
//                    centroid, the mean distance, the 60 Gram products, per refinement pass 21 + 6 sums, ssq, dsum and
//                    the side count -- then goes through a fixed xor tree (32, 16, 8, 4, 2, 1): fp addition commutes,
//                    so all 64 lanes hold bitwise the same sums, take the same branches, and the result does not
//                    depend on the launch geometry.  The 12 x 12 Gram matrix and its eigenvectors live in LDS, 2 x 144
//                    doubles per wave (9216 B per workgroup): every lane runs the same Jacobi rotations and stores the
//                    same values (a wave's LDS operations complete in order, and a lane reads back what it stored
//                    itself), so no barrier is needed.  No atomics, no communication between workgroups; padding
//                    slots are skipped and the outputs go to the image's EXT row (Ctx::d_il_ext).
#include "fba_internal.h"
#include "fba_resect.h"

namespace fba {

constexpr int RS_WAVES = 4;  // waves (images) per k_resect workgroup

template <int NK>
__global__ __launch_bounds__(256) void k_resect_gather(const double* __restrict__ xy, const int32_t* __restrict__ cam,
                                                       const int32_t* __restrict__ pt, const int32_t* __restrict__ xoff,
                                                       const double* __restrict__ ctl, const double* __restrict__ xfull,
                                                       const double* __restrict__ cam_tab, const int32_t* __restrict__ il_obs,
                                                       int64_t n_obs, int type, int cam_stride, int use_all,
                                                       double* __restrict__ rec, int32_t* __restrict__ use) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n_obs) return;
    const int64_t o = il_obs[i];
    const double2 xyv = *reinterpret_cast<const double2*>(xy + 2 * o);
    const double* ct = cam_tab + (int64_t)cam[o] * cam_stride;
    double xu, yu, d0, d1, d2;
    const int st = ray_unproject<NK>(xyv.x, xyv.y, ct[0], ct[1], ct[2], ct[3], ct[4], ct[5], ct + CAM_TAB_HDR, NK, type,
                                     xu, yu, d0, d1, d2);
    const int p = pt[o];
    const double* X = p >= 0 ? xfull + xoff[o] : ctl + 3 * (int64_t)(-1 - p);
    double2* r = reinterpret_cast<double2*>(rec + RESECT_REC * i);
    r[0] = double2{xu, yu};
    r[1] = double2{d0, d1};
    r[2] = double2{d2, X[0]};
    r[3] = double2{X[1], X[2]};
    use[i] = (st == FBA_RAY_OK && (use_all || p < 0)) ? 1 : 0;
}

// sum over the 64 lanes of the wave, the same value in all of them
__device__ __forceinline__ double wave_sum(double v) {
    v += __shfl_xor(v, 32, 64);
    v += __shfl_xor(v, 16, 64);
    v += __shfl_xor(v, 8, 64);
    v += __shfl_xor(v, 4, 64);
    v += __shfl_xor(v, 2, 64);
    v += __shfl_xor(v, 1, 64);
    return v;
}

// the wave's source of sums (resect_solve): the records [i0, i1) of one image
struct ResectWaveSrc {
    const double* __restrict__ rec;
    const int32_t* __restrict__ use;
    const int32_t* __restrict__ il_obs;
    const int32_t* __restrict__ cam;
    const double* __restrict__ cam_tab;
    int cam_stride, i0, i1, lane;

    __device__ __forceinline__ void moments(double* o) const {
        double n = 0.0, s0 = 0.0, s1 = 0.0, s2 = 0.0;
        for (int i = i0 + lane; i < i1; i += 64) {
            if (!use[i]) continue;
            const double* r = rec + RESECT_REC * (int64_t)i;
            n += 1.0; s0 += r[5]; s1 += r[6]; s2 += r[7];
        }
        o[0] = wave_sum(n); o[1] = wave_sum(s0); o[2] = wave_sum(s1); o[3] = wave_sum(s2);
    }
    __device__ __forceinline__ double spread(double m0, double m1, double m2) const {
        double d = 0.0;
        for (int i = i0 + lane; i < i1; i += 64) {
            if (!use[i]) continue;
            const double* r = rec + RESECT_REC * (int64_t)i;
            d += sqrt((r[5] - m0) * (r[5] - m0) + (r[6] - m1) * (r[6] - m1) + (r[7] - m2) * (r[7] - m2));
        }
        return wave_sum(d);
    }
    template <int I, int K>
    __device__ __forceinline__ static void gram_block(double (&g)[10], double* A) {
#pragma unroll
        for (int q = 0; q < 10; ++q) g[q] = wave_sum(g[q]);
        resect_gram_fill<I, K>(g, A);
    }
    __device__ __forceinline__ void gram(double m0, double m1, double m2, double is, double* A) const {
        double g0[10], g1[10], g2[10], g3[10], g4[10], g5[10];
#pragma unroll
        for (int q = 0; q < 10; ++q) g0[q] = g1[q] = g2[q] = g3[q] = g4[q] = g5[q] = 0.0;
        for (int i = i0 + lane; i < i1; i += 64) {
            if (!use[i]) continue;
            resect_gram_add(rec + RESECT_REC * (int64_t)i, m0, m1, m2, is, g0, g1, g2, g3, g4, g5);
        }
        gram_block<0, 0>(g0, A); gram_block<0, 1>(g1, A); gram_block<0, 2>(g2, A);
        gram_block<1, 1>(g3, A); gram_block<1, 2>(g4, A); gram_block<2, 2>(g5, A);
    }
    __device__ __forceinline__ void eval(int type, const ResectPose& P, double wx, double wy, double* acc) const {
#pragma unroll
        for (int q = 0; q < RESECT_EVAL; ++q) acc[q] = 0.0;
        for (int i = i0 + lane; i < i1; i += 64) {
            if (!use[i]) continue;
            const double* ct = cam_tab + (int64_t)cam[il_obs[i]] * cam_stride;
            resect_eval_add(type, P, rec + RESECT_REC * (int64_t)i, ct[2], ct[3], wx, wy, acc);
        }
#pragma unroll
        for (int q = 0; q < RESECT_EVAL; ++q) acc[q] = wave_sum(acc[q]);
    }
};

__global__ __launch_bounds__(64 * RS_WAVES) void k_resect(
    const double* __restrict__ rec, const int32_t* __restrict__ use, const int32_t* __restrict__ il_start,
    const int32_t* __restrict__ il_obs, const int32_t* __restrict__ il_ext, const int32_t* __restrict__ cam,
    const double* __restrict__ cam_tab, int cam_stride, int n_slots, int type, double wx, double wy, int refine_iters,
    double min_ratio, double refine_tol, int write, double* __restrict__ xfull, double* __restrict__ eop_out,
    double* __restrict__ qual_out, int32_t* __restrict__ stat) {
    __shared__ double sh[RS_WAVES][288];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int slot = blockIdx.x * RS_WAVES + wave;  // whole waves leave together
    if (slot >= n_slots) return;
    const int ext = il_ext[slot];
    if (ext < 0) return;
    double* xcur = xfull + 6 * (int64_t)slot;
    double cur[6], eop[6], qual[5];
#pragma unroll
    for (int q = 0; q < 6; ++q) cur[q] = xcur[q];
    const ResectWaveSrc src{rec, use, il_obs, cam, cam_tab, cam_stride, il_start[slot], il_start[slot + 1], lane};
    int status;
    resect_solve(src, type, wx, wy, refine_iters, min_ratio, refine_tol, sh[wave], sh[wave] + 144, cur, eop, qual, status);
    if (lane == 0) {
#pragma unroll
        for (int q = 0; q < 6; ++q) eop_out[6 * (int64_t)ext + q] = eop[q];
#pragma unroll
        for (int q = 0; q < 5; ++q) qual_out[5 * (int64_t)ext + q] = qual[q];
        stat[ext] = status;
        if (write && (status == FBA_RESECT_OK || status == FBA_RESECT_REFINE)) {
#pragma unroll
            for (int q = 0; q < 6; ++q) xcur[q] = eop[q];
        }
    }
}

int launch_resect_gather(Ctx& c, bool use_all, double* rec, int32_t* use) {
    if (c.n_obs <= 0) return FBA_OK;
    const unsigned nblk = (unsigned)((c.n_obs + 255) / 256);
#define RG(NKV)                                                                                                        \
    k_resect_gather<NKV><<<nblk, 256, 0, c.stream>>>(c.d_xy, c.d_cam, c.d_pt, c.d_xoff, c.d_ctl, c.d_xfull, c.d_cam_tab, \
                                                     c.d_il_obs, c.n_obs, c.set.type, c.cam_tab_stride, use_all ? 1 : 0, \
                                                     rec, use)
    switch (c.L.nk) {
        case 1: RG(1); break;
        case 2: RG(2); break;
        case 3: RG(3); break;
        case 4: RG(4); break;
        case 5: RG(5); break;
        case 6: RG(6); break;
        case 7: RG(7); break;
        case 8: RG(8); break;
        default: set_error("num_radial out of range"); return FBA_ERR_UNSUPPORTED;
    }
#undef RG
    FBA_HIP(hipGetLastError());
    return FBA_OK;
}

int launch_resect(Ctx& c, const double* rec, const int32_t* use, int refine_iters, double min_ratio, double refine_tol,
                  bool write, double* eop, double* qual, int32_t* st) {
    if (c.L.n_img <= 0) return FBA_OK;
    const unsigned nblk = (unsigned)((c.L.n_img + RS_WAVES - 1) / RS_WAVES);
    const double wx = 1.0 / (c.set.meas_std_x * c.set.meas_std_x), wy = 1.0 / (c.set.meas_std_y * c.set.meas_std_y);
    k_resect<<<nblk, 64 * RS_WAVES, 0, c.stream>>>(rec, use, c.d_il_start, c.d_il_obs, c.d_il_ext, c.d_cam, c.d_cam_tab,
                                                   c.cam_tab_stride, c.L.n_img, c.set.type, wx, wy, refine_iters, min_ratio,
                                                   refine_tol, write ? 1 : 0, c.d_xfull, eop, qual, st);
    FBA_HIP(hipGetLastError());
    return FBA_OK;
}

}  // namespace fba
