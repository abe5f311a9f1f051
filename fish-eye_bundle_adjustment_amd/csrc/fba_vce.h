// fba_vce.h -- variance component estimation over observation groups, fp64: the per-row and per-group arithmetic of
// k_vce_sums / k_vce_finish (fba_vce.hip) and, the same arithmetic, of the host (fba_vce_host).  No reference
// counterpart: main.m:397-402 gives every image measurement the weight 1 / Meas_std^2 and never revisits it.
//
// Foerstner's simplified estimator for a diagonal weight matrix.  Observation row i of group g, with the a-priori
// sigma of its axis, the current sqrt weight s (P_ii = s^2 / sigma^2), the raw residual v and q = a Cx a' of its
// whitened Jacobian row:
//   r_i = 1 - q / sigma^2           the row's redundancy number (fba_rel.hip's)
//   t_i = (s v / sigma)^2           its share of v'Pv
//   R_g = sum r_i, T_g = sum t_i, n_g the row count;  sigma2_g = T_g / R_g the group's variance factor
// A group is EMPTY without rows, WEAK when R_g < min_redundancy (its factor is 1: too little redundancy to say
// anything), CLIPPED when the estimate leaves [1 / clip, clip] (T_g = 0 lands on 1 / clip), OK otherwise.  The rows of
// the group are re-weighted by sqrt weight *= 1 / sqrt(sigma2_g).
//
// The device (one xor tree per wave, then wave, block order) and the host (index order) differ in the order of the
// three sums alone.
#pragma once
#include <cmath>
#include <cstdint>

#include "../../include/fba.h"

#ifndef FBA_HD
#if defined(__HIPCC__) || defined(__CUDACC__)
#define FBA_HD __host__ __device__
#else
#define FBA_HD
#endif
#endif

namespace fba {

constexpr int VCE_SUMS = 3;  // R, T, n per group
constexpr int VCE_OUT = 6;   // R, T, n, sigma2, factor, status per group (k_vce_finish's row)

// the row quantities; s = 1 while no weights are on
FBA_HD inline void vce_row(double q, double v, double s, double sigma, double& r, double& t) {
    r = 1.0 - q / (sigma * sigma);
    const double z = s * v / sigma;
    t = z * z;
}

// estimate, clamp, factor and status of one estimated group from its sums.  sigma2 is the factor the round applies
// to the group's variance: 1 for EMPTY and WEAK, the clamped estimate for CLIPPED.  Non-finite sums come out as OK
// with a non-finite sigma2; the callers test the sums
FBA_HD inline void vce_group(double R, double T, double n, double min_redundancy, double clip, double& sigma2,
                             double& factor, int& status) {
    sigma2 = 1.0;
    factor = 1.0;
    if (n == 0.0) { status = FBA_VCE_EMPTY; return; }
    if (R < min_redundancy) { status = FBA_VCE_WEAK; return; }
    const double lo = 1.0 / clip;
    double e = T / R;
    status = FBA_VCE_OK;
    if (e < lo) { e = lo; status = FBA_VCE_CLIPPED; }
    else if (e > clip) { e = clip; status = FBA_VCE_CLIPPED; }
    sigma2 = e;
    factor = 1.0 / sqrt(e);
}

// the rows of no estimated group (id -1): reported, never rescaled; sigma2 = T / R where that means something
FBA_HD inline void vce_rest(double R, double T, double n, double& sigma2, double& factor, int& status) {
    factor = 1.0;
    status = n == 0.0 ? FBA_VCE_EMPTY : FBA_VCE_OK;
    sigma2 = (n > 0.0 && R > 0.0) ? T / R : 1.0;
}

// the host's source of sums: rows in index order into sums [n_groups + 1][VCE_SUMS] (zeroed here); an id outside
// [0, n_groups) counts as -1, the last row
inline void vce_sum_rows(int64_t n_rows, int n_groups, const int32_t* group, const double* r, const double* t, double* sums) {
    for (int i = 0; i < (n_groups + 1) * VCE_SUMS; ++i) sums[i] = 0.0;
    for (int64_t i = 0; i < n_rows; ++i) {
        const int id = group[i];
        double* g = sums + VCE_SUMS * ((id >= 0 && id < n_groups) ? id : n_groups);
        g[0] += r[i];
        g[1] += t[i];
        g[2] += 1.0;
    }
}

}  // namespace fba
