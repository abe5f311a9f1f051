/*
 * fba.h -- C-ABI of libfba.so, the MI355X-native Gauss-Newton bundle-adjustment inner loop.
 *
 * Drop-in boundary for the reference's MATLAB hot path (wynandtredoux/Fish-Eye_Bundle_Adjustment):
 *
 *   fba_buildxhat     replaces  [error, xhat, xhatnames] = Buildxhat(data, EXT, INT, TIE, CNT)
 *                               functions/Buildxhat.m:2 (called at main.m:388)
 *   fba_build_awg     replaces  [error, A, misclosure, G, dist_scaling] = BuildAwG(data, xhat)
 *                               functions/BuildAwG.m:14 (called at main.m:416); dense debug form
 *   fba_accumulate +
 *   fba_solve_update  replace   one pass of the inline loop body main.m:413-488
 *                               (BuildAwG -> u = A'Pw, N = A'PA -> bordered solve -> de-scale ->
 *                               xhat += delta -> deltasum = sumabs(delta)), split at the point where a
 *                               multi-GPU caller all-reduces the normal equations
 *   fba_step          = fba_accumulate + fba_solve_update (single GPU)
 *   fba_adjust        replaces  the whole loop main.m:407-494 (while deltasum > threshold, cap)
 *   fba_build_rsd     replaces  RSD = BuildRSD(v, data, xhat) (functions/BuildRSD.m:1) for a given v
 *   fba_residuals     replaces  v = A*delta + w (main.m:569), RSD = BuildRSD(v, data, xhat)
 *                               (functions/BuildRSD.m:1, main.m:571), RMSx/RMSy/RMS (main.m:594-598),
 *                               sigma02 = v'Pv/(n-u) (main.m:601)
 *
 * Conventions (mirroring the reference's): every function returns 0 on success and a nonzero
 * FBA_ERR_* code where the reference would set error = 1 (BuildAwG.m:16, Buildxhat.m:3); the message
 * is available from fba_last_error().  No exceptions cross the ABI.  All arrays are caller-owned
 * host buffers; indices are 0-based (the reference's are 1-based); reals are IEEE fp64.
 * A context owns its device memory and is bound to one GPU; it is not re-entrant.
 */
#ifndef FBA_H_
#define FBA_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FBA_ABI_VERSION 2

/* projection models, BuildAwG.m:184-213 (the reference's `typeint`) */
enum {
    FBA_TYPE_FISHEYE = 0,       /* equidistant:  -c*U/R*atan(R/W)           */
    FBA_TYPE_PINHOLE = 1,       /* collinearity: -c*U/W                     */
    FBA_TYPE_EQUISOLID = 2,     /* -2c*U/R*sin(atan(R/W)/2)                 */
    FBA_TYPE_ORTHOGRAPHIC = 3,  /* -c*U/R*sin(atan(R/W))                    */
    FBA_TYPE_STEREOGRAPHIC = 4  /* -2c*U/R*tan(atan(R/W)/2)                 */
};

/* error codes */
enum {
    FBA_OK = 0,
    FBA_ERR_ARG = 1,         /* invalid argument / inconsistent problem                  */
    FBA_ERR_TYPE = 2,        /* invalid Type (BuildAwG.m:209-213)                        */
    FBA_ERR_HIP = 3,         /* HIP runtime failure                                      */
    FBA_ERR_NOT_SPD = 4,     /* reduced normal matrix not positive definite              */
    FBA_ERR_UNSUPPORTED = 5, /* input outside what this build implements (message says) */
    FBA_ERR_NONFINITE = 6    /* non-finite correction (divergence guard)                 */
};

#define FBA_NK_MAX 8 /* maximum Num_Radial_Distortions */

/* The .cfg flags that parameterise the hot path (main.m:150-171, findSetting.m). */
typedef struct fba_settings {
    int32_t est_Xc, est_Yc, est_Zc, est_omega, est_phi, est_kappa; /* Estimate_Xc..Estimate_Kappa */
    int32_t est_xp, est_yp, est_c;                                  /* Estimate_xp/_yp/_c          */
    int32_t est_radial;                                             /* Estimate_Radial_Distortions */
    int32_t est_decent;                                             /* Estimate_Decentering_...    */
    int32_t num_radial;        /* Num_Radial_Distortions (clamped >= 1, BuildAwG.m:18-20)   */
    int32_t type;              /* FBA_TYPE_*                                                */
    int32_t inner_constraints; /* Inner_Constraints                                         */
    int32_t iteration_cap;     /* Iteration_Cap                                             */
    int32_t reserved;
    double threshold;          /* Threshold_Value                                           */
    double meas_std_x;         /* Meas_std                                                  */
    double meas_std_y;         /* Meas_std_y (= Meas_std when absent, main.m:397-402)       */
} fba_settings;

/*
 * Packed problem (structure-of-arrays).  This is the reference's `data` struct (main.m:280-383)
 * after its joins: one entry per PHO row, in PHO order.
 */
typedef struct fba_problem {
    int64_t n_pts;            /* image points = PHO rows (n = 2*n_pts observations)         */
    int32_t n_img;            /* numImg: images = EXT rows 0..n_img-1 (Buildxhat.m:22)      */
    int32_t n_cam;            /* numCam: cameras = INT pairs 0..n_cam-1 (Buildxhat.m:65)    */
    int32_t n_tie;            /* numtie: estimated object points (TIE order)                */
    int32_t reserved;
    const double* xy;         /* [2*n_pts]  x0 y0 x1 y1 ... (pixels)                        */
    const int32_t* img;       /* [n_pts]    ext_index (EXT row)                              */
    const int32_t* cam;       /* [n_pts]    cam_num (INT pair), must equal EXT's camera     */
    const int32_t* tie;       /* [n_pts]    tieIndex, or -1 for a fixed (control) point      */
    const double* xyz_fixed;  /* [3*n_pts]  CNT coordinates (used where tie < 0)            */
    const double* eop0;       /* [6*n_img]  EXT Xc Yc Zc omega phi kappa (radians)          */
    const double* iop0;       /* [n_cam*(5+num_radial)] INT xp yp c K1..Knk P1 P2           */
    const double* cam_info;   /* [5*n_cam]  y_dir xmin ymin xmax ymax                        */
    const double* tie0;       /* [3*n_tie]  CNT coordinates of the TIE list                  */
} fba_problem;

typedef struct fba_options {
    int32_t device;      /* HIP device ordinal                                              */
    int32_t rank;        /* this process's rank (observation shard), 0 for single GPU      */
    int32_t world;       /* number of ranks, 1 for single GPU                               */
    int32_t verbose;
    void* stream;        /* hipStream_t to run on, or NULL for a context-owned stream       */
    int32_t split;       /* world > 1: 0 = replicated solve (every rank factors the summed reduced
                          * system), 1 = subtree split: the elimination tree is cut into top
                          * columns and subtrees dealt to the ranks; tie points follow their
                          * images' subtree, each rank factors its subtrees in fba_accumulate and
                          * the reduce buffer carries only the top blocks (no reference
                          * counterpart: main.m:432 inverts the dense matrix on one CPU)          */
} fba_options;

typedef struct fba_ctx fba_ctx;

/* Thread-local message of the last failure. */
const char* fba_last_error(void);
int fba_abi_version(void);

/* Number of unknowns u of the reference's xhat (Buildxhat.m:6-15); host only. */
int fba_count_unknowns(const fba_problem* p, const fba_settings* s, int64_t* u_out);

/* Deterministic observation shard: owner rank of every tie point (contiguous ranges balanced by
 * observation count) and of every control observation; host only, no GPU needed. */
int fba_partition(const fba_problem* p, int32_t world, int32_t* tie_owner /*[n_tie]*/,
                  int32_t* ctl_owner /*[n_pts], -1 for tie observations*/);

/* Camera-side elimination order of the reduced system the device factorisation uses (host only, no
 * GPU): nested dissection of the images' co-visibility graph (fba_order.cpp).  Slot k of the reduced
 * system's image part (unknowns 6k..6k+5) holds EXT row order[k], or -1 for a padding slot (padding
 * keeps independent subtrees in separate 128-row blocks); the camera unknowns follow the last slot, and
 * inner constraints are bordered on the first min(n_slots, 21) slots.  order may be NULL to query
 * *n_slots.  No reference counterpart (main.m:432 inverts the dense bordered matrix): for callers that
 * factor the reduced system themselves on the same block pattern (oracle/fba_cpu.c's cpu_baseline). */
int fba_image_order(const fba_problem* p, int32_t* order /*[n_slots]*/, int32_t* n_slots);

int fba_create(const fba_problem* p, const fba_settings* s, const fba_options* o, fba_ctx** out);
void fba_destroy(fba_ctx* ctx);

/* Prior observations of unknowns (no reference counterpart: the reference's unknowns are free, or fixed by
 * switching an Estimate_* flag off or listing a control point): GNSS/INS-observed exterior orientation,
 * ground control with a stated accuracy, interior orientation / distortion values of a calibration
 * certificate.  Prior j observes unknown index[j] of the reference-layout xhat (0-based) with the value
 * value[j] and the standard deviation sigma[j], in the units of xhat (radians for angles, the natural,
 * de-scaled units for distortion terms); the priors are uncorrelated.  Each adds one unit row to the
 * Gauss-Markov model: the row e_index[j], misclosure w_j = xhat[index[j]] - value[j] (computed minus
 * observed, the reference's sign), weight p_j = 1 / sigma[j]^2.  The normal equations carry the distortion
 * unknowns in scaled units (BuildAwG.m:419-451), so the row's entry for a K_j or P unknown is
 * 1 / dist_scaling.  Robust loss and user weights act on image measurements only. */
typedef struct fba_priors {
    int64_t n;             /* number of priors                                               */
    const int64_t* index;  /* [n] index into the reference-layout xhat, each at most once    */
    const double* value;   /* [n] observed value l_j                                         */
    const double* sigma;   /* [n] standard deviation, finite and > 0                         */
} fba_priors;

/* fba_create with priors; pr == NULL or pr->n == 0 is fba_create itself.  The priors are constants of the
 * context: a tie point that carries one is accumulated by the general-point kernels instead of the chunked
 * fast path, and that plan is laid out here.  Checked on the host before any GPU call (FBA_ERR_ARG, with
 * a message): an index outside [0, u), an index given twice, a non-finite value, a sigma that is not
 * finite or not > 0.  With world > 1 every rank passes the full list; rank 0 adds the priors of image and
 * camera unknowns, a tie point's owner adds that point's, so the summed reduce buffer holds each once.
 * Together with fba_options.split = 1 priors are refused (FBA_ERR_UNSUPPORTED). */
int fba_create_priors(const fba_problem* p, const fba_settings* s, const fba_options* o, const fba_priors* pr,
                      fba_ctx** out);

/* The priors' residuals v_j = xhat[index[j]] - value[j] at the device xhat (the row is linear, so this
 * is the reference's v = A delta + w convention exactly) and v'Pv's prior term.  *n (may be NULL)
 * receives the number of priors; resid [n] (may be NULL): with world > 1, 0 for the priors this rank
 * does not add; vtpv (may be NULL): this rank's sum of p_j v_j^2, added in a fixed order.
 * fba_covariance and fba_reliability carry the priors through the normal equations; a prior's own
 * redundancy number is r_j = 1 - cx_diag[index[j]] / (sigma02 sigma[j]^2) and its test statistic
 * w_j = v_j / (sigma[j] sqrt(r_j)) (0 where r_j < 1e-10), host arithmetic on cx_diag. */
int fba_get_priors(fba_ctx* ctx, int64_t* n, double* resid /*[n]*/, double* vtpv);

/* The solve the context actually runs: *split = 1 when fba_options.split was honoured (subtree split:
 * reduce-buffer layout, ownership and the one-solve-per-accumulation rule of the split), 0 for the
 * replicated / single-GPU solve -- a split request falls back to the replicated solve when the block
 * pattern cannot be cut (no reference counterpart). */
int fba_solve_mode(fba_ctx* ctx, int32_t* split);

/* Buildxhat.m: initial xhat in the reference's layout.  xhat may be NULL to query u only. */
int fba_buildxhat(fba_ctx* ctx, double* xhat /*[u]*/, int64_t* u_out);

/* Set / get the device-resident xhat (reference layout).  With owned_only != 0 the entries this
 * rank does not own are returned as 0 (tie points of other ranks; camera entries on rank > 0), so
 * that a sum over ranks reassembles the full vector. */
int fba_set_xhat(fba_ctx* ctx, const double* xhat);
int fba_get_xhat(fba_ctx* ctx, double* xhat, int32_t owned_only);

/* BuildAwG.m (dense debug/parity form): A is n x u column-major (n = 2*n_pts, PHO row order),
 * w is n, G is u x 7 column-major (only when inner constraints are on; may be NULL),
 * dist_scaling is n_cam x (2+num_radial) column-major; columns 0-1 hold the reference's 1-based xhat
 * index of the first radial / decentering unknown (0 when not estimated, BuildAwG.m:138, :150),
 * columns 2.. rmax^(2j) (BuildAwG.m:424-426).
 * Any output pointer may be NULL. */
int fba_build_awg(fba_ctx* ctx, const double* xhat, double* A, double* w, double* G,
                  double* dist_scaling);

/* One Gauss-Newton iteration, split for multi-GPU callers:
 *   fba_accumulate      linearise this rank's observations at the device xhat and accumulate the
 *                       (point-reduced) normal equations into the reduce buffer;
 *   fba_reduce_buffer   device pointer + length (doubles) of that buffer: ranks sum it elementwise
 *                       (e.g. an RCCL all-reduce) between the two calls.  With world == 1 there is
 *                       nothing to sum and the buffer IS the context's reduced system; the solve
 *                       reads weights fba_accumulate already derived from it, so the caller must not
 *                       modify it between fba_accumulate and fba_solve_update (reading is fine);
 *   fba_solve_update    bordered solve, point back-substitution, de-scaling, xhat update.
 *                       *deltasum_part receives this rank's share of sumabs(delta) (sum over ranks
 *                       = the reference's deltasum).
 * fba_step does both halves on one GPU and returns the full deltasum. */
int fba_accumulate(fba_ctx* ctx);
int fba_reduce_buffer(fba_ctx* ctx, void** dev_ptr, int64_t* n_doubles);
/* Block until every operation queued on the context's stream has completed (needed before a
 * caller touches the reduce buffer from another stream or the host). */
int fba_synchronize(fba_ctx* ctx);
int fba_solve_update(fba_ctx* ctx, double* deltasum_part);
/* The same split without the host round trip in the middle (multi-GPU): fba_solve_update_async only
 * enqueues the solve on the context's stream; fba_deltasum_device gives the device address of this
 * rank's deltasum share (one double), which the caller may all-reduce in place on that stream;
 * fba_solve_finish synchronises, checks the solve and returns that (reduced) value. */
int fba_solve_update_async(fba_ctx* ctx);
int fba_deltasum_device(fba_ctx* ctx, void** dev_ptr);
int fba_solve_finish(fba_ctx* ctx, double* deltasum);
int fba_step(fba_ctx* ctx, double* deltasum);

/* main.m:407-494: iterate while deltasum > threshold, at most iteration_cap times.
 * deltasum_hist (may be NULL) receives one entry per iteration (capacity iteration_cap). */
int fba_adjust(fba_ctx* ctx, int32_t* iterations, double* deltasum_hist);

/* main.m:567-602 + BuildRSD.m: from the last iteration's linearisation and de-scaled delta.
 * v [2*n_pts] (PHO order), rsd [5*n_pts] row-major per point: r, vx, vy, vr, vt,
 * stats [6]: RMSx, RMSy, RMS, sigma02, vTPv, n-u.  Pointers may be NULL.  With world > 1 each rank
 * fills only its observations (others 0) and stats hold this rank's partial sums
 * (sum vx^2, sum vy^2, 0, 0, vTPv, n-u); fba_finish_stats turns reduced sums into RMS / sigma02.
 * With priors (fba_create_priors) stats[4] includes their term sum p_j v_j^2 (this rank's, with world > 1)
 * and stats[5] is n + n_prior - u, so stats[3] follows with world 1; v, rsd and the RMS values are the
 * image measurements' alone.  fba_finish_stats knows no priors: a multi-rank caller divides the reduced
 * vTPv by stats[5] itself. */
int fba_residuals(fba_ctx* ctx, double* v, double* rsd, double* stats);

/* BuildRSD.m:1 for a caller-given v (e.g. the reference's v = A*delta + w, main.m:569-571): per PHO
 * row [r, vx, vy, vr, vt] (BuildRSD.m:29-40) with xp, yp from xhat where estimated, else the INT
 * values (BuildRSD.m:12-26).  v [2*n_pts] x y interleaved (PHO order), xhat [u] the reference layout,
 * rsd [5*n_pts] row-major.  With world > 1 only this rank's rows are written (others 0). */
int fba_build_rsd(fba_ctx* ctx, const double* v, const double* xhat, double* rsd);
int fba_finish_stats(const fba_problem* p, const fba_settings* s, const double* sums /*[2]: sum vx^2, sum vy^2*/,
                     double vtpv, double* stats /*[6]*/);

/* Post-fit covariance of the unknowns (main.m:428-456, :460-482, :602): from the factor of the LAST
 * solve (call right after the iterations, before any further fba_accumulate / fba_step; the factor is
 * consumed).  sigma02 is the a-posteriori variance factor (fba_residuals stats[3] or fba_finish_stats).
 *   cx_diag [u] (may be NULL): diag(Cx) of the reference's final Cx = sigma02 * (bordered) inverse of
 *           the last normal matrix, distortion entries de-scaled by dist_scaling^2 (main.m:460-482,
 *           diagonal only, as the reference); xhat order.  With world > 1 the tie entries of other
 *           ranks are 0 (camera entries are replicated); with the subtree split (fba_options.split)
 *           the camera-side entries too are this rank's rows only (its subtrees' images, and the top's
 *           images and the camera unknowns on rank 0), so the ranks' outputs sum to the whole vector.
 *   corr [n_img][(u_img+u_cam)^2] (may be NULL): per EXT image, the reference's Correlation matrix
 *           (main.m:446-456) restricted to [the image's estimated EOPs, its camera's estimated
 *           IOP/distortion unknowns] in xhat order, full symmetric, row-major (main.m:831-840); with
 *           the subtree split only this rank's images (the rank owning the image's first row; wholly
 *           top images on rank 0), zeros for the others. */
int fba_covariance(fba_ctx* ctx, double sigma02, double* cx_diag, double* corr);

/* Observation reliability (no reference counterpart: main.m stops at BuildRSD's raw residuals).  Baarda's
 * redundancy number and standardised residual (w-test) of every image measurement, from the same factor
 * and the same state as fba_covariance:
 *   redundancy [2*n_pts] (may be NULL): r = 1 - p (a Cx a'), p = 1 / Meas_std^2 (Meas_std_y^2 for y), a the
 *           observation's row of the last linearisation and Cx the cofactor matrix (main.m:428-444, before
 *           the distortion de-scaling and the sigma02 factor); PHO order, x y interleaved like v.  The
 *           values lie in (0, 1) and sum to n - u (+ 7 with inner constraints).
 *   wstat [2*n_pts] (may be NULL): w = v / (sigma sqrt(r)) with fba_residuals' v; 0 where r < 1e-10 (the
 *           observation cannot be checked).
 * cx_diag and corr (either may be NULL) are filled exactly as by fba_covariance (bit-identical), so a
 * caller who wants both calls this function alone: like fba_covariance it needs the factor of the last
 * solve and consumes it (FBA_ERR_ARG otherwise).  With world > 1 and the replicated solve a rank fills its
 * own observations and writes 0 elsewhere (the ranks' outputs sum to the whole vectors).  With the subtree
 * split (fba_solve_mode gives 1) it returns FBA_ERR_UNSUPPORTED and leaves the factor in place. */
int fba_reliability(fba_ctx* ctx, double sigma02, double* cx_diag, double* corr,
                    double* redundancy /*[2*n_pts]*/, double* wstat /*[2*n_pts]*/);

/* Point precision: the full 3 x 3 covariance of every object (tie) point and its error ellipsoid (no reference
 * counterpart: main.m:460-482 keeps the diagonal).  One call for every post-fit output, from the same factor and
 * the same state as fba_covariance: it needs the factor of the last undamped solve and consumes it (FBA_ERR_ARG
 * before any solve, after a damped solve, or on a second call).
 *   cx_diag, corr, redundancy, wstat: exactly fba_covariance's / fba_reliability's outputs (bit-identical).
 *   cx_tie [6*n_tie] (TIE order): XX XY XZ YY YZ ZZ of sigma02 * Cx_pp, Cx_pp = V^-1 + T' C T the point's block of
 *           the cofactor matrix (main.m:428-444); its XX YY ZZ are cx_diag's tie entries up to the order of an
 *           fp64 sum.  Tie entries carry no distortion de-scaling.
 *   ellipsoid [12*n_tie] (TIE order): the 1-sigma semi-axes a >= b >= c, a = sqrt(max(lambda, 0)) of that block's
 *           eigenvalues (cyclic Jacobi, fp64), then the three unit axis vectors as rows in the same order, each
 *           with its largest-magnitude component positive (on ties the first component wins).  A non-finite
 *           block gives NaNs for that point.  Scale the axes by sqrt(chi2_3(0.95)) = 2.7955 for the 95 % region.
 * Any pointer may be NULL; with ellipsoid set and cx_tie NULL the blocks stay in workspace.  With world > 1 the
 * tie points of other ranks get zeros in cx_tie and ellipsoid (the ranks' outputs sum to the whole).  With the
 * subtree split cx_tie and ellipsoid follow cx_diag's tie entries; a non-NULL redundancy or wstat returns
 * FBA_ERR_UNSUPPORTED as fba_reliability does and leaves the factor in place. */
typedef struct fba_postfit {
    double* cx_diag;    /* [u]                     as fba_covariance            */
    double* corr;       /* [n_img][(u_img+u_cam)^2] as fba_covariance           */
    double* redundancy; /* [2 n_pts]               as fba_reliability           */
    double* wstat;      /* [2 n_pts]               as fba_reliability           */
    double* cx_tie;     /* [6 n_tie]  XX XY XZ YY YZ ZZ of sigma02 * Cx_pp      */
    double* ellipsoid;  /* [12 n_tie] a b c, then the three axis vectors (rows) */
} fba_postfit;          /* any pointer may be NULL */
int fba_postfit_outputs(fba_ctx* ctx, double sigma02, const fba_postfit* out);
/* host only, no GPU: the device's eigen routine run on the CPU (tests).  blk [6*n] XX XY XZ YY YZ ZZ per block,
 * ell [12*n] as ellipsoid above (no reference counterpart: main.m:460-482 keeps the diagonal). */
int fba_eig3_host(int64_t n, const double* blk /*[6n]*/, double* ell /*[12n]*/);

/* Per-observation weights and robust loss (no reference counterpart: main.m:397-402 gives every observation
 * the weight 1 / Meas_std^2).  Both setters may be called at any point between iterations (not between
 * fba_solve_update_async and fba_solve_finish); both invalidate the last linearisation and the factor of the last
 * solve, so fba_residuals, fba_covariance and fba_reliability return FBA_ERR_ARG until the next iteration.  The
 * linearising kernels scale an observation's Jacobian row and misclosure by s = sqrt(weight x loss factor), so
 * the normal equations, the covariance and the reliability quantities all carry the weight matrix
 * P = diag(s^2 / Meas_std^2); fba_residuals reports v and the RSD rows in pixels (un-scaled), RMSx / RMSy from
 * them, and v'Pv, sigma02 with the weights in.  fba_build_awg returns the raw A and w as before.
 *
 * fba_set_weights (no reference counterpart): weight [2*n_pts], PHO order, x y interleaved like v, multiplies
 *   the a-priori weight: p_i = weight_i / Meas_std^2 (Meas_std_y^2 for y).  NULL restores all 1, and an array of
 *   all 1 is taken as NULL (the unweighted kernels run, bit for bit a context that never had weights).  Every entry
 *   must be finite and > 0 (FBA_ERR_ARG otherwise, checked on the host before anything else happens): an exact
 *   0 is refused because the raw residual is recovered by division; a value such as 1e-12 excludes a
 *   measurement.  With world > 1 every rank passes the full-length array and keeps its own observations'.
 * fba_set_loss (no reference counterpart): loss = FBA_LOSS_*, k > 0 and finite in units of sigma (ignored for
 *   FBA_LOSS_NONE).  Per image point t^2 = p_x w0^2 + p_y w1^2 from the misclosures at the linearisation point
 *   (user weights included); both rows of the point are down-weighted by  Huber: 1 (t <= k), k / t   Cauchy:
 *   1 / (1 + t^2 / k^2), re-evaluated inside every linearisation (IRLS).  Set it after the L2 iterations have
 *   converged: at poor starting values every misclosure is large and everything would be down-weighted.
 * fba_get_weights (no reference counterpart): weight [2*n_pts] receives the effective weights of the last
 *   linearisation, user weight x loss factor (all 1 with neither set); same preconditions as fba_residuals.
 *   With world > 1 the entries of other ranks' observations are 0 (the ranks' outputs sum to the whole). */
enum { FBA_LOSS_NONE = 0, FBA_LOSS_HUBER = 1, FBA_LOSS_CAUCHY = 2 };
int fba_set_weights(fba_ctx* ctx, const double* weight /*[2*n_pts], PHO order, x y interleaved; NULL: all 1*/);
int fba_set_loss(fba_ctx* ctx, int32_t loss, double k);
int fba_get_weights(fba_ctx* ctx, double* weight /*[2*n_pts]*/);

/* Levenberg-Marquardt damping with step control (no reference counterpart: main.m:407-494 takes every
 * Gauss-Newton step at full length, whatever it does to the cost).
 *
 * fba_set_damping: lambda = 0 (the default) is Gauss-Newton on the kernels and launches as they are without
 *   this call; lambda > 0 damps every following solve of the context: it solves (N + lambda D) delta = -A'Pw,
 *   with inner constraints the same bordered system with N + lambda D in place of N.  D is a positive
 *   diagonal: for a tie point diag(V) of its block V = Jp'PJp (weights, loss factor and priors included), so the
 *   point is eliminated with V_l = V + lambda diag(V); for the image and camera unknowns diag(S') of the reduced
 *   system S' = N_cc - N_cp V_l^-1 N_pc formed with the damped V (camera-side priors and the ranks' sum
 *   included), so the solve factors S' + lambda diag(S').  A valid Levenberg-Marquardt metric, but not
 *   Marquardt's diag(N) on the camera rows.  A negative or non-finite lambda is FBA_ERR_ARG; lambda > 0 on a
 *   subtree-split context (fba_solve_mode 1) is FBA_ERR_UNSUPPORTED.  Not between fba_solve_update_async and
 *   fba_solve_finish.  Any change of lambda invalidates the last linearisation (the tie points were eliminated
 *   with the earlier lambda): fba_solve_update then asks for a new fba_accumulate.  Switching damping on or off
 *   also re-captures the graphs, like fba_set_weights; changing lambda between damped steps costs one scalar
 *   copy and re-captures nothing.  After a damped solve the factor is not that of
 *   N: fba_covariance and fba_reliability return FBA_ERR_ARG until an undamped solve; fba_residuals works.
 * fba_cost: the objective at the device xhat, from the forward model alone (no linearisation is needed or
 *   touched; xhat and every later step are bitwise as without the call):
 *     F = sum over image points rho(t^2) + sum over priors p_j (xhat[index_j] - l_j)^2,
 *     t^2 = px (s0 w0)^2 + py (s1 w1)^2,  w the misclosure, s = sqrt(user weight) (1 without),
 *     rho(t^2) = t^2 (no loss) | Huber: t^2 (t <= k), 2 k t - k^2 | Cauchy: k^2 ln(1 + t^2 / k^2)
 *   -- the losses whose IRLS factors fba_set_loss applies; without weights or loss F = w'Pw of BuildAwG's
 *   misclosure.  cost[0] total, [1] image part, [2] prior part, each added in a fixed order (two calls are
 *   bitwise equal).  With world > 1 this rank's share: its observations, and the priors it adds (fba_get_priors).
 * fba_adjust_lm: the damped loop, then undamped passes, from the context's current xhat (world == 1 only,
 *   FBA_ERR_UNSUPPORTED otherwise):
 *     F = cost at x; lambda = lambda0
 *     trial: save x (device copy); one step at lambda; Fn = cost at x + delta
 *       |Fn - F| <= ftol F    -> keep the step if Fn <= F, else restore x; end the damped phase
 *       Fn finite and Fn < F  -> accept; F = Fn; lambda = max(lambda / down, lambda_min);
 *                                end the damped phase if deltasum <= Threshold_Value
 *       otherwise             -> restore x; lambda = lambda up; lambda > lambda_max: FBA_ERR_NONFINITE
 *                                (not converged; message set)
 *       FBA_ERR_NOT_SPD from the trial's solve counts as "otherwise"; any other error returns
 *     polish: damping off; plain Gauss-Newton steps while deltasum > Threshold_Value (at least one)
 *   Iteration_Cap bounds trials + polish passes together, as main.m:490-493 bounds passes; the damped phase
 *   takes at most Iteration_Cap - 1 of them.  The polish passes make v, sigma02, Cx and the reliability numbers
 *   those of an undamped last pass, exactly as after fba_adjust.  The ftol rule ends the damped phase where
 *   the cost differences fall to rounding and accept / reject would be noise.  *trials and *polish (may be
 *   NULL) receive the two counts; hist (may be NULL, capacity 4 * Iteration_Cap) one row per trial and pass:
 *   lambda, the cost after it, deltasum, accepted (1 / 0); polish rows carry lambda = 0 and accepted = 1. */
typedef struct fba_lm_options {
    double lambda0, up, down, lambda_min, lambda_max, ftol;
} fba_lm_options; /* NULL: 1e-3, 10, 10, 1e-12, 1e8, 1e-9 */
int fba_set_damping(fba_ctx* ctx, double lambda);
int fba_cost(fba_ctx* ctx, double* cost /*[3]: total, image part, prior part*/);
int fba_adjust_lm(fba_ctx* ctx, const fba_lm_options* o, int32_t* trials, int32_t* polish,
                  double* hist /*[4*Iteration_Cap]: lambda, cost after, deltasum, accepted (1/0)*/);

/* Forward intersection: starting values of the object points from the measured image rays (no reference
 * counterpart: Buildxhat.m:107-134 copies the .cnt coordinates of the .tie targets, and main.m has no routine that
 * derives them from the measurements).
 *
 * The image ray of a measurement is closed-form in this model, because BuildAwG.m:168-187 evaluates the distortion at
 * the MEASURED coordinates: xb = x - xp, yb = y - yp, dr = sum K_j r^2j, decx / decy from P1, P2, and the model's
 * condition w = 0 reads xu = xb - dr xb - decx = -c s U, yu = yb - dr yb - decy = -c ydir s V with s = g(t) / R,
 * t = atan(R / W).  So rho = hypot(xu, yu) = c |g(t)|, t = ginv(rho / c) per Type -- q (fisheye), atan q (pinhole),
 * 2 asin(q / 2) (equisolid), asin q (orthographic), 2 atan(q / 2) (stereographic) -- and the unit direction in the
 * camera frame is (-sin t xu / rho, -ydir sin t yu / rho, cos t); rho = 0 gives the axis (0, 0, 1).  The ray is a LINE
 * through the projection centre: W > 0 and W < 0 give the same line with the direction reversed, and nothing here
 * depends on that sign.
 *
 * fba_unproject_host (no reference counterpart; host only, no GPU): the device's inverse model (csrc/fba_ray.h) run on
 *   the CPU.  xy [2 n] pixels; camtab [6 + nk]: xp yp c ydir P1 P2 K1..Knk, one camera for all n; out [5 n] per
 *   measurement xu yu and the direction; status [n] FBA_RAY_*.  An out-of-range q (orthographic |q| > 1, equisolid
 *   |q| > 2) or any non-finite input gives FBA_RAY_DOMAIN, xu yu as computed and a zero direction.  out or status may
 *   be NULL.
 * fba_image_rays (no reference counterpart): the rays of every image measurement, tie and control alike, at the device
 *   xhat: ray [6 n_pts] per PHO row the projection centre C (the image's Xc Yc Zc, bit for bit xhat's) and the unit
 *   direction M' d in the object frame; status [n_pts] FBA_RAY_*.  With world > 1 a rank fills its own observations
 *   and writes 0 elsewhere (the ranks' outputs sum to the whole; this is why OK is 0).
 * fba_intersect (no reference counterpart): per tie point, from its rays with status OK (n of them),
 *   (a) the linear solution of sum (I - d d')(X - C) = 0 -- the point closest to all its lines, independent of the
 *       directions' signs -- with the origin at the first ray's centre, by the symmetric adjugate; lambda_min /
 *       lambda_max of A = sum (I - d d') (csrc/fba_eig3.h) measures the intersection geometry: for two rays meeting
 *       at the angle a it is (1 - |cos a|) / 2;
 *   (b) up to refine_iters point-only Gauss-Newton passes X <- X - V^-1 b, V = Jp'PJp, b = Jp'Pw of the forward
 *       model's tie columns with P = diag(1 / Meas_std^2, 1 / Meas_std_y^2) (no user weights, no loss, no priors, no
 *       damping: contexts that carry them give the same result), stopped when |dX|_inf <= refine_tol x the mean
 *       distance of X (before the pass) to the rays' centres;
 *   (c) the RMS reprojection residual sqrt(sum (wx^2 + wy^2) / n) in pixels through the forward model, at the linear
 *       and at the final solution.
 *   status per point: FBA_ISECT_OK; FBA_ISECT_FEW fewer than 2 usable rays; FBA_ISECT_WEAK the ratio below min_ratio;
 *   FBA_ISECT_REFINE the refinement went non-finite or raised the RMS (by more than 1e-9 px), the linear solution is
 *   returned.  A point intersected on the wrong half-line (a camera looking away from it) is a valid line
 *   intersection and shows up as a huge RMS: the forward model's atan(R / W) folds it back, and this function does not
 *   guess the camera's sign convention.
 *   xyz [3 n_tie] (TIE order): the solution; for FEW and WEAK the point's current xhat value.  quality [4 n_tie]: rays
 *   used, lambda_min / lambda_max, RMS px linear, RMS px final (FEW: 0 0 0; WEAK: the ratio, 0 0).  status [n_tie].
 *   *n_not_ok: this rank's points with a status other than OK.  Any output pointer may be NULL.  With world > 1 (the
 *   subtree split included) a rank fills the tie points it owns -- all of a point's rays live on its owner -- and
 *   writes 0 elsewhere.
 *   write_xhat != 0: the OK and REFINE points replace their tie entries of the device xhat (FEW and WEAK keep theirs
 *   bit for bit), which invalidates the last linearisation and the factor as fba_set_xhat does: fba_residuals and the
 *   post-fit functions return FBA_ERR_ARG until the next iteration.  Without it the context is untouched: a following
 *   fba_step gives bitwise the xhat it gives without the call.  Plain launches on the context's stream, fixed-order
 *   sums (two calls are bitwise equal).  Not between fba_solve_update_async and fba_solve_finish (FBA_ERR_ARG).  With
 *   fba_set_timing on, fba_last_timings' [7] afterwards holds the device time of this call's kernels, [0..6] 0. */
enum { FBA_RAY_OK = 0, FBA_RAY_DOMAIN = 1 };
enum { FBA_ISECT_OK = 0, FBA_ISECT_FEW = 1, FBA_ISECT_WEAK = 2, FBA_ISECT_REFINE = 3 };
typedef struct fba_intersect_options {
    int32_t refine_iters;  /* 0: linear only; default (NULL options) 10 */
    int32_t write_xhat;    /* != 0: OK / REFINE points replace the tie entries of the device xhat */
    double  min_ratio;     /* default (1 - cos 1deg) / 2 = 7.6e-5: two rays meeting at 1 degree */
    double  refine_tol;    /* default 1e-10 */
} fba_intersect_options;
int fba_unproject_host(int32_t type, int32_t nk, int64_t n, const double* xy /*[2n]*/,
                       const double* camtab /*[6+nk]: xp yp c ydir P1 P2 K1..Knk*/, double* out /*[5n]: xu yu d*/,
                       int32_t* status /*[n]*/);
int fba_image_rays(fba_ctx* ctx, double* ray /*[6 n_pts] C, d; PHO order*/, int32_t* status /*[n_pts]*/);
int fba_intersect(fba_ctx* ctx, const fba_intersect_options* o, double* xyz /*[3 n_tie]*/,
                  double* quality /*[4 n_tie]: rays used, lambda_min/lambda_max, rms px linear, rms px final*/,
                  int32_t* status /*[n_tie]*/, int64_t* n_not_ok);

/* Space resection: starting values of the images' exterior orientation from object points and the measured image
 * rays (no reference counterpart: Buildxhat.m:22-63 copies the .ext rows, and main.m has no routine that derives them).
 * Resection from control, then fba_intersect, then the adjustment starts a block from control points and measurements.
 *
 * The forward model is a function of the LINE through the projection centre, so for a measurement with the
 * camera-frame direction d (fba_unproject_host's) and a known object point X the constraint d x (M (X - C)) = 0 does
 * not depend on d's sign and is linear in the 12 entries of P = [M | -M C] (csrc/fba_resect.h):
 *   (a) the linear solution, per image over its usable points (n of them): m their centroid, s their mean distance to
 *       it, X~ = ((X - m) / s, 1); G = sum (I - d d') (x) (X~ X~') (12 x 12); P the eigenvector of G's smallest
 *       eigenvalue (cyclic Jacobi), its sign such that det(P[:, :3]) > 0; M the polar factor A (A'A)^(-1/2) of
 *       A = P[:, :3], lambda the mean singular value of A, t~ = P[:, 3] / lambda, C = m - s M' t~; the angles by
 *       phi = asin(clamp(M20)), omega = atan2(-M21, M22), kappa = atan2(-M10, M00) (BuildAwG.m:163-165), and where
 *       cos^2 phi = M21^2 + M22^2 <= 1e-14 (the quotients are rounding noise there): omega = 0, kappa = atan2(M01, M11).
 *       The ratio lambda_1 / lambda_11 of G's second smallest to its largest eigenvalue measures the geometry: 0 for
 *       coplanar points, about (relief / extent)^2 otherwise;
 *   (b) up to refine_iters Gauss-Newton passes on the image's six unknowns alone, x <- x - N^-1 g, N = J'PJ, g = J'Pw,
 *       w = (px - xu, py - yu) through the forward model, P = diag(1 / Meas_std^2, 1 / Meas_std_y^2) (no user weights,
 *       no loss, no priors, no damping: contexts that carry them give the same result), N solved by Cholesky; stopped
 *       when |dC|_inf <= refine_tol x the mean distance of C (before the pass) to the points and |d angles|_inf <=
 *       refine_tol;
 *   (c) the RMS reprojection residual sqrt(sum (wx^2 + wy^2) / n) in pixels at the linear and at the final solution.
 *   A point is usable when its ray's status is FBA_RAY_OK and it belongs to the `use` class: FBA_RESECT_USE_CONTROL the
 *   control observations (tie < 0, xyz_fixed), FBA_RESECT_USE_ALL also the tie observations at the device xhat's current
 *   tie coordinates.  A measurement taken twice counts twice.
 *   status per image: FBA_RESECT_OK; FBA_RESECT_FEW fewer than 6 usable points (an image without observations
 *   included); FBA_RESECT_WEAK the ratio below min_ratio, or a NaN; FBA_RESECT_REFINE a non-positive pivot, a
 *   non-finite value, or a final RMS above the linear one by more than 1e-9 px: the linear solution is returned.
 *   eop [6 n_img] (EXT order): Xc Yc Zc omega phi kappa; for FEW and WEAK the image's current xhat values.  quality
 *   [5 n_img]: points used, the ratio, RMS px linear, RMS px final, and the share of the used points with
 *   d . M (X - C) > 0 -- 1 or 0 for a consistent solution (it tells which side W has), anything between means mirrored
 *   geometry (FEW: n 0 0 0 0; WEAK: n, the ratio, 0 0 0).  status [n_img].  *n_not_ok: the images with a status other
 *   than OK.  Any output pointer may be NULL.
 *   write_xhat != 0: the OK and REFINE images replace their six entries of the device xhat (FEW and WEAK keep theirs
 *   bit for bit), which invalidates the last linearisation and the factor as fba_set_xhat does; with any of
 *   Estimate_Xc .. Estimate_Kappa off it returns FBA_ERR_UNSUPPORTED (a fixed exterior orientation is the user's).
 *   Without it the call works under any flag set and leaves the context untouched: a following fba_step gives bitwise
 *   the xhat it gives without the call.  world > 1 returns FBA_ERR_UNSUPPORTED: an image's observations are spread
 *   over the ranks.  One GPU, plain launches on the context's stream, fixed-order sums (two calls are bitwise equal).
 *   Not between fba_solve_update_async and fba_solve_finish (FBA_ERR_ARG).  With fba_set_timing on, fba_last_timings'
 *   [7] afterwards holds the device time of this call's kernels, [0..6] 0.
 * fba_resect_host (no reference counterpart; host only, no GPU): the same per-image routines on the CPU for one image,
 *   the sums in index order: xyz [3 n] the object points, ray [5 n] fba_unproject_host's rows of their measurements,
 *   ray_status [n] (NULL: all FBA_RAY_OK), c and ydir of the camera, the two standard deviations.  `use` and
 *   write_xhat are ignored; for FEW and WEAK eop is zeros. */
enum { FBA_RESECT_OK = 0, FBA_RESECT_FEW = 1, FBA_RESECT_WEAK = 2, FBA_RESECT_REFINE = 3 };
enum { FBA_RESECT_USE_CONTROL = 0, FBA_RESECT_USE_ALL = 1 };
typedef struct fba_resect_options {
    int32_t use;           /* CONTROL: control observations only (tie < 0, xyz_fixed); ALL: also tie
                              observations, at the device xhat's current tie coordinates */
    int32_t refine_iters;  /* 0: linear only; default (NULL options) 10 */
    int32_t write_xhat;    /* != 0: OK / REFINE images replace their six EOP entries of the device xhat */
    int32_t reserved;
    double  min_ratio;     /* default 1e-6 */
    double  refine_tol;    /* default 1e-10 */
} fba_resect_options;
int fba_resect(fba_ctx* ctx, const fba_resect_options* o, double* eop /*[6 n_img], EXT order*/,
               double* quality /*[5 n_img]*/, int32_t* status /*[n_img]*/, int64_t* n_not_ok);
int fba_resect_host(int32_t type, int64_t n, const double* xyz /*[3n]*/,
                    const double* ray /*[5n]: xu yu d, fba_unproject_host's rows*/,
                    const int32_t* ray_status /*[n] or NULL*/, double c, double ydir, double std_x, double std_y,
                    const fba_resect_options* o, double* eop /*[6]*/, double* quality /*[5]*/, int32_t* status);

/* Variance component estimation over groups of image measurements (no reference counterpart: main.m:397-402 gives
 * every measurement the weight 1 / Meas_std^2 and everything after the loop inherits it).  Foerstner's simplified
 * estimator for a diagonal weight matrix (csrc/fba_vce.h).  The 2 n_pts observation rows (PHO order, x y interleaved
 * like v) carry a group id in [0, n_groups), or -1: the row belongs to no estimated group and keeps its weight.
 * One round:
 *   1  Gauss-Newton steps from the device xhat while deltasum > Threshold_Value, at least one, at most Iteration_Cap;
 *   2  the selected inverse and q = a Cx a' per row, as the reliability function forms it;
 *   3  per row r = 1 - q / sigma^2 and t = (s v / sigma)^2, s the current sqrt weight (1 without weights), sigma
 *      Meas_std (Meas_std_y for a y row); per group R = sum r, T = sum t, n the row count; sigma2 = T / R;
 *   4  status per group: EMPTY n = 0; WEAK R < min_redundancy (factor 1, weights kept); CLIPPED the estimate lies
 *      outside [1 / clip, clip] and is clamped to it (T = 0 gives 1 / clip); OK otherwise.  Converged: every OK group
 *      has |sigma2 - 1| <= tol and no group is CLIPPED;
 *   5  not converged and not the last allowed round: the sqrt weights of each group's rows are multiplied in place by
 *      1 / sqrt(sigma2) and component[g] *= sigma2 -- the group's cumulative variance factor relative to its
 *      starting weights (user weights are allowed: they are the starting weights).
 * After the last round one further plain Gauss-Newton step leaves the context as the adjustment loop leaves one that
 * was given these weights: the residuals, the post-fit outputs and the weight getter work unchanged, and the getter
 * returns starting weight / component[group].
 * Two further entries close the redundancy sum (sum of R over all n_groups + 2 = n + n_prior - u, + 7 with inner
 * constraints); they are reported and never rescaled (component 1): [n_groups] the rows with id -1, [n_groups + 1]
 * the context's priors, R = sum (1 - p_j Cx_jj), T = sum p_j v_j^2, host arithmetic on the cofactor diagonal.  The
 * priors' sigma stay constants of the context: the image groups are estimated RELATIVE TO the stated prior accuracies.
 *   component [n_groups + 2]; table [max_rounds][n_groups + 2][4]: R, T, n and the sigma2 the round found (1 for EMPTY
 *   and WEAK, the clamped value for CLIPPED; T / R for the two report entries), rows of rounds not run are left alone;
 *   status [n_groups + 2] of the last round (the report entries: OK, or EMPTY without rows); *rounds the rounds run;
 *   *iterations every Gauss-Newton step of the call, the final one included; *converged 1 / 0.  Any output pointer
 *   may be NULL.  max_rounds exhausted is FBA_OK with *converged = 0; max_rounds = 1 estimates only and leaves the
 *   weighting untouched.  A non-finite sum returns FBA_ERR_NONFINITE.
 * Checked on the host before any GPU call, FBA_ERR_ARG: n_groups outside [1, FBA_VCE_MAX_GROUPS], an id outside
 * [-1, n_groups), a non-finite or out-of-range option (max_rounds >= 1, tol >= 0, min_redundancy >= 0, clip >= 1), a
 * call between the asynchronous solve and its finish.  FBA_ERR_UNSUPPORTED: world > 1; a robust loss (its IRLS factor
 * and a variance component would fight over the same residuals); damping > 0.  A refused call leaves the context
 * untouched.  The first rescale of an unweighted context switches its weights on (the accumulation graph is
 * re-captured once, as by the weight setter); later rescales write in place and re-capture nothing.  One GPU, plain
 * launches on the context's stream, fixed-order sums: two calls on two fresh contexts are bitwise equal.  With
 * fba_set_timing on, fba_last_timings' [7] afterwards holds the device time of the call's own kernels (the
 * reliability part and the group sums of every round, not the steps), [0..6] 0.
 * fba_vce_host (host only, no GPU): the group sums in index order over n_rows rows with given r and t, then the same
 *   estimate, clamp, factor and status: sums [n_groups + 1][3] R T n (row n_groups: id -1), sigma2 / factor / status
 *   [n_groups].  Non-finite sums: the outputs are filled and FBA_ERR_NONFINITE is returned. */
enum { FBA_VCE_OK = 0, FBA_VCE_EMPTY = 1, FBA_VCE_WEAK = 2, FBA_VCE_CLIPPED = 3 };
#define FBA_VCE_MAX_GROUPS 256
typedef struct fba_vce_options {
    int32_t max_rounds;      /* >= 1; default (NULL options) 10; 1 = estimate only, nothing re-weighted */
    int32_t reserved;
    double  tol;             /* default 1e-3 */
    double  min_redundancy;  /* default 1.0  */
    double  clip;            /* default 100  */
} fba_vce_options;
int fba_vce(fba_ctx* ctx, int32_t n_groups, const int32_t* group /*[2 n_pts] PHO order, x y interleaved*/,
            const fba_vce_options* o, double* component /*[n_groups+2]*/,
            double* table /*[max_rounds][n_groups+2][4]: R, T, n, sigma2 of the round*/,
            int32_t* status /*[n_groups+2], last round*/, int32_t* rounds, int32_t* iterations, int32_t* converged);
int fba_vce_host(int64_t n_rows, int32_t n_groups, const int32_t* group, const double* r, const double* t,
                 const fba_vce_options* o, double* sums /*[n_groups+1][3]*/, double* sigma2, double* factor,
                 int32_t* status);

/* Baarda data snooping over the image points (no reference counterpart: main.m never tests a measurement): the
 * measurements whose w-test exceeds crit are eliminated and, once the adjustment is clean, re-checked -- on the device,
 * from the reliability function's q and v (csrc/fba_snoop.h).  State is kept per image point (a PHO row: its x and y
 * rows together): active, excluded -- both weights are 1e-12 x the starting weight, the weight setter's way of
 * excluding a measurement -- or re-admitted.  One round:
 *   1  Gauss-Newton steps from the device xhat while deltasum > Threshold_Value, at least one, at most Iteration_Cap;
 *   2  the selected inverse and q = a Cx a' per row, as the reliability function forms it;
 *   3  per active point W = max(|w_x|, |w_y|), r and w as the reliability function's (0 where r < 1e-10); per excluded
 *      point the statistic of its predicted residual, W~ = max over its rows of |s0 v| / sqrt(sigma^2 + q / 1e-12), s0
 *      the starting sqrt weight: a division, so a row whose r = 1 - 1e-12 x has lost x keeps its statistic;
 *   4  candidates: the active points with W > crit whose removal leaves their tie point at least min_rays active
 *      observations (a control observation has no tie point) and their image at least min_img_points, and that were
 *      not re-admitted before (a re-admitted point is never a candidate again, so the rounds cannot cycle);
 *   5  a candidate is eliminated when it has the largest W among the candidates of its tie point and among those of its
 *      image, the lower PHO row between equal W: at most one per tie point and one per image in a round, so the
 *      neighbours a gross error smears over wait for the next round, where they usually pass;
 *   6  a round that eliminates nothing runs the back-check: every excluded point with W~ <= crit is re-admitted at
 *      exactly its starting weights, the points the caller pre-excluded included.  Neither: converged;
 *   7  otherwise the weights are changed and the next round begins.  The picks of the round max_rounds are found and
 *      not applied (FBA_OK, *converged = 0); so are those that would take the excluded share past max_share of n_pts
 *      (*converged = 0, bit 1 of *status_bits).
 * Every solve of the call is followed by the selected inverse, which consumes its factor: afterwards xhat, the
 * residuals function and the weight getter are those of the adjustment loop run with the final weights, and the
 * post-fit outputs need one further step first, as after any other consumer of the factor.  Where nothing was changed
 * (no candidate, or max_rounds = 1 without pre-excluded points) xhat and the weighting are bitwise those of fba_adjust.
 *   excluded [n_pts], PHO order, in/out, may be NULL (all active): on entry nonzero = the point starts excluded (its
 *   weights are lowered before round 1, also with max_rounds = 1); on exit 0 active, 1 excluded, 2 re-admitted.
 *   stat [n_pts]: W or W~ of the last round.  table [max_rounds][4]: per round the points it picked, the points its
 *   back-check passed, the points excluded after it, the largest W of an active point; rows of rounds not run are left
 *   alone.  *rounds, *iterations (every Gauss-Newton step of the call), *converged.  Any output pointer may be NULL.
 * Checked on the host before any GPU call, FBA_ERR_ARG: max_rounds, min_rays or min_img_points < 1, crit not finite or
 * <= 0, max_share not in (0, 1], a call between the asynchronous solve and its finish.  FBA_ERR_UNSUPPORTED: world > 1,
 * a robust loss, damping > 0 (the variance component function's refusals).  A refused call leaves the context untouched.
 * Priors are never candidates.  The first change of an unweighted context switches its weights on (the accumulation
 * graph is re-captured once); later rounds write in place.  Plain launches on the context's stream, no atomics: two
 * calls on two fresh contexts are bitwise equal.  With fba_set_timing on, fba_last_timings' [7] afterwards holds the
 * device time of the call's own kernels (the reliability part and the selection of every round, not the steps).
 * fba_snoop_host (host only, no GPU): one round's selection (steps 4 - 7's stop) by the same routines in index order.
 *   n points, W (or W~), state (0 / 1 / 2), tie (< 0: a control observation, else < n_tie), img (in [0, n_img)); the
 *   PHO row of a point is its index and n_pts = n.  pick / readmit [n]: 1 where the round eliminates / re-admits;
 *   *status_bits: bit 1 where the max_share stop cleared the picks. */
typedef struct fba_snoop_options {
    int32_t max_rounds;      /* >= 1; default (NULL options) 20; 1 = test only, nothing eliminated or re-admitted */
    int32_t min_rays;        /* default 2: a tie point keeps at least this many active rays */
    int32_t min_img_points;  /* default 6: the resection's minimum */
    int32_t reserved;
    double  crit;            /* default 3.29, the reliability table's flag line */
    double  max_share;       /* default 0.05 of n_pts */
} fba_snoop_options;
int fba_snoop(fba_ctx* ctx, const fba_snoop_options* o, uint8_t* excluded /*[n_pts] PHO order, in/out; may be NULL*/,
              double* stat /*[n_pts] W or W~ of the last round*/, double* table /*[max_rounds][4]*/, int32_t* rounds,
              int32_t* iterations, int32_t* converged, int32_t* status_bits);
int fba_snoop_host(int64_t n, const double* W, const uint8_t* state, const int32_t* tie, const int32_t* img,
                   int32_t n_tie, int32_t n_img, const fba_snoop_options* o, uint8_t* pick /*[n]*/,
                   uint8_t* readmit /*[n]*/, int32_t* status_bits);

/* Per-phase device timings of the last fba_step / fba_accumulate+fba_solve_update, in ms:
 * [0] params+linearize, [1] point-side, [2] image/pair/camera accumulation, [3] border,
 * [4] Cholesky+forward, [5] backward+border solve, [6] back-substitution+update, [7] total. */
int fba_last_timings(fba_ctx* ctx, double* ms /*[8]*/);
int fba_set_timing(fba_ctx* ctx, int32_t enabled);

/* Kernel probe (measurement only; no reference counterpart): while enabled, every launch of one
 * Cholesky kernel is bracketed by HIP events on the stream it runs on -- enabled = 1: k_syrk_multi (the
 * bulk trailing update of a tree level), 2: k_panel (the level's diagonal-block factorisations and
 * panel solves, the critical path); 0 turns the probe off.  fba_probe_stats synchronises and returns,
 * over the launches since the probe was enabled: out[0] launches, out[1] summed kernel ms, out[2]
 * algorithmic flops, out[3] reserved.  The probe records at most one step's worth of launches. */
int fba_set_probe(fba_ctx* ctx, int32_t enabled);
int fba_probe_stats(fba_ctx* ctx, double* out /*[4]*/);

/* (tests) The bound of every device hand-off poll of this context, in sleeps (0: the default
 * 1 << 22, ~0.3 s; negative: FBA_ERR_ARG; values above 2^32 - 1 are clamped to it; FBA_FLAG_SPINS in
 * the environment sets it at fba_create, where <= 0 is the default): a low bound forces the timeout path -- the abort
 * reaches every wait, the step returns FBA_ERR_HIP and xhat stays as before it. */
int fba_set_spin_bound(fba_ctx* ctx, int64_t spins);

/* Test hook (no reference counterpart): the 14x14 bordered solve of the inner-constraint combine
 * (k_border_combine, one workgroup on `device`) for a given symmetric 15x15 Gram matrix of the
 * forward-solved rows [y | A (7) | B (7)] (row-major): coef = [z; k] solving
 * [[A'A - I, A'B], [B'A, B'B]] [z; k] = -[A'y; B'y]. */
int fba_test_border_solve(int32_t device, const double* gram /*[225]*/, double* coef /*[14]*/);

/* Test hook (no reference counterpart): the number of device and pinned allocations the library holds in
 * this process right now, over all contexts.  fba_destroy, and a failed fba_create, leave it where it was. */
int fba_test_live_allocations(int64_t* n);

#ifdef __cplusplus
}
#endif
#endif /* FBA_H_ */
