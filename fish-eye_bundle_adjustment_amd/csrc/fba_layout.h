// fba_layout.h -- the layout of every device buffer, named once (included by fba_internal.h).
//
// The kernel that writes a buffer, the kernels that read it and the allocation that sizes it all take
// the row widths, offsets and totals from here.  Plain constexpr declarations only, no HIP qualifiers:
// the host-only planner and its checkers compile against it.
#pragma once
#include <cstdint>

namespace fba {

// ---- fixed row widths ----
constexpr int OBS_REC = 12;      // d_WT row: Jp and the EOP rotation columns (obs_rec_rows, fba_kernels.hip)
constexpr int T_ROW = 18;        // T = W Vinv / U = W R row of one observation (6 x 3, row a at 3 a)
constexpr int PAIR_BLK = 36;     // pair-block partial (6 x 6), d_ppart row
constexpr int G_ROW = 7;         // inner-constraint columns of one EOP row
constexpr int G_BLK = 6 * G_ROW; // d_G block of one image (6 x 7, row-major): 42
constexpr int GPT = 18;          // general point table: Vinv 6 | R 6 | rb 3 | vb 3
constexpr int GUG = 36;          // gimg table: Ug 18 | sum of T_o 18
constexpr int GUG_T = 18;        // offset of its T half
constexpr int BORDER_COLS = 14;  // border columns: W_l 0..6 | D^2 7..13 (A and B right-hand sides)
constexpr int GRAM_N = 120;      // Gram entries: lower triangle of the 15 forward-solved RHS rows
constexpr int GRAM_BLK = 256;    // d_gblk row: one column block's [16][16] Gram partial
constexpr int CAM_SEG = 64;      // k_red_cam_seg: segments of a camera's chunk list, d_cseg [n_cam][CAM_SEG][cam_part]
constexpr int BW_SEG = 32;       // k_border_weights: segments of the EOP rows
constexpr int GRAM_SEG = 16;     // k_border_gram: segments of the rows
constexpr int ELL_OUT = 12;      // error ellipsoid of one tie point: 3 semi-axes | 3 x 3 axes
constexpr int TIE_BLK = 6;       // tie point's 3 x 3 covariance block (00 01 02 11 12 22)
constexpr int RSD_ROW = 5;       // BuildRSD row
constexpr int RES_ROW = 2 + RSD_ROW;  // d_res per observation: v (2) + rsd (5)
constexpr int RAY_REC = 6;       // image ray: C, d in the object frame
constexpr int RESECT_REC = 8;    // resection record (64 B): xu yu | d in the camera frame | X Y Z of the object point

constexpr int CHUNK_OBS = 256;  // observations per k_lin_reduce / k_lin_point workgroup (chunk)
constexpr int LR_PROF = 10;     // FBA_LR_PROFILE: 64-bit words per chunk (k_lin_reduce's stamps, fba_capi.cpp's print)
constexpr int PTRACE_WG = 2048; // FBA_PANEL_TRACE: workgroup slots per level
constexpr int FTRACE = 56;      // FBA_PANEL_TRACE: stamps per k_chol_flow record ([48]: its workgroup's start)
// tie points per chunk and co-visibility terms per chunk staged in LDS (a single larger point's are
// read from HBM instead): smaller for nK >= 6, whose wider Jacobian rows leave less of the 160 KiB LDS
// (k_lin_reduce's LR<NK>::LDS, static_assert there); the host chunking uses the same numbers
constexpr int chunk_pts(int nk) { return nk <= 5 ? 64 : 32; }
constexpr int chunk_terms(int nk) { return nk <= 5 ? 2048 : 1024; }

// per-image device table (k_params): eop[6], M[9], dM/domega[9], dM/dphi[9], dM/dkappa[9], pad
constexpr int IMG_TAB = 48;
// per-camera device table: xp yp c ydir P1 P2 rmax2 pad, K[nK], scale[nK] (rmax^(2j)), 1 / scale[nK]
constexpr int CAM_TAB_HDR = 8;

// ---- widths that depend on cw = 5 + nK, the IOPs of one camera ----
constexpr int cam_width(int nk) { return 5 + nk; }
constexpr int cam_tab_row(int cw) { return CAM_TAB_HDR + 3 * (cw - 5); }
constexpr int jac_cols(int cw) { return 9 + cw; }                  // 6 EOP | cw camera | 3 XYZ
constexpr int jac_stride(int cw) { return 2 * jac_cols(cw) + 2; }  // d_J row: row x, row y, w
// d_pt_tab row: Vinv 6 | vb 3 | b 3 | Wc 3cw | Tc 3cw
constexpr int PT_VINV = 0, PT_VB = 6, PT_B = 9, PT_WC = 12;
constexpr int pt_tc(int cw) { return PT_WC + 3 * cw; }
constexpr int pt_stride(int cw) { return PT_WC + 6 * cw; }
// d_ipart row: 21 lower of the diagonal block | 6 RHS | 6cw image-camera
constexpr int IMG_PART_CAM = 27;
constexpr int img_part(int cw) { return IMG_PART_CAM + 6 * cw; }
// d_cpart / d_cseg row: packed lower triangle of the camera block | cw RHS
constexpr int cam_tri(int cw) { return cw * (cw + 1) / 2; }
constexpr int cam_part(int cw) { return cam_tri(cw) + cw; }
constexpr int gpc_tab(int cw) { return 6 * cw; }        // d_gcu row: Uc 3cw | Tc 3cw
constexpr int xcam_part(int cw) { return 6 * cw; }      // d_xpart row: image x foreign camera
constexpr int campair_part(int cw) { return cw * cw; }  // d_kpart row: camera x camera

// the same per instantiation: Lay<NK>, LR<NK> (fba_kernels.hip) and GL<NK> (fba_general.hip) derive from it
template <int NK>
struct LayNK {
    static constexpr int CW = cam_width(NK), NJ = jac_cols(CW), JS = jac_stride(CW), PS = pt_stride(CW);
    static constexpr int NIMG = img_part(CW), NPK = cam_tri(CW), NCAM = cam_part(CW);
    static constexpr int NX = xcam_part(CW), NKK = campair_part(CW), GC = gpc_tab(CW);
};

// ---- d_bscr, the border scratch ----
constexpr int BSC_WSEG = 0;                                 // [BW_SEG][BORDER_COLS] k_border_weights segment sums
constexpr int BSC_GRAM = BSC_WSEG + BW_SEG * BORDER_COLS;   // [GRAM_SEG][GRAM_N] Gram segments
constexpr int BSC_COEF = BSC_GRAM + GRAM_SEG * GRAM_N;      // [16] combine coefficients
constexpr int BSC_SCALE = BSC_COEF + 16;                    // [16] the subtree split's B-row scales sqrt(W_d)
constexpr int BSC_TOTAL = BSC_SCALE + 16;

// ---- d_scal, the scalars of a solve, and their mirror in the pinned h_pinned ----
constexpr int SCAL_SPARE0 = 0; // (mirrored, no writer today)
constexpr int SCAL_FAIL = 1;   // failure word: 0 ok, row + 1 > 0 a non-positive pivot, -1 a hand-off timeout
constexpr int SCAL_DSUM = 2;   // deltasum (this rank's share; fba_deltasum_device hands out its address)
constexpr int SCAL_SPARE3 = 3; // (mirrored, no writer today)
constexpr int SCAL_MIRROR = 4; // slots [0, SCAL_MIRROR) go to h_pinned at the same index (k_sum_parts)
constexpr int SCAL_SEQ = 5;    // k_sum_parts' running count of solves
constexpr int SCAL_SPINS = 6;  // this context's hand-off poll bound (fba_chol.hip spin_expired)
constexpr int SCAL_DAMP = 7;   // the Levenberg-Marquardt damping parameter lambda (fba_set_damping; 0: off)
constexpr int SCAL_WL = 8;     // [G_ROW] border weights W_l
constexpr int SCAL_D2 = 16;    // [G_ROW] border weights D^2
constexpr int SCAL_ZEROED = 16;      // slots zeroed at creation
constexpr int SCAL_TOTAL = 32 + 256; // allocation (the tail is spare)
constexpr int HPIN_FAIL = SCAL_FAIL, HPIN_DSUM = SCAL_DSUM;
constexpr int HPIN_SEQ = 4;    // the count of finished solves, written after the mirrored slots
constexpr int HPIN_TOTAL = 64;
static_assert(SCAL_WL + G_ROW <= SCAL_D2 && SCAL_D2 + G_ROW <= SCAL_TOTAL && HPIN_SEQ >= SCAL_MIRROR, "d_scal slots overlap");

}  // namespace fba
