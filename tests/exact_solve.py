"""An exact solve of one pass of the adjustment, in 50-digit mpmath: the reference of tests/test_weak_points_host.py
and tests/test_gpu_weak_points.py, where a tie point's 3 x 3 block V = Jp'PJp has cond 1e4 .. 1e10 and no fp64 solve
-- the oracle's explicit inverse least of all -- is accurate enough to judge another.

TEST INFRASTRUCTURE ONLY (host, no GPU).  The inputs are fp64 arrays (every fp64 number is an exact mpf); all arithmetic
runs at mp.dps = 50, so the algorithm shares no rounding with anything in fp64; the outputs are rounded to fp64 once.

The unknowns are laid out as the reference's xhat: `uc` camera-side unknowns (EOPs, IOPs, distortions), then 3 per
tie point.  With N = A'PA = [[Ncc, Ncp], [Npc, V]] (V block diagonal), b = A'Pw:

    block form (solve):   S = Ncc - sum_t W_t V_t^-1 W_t',  r = b_c - sum_t W_t V_t^-1 b_t,  W_t = Ncp's columns of t
                          [[S, Gc], [Gc', 0]] [dc; k] = [-r; 0]   (Gc = G's camera rows; G's tie rows are zero,
                          BuildAwG.m:514-527, asserted)           dp_t = -V_t^-1 (b_t + W_t' dc)
                          C = the camera block of that bordered inverse,  T_t = V_t^-1 W_t',
                          Cx_pp(t) = V_t^-1 + T_t C T_t',  Cx_pc(t) = -T_t C,
                          a Cx a' = ac C ac' - 2 ap (T_t C) ac' + ap Cx_pp(t) ap'  for a row a = [ac, ap] of point t
    dense form (solve_dense): mp.lu_solve / mp.inverse of the full (bordered) N -- a cross-check on tiny inputs.

Damping (include/fba.h, fba_set_damping): V_l = V + lambda diag(V), S' formed with V_l, then S' + lambda diag(S'),
bordered as before; the cofactors returned with lambda > 0 are those of the damped matrix.
"""
import numpy as np
from mpmath import mp, mpf

DPS = 50


def _mp(x):
    return mpf(float(x))


def _inv3(V):
    """3 x 3 inverse by the adjugate, in mp (exact to ~cond x 1e-50)"""
    c00 = V[1][1] * V[2][2] - V[1][2] * V[2][1]
    c01 = V[0][2] * V[2][1] - V[0][1] * V[2][2]
    c02 = V[0][1] * V[1][2] - V[0][2] * V[1][1]
    det = V[0][0] * c00 + V[1][0] * c01 + V[2][0] * c02
    c11 = V[0][0] * V[2][2] - V[0][2] * V[2][0]
    c12 = V[0][2] * V[1][0] - V[0][0] * V[1][2]
    c22 = V[0][0] * V[1][1] - V[0][1] * V[1][0]
    c10 = V[1][2] * V[2][0] - V[1][0] * V[2][2]
    c20 = V[1][0] * V[2][1] - V[1][1] * V[2][0]
    c21 = V[0][1] * V[2][0] - V[0][0] * V[2][1]
    return [[c00 / det, c01 / det, c02 / det], [c10 / det, c11 / det, c12 / det], [c20 / det, c21 / det, c22 / det]]


def _rows(A, uc):
    """per row of A: (camera columns, their values in mp, tie point or -1, its three tie values in mp)"""
    n, u = A.shape
    nt = (u - uc) // 3
    assert uc + 3 * nt == u
    out = []
    for i in range(n):
        nz = np.nonzero(A[i])[0]
        cc = [int(j) for j in nz if j < uc]
        tp = sorted({(int(j) - uc) // 3 for j in nz if j >= uc})
        assert len(tp) <= 1, "a row of A touches one tie point at most"
        t = tp[0] if tp else -1
        ap = [_mp(A[i, uc + 3 * t + k]) for k in range(3)] if t >= 0 else None
        out.append((cc, [_mp(A[i, j]) for j in cc], t, ap))
    return out, nt


def solve(A, w, P, uc, G=None, lam=0.0, raw=False):
    """The block form.  A (n, u), w (n), P (n) fp64; uc camera-side unknowns; G (u, d) or None; lam the damping.
    -> dict(delta (u), cx_tie (nt, 3, 3), cx_cam_diag (uc), aCa (n)), fp64, delta in the scaled units of A
    (oracle.descale is the caller's).  raw=True keeps the mp numbers (object arrays), for comparisons below fp64."""
    rnd, dt = ((lambda x: x), object) if raw else (float, np.float64)
    A = np.asarray(A, dtype=np.float64)
    n, u = A.shape
    with mp.workdps(DPS):
        rows, nt = _rows(A, uc)
        lam_ = _mp(lam)
        Pm = [_mp(p) for p in P]
        wm = [_mp(x) for x in w]
        zero = mpf(0)
        Ncc = [[zero] * uc for _ in range(uc)]
        bc = [zero] * uc
        V = [[[zero] * 3 for _ in range(3)] for _ in range(nt)]
        bp = [[zero] * 3 for _ in range(nt)]
        W = [dict() for _ in range(nt)]  # camera column -> its three entries of Ncp
        for i, (cc, cv, t, ap) in enumerate(rows):
            p = Pm[i]
            pw = p * wm[i]
            pc = [p * v for v in cv]
            for a, ja in enumerate(cc):
                bc[ja] += cv[a] * pw
                row = Ncc[ja]
                for b_, jb in enumerate(cc):
                    row[jb] += pc[a] * cv[b_]
            if t >= 0:
                pa = [p * v for v in ap]
                for k in range(3):
                    bp[t][k] += ap[k] * pw
                    for m in range(3):
                        V[t][k][m] += pa[k] * ap[m]
                Wt = W[t]
                for a, ja in enumerate(cc):
                    e = Wt.setdefault(ja, [zero, zero, zero])
                    for k in range(3):
                        e[k] += cv[a] * pa[k]
        # eliminate the points
        Vi, Tt, supp = [], [], []
        S = [r[:] for r in Ncc]
        r = bc[:]
        for t in range(nt):
            Vl = [row[:] for row in V[t]]
            for k in range(3):
                Vl[k][k] = Vl[k][k] * (1 + lam_)
            vi = _inv3(Vl)
            Vi.append(vi)
            cols = sorted(W[t])
            supp.append(cols)
            # T = V^-1 W' : per camera column j the 3-vector V^-1 W_j
            T = {j: [sum(vi[k][m] * W[t][j][m] for m in range(3)) for k in range(3)] for j in cols}
            Tt.append(T)
            vb = [sum(vi[k][m] * bp[t][m] for m in range(3)) for k in range(3)]
            for ja in cols:
                wa = W[t][ja]
                r[ja] -= sum(wa[k] * vb[k] for k in range(3))
                row = S[ja]
                for jb in cols:
                    tb = T[jb]
                    row[jb] -= wa[0] * tb[0] + wa[1] * tb[1] + wa[2] * tb[2]
        if lam:
            for j in range(uc):
                S[j][j] = S[j][j] * (1 + lam_)
        d = 0
        if G is not None:
            G = np.asarray(G, dtype=np.float64)
            assert not G[uc:].any(), "the inner constraints touch the camera-side rows only"
            d = G.shape[1]
        K = mp.matrix(uc + d, uc + d)
        for i in range(uc):
            for j in range(uc):
                K[i, j] = S[i][j]
            for j in range(d):
                K[i, uc + j] = K[uc + j, i] = _mp(G[i, j])
        rhs = mp.matrix(uc + d, 1)
        for i in range(uc):
            rhs[i] = -r[i]
        # mp.lu_solve's own steps, with the one factorisation shared by the right-hand side and the inverse's columns
        LU, piv = mp.LU_decomp(K)
        sol = mp.U_solve(LU, mp.L_solve(LU, rhs, piv))
        dc = [sol[i] for i in range(uc)]
        C = []  # the camera block of the bordered inverse, column by column (symmetric: columns are rows)
        for j in range(uc):
            e = mp.matrix(uc + d, 1)
            e[j] = 1
            col = mp.U_solve(LU, mp.L_solve(LU, e, piv))
            C.append([col[i] for i in range(uc)])
        delta = np.zeros(u, dtype=dt)
        delta[:uc] = [rnd(x) for x in dc]
        cx_tie = np.zeros((nt, 3, 3), dtype=dt)
        CPP = []
        TC = []  # per point: camera column j of its support -> the 3-vector (T C)[:, j]
        for t in range(nt):
            cols, T, vi = supp[t], Tt[t], Vi[t]
            g = [bp[t][k] + sum(W[t][j][k] * dc[j] for j in cols) for k in range(3)]
            for k in range(3):
                delta[uc + 3 * t + k] = rnd(-sum(vi[k][m] * g[m] for m in range(3)))
            tc = {j: [sum(T[i][k] * C[i][j] for i in cols) for k in range(3)] for j in cols}
            TC.append(tc)
            cpp = [[vi[k][m] + sum(tc[j][k] * T[j][m] for j in cols) for m in range(3)] for k in range(3)]
            CPP.append(cpp)
            for k in range(3):
                for m in range(3):
                    cx_tie[t, k, m] = rnd(cpp[k][m])
        aCa = np.zeros(n, dtype=dt)
        for i, (cc, cv, t, ap) in enumerate(rows):
            q = zero
            for a, ja in enumerate(cc):
                q += cv[a] * sum(C[ja][jb] * cv[b_] for b_, jb in enumerate(cc))
            if t >= 0:
                tc, cpp = TC[t], CPP[t]
                # ap (T C) ac' over the row's camera columns (all of them in the point's support)
                cross = sum(cv[a] * sum(ap[k] * tc[ja][k] for k in range(3)) for a, ja in enumerate(cc))
                q += -2 * cross + sum(ap[k] * cpp[k][m] * ap[m] for k in range(3) for m in range(3))
            aCa[i] = rnd(q)
        cam_diag = np.array([rnd(C[j][j]) for j in range(uc)], dtype=dt)
    return dict(delta=delta, cx_tie=cx_tie, cx_cam_diag=cam_diag, aCa=aCa)


def solve_dense(A, w, P, uc, G=None):
    """The same quantities of the undamped system from the full (bordered) N by mp.lu_solve and mp.inverse: a
    cross-check on tiny inputs (u^3 mp operations).  -> the same dict, plus "mp": delta, the tie blocks and a Cx a'
    as mp numbers, for comparisons below fp64."""
    A = np.asarray(A, dtype=np.float64)
    n, u = A.shape
    nt = (u - uc) // 3
    with mp.workdps(DPS):
        Am = mp.matrix(A.tolist())
        PA = mp.matrix(n, u)
        for i in range(n):
            p = _mp(P[i])
            for j in np.nonzero(A[i])[0]:
                PA[i, int(j)] = p * Am[i, int(j)]
        N = Am.T * PA
        b = PA.T * mp.matrix([_mp(x) for x in w])
        d = 0 if G is None else G.shape[1]
        K = mp.matrix(u + d, u + d)
        for i in range(u):
            for j in range(u):
                K[i, j] = N[i, j]
            for j in range(d):
                K[i, u + j] = K[u + j, i] = _mp(G[i, j])
        rhs = mp.matrix(u + d, 1)
        for i in range(u):
            rhs[i] = -b[i]
        sol = mp.lu_solve(K, rhs)
        Cx = mp.inverse(K)
        aCa = []
        for i in range(n):
            nz = [int(j) for j in np.nonzero(A[i])[0]]
            aCa.append(sum(Am[i, ja] * Cx[ja, jb] * Am[i, jb] for ja in nz for jb in nz))
        out = dict(delta=np.array([float(sol[i]) for i in range(u)]),
                   cx_tie=np.array([[[float(Cx[uc + 3 * t + k, uc + 3 * t + m]) for m in range(3)] for k in range(3)]
                                    for t in range(nt)]).reshape(nt, 3, 3),
                   cx_cam_diag=np.array([float(Cx[j, j]) for j in range(uc)]),
                   aCa=np.array([float(q) for q in aCa]),
                   mp=dict(delta=[sol[i] for i in range(u)], aCa=aCa, cx_cam_diag=[Cx[j, j] for j in range(uc)],
                           cx_tie=[[[Cx[uc + 3 * t + k, uc + 3 * t + m] for m in range(3)] for k in range(3)]
                                   for t in range(nt)]))
    return out
