"""TwoViewReconstruction::Reconstruct (reference src/TwoViewReconstruction.cc) transcribed line by line, one hypothesis after the other, with
the reference's own choices: numpy.linalg.svd where it calls Eigen's JacobiSVD, numpy.linalg.inv where it calls .inverse(), sequential
sums, math.acos, float32 where it uses float.  It is the yardstick for the cost of departures (a) - (c) of DESIGN.md 6o; parity with an
Eigen build stays unpinned (LAPACK's signs are not Eigen's).  Citations are line numbers of that file."""
import math

import numpy as np

F32 = np.float32


def random_int_sets(draws, N, its):
    """:99-115 with DUtils::Random::RandomInt(0, size - 1) = (int)(((double)rand() / ((double)RAND_MAX + 1.0)) * size), literally: a
    list of all indices, the drawn position replaced by the back, the back popped"""
    sets = []
    for it in range(its):
        avail = list(range(N))                                            # :101
        row = []
        for j in range(8):
            d = len(avail) - 1 - 0 + 1
            randi = int((float(int(draws[it][j])) / (2147483647.0 + 1.0)) * d) + 0        # :106
            row.append(avail[randi])                                      # :107-109
            avail[randi] = avail[-1]                                      # :112
            avail.pop()                                                   # :113
        sets.append(row)
    return sets


def seq_sum(x):
    x = np.asarray(x, F32)
    return np.cumsum(x, dtype=F32)[-1] if len(x) else F32(0)


def normalize(k):                                                         # :949-1000
    k = np.asarray(k, F32)
    N = F32(len(k))
    meanX, meanY = seq_sum(k[:, 0]) / N, seq_sum(k[:, 1]) / N
    x, y = k[:, 0] - meanX, k[:, 1] - meanY
    meanDevX, meanDevY = seq_sum(np.abs(x)) / N, seq_sum(np.abs(y)) / N
    sX, sY = F32(1.0 / float(meanDevX)), F32(1.0 / float(meanDevY))
    T = np.zeros((3, 3), F32)
    T[0, 0], T[1, 1], T[0, 2], T[1, 2], T[2, 2] = sX, sY, -meanX * sX, -meanY * sY, 1
    return np.stack([x * sX, y * sY], 1), T


def compute_h21(p1, p2):                                                  # :287-326
    A = np.zeros((16, 9), F32)
    for i in range(8):
        u1, v1, u2, v2 = p1[i][0], p1[i][1], p2[i][0], p2[i][1]
        A[2 * i] = [0, 0, 0, -u1, -v1, -1, v2 * u1, v2 * v1, v2]
        A[2 * i + 1] = [u1, v1, 1, 0, 0, 0, -u2 * u1, -u2 * v1, -u2]
    return np.linalg.svd(A)[2][8].reshape(3, 3).astype(F32)


def compute_f21(p1, p2):                                                  # :338-373
    A = np.zeros((8, 9), F32)
    for i in range(8):
        u1, v1, u2, v2 = p1[i][0], p1[i][1], p2[i][0], p2[i][1]
        A[i] = [u2 * u1, u2 * v1, u2, v2 * u1, v2 * v1, v2, u1, v1, 1]
    Fpre = np.linalg.svd(A)[2][8].reshape(3, 3).astype(F32)
    U, w, Vt = np.linalg.svd(Fpre)
    w[2] = 0
    return ((U * w[None, :]) @ Vt).astype(F32)


def check_homography(H21, H12, u1, v1, u2, v2, sigma):                    # :382-466, the per-match arithmetic as arrays, the score summed in match order
    th = F32(5.991)
    inv = F32(1.0 / float(sigma * sigma))
    h, g = H21.reshape(-1), H12.reshape(-1)
    with np.errstate(all="ignore"):
        w2 = (1.0 / (g[6] * u2 + g[7] * v2 + g[8]).astype(np.float64)).astype(F32)
        a, b = (g[0] * u2 + g[1] * v2 + g[2]) * w2, (g[3] * u2 + g[4] * v2 + g[5]) * w2
        chi1 = ((u1 - a) * (u1 - a) + (v1 - b) * (v1 - b)) * inv
        w1 = (1.0 / (h[6] * u1 + h[7] * v1 + h[8]).astype(np.float64)).astype(F32)
        c, d = (h[0] * u1 + h[1] * v1 + h[2]) * w1, (h[3] * u1 + h[4] * v1 + h[5]) * w1
        chi2 = ((u2 - c) * (u2 - c) + (v2 - d) * (v2 - d)) * inv
        o1, o2 = chi1 > th, chi2 > th
        terms = np.stack([np.where(o1, F32(0), th - chi1), np.where(o2, F32(0), th - chi2)], 1).reshape(-1)
        return F32(0) + seq_sum(terms), ~(o1 | o2)


def check_fundamental(F21, u1, v1, u2, v2, sigma):                        # :474-556
    th, thScore = F32(3.841), F32(5.991)
    inv = F32(1.0 / float(sigma * sigma))
    f = F21.reshape(-1)
    with np.errstate(all="ignore"):
        a2, b2, c2 = f[0] * u1 + f[1] * v1 + f[2], f[3] * u1 + f[4] * v1 + f[5], f[6] * u1 + f[7] * v1 + f[8]
        num2 = a2 * u2 + b2 * v2 + c2
        chi1 = (num2 * num2 / (a2 * a2 + b2 * b2)) * inv
        a1, b1, c1 = f[0] * u2 + f[3] * v2 + f[6], f[1] * u2 + f[4] * v2 + f[7], f[2] * u2 + f[5] * v2 + f[8]
        num1 = a1 * u1 + b1 * v1 + c1
        chi2 = (num1 * num1 / (a1 * a1 + b1 * b1)) * inv
        o1, o2 = chi1 > th, chi2 > th
        terms = np.stack([np.where(o1, F32(0), thScore - chi1), np.where(o2, F32(0), thScore - chi2)], 1).reshape(-1)
        return F32(0) + seq_sum(terms), ~(o1 | o2)


def check_rt(R, t, K, u1, v1, u2, v2, inl, th2):                          # :1016-1155 with GeometricTools::Triangulate
    fx, fy, cx, cy = K[0, 0], K[1, 1], K[0, 2], K[1, 2]
    P1 = np.zeros((3, 4), F32)
    P1[:, :3] = K
    P2 = (K @ np.concatenate([R, t[:, None]], 1)).astype(F32)
    O2 = (-R.T @ t).astype(F32)
    N = len(u1)
    good = np.zeros(N, bool)
    counted = np.zeros(N, bool)
    p3d = np.zeros((N, 3), F32)
    cosines = []
    for i in range(N):
        if not inl[i]:
            continue
        A = np.stack([u1[i] * P1[2] - P1[0], v1[i] * P1[2] - P1[1], u2[i] * P2[2] - P2[0], v2[i] * P2[2] - P2[1]]).astype(F32)
        x = np.linalg.svd(A)[2][3]
        if x[3] == 0:                                                     # departure (e) of 6o: the reference reads an unset vector here
            continue
        with np.errstate(all="ignore"):
            p = (x[:3] / x[3]).astype(F32)
            if not np.isfinite(p).all():
                continue
            n1, n2 = p, p - O2
            d1, d2 = np.sqrt(F32(n1 @ n1)), np.sqrt(F32(n2 @ n2))
            cosP = F32(n1 @ n2) / (d1 * d2)
            if p[2] <= 0 and float(cosP) < 0.99998:
                continue
            q = (R @ p + t).astype(F32)
            if q[2] <= 0 and float(cosP) < 0.99998:
                continue
            iz1 = F32(1.0 / float(p[2]))
            e1 = (fx * p[0] * iz1 + cx - u1[i]) ** 2 + (fy * p[1] * iz1 + cy - v1[i]) ** 2
            if e1 > th2:
                continue
            iz2 = F32(1.0 / float(q[2]))
            e2 = (fx * q[0] * iz2 + cx - u2[i]) ** 2 + (fy * q[1] * iz2 + cy - v2[i]) ** 2
            if e2 > th2:
                continue
        cosines.append(cosP)
        p3d[i] = p
        counted[i] = True
        if float(cosP) < 0.99998:
            good[i] = True
    if cosines:
        cs = sorted(cosines)
        c = cs[min(50, len(cs) - 1)]
        parallax = F32(F32(F32(math.acos(min(1.0, max(-1.0, float(c))))) * F32(180)) / math.pi)
    else:
        parallax = F32(0)
    return len(cosines), parallax, good, counted, p3d


def reconstruct(P, kpts1, kpts2, matches, draws):
    """matches [N,2] (i ascending); draws [its,8] raw rand() results.  Returns a dict: ret, model (0 none, 1 H, 2 F), exit (the codes of
    two_view_ref), R21, t21, p3d / triangulated indexed by the feature of frame 1, inliers_h / inliers_f, SH, SF, RH."""
    import two_view_ref as R
    kpts1, kpts2 = np.asarray(kpts1, F32), np.asarray(kpts2, F32)
    m = np.asarray(matches).reshape(-1, 2)
    N = len(m)
    its = 200 if int(P["its"]) == 0 else int(P["its"])
    sigma = F32(1) if P["sigma"] == 0 else F32(P["sigma"])
    rh_thr = 0.5 if P["rh_threshold"] == 0 else float(F32(P["rh_threshold"]))
    minParallax = F32(1) if P["min_parallax"] == 0 else F32(P["min_parallax"])
    minTri = 50 if P["min_triangulated"] == 0 else int(P["min_triangulated"])
    K = np.array([[P["fx"], 0, P["cx"]], [0, P["fy"], P["cy"]], [0, 0, 1]], F32)
    sets = random_int_sets(draws, N, its)
    vPn1, T1 = normalize(kpts1)
    vPn2, T2 = normalize(kpts2)
    T2inv, T2t = np.linalg.inv(T2).astype(F32), T2.T
    u1, v1, u2, v2 = kpts1[m[:, 0], 0], kpts1[m[:, 0], 1], kpts2[m[:, 1], 0], kpts2[m[:, 1], 1]
    SH, SF, H21, F21 = F32(0), F32(0), np.zeros((3, 3), F32), np.zeros((3, 3), F32)
    inlH, inlF = np.zeros(N, bool), np.zeros(N, bool)
    win = [-1, -1]
    for it in range(its):                                                 # FindHomography :186-210, FindFundamental :243-267
        p1, p2 = vPn1[m[sets[it], 0]], vPn2[m[sets[it], 1]]
        with np.errstate(all="ignore"):
            H21i = (T2inv @ compute_h21(p1, p2) @ T1).astype(F32)
            H12i = np.linalg.inv(H21i).astype(F32) if np.isfinite(H21i).all() and np.linalg.det(H21i.astype(np.float64)) != 0 else np.full((3, 3), np.nan, F32)
            s, inl = check_homography(H21i, H12i, u1, v1, u2, v2, sigma)
            if s > SH:
                SH, H21, inlH, win[0] = s, H21i, inl, it
            F21i = (T2t @ compute_f21(p1, p2) @ T1).astype(F32)
            s, inl = check_fundamental(F21i, u1, v1, u2, v2, sigma)
            if s > SF:
                SF, F21, inlF, win[1] = s, F21i, inl, it
    out = {"ret": False, "model": 0, "exit": R.EXIT_OK, "R21": np.eye(3, dtype=F32), "t21": np.zeros(3, F32), "p3d": np.zeros((len(kpts1), 3), F32),
           "triangulated": np.zeros(len(kpts1), bool), "inliers_h": inlH, "inliers_f": inlF, "SH": SH, "SF": SF, "RH": F32(0), "win": win}
    if SH + SF == 0:                                                      # :132
        out["exit"] = R.EXIT_NO_SCORE
        return out
    RH = SH / (SH + SF)
    out["RH"] = RH
    th2 = F32(4.0 * float(sigma * sigma))

    def finish(Rm, t, good, counted, p3d):
        out["ret"], out["R21"], out["t21"] = True, Rm, t
        out["triangulated"][m[good, 0]] = True
        out["p3d"][m[counted, 0]] = p3d[counted]
        return out

    if float(RH) > rh_thr:                                                # ReconstructH :746-941
        out["model"] = 1
        Nin = int(inlH.sum())
        A = (np.linalg.inv(K) @ H21 @ K).astype(F32)
        U, w, Vt = np.linalg.svd(A)
        V = Vt.T
        s = F32(np.linalg.det(U) * np.linalg.det(Vt))
        d1, d2, d3 = w
        if float(d1 / d2) < 1.00001 or float(d2 / d3) < 1.00001:
            out["exit"] = R.EXIT_SINGULAR
            return out
        aux1, aux3 = np.sqrt((d1 * d1 - d2 * d2) / (d1 * d1 - d3 * d3)), np.sqrt((d2 * d2 - d3 * d3) / (d1 * d1 - d3 * d3))
        x1, x3 = [aux1, aux1, -aux1, -aux1], [aux3, -aux3, aux3, -aux3]
        aux_st = np.sqrt((d1 * d1 - d2 * d2) * (d2 * d2 - d3 * d3)) / ((d1 + d3) * d2)
        ctheta = (d2 * d2 + d1 * d3) / ((d1 + d3) * d2)
        stheta = [aux_st, -aux_st, -aux_st, aux_st]
        vR, vt = [], []
        for i in range(4):
            Rp = np.array([[ctheta, 0, -stheta[i]], [0, 1, 0], [stheta[i], 0, ctheta]], F32)
            vR.append((s * U @ Rp @ Vt).astype(F32))
            t = (U @ (np.array([x1[i], 0, -x3[i]], F32) * (d1 - d3))).astype(F32)
            vt.append(t / np.sqrt(F32(t @ t)))
        aux_sp = np.sqrt((d1 * d1 - d2 * d2) * (d2 * d2 - d3 * d3)) / ((d1 - d3) * d2)
        cphi = (d1 * d3 - d2 * d2) / ((d1 - d3) * d2)
        sphi = [aux_sp, -aux_sp, -aux_sp, aux_sp]
        for i in range(4):
            Rp = np.array([[cphi, 0, sphi[i]], [0, -1, 0], [sphi[i], 0, -cphi]], F32)
            vR.append((s * U @ Rp @ Vt).astype(F32))
            t = (U @ (np.array([x1[i], 0, x3[i]], F32) * (d1 + d3))).astype(F32)
            vt.append(t / np.sqrt(F32(t @ t)))
        bestGood, second, bestIdx, bestPar, bestRes = 0, 0, -1, F32(-1), None
        for i in range(8):
            nGood, par, good, counted, p3d = check_rt(vR[i], vt[i], K, u1, v1, u2, v2, inlH, th2)
            if nGood > bestGood:
                second, bestGood, bestIdx, bestPar, bestRes = bestGood, nGood, i, par, (good, counted, p3d)
            elif nGood > second:
                second = nGood
        if not second < 0.75 * bestGood:
            out["exit"] = R.EXIT_NO_WINNER
        elif not bestPar >= minParallax:
            out["exit"] = R.EXIT_PARALLAX
        elif not (bestGood > minTri and bestGood > 0.9 * Nin):
            out["exit"] = R.EXIT_FEW
        else:
            return finish(vR[bestIdx], vt[bestIdx], *bestRes)             # assigns vP3D too: the stated difference of 6o
        return out
    out["model"] = 2                                                      # ReconstructF :569-674
    Nin = int(inlF.sum())
    E21 = (K.T @ F21 @ K).astype(F32)
    U, w, Vt = np.linalg.svd(E21)                                         # DecomposeE :1194-1221
    t = U[:, 2] / np.sqrt(F32(U[:, 2] @ U[:, 2]))
    W = np.array([[0, -1, 0], [1, 0, 0], [0, 0, 1]], F32)
    R1 = (U @ W @ Vt).astype(F32)
    if np.linalg.det(R1) < 0:
        R1 = -R1
    R2 = (U @ W.T @ Vt).astype(F32)
    if np.linalg.det(R2) < 0:
        R2 = -R2
    hyp = [(R1, t), (R2, t), (R1, -t), (R2, -t)]
    res = [check_rt(Rm, tt, K, u1, v1, u2, v2, inlF, th2) for Rm, tt in hyp]
    goods = [r[0] for r in res]
    maxGood = max(goods)
    nMinGood = max(int(0.9 * Nin), minTri)
    nsimilar = sum(1 for g in goods if g > 0.7 * maxGood)
    if maxGood < nMinGood:
        out["exit"] = R.EXIT_FEW
        return out
    if nsimilar > 1:
        out["exit"] = R.EXIT_NO_WINNER
        return out
    c = goods.index(maxGood)
    if res[c][1] > minParallax:
        return finish(hyp[c][0], hyp[c][1], *res[c][2:])
    out["exit"] = R.EXIT_PARALLAX
    return out
