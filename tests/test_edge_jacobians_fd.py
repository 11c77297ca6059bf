"""CPU: the analytic Jacobians of the reprojection edges (EdgeSE3ProjectXYZ, EdgeStereoSE3ProjectXYZ and their pose-only forms) against
central differences of an error function stated here on its own.  The kernels and the restatements (tests/local_ba_ref.py,
tests/global_ba_ref.py, tests/pose_opt_ref.py) are held to each other bit for bit, so a wrong entry that both carry is invisible to that
comparison, and Levenberg-Marquardt still descends with it; a difference quotient is independent of both.

200 edges, half of them stereo, depths 3 .. 9 m, three pyramid levels, 0.7 px of noise; central differences at h = 1e-6 in the six pose
directions (left update exp(omega, upsilon)) and the three point directions.  From the numeric Jacobian J = de/d(pose, point) and the
weight w = rho1 invSigma2: Hll = Ji^T w Ji, bl = -Ji^T w e, Hpp = Jj^T w Jj, bp = -Jj^T w e and the 6 x 3 block Jj^T w Ji.

Measure: per edge and block, the largest |analytic - numeric| over the block's largest |numeric| entry; the maximum over the edges.

    bound        Hessian-type 1e-6        gradient 1e-3
    measured     Hll      Hpp      Hpl      bl       bp
    local_ba     3.2e-09  4.0e-10  2.1e-09  2.4e-04  2.0e-04     (robust)
    global_ba    3.2e-09  4.0e-10  2.1e-09  2.4e-04  2.0e-04     (robust = False)
    pose_opt              4.0e-10                    2.0e-04     (H: 21 columns, b: 6 columns)

The Hessian-type figures are the truncation and round-off of the difference quotient (about 1e-8 on entries of order 1e2).  The gradient
figures come from the stereo path of the restated error alone, which rounds 1 / z to float as the reference does: up to 4e-5 px on a
projection of some hundred px.  The mono edges of the same draw show 1e-9 in bl and 2e-10 in bp.  The three restatements share the
figures because all three take the error from one formula, and none of the 200 edges lies past the Huber bound, so the robust and the
plain weight are equal here (test_huber_region_mono draws edges that do).

The gradient figures sit within ten times their bound (a fifth of it).  That is the measure, not the Jacobian: it divides by the
edge's own largest gradient entry, which is proportional to the edge's own error, and the worst edge (a stereo one) happens to have
errors of 0.15, 0.06 and -0.04 px, a fifth of the typical 0.7 px, so the same 4e-5 px weighs five times as much.  Relative to the
largest gradient entry of all 200 edges the figures are 1.2e-05 and 1.1e-05.  A wrong sign or a swapped entry moves either kind by
order one (test_the_draw_and_the_check)."""
import numpy as np

import global_ba_ref as G
import local_ba_ref as LR
import pose_opt_ref as R6

F32, F64 = np.float32, np.float64
N_EDGES, H_STEP = 200, 1e-6
BOUND_HESSIAN, BOUND_GRADIENT = 1e-6, 1e-3
CAM = {k: F64(F32(v)) for k, v in (("fx", 458.654), ("fy", 457.296), ("cx", 367.215), ("cy", 248.375), ("bf", 47.91))}


# ---------------------------------------------------------------- the error, stated on its own in float64
def rotation(q):
    x, y, z, w = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]], F64)


def updated(d, Rm, t):
    """exp(d) (R, t) with omega = d[:3] first and upsilon = d[3:] second, to second order in omega (the third is 1e-18 at h = 1e-6)"""
    W = np.array([[0, -d[2], d[1]], [d[2], 0, -d[0]], [-d[1], d[0], 0]], F64)
    Rd = np.eye(3) + W + W @ W / 2
    return Rd @ Rm, Rd @ t + (np.eye(3) + W / 2) @ d[3:]


def error(Rm, t, X, obs, stereo):
    x, y, z = Rm @ X + t
    u = CAM["fx"] * x / z + CAM["cx"]
    e = [obs[0] - u, obs[1] - (CAM["fy"] * y / z + CAM["cy"])]
    if stereo:
        e.append(obs[2] - (u - CAM["bf"] / z))
    return np.array(e, F64)


def numeric(q, t, X, obs, stereo):
    """(e, J [rows, 9]): the pose directions in columns 0 .. 5, the point directions in 6 .. 8"""
    Rm = rotation(q)
    J = np.zeros((3 if stereo else 2, 9), F64)
    for k in range(9):
        d = np.zeros(9, F64)
        d[k] = H_STEP
        Rp, tp = updated(d[:6], Rm, t)
        Rn, tn = updated(-d[:6], Rm, t)
        J[:, k] = (error(Rp, tp, X + d[6:], obs, stereo) - error(Rn, tn, X - d[6:], obs, stereo)) / (2 * H_STEP)
    return error(Rm, t, X, obs, stereo), J


# ---------------------------------------------------------------- the edges and their numeric blocks, computed once
def edges(seed=20, n=N_EDGES, noise=0.7, every=2):
    """n edges, every `every`-th one stereo (0: none)"""
    rng = np.random.default_rng(seed)
    q = np.stack([R6.quat_from_rotvec(rng.standard_normal(3) * 0.3) for _ in range(n)])
    t = rng.standard_normal((n, 3)) * 0.5
    z = rng.uniform(3.0, 9.0, n)
    u, v = rng.uniform(20, 730, n), rng.uniform(20, 460, n)
    Xc = np.stack([(u - CAM["cx"]) / CAM["fx"] * z, (v - CAM["cy"]) / CAM["fy"] * z, z], 1)
    X = np.stack([rotation(q[i]).T @ (Xc[i] - t[i]) for i in range(n)])
    stereo = np.arange(n) % every == 1 if every else np.zeros(n, bool)
    level = rng.integers(0, 3, n)
    obs = np.stack([u, v, u - CAM["bf"] / z], 1) + noise * rng.standard_normal((n, 3))
    obs = obs.astype(F32).astype(F64)                              # observations are float keypoints
    isg = (1.0 / 1.44 ** level).astype(F32).astype(F64)
    return {"q": q, "t": t, "X": X, "obs": obs, "stereo": stereo, "isg": isg}


def inputs(E):
    """6l's per-edge input arrays"""
    n = len(E["isg"])
    I = {k: np.full(n, CAM[k], F64) for k in CAM}
    I.update(u=E["obs"][:, 0], v=E["obs"][:, 1], ur=np.where(E["stereo"], E["obs"][:, 2], -1.0), stereo=E["stereo"], isg=E["isg"])
    return I


def numeric_blocks(E, robust):
    """[n, 54] in 6l's layout from the numeric Jacobian; rho1 from this file's own error"""
    n = len(E["isg"])
    lin = np.zeros((n, 54), F64)
    huber = 0
    for i in range(n):
        st = bool(E["stereo"][i])
        e, J = numeric(E["q"][i], E["t"][i], E["X"][i], E["obs"][i], st)
        chi2 = E["isg"][i] * float(e @ e)
        delta, dsqr = (R6.DELTA_STEREO, R6.DSQR_STEREO) if st else (R6.DELTA_MONO, R6.DSQR_MONO)
        rho1 = delta / np.sqrt(chi2) if robust and chi2 > dsqr else 1.0
        huber += rho1 != 1.0
        w = rho1 * E["isg"][i]
        Jj, Ji = J[:, :6], J[:, 6:]
        Hll, Hpp, Hpl = Ji.T @ Ji * w, Jj.T @ Jj * w, Jj.T @ Ji * w
        lin[i] = np.concatenate([Hll[np.triu_indices(3)], -Ji.T @ e * w, Hpp[np.triu_indices(6)], -Jj.T @ e * w, Hpl.ravel()])
    return lin, huber


BLOCKS = {"Hll": slice(0, 6), "bl": slice(6, 9), "Hpp": slice(9, 30), "bp": slice(30, 36), "Hpl": slice(36, 54)}
_CACHE = {}


def cached(robust):
    if robust not in _CACHE:
        E = _CACHE.setdefault("edges", edges())
        _CACHE[robust] = numeric_blocks(E, robust)
    return _CACHE["edges"], _CACHE[robust][0]


def relative(analytic, num):
    """per edge: the largest difference over the block's largest numeric entry; the maximum over the edges"""
    return float((np.abs(analytic - num).max(1) / np.abs(num).max(1)).max())


def compare(name, lin, num, blocks=BLOCKS):
    out = {}
    for b, sl in blocks.items():
        out[b] = relative(lin[:, sl], num[:, sl])
    print(name, " ".join(f"{b} {v:.1e}" for b, v in out.items()))
    for b, v in out.items():
        assert v <= (BOUND_GRADIENT if b.startswith("b") else BOUND_HESSIAN), (name, b, v)
    return out


def quats(E):
    return np.stack([np.array(R6.normalize_rotation(list(q)), F64) for q in E["q"]])


# ---------------------------------------------------------------- the three restatements
def test_local_ba_edge_robust():
    E, num = cached(True)
    hub = LR.huber(LR.TH2_MONO) + LR.huber(LR.TH2_STEREO)
    _, _, lin = LR.edge_linearise(inputs(E), hub, quats(E), E["t"], E["X"])
    compare("local_ba robust", lin, num)


def test_global_ba_edge_plain():
    E, num = cached(False)
    hub = G.huber(G.HUBER2_MONO) + G.huber(G.HUBER2_STEREO)
    _, _, lin = G.edge_linearise(inputs(E), hub, quats(E), E["t"], E["X"], robust=False)
    compare("global_ba plain", lin, num)


def pose_opt_terms(E):
    """edge_terms takes one pose and many features: one call per edge"""
    P = R6.params(CAM["fx"], CAM["fy"], CAM["cx"], CAM["cy"], CAM["bf"])
    rows = []
    for i in range(len(E["isg"])):
        f = {"u": E["obs"][i:i + 1, 0], "v": E["obs"][i:i + 1, 1], "ur": np.where(E["stereo"][i:i + 1], E["obs"][i:i + 1, 2], -1.0),
             "stereo": E["stereo"][i:i + 1], "X": E["X"][i:i + 1], "invsigma2": E["isg"][i:i + 1]}
        q = [F64(v) for v in R6.normalize_rotation(list(E["q"][i]))]
        _, _, _, terms = R6.edge_terms(P, q, [F64(v) for v in E["t"][i]], f, True)
        rows.append(terms[0, :27])
    return np.stack(rows)


def test_pose_opt_edge():
    E, num = cached(True)
    terms = pose_opt_terms(E)
    # edge_terms keeps the 6 sums whose NEGATIVE is b: J^T w e = -bp
    lin = np.concatenate([terms[:, :21], -terms[:, 21:27]], 1)
    compare("pose_opt", lin, num[:, 9:36], {"Hpp": slice(0, 21), "bp": slice(21, 27)})


def test_huber_region_mono():
    """the draw above has no edge past the Huber bound, so rho1 = 1 in every weight.  60 mono edges with 3 px of noise put about half of
    them past it; a mono edge's restated error is all double, so this file's own rho1 agrees with the restatement's to round-off and
    the same bounds hold for the weighted columns (measured: Hessian-type 2.3e-09 at most, gradient 1.6e-09)"""
    E = edges(seed=21, n=60, noise=3.0, every=0)
    num, huber = numeric_blocks(E, True)
    assert 15 <= huber <= 45, huber
    hub = LR.huber(LR.TH2_MONO) + LR.huber(LR.TH2_STEREO)
    _, _, lin = LR.edge_linearise(inputs(E), hub, quats(E), E["t"], E["X"])
    compare("local_ba robust, Huber region", lin, num)
    P = pose_opt_terms(E)
    compare("pose_opt, Huber region", np.concatenate([P[:, :21], -P[:, 21:27]], 1), num[:, 9:36], {"Hpp": slice(0, 21), "bp": slice(21, 27)})


def test_the_draw_and_the_check():
    """half the edges stereo, three levels, errors of about a pixel; and the check sees a wrong entry: a flipped sign or two swapped
    entries of one block move the measure to order one"""
    E, num = cached(True)
    assert E["stereo"].sum() == N_EDGES // 2 and len(set(E["isg"].tolist())) == 3
    e = np.stack([error(rotation(E["q"][i]), E["t"][i], E["X"][i], E["obs"][i], True) for i in range(N_EDGES)])
    assert 0.4 < np.abs(e).mean() < 1.2
    for col, other in ((9 + 1, None), (36 + 4, None), (6, 7), (30, 33)):
        bad = num.copy()
        if other is None:
            bad[:, col] = -bad[:, col]
        else:
            bad[:, [col, other]] = bad[:, [other, col]]
        block = next(sl for sl in BLOCKS.values() if sl.start <= col < sl.stop)
        assert relative(bad[:, block], num[:, block]) > 0.1
