"""GPU: TwoViewReconstruction on the device (rfe_two_view / _dev) against the contract of DESIGN.md 6o restated in tests/two_view_ref.py.
Every comparison is exact (np.array_equal on R21, t21, p3d, triangulated, inliers_h, inliers_f, scores, models, cand and stats), in host
and device form; every capacity is padded and poisoned."""
import ctypes

import numpy as np
import pytest

import two_view_ref as R

pytestmark = pytest.mark.gpu
F32, I32 = np.float32, np.int32
OUT = R.OUT
OPTIONAL = ("p3d", "triangulated", "inliers_h", "inliers_f", "scores", "models", "cand")
SENT = {"p3d": F32(-7.5), "triangulated": 7, "inliers_h": 9, "inliers_f": 11, "scores": F32(-3.0), "cand": F32(-5.0)}


@pytest.fixture(scope="module")
def ctx():
    from rover_slam_amd import capi            # not at import time: collection must not load the library in front of the modules that load torch
    c = capi.Context(0)
    yield c
    c.close()


def batch(cases, pad=(3, 5, 2, 1)):
    """B cases stacked: case b keeps its n1 / n2 keypoints, its S matches and its `its` draws in front; what lies behind is padding: NaN
    keypoints, pair indices and draws far out of range"""
    B = len(cases)
    N1 = max([c["P"]["n1"] for c in cases] + [0]) + pad[0]
    N2 = max([c["P"]["n2"] for c in cases] + [0]) + pad[1]
    K = max([len(c["pairs"]) for c in cases] + [0]) + pad[2]
    its = [200 if c["P"]["its"] == 0 else c["P"]["its"] for c in cases]
    H = max(its + [1]) + pad[3]
    a = {"P": [dict(c["P"]) for c in cases], "kpts1": np.full((B, N1, 2), np.nan, F32), "kpts2": np.full((B, N2, 2), np.nan, F32),
         "S": np.zeros(B, I32), "pairs": np.full((B, K, 2), 1 << 30, I32), "draws": np.full((B, H, 8), -(1 << 30), I32)}
    for b, c in enumerate(cases):
        n1, n2, S = c["P"]["n1"], c["P"]["n2"], c["S"]
        a["kpts1"][b, :n1], a["kpts2"][b, :n2] = c["kpts1"][:n1], c["kpts2"][:n2]
        a["S"][b] = S
        a["pairs"][b, :len(c["pairs"])] = c["pairs"]
        if S < len(c["pairs"]):
            a["pairs"][b, max(S, 0):] = 1 << 30
        a["draws"][b, :its[b]] = c["draws"][:its[b]]
    return a


def shapes(a):
    B, N1 = a["kpts1"].shape[:2]
    K, H = a["pairs"].shape[1], a["draws"].shape[1]
    return B, N1, a["kpts2"].shape[1], K, H, {"R21": (B, 9), "t21": (B, 3), "p3d": (B, N1, 3), "triangulated": (B, N1), "inliers_h": (B, K),
                                              "inliers_f": (B, K), "scores": (B, H, 2), "models": (B, 2, 9), "cand": (B, 8, 16), "stats": (B, 16)}


def fills(a):
    sh = shapes(a)[-1]
    return {k: np.full(sh[k], SENT[k], OUT[k]) for k in SENT}


_REF = {}


def reference(a, key=None):
    """the restatement per problem, computed once per key"""
    if key is not None and key in _REF:
        return _REF[key]
    B, sh = shapes(a)[0], shapes(a)[-1]
    f = fills(a)
    rs = [R.two_view(a["P"][b], a["kpts1"][b], a["kpts2"][b], a["S"][b], a["pairs"][b], a["draws"][b], fill={k: f[k][b] for k in f}) for b in range(B)]
    ref = {k: np.stack([np.asarray(r[k], OUT[k]) for r in rs]) if B else np.zeros(sh[k], OUT[k]) for k in OUT}
    if key is not None:
        _REF[key] = ref
    return ref


def same(got, ref, keys=tuple(OUT)):
    for k in keys:
        assert got[k].dtype == ref[k].dtype == OUT[k] and got[k].shape == ref[k].shape, (k, got[k].dtype, got[k].shape, ref[k].shape)
        g, r = got[k], ref[k]
        eq = (g == r) | (np.isnan(g.astype(np.float64)) & np.isnan(r.astype(np.float64)))
        assert eq.all(), (k, np.argwhere(~eq)[:8].tolist(), g[~eq][:8], r[~eq][:8], got["stats"].tolist(), ref["stats"].tolist())


def host(ctx, a, outputs=OPTIONAL):
    f = fills(a)
    return ctx.two_view(a["P"], a["kpts1"], a["kpts2"], a["S"], a["pairs"], a["draws"], fill={k: v for k, v in f.items() if k in outputs},
                        outputs=outputs)


def dev_enqueue(ctx, a, outputs=OPTIONAL):
    """rfe_two_view_dev on uploaded copies, not waited for; returns finish(), which synchronises, downloads the host form's dict and frees"""
    B, N1, N2, K, H, sh = shapes(a)
    bufs = []

    def up(x, dt):
        x = np.ascontiguousarray(x, dt)
        bufs.append(ctx.alloc(max(x.nbytes, 4)))
        return bufs[-1].upload(x) if x.nbytes else bufs[-1]
    f = fills(a)
    init = {k: f[k] if k in f else np.full(sh[k], 55, OUT[k]) for k in OUT}
    out = {k: up(init[k], OUT[k]) for k in ("R21", "t21", "stats") + tuple(outputs)}
    ctx.two_view_dev(a["P"], up(a["kpts1"], F32), up(a["kpts2"], F32), up(a["S"], I32), up(a["pairs"], I32), up(a["draws"], I32), B, N1, N2, K, H,
                     out["R21"], out["t21"], out["stats"], **{k: out[k] for k in outputs})

    def finish():
        try:
            ctx.synchronize()
            return {k: out[k].download(sh[k], OUT[k]) if np.prod(sh[k]) else np.zeros(sh[k], OUT[k]) for k in out}
        finally:
            for b in bufs:
                b.free()
    return finish


def dev(ctx, a, outputs=OPTIONAL):
    return dev_enqueue(ctx, a, outputs)()


def both(ctx, a, key=None):
    ref = reference(a, key)
    h = host(ctx, a)
    same(h, ref)
    same(dev(ctx, a), ref)
    return h, ref


# ---------------------------------------------------------------- 1. sizes, one problem
@pytest.mark.parametrize("n", [8, 9, 63, 64, 65, 100, 257, 1024, 4096])
def test_match_counts(ctx, n):
    c = R.scene(300 + n, n, its=5, extra1=0 if n == 4096 else 17, extra2=0 if n == 4096 else 29)
    a = batch([c], pad=(0, 0, 0, 1) if n == 4096 else (3, 5, 2, 1))
    h, ref = both(ctx, a)
    st = ref["stats"][0]
    assert st[2] == n and st[12] == 0 and (h["inliers_f"][0, n:] == SENT["inliers_f"]).all() and (h["scores"][0, 5:] == SENT["scores"]).all()
    if n >= 63:
        assert st[6] >= int(0.85 * n)
    print(f"n={n}: stats {st[:8].tolist()} exit {st[11]}")


@pytest.mark.parametrize("its", [1, 3, 4, 5, 200, 1024])
def test_iteration_counts(ctx, its):
    c = R.scene(400 + its, 300, its=0 if its == 200 else its)
    h, ref = both(ctx, batch([c], pad=(3, 5, 2, 0 if its == 1024 else 2)))
    assert ref["stats"][0, 1] == 2 and ref["stats"][0, 4] >= 0 and (its < 200 or ref["stats"][0, 0] == 1)
    print(f"its={its}: stats {ref['stats'][0, :8].tolist()} exit {ref['stats'][0, 11]}")


def test_largest(ctx):
    c = R.scene(77, 4096, its=1024, extra1=0, extra2=0)
    both(ctx, batch([c], pad=(0, 0, 0, 0)))


def test_n1_differs_from_n2(ctx):
    c = R.scene(31, 100, its=5, extra1=50, extra2=3)
    h, ref = both(ctx, batch([c], pad=(40, 7, 9, 3)))
    assert c["P"]["n1"] == 150 and c["P"]["n2"] == 103 and (h["triangulated"][0, 150:] == SENT["triangulated"]).all()


# ---------------------------------------------------------------- 2. several problems
def test_batch_of_three(ctx):
    cases = [R.scene(41, 300, its=40), R.scene(42, 65, kind="plane", its=7, fx=420.0, fy=430.0, cx=300.0, cy=250.0),
             R.scene(43, 700, kind="low_parallax", its=25, sigma=1.5)]
    h, ref = both(ctx, batch(cases))
    assert ref["stats"][:, 2].tolist() == [300, 65, 700] and len({t.tobytes() for t in ref["models"]}) == 3
    assert h["ret"] == ref["stats"][0, 0]


def test_batch_of_sixteen(ctx):
    cases = [R.scene(500 + b, 40 + 9 * b, kind=("general", "plane", "rotation", "low_parallax")[b % 4], its=3 + b % 5) for b in range(16)]
    both(ctx, batch(cases))


def test_optional_outputs_null(ctx):
    a = batch([R.scene(64, 300, its=20), R.scene(65, 200, kind="plane", its=20)])
    ref = reference(a)
    for outputs in ((), ("scores",), ("p3d", "inliers_f"), ("triangulated", "inliers_h", "models", "cand")):
        keys = ("R21", "t21", "stats") + outputs
        same(host(ctx, a, outputs=outputs), ref, keys)
        same(dev(ctx, a, outputs=outputs), ref, keys)


def test_back_to_back_calls(ctx):
    a1 = batch([R.scene(71, 600, its=100), R.scene(72, 500, its=100)])
    a2 = batch([R.scene(73, 65, its=5)])
    r1, r2 = reference(a1), reference(a2)
    same(dev(ctx, a1), r1)                                                # sizes the workspace
    f1, f2 = dev_enqueue(ctx, a1, outputs=("p3d", "models")), dev_enqueue(ctx, a2)     # no wait in between
    g2, g1 = f2(), f1()
    same(g1, r1, ("R21", "t21", "stats", "p3d", "models"))
    same(g2, r2)
    same(dev(ctx, a2), r2)


# ---------------------------------------------------------------- 3. the forced paths of the CPU tests
@pytest.mark.parametrize("name", R.FORCED)
def test_forced_paths(ctx, name):
    c, want = R.forced(name)
    h, ref = both(ctx, batch([c]))
    st = ref["stats"][0]
    got = (st[0], st[1], st[11], st[12])
    assert all(w is None or w == g for w, g in zip(want, got)), (name, want, got)
    if name == "identical_sets":
        assert st[3] == 0 and st[4] == 0 and ref["scores"][0, 0, 1] == ref["scores"][0, 1, 1]
    if name == "nan_keypoint":
        assert np.isnan(h["scores"][0, :5]).all()


# ---------------------------------------------------------------- 4. the chain rfe_match_dev -> rfe_two_view_dev on one ctx
def test_chain_behind_the_matcher(ctx):
    from rover_slam_amd import capi, weights as Wt
    ctx.set_weights(capi.KIND_LIGHTGLUE, Wt.make_lightglue(seed=11))
    g = np.random.default_rng(5)
    M = N = 96
    Kcap, H = 96, 8
    k0 = np.stack([g.uniform(10, 630, M), g.uniform(10, 470, M)], 1).astype(F32)
    k1 = (k0 + g.normal(0, 2.0, k0.shape)).astype(F32)
    d0 = g.normal(size=(M, 256)).astype(F32)
    d0 /= np.linalg.norm(d0, axis=1, keepdims=True)
    d1 = (d0 + 0.05 * g.normal(size=d0.shape)).astype(F32)
    d1 /= np.linalg.norm(d1, axis=1, keepdims=True)
    norm = lambda k: ((k - np.array([320, 240], F32)) / F32(320)).astype(F32)   # noqa: E731
    bufs = []

    def up(x, dt):
        x = np.ascontiguousarray(x, dt)
        bufs.append(ctx.alloc(max(x.nbytes, 4)))
        return bufs[-1].upload(x)
    try:
        dS, dP, dms = up(np.zeros(1, I32), I32), up(np.full((Kcap, 2), -1, I32), I32), up(np.zeros(Kcap, F32), F32)
        rc = capi.lib.rfe_match_dev(ctx.h, capi._dev(up(norm(k0), F32)), capi._dev(up(norm(k1), F32)), capi._dev(up(d0, F32)), capi._dev(up(d1, F32)),
                                    capi._dev(up(np.array([M], I32), I32)), capi._dev(up(np.array([N], I32), I32)), 1, M, N, 0.0, capi._dev(dS),
                                    capi._dev(dP), capi._dev(dms))
        assert rc == 0, capi.lib.rfe_last_error(ctx.h)
        draws = g.integers(0, 2 ** 31, (1, H, 8)).astype(I32)
        P = [R.params(its=H, n1=M, n2=N)]
        out = {"R21": up(np.zeros(9, F32), F32), "t21": up(np.zeros(3, F32), F32), "stats": up(np.zeros(16, I32), I32),
               "scores": up(np.zeros((H, 2), F32), F32), "inliers_f": up(np.zeros(Kcap, np.uint8), np.uint8)}
        ctx.two_view_dev(P, up(k0, F32), up(k1, F32), dS, dP, up(draws, I32), 1, M, N, Kcap, H, out["R21"], out["t21"], out["stats"],
                         scores=out["scores"], inliers_f=out["inliers_f"])
        ctx.synchronize()
        S, pairs = dS.download((1,), I32), dP.download((1, Kcap, 2), I32)
        got = {"R21": out["R21"].download((1, 9), F32), "t21": out["t21"].download((1, 3), F32), "stats": out["stats"].download((1, 16), I32),
               "scores": out["scores"].download((1, H, 2), F32), "inliers_f": out["inliers_f"].download((1, Kcap), np.uint8)}
    finally:
        for b in bufs:
            b.free()
    assert S[0] >= 8, S
    h = ctx.two_view(P, k0[None], k1[None], S, pairs, draws, outputs=("scores", "inliers_f"))
    same(got, h, ("R21", "t21", "stats", "scores", "inliers_f"))
    ref = R.two_view(P[0], k0, k1, S[0], pairs[0], draws[0])
    assert np.array_equal(h["stats"][0], ref["stats"]) and np.array_equal(h["scores"][0], ref["scores"], equal_nan=True)


# ---------------------------------------------------------------- 5. the gates through the hooks
def _at_threshold(th, sigmas=(1.0,)):
    """(du, dv, sigma) whose chi2 = fl(fl(du du + dv dv) invSigma2) is exactly th, and one whose chi2 is its upper neighbour"""
    th = F32(th)
    up = np.nextafter(th, F32(np.inf))
    found = {}
    for sigma in sigmas:
        inv = F32(1) / (F32(sigma) * F32(sigma))
        dv = (np.arange(0, 2048, dtype=F32) * F32(2.0 ** -11))[:, None]
        with np.errstate(all="ignore"):
            base = np.sqrt(np.maximum(th / inv - dv * dv, 0)).astype(F32)
        for k in range(-6, 7):
            du = base
            for _ in range(abs(k)):
                du = np.nextafter(du, F32(np.inf) if k > 0 else F32(0))
            chi = (du * du + dv * dv) * inv
            for want, name in ((th, "at"), (up, "above")):
                hit = np.argwhere(chi == want)
                if len(hit) and name not in found:
                    i = hit[0][0]
                    found[name] = (F32(du[i, 0]), F32(dv[i, 0]), float(sigma))
    assert set(found) == {"at", "above"}
    return found


@pytest.mark.parametrize("direction", [1, 2])
def test_homography_bound(ctx, direction):
    # H = diag(2, 2, 1): the error in image 2 is 4 times the one in image 1; H = diag(1/2, 1/2, 1) the other way round.  Both inverses are exact
    f = _at_threshold(5.991)
    for name, (du, dv, sigma) in f.items():
        if direction == 2:
            M, pts = [2, 0, 0, 0, 2, 0, 0, 0, 1], [[0, 0, du, dv]]
        else:
            M, pts = [0.5, 0, 0, 0, 0.5, 0, 0, 0, 1], [[du, dv, 0, 0]]
        contrib, inl = ctx.k_two_view_check(0, M, pts, sigma)
        rc, ri = R.check(0, M, pts, sigma)
        assert np.array_equal(contrib, rc) and np.array_equal(inl, ri) and ri[0] == (name == "at"), (name, contrib, rc, inl, ri)


@pytest.mark.parametrize("direction", [1, 2])
def test_fundamental_bound(ctx, direction):
    # lines v2 = 2 v1: the distance in one image is twice the one in the other
    f = _at_threshold(3.841, sigmas=(1.0, 1.25, 1.5, 0.75))
    for name, (du, dv, sigma) in f.items():
        if dv != 0:                                                       # one dimension only: the point-line distance
            g = _at_threshold_1d(3.841, name)
            du, sigma = g
        if direction == 1:
            M, pts = [0, 0, 0, 0, 0, -1, 0, 2, 0], [[0, 0, 0, du]]         # image 2: (2 v1 - v2)^2 / 1; image 1: a quarter of it
        else:
            M, pts = [0, 0, 0, 0, 0, -2, 0, 1, 0], [[0, du, 0, 0]]
        contrib, inl = ctx.k_two_view_check(1, M, pts, sigma)
        rc, ri = R.check(1, M, pts, sigma)
        assert np.array_equal(contrib, rc) and np.array_equal(inl, ri) and ri[0] == (name == "at"), (name, contrib, rc, inl, ri)


def _at_threshold_1d(th, name):
    th = F32(th)
    want = th if name == "at" else np.nextafter(th, F32(np.inf))
    for sigma in np.arange(0.5, 2.0, 1.0 / 64):
        inv = F32(1) / (F32(sigma) * F32(sigma))
        e = np.sqrt(th / inv).astype(F32)
        cand = [e]
        for _ in range(8):
            cand.append(np.nextafter(cand[-1], F32(np.inf)))
        lo = e
        for _ in range(8):
            lo = np.nextafter(lo, F32(0))
            cand.append(lo)
        for d in cand:
            if ((d * d) / F32(1)) * inv == want:
                return F32(d), float(sigma)
    raise AssertionError("no exactly representable distance found")


def test_check_rt_gates(ctx):
    K4 = (500.0, 500.0, 320.0, 240.0)
    Rm, t = np.eye(3, dtype=F32), np.array([1, 0, 0], F32)               # camera 2 one unit to the left: x2 = x1 + t
    g = np.random.default_rng(3)
    X = np.stack([g.uniform(-2, 2, 64), g.uniform(-1.5, 1.5, 64), g.uniform(4, 9, 64)], 1)
    proj = lambda Y: np.stack([500 * Y[:, 0] / Y[:, 2] + 320, 500 * Y[:, 1] / Y[:, 2] + 240], 1)   # noqa: E731
    pts = np.concatenate([proj(X), proj(X + t) + g.normal(0, 0.3, (64, 2))], 1).astype(F32)
    far = np.stack([np.zeros(4000), np.zeros(4000), np.linspace(150, 170, 4000)], 1)               # cosParallax around 0.99998
    pts = np.concatenate([pts, np.concatenate([proj(far), proj(far + t)], 1).astype(F32)])
    behind = np.array([[320 + 50, 240, 320 - 60, 240],                    # rays that meet behind both cameras
                       [320, 240, 320, 240]], F32)                        # P2 row == P1 row at the principal point: see below
    pts = np.concatenate([pts, behind])
    code, cosp, p3d = ctx.k_two_view_check_rt(Rm, t, K4, 4.0, pts)
    rc, rcos, rp = R.check_rt(Rm.reshape(1, 9), t.reshape(1, 3), *K4, 4.0, pts[:, 0], pts[:, 1], pts[:, 2], pts[:, 3])
    assert np.array_equal(code, rc[0]) and np.array_equal(cosp, rcos[0], equal_nan=True) and np.array_equal(p3d, rp[0], equal_nan=True)
    assert (rc[0, :64] == 2).sum() > 40 and rc[0, -2] == 0 and rp[0, -2, 2] < 0
    # behind camera 2 alone: a second camera that looks back at the first; the points lie in front of camera 1 and behind camera 2
    Rb, tb = np.array([-1, 0, 0, 0, 1, 0, 0, 0, -1], F32), np.array([0.5, 0, 3.0], F32)
    Xb = X[:16] @ Rb.reshape(3, 3).astype(np.float64).T + tb
    ptsb = np.concatenate([proj(X[:16]), proj(Xb)], 1).astype(F32)
    code, cosp, p3d = ctx.k_two_view_check_rt(Rb, tb, K4, 4.0, ptsb)
    bc, bcos, bp = R.check_rt(Rb.reshape(1, 9), tb.reshape(1, 3), *K4, 4.0, *(ptsb[:, j] for j in range(4)))
    assert np.array_equal(code, bc[0]) and np.array_equal(cosp, bcos[0]) and np.array_equal(p3d, bp[0])
    assert (Xb[:, 2] < 0).all() and (bp[0, :, 2] > 0).all() and not bc.any() and (bcos[0] < R.COS_99998).all()
    # either side of the 0.99998 constant: both neighbours occur among the far points, counted with and without vbGood
    fc, fk = rcos[0, 64:4064], rc[0, 64:4064]
    lo = F32(0.99998)
    assert (fc == lo).any() and (fc == R.COS_99998).any() and (fk[fc == lo] == 2).all() and (fk[fc == R.COS_99998] == 1).all()
    # one ulp either side of th2: the bound set to a point's own squared error in image 2, and to the float below it
    e2 = _square_error_2(Rm, t, K4, pts[:64], rp[0, :64])
    e1 = _square_error_2(np.eye(3, dtype=F32), np.zeros(3, F32), K4, pts[:64, [2, 3, 0, 1]], rp[0, :64])      # image 1: R = I, t = 0, against (u1, v1)
    k = int(np.argmax(e2 * ((rc[0, :64] == 2) & (e1 < e2))))             # the gate of image 1 must stay open under the smaller bound
    for th2, want in ((e2[k], 2), (np.nextafter(e2[k], F32(0)), 0)):
        code, _, _ = ctx.k_two_view_check_rt(Rm, t, K4, th2, pts[k:k + 1])
        assert code[0] == want == R.check_rt(Rm.reshape(1, 9), t.reshape(1, 3), *K4, th2, *(pts[k:k + 1, j] for j in range(4)))[0][0, 0]
    # a zero fourth component: with P2 = P1 and both keypoints at the principal point the system has two zero columns, no pair is rotated
    # and the first minimum is the third column: h = (0, 0, 1, 0)
    code, cosp, p3d = ctx.k_two_view_check_rt(Rm, np.zeros(3, F32), K4, 4.0, behind[1:])
    assert code[0] == 0 and cosp[0] == 0 and not p3d.any()
    assert R.check_rt(Rm.reshape(1, 9), np.zeros((1, 3), F32), *K4, 4.0, *(behind[1:, j] for j in range(4)))[0][0, 0] == 0


def _square_error_2(Rm, t, K4, pts, p):
    """squareError2 of CheckRT, as the restatement forms it"""
    fx, fy, cx, cy = (F32(v) for v in K4)
    Rm = Rm.reshape(-1)
    x2 = ((Rm[0] * p[:, 0] + Rm[1] * p[:, 1]) + Rm[2] * p[:, 2]) + t[0]
    y2 = ((Rm[3] * p[:, 0] + Rm[4] * p[:, 1]) + Rm[5] * p[:, 2]) + t[1]
    z2 = ((Rm[6] * p[:, 0] + Rm[7] * p[:, 1]) + Rm[8] * p[:, 2]) + t[2]
    iz = F32(1) / z2
    ex, ey = ((fx * x2) * iz + cx) - pts[:, 2], ((fy * y2) * iz + cy) - pts[:, 3]
    return (ex * ex + ey * ey).astype(F32)


# ---------------------------------------------------------------- 6. refusals
def test_refusals(ctx):
    from rover_slam_amd import capi
    c = R.scene(81, 20, its=6, extra1=2, extra2=3)
    a = batch([c], pad=(0, 0, 0, 2))
    B, N1, N2, K, H, sh = shapes(a)

    def refused(null=(), form="both", params=None, **over):
        P = capi.two_view_params(a["P"] if params is None else params)
        o = {k: np.zeros(sh[k], OUT[k]) for k in ("R21", "t21", "p3d", "triangulated", "inliers_h", "inliers_f", "scores", "models", "cand", "stats")}
        args = {"params": ctypes.addressof(P), "kpts1": a["kpts1"].ctypes.data, "kpts2": a["kpts2"].ctypes.data, "S": a["S"].ctypes.data,
                "pairs": a["pairs"].ctypes.data, "draws": a["draws"].ctypes.data, "B": B, "N1max": N1, "N2max": N2, "Kmax": K, "H": H}
        args.update({k: v.ctypes.data for k, v in o.items()})
        args.update(over)
        for k in null:
            args[k] = None
        # the _dev form checks its arguments before it touches a pointer, so host addresses do for the refusals
        fns = {"both": (capi.lib.rfe_two_view, capi.lib.rfe_two_view_dev), "host": (capi.lib.rfe_two_view,)}[form]
        for fn in fns:
            assert fn(ctx.h, *args.values()) == -1 and b"two_view" in capi.lib.rfe_last_error(ctx.h)     # RFE_ERR_INVALID
        return True

    assert refused(B=-1) and refused(B=17, params=a["P"] * 17) and refused(H=0) and refused(H=1025)
    for k in ("N1max", "N2max", "Kmax"):
        assert refused(**{k: -1}) and refused(**{k: 4097})
    for field, v in (("its", -1), ("its", H + 1), ("n1", -1), ("n1", N1 + 1), ("n2", -1), ("n2", N2 + 1), ("min_triangulated", -1)):
        assert refused(params=[dict(a["P"][0], **{field: v})])
    assert refused(params=[dict(a["P"][0], its=0)])                       # 200 > H
    for k in ("params", "draws", "S", "R21", "t21", "stats", "kpts1", "kpts2", "pairs"):
        assert refused(null=(k,))
    for field in ("fx", "fy", "cx", "cy", "sigma"):
        for bad in (np.nan, np.inf):
            assert refused(params=[dict(a["P"][0], **{field: bad})], form="host")
    both(ctx, a)                                                          # and the context still works
