"""GPU: the drop-ins of include/rfe/global_ba.h (GlobalBundleAdjustemnt_rfe, BundleAdjustment_rfe) over mock KeyFrame / MapPoint / Map
classes (tests/cpp/global_ba_driver.cpp) against the restatement tests/global_ba_ref.py: both write-back modes, bad keyframes and points,
a late keyframe past maxKFid, an edge-less point and "not served"."""
import shutil

import numpy as np
import pytest

import dropin_driver as DD
import global_ba_ref as G

pytestmark = pytest.mark.gpu
F32 = np.float32
NOT_SERVED = -12
KF_ID, MP_ID = (lambda k: 10 + 2 * k), (lambda p: 1000 + 3 * p)


def write_case(path, c, loop_kf, origin=0, robust=False, iterations=10, camera2=-1, fisheye=-1, through_map=True, bad_kf=(), late_kf=(), bad_points=(),
               order_seed=1, levels=None):
    """the scene as a map.  mnIds ascend with the scene's indices, so the sorted order the drop-in builds is the scene's; every keyframe's
    features are handed over shuffled, so that it has to gather.  The init keyframe is the first fixed one of the scene"""
    rng = np.random.default_rng(order_seed)
    K, L = len(c["fixed"]), len(c["xw"])
    off = c["kf_feat_off"]
    fixed = np.nonzero(c["fixed"])[0]
    init_id = KF_ID(int(fixed[0])) if len(fixed) else 5          # 5: nobody's mnId
    with open(path, "wb") as f:
        np.array([K, L, init_id, KF_ID(origin), loop_kf, int(robust), iterations, camera2, fisheye, int(through_map)], np.int32).tofile(f)
        slot = {}
        for k in range(K):
            n = int(off[k + 1] - off[k])
            perm = rng.permutation(n)
            rows = off[k] + perm
            nl = int(c["kf_nlevels"][k]) if not levels or k not in levels else levels[k]
            np.array([KF_ID(k), 1 if k in bad_kf else 2 if k in late_kf else 0, n, nl], np.int32).tofile(f)
            np.asarray(c["kf_pose"][k], F32).tofile(f)
            np.asarray(c["kf_cam"][k], F32).tofile(f)
            (np.asarray(c["kf_sigma2"][k][:nl], F32) if not levels or k not in levels else np.ones(nl, F32)).tofile(f)
            np.asarray(c["kpts"][rows], F32).tofile(f)
            np.asarray(c["octave"][rows], np.int32).tofile(f)
            np.asarray(c["uright"][rows], F32).tofile(f)
            for e in np.nonzero(c["edge_kf"] == k)[0]:
                slot[(k, int(c["edge_point"][e]))] = int(np.nonzero(perm == c["edge_feat"][e])[0][0])
        for p in range(L):
            es = np.nonzero(c["edge_point"] == p)[0]
            np.array([MP_ID(p), int(p in bad_points), len(es)], np.int32).tofile(f)
            np.asarray(c["xw"][p], F32).tofile(f)
            for e in es:
                np.array([c["edge_kf"][e], slot[(int(c["edge_kf"][e]), p)]], np.int32).tofile(f)


def read_out(path, K, L):
    raw = np.fromfile(path, np.uint8)
    o = {"ret": int(raw[:4].view(np.int32)[0]), "stats": raw[4:36].view(np.int32)}
    at = 36
    kf = raw[at:at + K * 64].view(np.int32).reshape(K, 16)
    o["set_pose_calls"], o["kf_mark"], o["pose"], o["pose_gba"] = kf[:, 0].copy(), kf[:, 1].copy(), kf[:, 2:9].copy().view(F32), kf[:, 9:].copy().view(F32)
    at += K * 64
    mp = raw[at:at + L * 36].view(np.int32).reshape(L, 9)
    o["set_pos_calls"], o["update_calls"], o["mp_mark"] = mp[:, 0].copy(), mp[:, 1].copy(), mp[:, 2].copy()
    o["point"], o["point_gba"] = mp[:, 3:6].copy().view(F32), mp[:, 6:].copy().view(F32)
    assert len(raw) == at + L * 36
    return o


def run(exe, tmp_path, c, loop_kf, **kw):
    write_case(str(tmp_path / "case.bin"), c, loop_kf, **kw)
    DD.run(exe, str(tmp_path / "case.bin"), str(tmp_path / "out.bin"))
    return read_out(str(tmp_path / "out.bin"), len(c["fixed"]), len(c["xw"]))


def untouched(got, c):
    return (got["set_pose_calls"] == 0).all() and (got["set_pos_calls"] == 0).all() and (got["kf_mark"] == -1).all() and \
        (got["mp_mark"] == -1).all() and np.array_equal(got["pose"], c["kf_pose"]) and np.array_equal(got["point"], c["xw"])


def subcase(c, kfs, pts):
    """the scene restricted to the keyframes and points listed (ascending), packed as the drop-in packs it: every keyframe's features
    are the ones its edges observe, in edge order"""
    kfs, pts = np.asarray(kfs, np.int64), np.asarray(pts, np.int64)
    K = len(c["fixed"])
    new_kf, new_pt = np.full(K, -1, np.int64), np.full(len(c["xw"]), -1, np.int64)
    new_kf[kfs], new_pt[pts] = np.arange(len(kfs)), np.arange(len(pts))
    keep = (new_kf[c["edge_kf"]] >= 0) & (new_pt[c["edge_point"]] >= 0)
    ep, ek = new_pt[c["edge_point"][keep]], new_kf[c["edge_kf"][keep]]
    old_f = (np.asarray(c["kf_feat_off"], np.int64)[c["edge_kf"]] + c["edge_feat"])[keep]
    cnt = np.bincount(ek, minlength=len(kfs))
    off = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int32)
    order = np.argsort(ek, kind="stable")
    ef = np.zeros(len(ep), np.int64)
    ef[order] = np.arange(len(ep)) - off[ek[order]]
    rows = np.zeros(len(ep), np.int64)
    rows[off[ek] + ef] = old_f
    d = dict(c)
    for n in ("fixed", "kf_pose", "kf_cam", "kf_nlevels", "kf_sigma2"):
        d[n] = np.asarray(c[n])[kfs]
    d.update(xw=c["xw"][pts], edge_point=ep.astype(np.int32), edge_kf=ek.astype(np.int32), edge_feat=ef.astype(np.int32), kf_feat_off=off,
             kpts=c["kpts"][rows], octave=c["octave"][rows], uright=c["uright"][rows])
    return d


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_drop_in(tmp_path):
    exe = DD.build(tmp_path, "global_ba_driver")
    K = 9
    c = G.scene(70, K, [0], G.pattern("loop", K, ppk=5), "mixed", ring=True, edgeless=(4,))
    L = len(c["xw"])
    allk, allp = np.arange(K), np.arange(L)
    # behind a loop: nLoopKF is not the origin keyframe; mTcwGBA, mPosGBA and the marks, no SetPose
    ref = G.global_ba(c, G.params(iterations=10, max_trials=10, robust=False))
    got = run(exe, tmp_path, c, loop_kf=KF_ID(6))
    assert got["ret"] == ref["ret"] > 0 and np.array_equal(got["stats"], ref["stats"])
    assert np.array_equal(got["pose_gba"], ref["pose_f32"]) and (got["kf_mark"] == KF_ID(6)).all() and (got["set_pose_calls"] == 0).all()
    assert np.array_equal(got["pose"], c["kf_pose"]) and np.array_equal(got["point"], c["xw"]) and (got["set_pos_calls"] == 0).all()
    inc = ref["included"] == 1
    assert not inc[4] and inc.sum() == L - 1                  # the edge-less point is left alone
    assert np.array_equal(got["point_gba"][inc], ref["point_f32"][inc]) and (got["mp_mark"][inc] == KF_ID(6)).all() and got["mp_mark"][4] == -1
    assert not got["point_gba"][4].any()
    # the monocular initialisation: nLoopKF is the origin keyframe, robust, 20 iterations, through the vectors; SetPose and SetWorldPos
    ref_r = G.global_ba(c, G.params(iterations=20, max_trials=10, robust=True))
    got = run(exe, tmp_path, c, loop_kf=KF_ID(0), robust=True, iterations=20, through_map=False)
    assert got["ret"] == ref_r["ret"] and np.array_equal(got["stats"], ref_r["stats"])
    assert np.array_equal(got["pose"], ref_r["pose_f32"]) and (got["set_pose_calls"] == 1).all() and (got["kf_mark"] == -1).all()
    assert np.array_equal(got["point"][inc], ref_r["point_f32"][inc]) and (got["set_pos_calls"][inc] == 1).all() and (got["update_calls"][inc] == 1).all()
    assert got["set_pos_calls"][4] == 0 and np.array_equal(got["point"][4], c["xw"][4]) and (got["mp_mark"] == -1).all()
    assert not np.array_equal(ref_r["pose_f32"], ref["pose_f32"])
    # a bad keyframe and two bad points are no vertices: the problem is the scene without them, and they are not written
    kk, pp = np.delete(allk, 3), np.delete(allp, [2, 7])
    sub = subcase(c, kk, pp)
    ref_s = G.global_ba(sub, G.params(iterations=10, max_trials=10))
    got = run(exe, tmp_path, c, loop_kf=KF_ID(6), bad_kf=(3,), bad_points=(2, 7))
    assert np.array_equal(got["stats"], ref_s["stats"]) and np.array_equal(got["pose_gba"][kk], ref_s["pose_f32"])
    assert got["kf_mark"][3] == -1 and (got["mp_mark"][[2, 7]] == -1).all()
    inc_s = ref_s["included"] == 1
    assert np.array_equal(got["point_gba"][pp][inc_s], ref_s["point_f32"][inc_s])
    # a late keyframe: the last one is not in the vectors, so its mnId lies past maxKFid and its observations are skipped
    kk = allk[:-1]
    sub = subcase(c, kk, allp)
    ref_l = G.global_ba(sub, G.params(iterations=10, max_trials=10))
    got = run(exe, tmp_path, c, loop_kf=KF_ID(6), late_kf=(K - 1,))
    assert np.array_equal(got["stats"], ref_l["stats"]) and np.array_equal(got["pose_gba"][kk], ref_l["pose_f32"]) and got["kf_mark"][K - 1] == -1
    inc_l = ref_l["included"] == 1
    assert np.array_equal(got["point_gba"][inc_l], ref_l["point_f32"][inc_l]) and ref_l["stats"][5] == K - 2
    # not served: a second camera, a fisheye camera, a level table that is empty or longer than RFE_MAX_LEVELS
    for kw in ({"camera2": 2}, {"fisheye": 5}, {"levels": {1: 0}}, {"levels": {4: 17}}):
        got = run(exe, tmp_path, c, loop_kf=KF_ID(6), **kw)
        assert got["ret"] == NOT_SERVED and untouched(got, c) and (got["stats"] == 0).all()
    # not served: over the keyframe cap
    big = G.scene(72, G.MAX_KF + 1, [0], [[0, 1]] * 2, "mono")
    got = run(exe, tmp_path, big, loop_kf=KF_ID(6))
    assert got["ret"] == NOT_SERVED and untouched(got, big) and (got["stats"] == 0).all()
