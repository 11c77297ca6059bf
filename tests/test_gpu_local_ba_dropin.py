"""GPU: the drop-in of include/rfe/local_ba.h (LocalBundleAdjustment_rfe) over mock KeyFrame / MapPoint / Map classes
(tests/cpp/local_ba_driver.cpp) against the restatement tests/local_ba_ref.py: the poses and positions written back, the erased
observations, the four counters, the early returns and "not served"."""
import shutil

import numpy as np
import pytest

import dropin_driver as DD
import local_ba_ref as R

pytestmark = pytest.mark.gpu
F32 = np.float32
NO_FIXED, STOPPED, NOT_SERVED = -10, -11, -12


def write_case(path, c, init_id=0, inertial=False, stop=False, camera2=-1, fisheye=-1, bad_points=(), order_seed=1, levels=None):
    """the scene as a map: keyframes 0 .. P-1 are the current keyframe (0) and its covisibles, the others see local points without being
    local.  levels: {keyframe: n} hands that keyframe an mvInvLevelSigma2 of n ones.  mnIds ascend with the scene's indices, so the sorted order the drop-in builds is the scene's; the covisibles and every
    keyframe's features are handed over shuffled, so that it has to sort."""
    rng = np.random.default_rng(order_seed)
    P, K, L = c["P"], c["P"] + c["F"], len(c["xw"])
    off = c["kf_feat_off"]
    with open(path, "wb") as f:
        cov = rng.permutation(np.arange(1, P)).astype(np.int32)
        np.array([K, L, 0, init_id, int(inertial), int(stop), camera2, fisheye, len(cov)], np.int32).tofile(f)
        cov.tofile(f)
        slot = {}                                  # (keyframe, scene feature) -> index in the keyframe's shuffled arrays
        for k in range(K):
            n = int(off[k + 1] - off[k])
            perm = rng.permutation(n)
            rows = off[k] + perm
            nl = int(c["kf_nlevels"][k]) if not levels or k not in levels else levels[k]
            np.array([10 + 2 * k, 0, n, nl], np.int32).tofile(f)
            np.asarray(c["kf_pose"][k], F32).tofile(f)
            np.asarray(c["kf_cam"][k], F32).tofile(f)
            (np.asarray(c["kf_sigma2"][k][:nl], F32) if not levels or k not in levels else np.ones(nl, F32)).tofile(f)
            np.asarray(c["kpts"][rows], F32).tofile(f)
            np.asarray(c["octave"][rows], np.int32).tofile(f)
            np.asarray(c["uright"][rows], F32).tofile(f)
            mp_of = np.full(n, -1, np.int32)
            for e in np.nonzero(c["edge_kf"] == k)[0]:
                j = int(np.nonzero(perm == c["edge_feat"][e])[0][0])
                mp_of[j] = c["edge_point"][e]
                slot[(k, int(c["edge_point"][e]))] = j
            mp_of.tofile(f)
        for p in range(L):
            es = np.nonzero(c["edge_point"] == p)[0]
            np.array([1000 + 3 * p, int(p in bad_points), len(es)], np.int32).tofile(f)
            np.asarray(c["xw"][p], F32).tofile(f)
            for e in es:
                np.array([c["edge_kf"][e], slot[(int(c["edge_kf"][e]), p)]], np.int32).tofile(f)


def read_out(path, K, L):
    raw = np.fromfile(path, np.uint8)
    head = raw[:28].view(np.int32)
    o = {"ret": int(head[0]), "counters": [int(v) for v in head[1:5]], "change_index": int(head[5]), "stats": raw[28:60].view(np.int32)}
    n_er = int(head[6])
    at = 60
    kf = raw[at:at + K * 32].view(np.int32).reshape(K, 8)
    o["set_pose_calls"], o["pose"] = kf[:, 0].copy(), kf[:, 1:].copy().view(F32)
    at += K * 32
    mp = raw[at:at + L * 20].view(np.int32).reshape(L, 5)
    o["set_pos_calls"], o["update_calls"], o["point"] = mp[:, 0].copy(), mp[:, 1].copy(), mp[:, 2:].copy().view(F32)
    at += L * 20
    o["erased"] = raw[at:at + n_er * 8].view(np.int32).reshape(n_er, 2)
    assert len(raw) == at + n_er * 8
    return o


def run(exe, tmp_path, c, **kw):
    write_case(str(tmp_path / "case.bin"), c, **kw)
    DD.run(exe, str(tmp_path / "case.bin"), str(tmp_path / "out.bin"))
    return read_out(str(tmp_path / "out.bin"), c["P"] + c["F"], len(c["xw"]))


def untouched(got, c):
    return (got["set_pose_calls"] == 0).all() and (got["set_pos_calls"] == 0).all() and np.array_equal(got["pose"], c["kf_pose"]) and \
        np.array_equal(got["point"], c["xw"]) and len(got["erased"]) == 0 and got["change_index"] == 0


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_drop_in(tmp_path):
    exe = DD.build(tmp_path, "local_ba_driver")
    c = R.scene(70, 4, 3, 120, "mixed", obs=5, gross=0.1, gross_px=(10.0, 20.0))
    P, K, L, E = c["P"], 7, 120, len(c["edge_point"])
    ref = R.local_ba(c, R.params(max_trials=10))
    got = run(exe, tmp_path, c)
    assert got["ret"] == ref["ret"] > 0 and np.array_equal(got["stats"], ref["stats"])
    assert got["counters"] == [c["F"], P, L, E] and got["change_index"] == 1
    assert np.array_equal(got["pose"][:P], ref["pose_f32"]) and (got["set_pose_calls"][:P] == 1).all()
    assert np.array_equal(got["pose"][P:], c["kf_pose"][P:]) and (got["set_pose_calls"][P:] == 0).all()
    assert np.array_equal(got["point"], ref["point_f32"]) and (got["set_pos_calls"] == 1).all() and (got["update_calls"] == 1).all()
    want = sorted((int(c["edge_kf"][e]), int(c["edge_point"][e])) for e in np.nonzero(ref["erase"])[0])
    assert sorted(map(tuple, got["erased"].tolist())) == want
    # an inertial map starts at lambda 100
    ref_in = R.local_ba(c, R.params(max_trials=10, user_lambda_init=100.0))
    got = run(exe, tmp_path, c, inertial=True)
    assert np.array_equal(got["stats"], ref_in["stats"]) and np.array_equal(got["point"], ref_in["point_f32"])
    assert not np.array_equal(ref_in["trace"], ref["trace"])
    # a bad point is no local point at all (:1779): the problem is the scene without it
    bad = int(c["edge_point"][np.nonzero(ref["erase"])[0][0]])
    got = run(exe, tmp_path, c, bad_points=(bad,))
    keep = c["edge_point"] != bad
    assert not any(p == bad for _, p in got["erased"].tolist()) and got["set_pos_calls"][bad] == 0 and got["counters"][2] == L - 1
    assert got["counters"][3] == int(keep.sum())
    # the init keyframe among the local ones is fixed: one more fixed keyframe, and its pose stays
    got = run(exe, tmp_path, c, init_id=10 + 2 * 1)
    c_init = init_fixed(c, 1)
    ref_i = R.local_ba(c_init, R.params(max_trials=10))
    assert got["counters"][:2] == [c["F"] + 1, P] and got["set_pose_calls"][1] == 0 and np.array_equal(got["pose"][1], c["kf_pose"][1])
    assert np.array_equal(got["stats"], ref_i["stats"]) and np.array_equal(got["pose"][[0, 2, 3]], ref_i["pose_f32"])
    assert np.array_equal(got["point"], ref_i["point_f32"])
    # the early returns: no fixed keyframe; the stop flag set
    c0 = R.scene(71, 3, 0, 30, "mixed")
    got = run(exe, tmp_path, c0)
    assert got["ret"] == NO_FIXED and got["counters"][0] == 0 and untouched(got, c0)
    got = run(exe, tmp_path, c, stop=True)
    assert got["ret"] == STOPPED and got["counters"] == [c["F"], P, L, E] and untouched(got, c)
    # not served: a second camera, a fisheye camera, a level table that is empty or longer than RFE_MAX_LEVELS
    for kw in ({"camera2": 2}, {"fisheye": 5}, {"levels": {1: 0}}, {"levels": {4: 17}}):
        got = run(exe, tmp_path, c, **kw)
        assert got["ret"] == NOT_SERVED and untouched(got, c) and (got["stats"] == 0).all()
    # not served: over the caps -- 65 free keyframes; 257 keyframes
    for Pn, Fn in ((65, 1), (3, 254)):
        big = R.scene(72, Pn, Fn, 4, "mixed", all_see=True)         # every keyframe sees every point
        got = run(exe, tmp_path, big)
        assert got["ret"] == NOT_SERVED and got["counters"][:2] == [Fn, Pn] and untouched(got, big) and (got["stats"] == 0).all()


def init_fixed(c, k):
    """the scene with free keyframe k moved behind the free ones (the fixed group is sorted by mnId, and k's is the smallest there)"""
    P, K = c["P"], c["P"] + c["F"]
    order = [i for i in range(P) if i != k] + [k] + list(range(P, K))
    new_of = {old: new for new, old in enumerate(order)}
    d = dict(c, P=P - 1, F=c["F"] + 1)
    for n in ("kf_pose", "kf_cam", "kf_nlevels", "kf_sigma2"):
        d[n] = np.asarray(c[n])[order]
    ek = np.array([new_of[int(v)] for v in c["edge_kf"]], np.int64)
    idx = np.lexsort((ek, c["edge_point"]))
    ep, ek = c["edge_point"][idx], ek[idx]
    # features: per keyframe in edge order
    cnt = np.bincount(ek, minlength=K)
    off = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int32)
    nxt = off[:-1].copy()
    ef = np.zeros(len(ep), np.int32)
    rows = np.zeros(len(ep), np.int64)
    old_f = (c["kf_feat_off"][c["edge_kf"]] + c["edge_feat"])[idx]
    for e in range(len(ep)):
        ef[e] = nxt[ek[e]] - off[ek[e]]
        rows[nxt[ek[e]]] = old_f[e]
        nxt[ek[e]] += 1
    d.update(edge_point=ep.astype(np.int32), edge_kf=ek.astype(np.int32), edge_feat=ef, kf_feat_off=off, kpts=c["kpts"][rows], octave=c["octave"][rows],
             uright=c["uright"][rows], planted=c["planted"][idx])
    return d
