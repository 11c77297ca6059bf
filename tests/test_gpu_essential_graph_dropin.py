"""GPU: the drop-in of include/rfe/essential_graph.h (OptimizeEssentialGraph_rfe) over mock KeyFrame / MapPoint / Map / Sim3 classes
(tests/cpp/essential_graph_driver.cpp) against the restatement tests/essential_graph_ref.py fed with the tables and the edge list that
steps 2-4 of the reference build from the same map: the poses and positions written back, the calls made under the map's mutex, the
change index, a bad keyframe, and the not-served cases."""
import shutil

import numpy as np
import pytest

import dropin_driver as DD
import essential_graph_ref as R

pytestmark = pytest.mark.gpu
F32, F64 = np.float32, np.float64
NOT_SERVED = -12


def mnid(k):
    return 10 + 2 * k


def make_map(seed=90, N=14, bad=(5,), imu=None):
    """a map as plain lists: keyframe k has parent k - 1, covisibles k - 1 (200), k - 2 (150), k - 3 (50), k + 1 (200, its child); keyframe
    9 and keyframe 2 hold a loop edge; the last three keyframes are corrected; the current keyframe N - 1 is connected to the loop keyframe
    0 (weight 10: kept, it is the pair itself) and to 1 (weight 30: dropped), keyframe N - 2 to 0 (weight 120: kept)"""
    g = R.graph(seed, N, corrected=3, drift=0.01)
    rng = np.random.default_rng(seed)
    m = {"N": N, "cur": N - 1, "loop": 0, "init": mnid(0), "pose": g["s_meas"][:, :7].astype(F32), "bad": set(bad), "imu": imu,
         "parent": [-1] + list(range(N - 1)), "children": [[k + 1] if k + 1 < N else [] for k in range(N)],
         "loop_edges": [[] for _ in range(N)], "covis": [[] for _ in range(N)], "corrected": {}, "non_corrected": {}, "connections": {}}
    m["loop_edges"][9], m["loop_edges"][2] = [2], [9]
    for k in range(N):
        for dk, w in ((-1, 200), (-2, 150), (-3, 50), (1, 200)):
            if 0 <= k + dk < N:
                m["covis"][k].append((k + dk, w))
    m["covis"][N - 1] += [(0, 10), (1, 30)]
    m["covis"][N - 2] += [(0, 120)]
    m["covis"][0] += [(N - 2, 120)]
    for k in range(N - 3, N):
        m["corrected"][k] = g["truth"][k].copy()
        m["non_corrected"][k] = g["s_meas"][k].copy()
    m["connections"] = {N - 1: [0, 1], N - 2: [0]}
    L = 12
    m["points"] = [{"bad": l == 3, "by": mnid(N - 1) if l % 4 == 0 else 0, "cref": mnid((l * 5) % N), "ref": 5 if l == 7 else int(rng.integers(0, N)),
                    "pos": rng.normal(0, 3, 3).astype(F32)} for l in range(L)]
    return m


def write_case(path, m, fix_scale):
    N = m["N"]
    with open(path, "wb") as f:
        np.array([N, len(m["points"]), m["cur"], m["loop"], m["init"], int(fix_scale), len(m["corrected"]), len(m["non_corrected"]),
                  len(m["connections"])], np.int32).tofile(f)
        for k in range(N):
            imu = m["imu"] == k
            np.array([mnid(k), int(k in m["bad"]), m["parent"][k], int(imu), k - 1 if imu else -1, len(m["loop_edges"][k]), len(m["covis"][k]),
                      len(m["children"][k])], np.int32).tofile(f)
            np.asarray(m["pose"][k], F32).tofile(f)
            np.array(m["loop_edges"][k], np.int32).tofile(f)
            np.array(m["covis"][k], np.int32).reshape(-1).tofile(f)
            np.array(m["children"][k], np.int32).tofile(f)
        for table in (m["corrected"], m["non_corrected"]):
            for k, S in table.items():
                np.array([k], np.int32).tofile(f)
                np.asarray(S, F64).tofile(f)
        for k, to in m["connections"].items():
            np.array([k, len(to)] + list(to), np.int32).tofile(f)
        for p in m["points"]:
            np.array([int(p["bad"]), p["by"], p["cref"], p["ref"]], np.int32).tofile(f)
            np.asarray(p["pos"], F32).tofile(f)


def expected_case(m):
    """steps 2-4 of the reference on the map, as the drop-in's header states them: (case dict, keyframes with a vertex, points handed over)"""
    N = m["N"]
    kfs = [k for k in range(N) if k not in m["bad"]]
    index = {k: n for n, k in enumerate(kfs)}
    s_est, s_meas = np.zeros((len(kfs), 8), F64), np.zeros((len(kfs), 8), F64)
    for n, k in enumerate(kfs):
        if k in m["corrected"]:
            s_est[n] = m["corrected"][k]
        else:
            q = m["pose"][k, :4].astype(F64)
            nn = np.sqrt(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3])
            s_est[n] = list(q / nn) + list(m["pose"][k, 4:].astype(F64)) + [1.0]
        s_meas[n] = m["non_corrected"].get(k, s_est[n])
    weight = [dict(c) for c in m["covis"]]
    edges, inserted = [], set()
    for i in sorted(m["connections"]):                       # the drop-in's map is keyed by pointer: the vector's order, which is the index order
        for j in sorted(m["connections"][i]):
            if (i != m["cur"] or j != m["loop"]) and weight[i].get(j, 0) < 100:
                continue
            if i in index and j in index:
                edges.append((index[i], index[j], 1))
                inserted.add((min(i, j), max(i, j)))
    for k in kfs:
        p = m["parent"][k]
        if p >= 0 and p in index:
            edges.append((index[k], index[p], 0))
        for l in sorted(m["loop_edges"][k]):
            if l < k and l in index:
                edges.append((index[k], index[l], 0))
        for n_, w in m["covis"][k]:
            if w >= 100 and n_ != p and n_ not in m["children"][k] and n_ not in m["bad"] and n_ < k and (min(k, n_), max(k, n_)) not in inserted:
                edges.append((index[k], index[n_], 0))
    order = sorted(range(len(edges)), key=lambda e: (edges[e][0], edges[e][1], e))
    e = np.array([edges[o] for o in order], np.int64).reshape(-1, 3)
    pts = [p for p in m["points"] if not p["bad"]]
    by_id = {mnid(k): n for k, n in index.items()}
    ref = [by_id.get(p["cref"] if p["by"] == mnid(m["cur"]) else mnid(p["ref"]), -1) for p in pts]
    fixed = np.array([mnid(k) == m["init"] for k in kfs], np.uint8)
    c = {"s_est": s_est, "s_meas": s_meas, "fixed": fixed, "edge_i": e[:, 0].astype(np.int32), "edge_j": e[:, 1].astype(np.int32),
         "edge_from_est": e[:, 2].astype(np.uint8), "xw": np.array([p["pos"] for p in pts], F32).reshape(-1, 3), "point_ref": np.array(ref, np.int32)}
    return c, kfs, [l for l, p in enumerate(m["points"]) if not p["bad"]]


def read_out(path, N, L):
    raw = np.fromfile(path, np.uint8)
    head = raw[:12].view(np.int32)
    o = {"ret": int(head[0]), "change_index": int(head[1]), "unlocked": int(head[2]), "stats": raw[12:44].view(np.int32)}
    at = 44
    kf = raw[at:at + N * 32].view(np.int32).reshape(N, 8)
    o["set_pose_calls"], o["pose"] = kf[:, 0].copy(), kf[:, 1:].copy().view(F32)
    at += N * 32
    mp = raw[at:at + L * 20].view(np.int32).reshape(L, 5)
    o["set_pos_calls"], o["update_calls"], o["point"] = mp[:, 0].copy(), mp[:, 1].copy(), mp[:, 2:].copy().view(F32)
    assert len(raw) == at + L * 20
    return o


def run(exe, tmp_path, m, fix_scale):
    write_case(str(tmp_path / "case.bin"), m, fix_scale)
    DD.run(exe, str(tmp_path / "case.bin"), str(tmp_path / "out.bin"))
    return read_out(str(tmp_path / "out.bin"), m["N"], len(m["points"]))


def untouched(got, m):
    return (got["set_pose_calls"] == 0).all() and (got["set_pos_calls"] == 0).all() and np.array_equal(got["pose"], m["pose"]) and \
        np.array_equal(got["point"], np.array([p["pos"] for p in m["points"]], F32)) and got["change_index"] == 0 and (got["stats"] == 0).all()


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_drop_in(tmp_path):
    exe = DD.build(tmp_path, "essential_graph_driver")
    for fix_scale in (True, False):
        m = make_map()
        c, kfs, pts = expected_case(m)
        assert len(kfs) == 13 and (c["edge_from_est"] == 1).sum() == 2 and (c["point_ref"] == -1).sum() >= 1
        ref = R.essential_graph(c, R.params(max_trials=10, fix_scale=fix_scale))
        got = run(exe, tmp_path, m, fix_scale)
        assert got["ret"] == ref["ret"] > 0 and np.array_equal(got["stats"], ref["stats"])
        assert got["change_index"] == 1 and got["unlocked"] == 0         # every write-back call was made with mMutexMapUpdate held, and it was released
        assert np.array_equal(got["pose"][kfs], ref["tiw_f32"]) and (got["set_pose_calls"][kfs] == 1).all()
        assert got["set_pose_calls"][5] == 0 and np.array_equal(got["pose"][5], m["pose"][5])      # the bad keyframe
        assert np.array_equal(got["point"][pts], ref["xw_out"]) and (got["set_pos_calls"][pts] == 1).all() and (got["update_calls"][pts] == 1).all()
        assert got["set_pos_calls"][3] == 0 and got["update_calls"][3] == 0                        # the bad point
        moved = c["point_ref"] >= 0
        assert not np.array_equal(ref["xw_out"][moved], c["xw"][moved]) and np.array_equal(ref["xw_out"][~moved], c["xw"][~moved])
    # not served: the inertial edge; more keyframes than the cap
    m = make_map(imu=6)
    got = run(exe, tmp_path, m, True)
    assert got["ret"] == NOT_SERVED and untouched(got, m)
    big = make_map(N=R.MAX_KF + 1, bad=())
    got = run(exe, tmp_path, big, True)
    assert got["ret"] == NOT_SERVED and untouched(got, big)
