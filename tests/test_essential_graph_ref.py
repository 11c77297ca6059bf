"""CPU: the contract of DESIGN.md 6m.  The vectorised restatement (essential_graph_ref.py) equals the sequential transcription
(essential_graph_seq.py) exactly; the stated departures are measured against g2o's own choices; the planted graph is corrected; Sim3 log
is exercised on both sides of its four branches; the forced paths take the paths they are named for; the exports exist."""
import math
import os
import re
import shutil

import numpy as np
import pytest

import dropin_driver as DD
import essential_graph_ref as R
import essential_graph_seq as S
import optimize_sim3_ref as OS

F64 = np.float64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ("siw", "tiw_f32", "swi", "xw_out", "chi2", "trace")


def equal(a, b):
    for k in KEYS:
        assert a[k].shape == b[k].shape and a[k].dtype == b[k].dtype, k
        assert np.array_equal(a[k], b[k], equal_nan=True), (k, np.argwhere(a[k] != b[k])[:5])
    assert list(a["stats"][:6]) == list(b["stats"][:6]) and a["ret"] == b["ret"]


SMALL = {"chain": dict(N=7, loops=2, corrected=2, L=6, drift=0.02), "band": dict(N=10, band=3, loops=2, corrected=2, L=4, drift=0.01, dscale=0.01),
         "star": dict(N=8, kind="star", fixed=3, L=3, drift=0.02), "arrowhead": dict(N=13, kind="arrowhead", corrected=3, drift=0.01),
         "shuffled": dict(N=9, band=2, loops=2, corrected=2, shuffle=True, fixed=4, L=5, dup=3)}


@pytest.mark.parametrize("fix_scale", [True, False])
@pytest.mark.parametrize("name", sorted(SMALL))
def test_restatement_equals_transcription(name, fix_scale):
    c = R.graph(70, **SMALL[name])
    P = R.params(iterations=4, fix_scale=fix_scale)
    equal(R.essential_graph(c, P), S.essential_graph(c, P))


@pytest.mark.parametrize("name", R.FORCED)
def test_forced_paths(name):
    c, P = R.forced(name)
    r = R.essential_graph(c, P)
    R.check_forced(name, r)
    equal(r, S.essential_graph(c, P))


def test_refusals():
    c = R.graph(71, 6, L=3)
    for key, idx, val in (("edge_i", 2, 6), ("edge_j", 2, -1), ("point_ref", 0, 6), ("point_ref", 0, -2)):
        bad = dict(c)
        bad[key] = c[key].copy()
        bad[key][idx] = val
        with pytest.raises(R.Invalid):
            R.essential_graph(bad)
    bad = dict(c, edge_j=c["edge_i"].copy())
    with pytest.raises(R.Invalid):
        R.essential_graph(bad)
    bad = dict(c, edge_i=c["edge_i"][::-1].copy(), edge_j=c["edge_j"][::-1].copy())
    with pytest.raises(R.Invalid):
        R.essential_graph(bad)
    for P in (R.params(iterations=-1), R.params(iterations=65), R.params(max_trials=-1), R.params(user_lambda_init=np.nan)):
        with pytest.raises(R.Invalid):
            R.essential_graph(c, P)


def test_departure_cost():
    """the transcription with the contract's choices against g2o's own (sequential sums, numpy.linalg.solve for the system and for W,
    libm's log / acos / sin / cos / exp) on four small graphs: the largest difference of any corrected Sim3 number"""
    worst = 0.0
    for n_, name in enumerate(("chain", "band", "star", "arrowhead")):
        c = R.graph(80 + n_, **SMALL[name])
        for fix_scale in (True, False):
            P = R.params(iterations=5, fix_scale=fix_scale)
            a, b = S.essential_graph(c, P), S.essential_graph(c, P, S.Choices.g2o())
            worst = max(worst, float(np.abs(a["siw"] - b["siw"]).max()))
    print("departure cost", worst)
    assert worst <= 8 * R.DEPARTURE_MAX


@pytest.mark.parametrize("fix_scale", [True, False])
def test_it_optimises(fix_scale):
    c = R.optimises_scene(fix_scale)
    r = R.essential_graph(c, R.params(fix_scale=fix_scale))
    before, after = R.pose_error(c["s_est"], c["truth"]), R.pose_error(r["siw"], c["truth"])
    gain = (before[0] / after[0], before[1] / after[1])
    print("gain", fix_scale, gain)
    want = R.OPTIMISES_GAIN[fix_scale]
    assert gain[0] >= want[0] / 16 and gain[1] >= want[1] / 16
    if fix_scale:
        assert np.all(r["siw"][:, 7] == c["s_est"][:, 7])
    # a point moves with its reference keyframe: its coordinates in that keyframe's frame stay what they were
    ref = c["point_ref"]
    for l in np.nonzero(ref >= 0)[0]:
        was = OS.sim3_map([F64(v) for v in c["s_est"][ref[l]]], [F64(v) for v in c["xw"][l]])
        now = OS.sim3_map([F64(v) for v in r["siw"][ref[l]]], [F64(v) for v in r["xw_out"][l]])
        assert np.allclose(was, now, atol=1e-4), l
    assert np.array_equal(r["xw_out"][ref < 0], c["xw"][ref < 0])


def test_log_acos_against_libm():
    rng = np.random.default_rng(0)
    x = np.concatenate([np.exp(rng.uniform(-30, 30, 50000)), rng.uniform(0.5, 2.0, 50000)])
    ulp = np.abs(R.log_(x) - np.log(x)) / np.spacing(np.abs(np.log(x)) + 1e-300)
    assert ulp.max() <= R.LOG_MAX_ULP
    assert R.log_(np.array([1.0]))[0] == 0.0 and R.log_(np.array([0.0]))[0] == -np.inf and np.isnan(R.log_(np.array([-1.0]))[0])
    assert R.log_(np.array([5e-324]))[0] == F64(math.log(5e-324))
    d = np.concatenate([rng.uniform(-1, 1, 100000), [0.5, -0.5, 1 - 1e-5, 0.0]])
    ulp = np.abs(R.acos_(d) - np.arccos(d)) / np.spacing(np.arccos(d) + 1e-300)
    assert ulp.max() <= R.ACOS_MAX_ULP
    assert R.acos_(np.array([1.0]))[0] == 0.0 and R.acos_(np.array([-1.0]))[0] == F64(math.pi) and np.isnan(R.acos_(np.array([1.0000001]))[0])


def _with_d_and_sigma(d, sigma, rng):
    """a Sim3 whose rotation has 0.5 (trace - 1) as close to d as a quaternion allows, and whose scale is exp(sigma)"""
    theta = math.acos(max(-1.0, min(1.0, d)))
    axis = rng.normal(size=3)
    axis /= np.linalg.norm(axis)
    q = list(axis * math.sin(theta / 2)) + [math.cos(theta / 2)]
    return [F64(v) for v in q] + [F64(v) for v in rng.normal(0, 1, 3)] + [F64(math.exp(sigma))]


def test_log_branches():
    """inputs one ulp either side of |sigma| = 1e-5 and of d = 1 - 1e-5: the branch taken is the one the comparison names, the vectorised
    log equals the sequential one bit for bit, and log(exp(x)) returns x within the measured bound on every branch"""
    rng = np.random.default_rng(1)
    eps = F64(0.00001)
    ch = S.Choices()
    seen = set()
    worst = 0.0
    for sig0 in (np.nextafter(eps, 0), eps, np.nextafter(eps, 1), -np.nextafter(eps, 0), F64(0.3)):
        for d0 in (np.nextafter(1 - eps, 0), 1 - eps, np.nextafter(1 - eps, 2), F64(0.2)):
            Sm = _with_d_and_sigma(float(d0), float(sig0), rng)
            v = R.sim3_log([np.array([x]) for x in Sm])
            s = S.Sim3.from_row(Sm).log(ch)
            assert [float(a[0]) for a in v] == [float(b) for b in s]
            Rm = R.quat_to_rot(Sm[:4])
            d = 0.5 * (((Rm[0][0] + Rm[1][1]) + Rm[2][2]) - 1)
            seen.add((bool(np.abs(s[6]) < eps), bool(d > 1 - eps)))
    assert seen == {(True, True), (True, False), (False, True), (False, False)}
    def round_trip(u):
        q, t, s = OS.sim3_exp([F64(x) for x in u])
        back = R.sim3_log([np.array([x]) for x in list(q) + list(t) + [s]])
        return max(abs(float(b[0]) - x) for b, x in zip(back, u))
    for u in ([0.3, -0.2, 0.5, 1, 2, 3, 0.1], [1e-7, 0, 0, 1, 2, 3, 0.1], [0.3, -0.2, 0.5, 1, 2, 3, 1e-7], [1e-7, 2e-7, 0, 1, 2, 3, 1e-7],
              [2.0, 1.5, -1.0, 1, 2, 3, -0.3], [0, 0, 0, 0, 0, 0, 0]):
        worst = max(worst, round_trip(u))
    band = round_trip([0.003, 0.003, 0.001, -4, 5, 6, 0.00001])
    print("log(exp(x)) - x", worst, "in the band", band)
    assert worst <= 8 * R.LOG_EXP_MAX and band <= 8 * R.LOG_EXP_BAND_MAX


def test_tile_fill():
    """the symbolic pass: a chain fills the band only, an arrowhead the band and the last rows, a dense graph everything"""
    def tiles(c):
        free_index = np.cumsum(c["fixed"] == 0) - 1
        free_index[c["fixed"] != 0] = -1
        Nf = int((c["fixed"] == 0).sum())
        return R.tile_fill(free_index, c["edge_i"].astype(np.int64), c["edge_j"].astype(np.int64), Nf)
    fill, n = tiles(R.graph(1, 41, kind="chain"))
    assert fill.shape == (10, 10) and n == 19
    fill, n = tiles(R.graph(1, 41, kind="arrowhead"))
    assert 19 < n < 55 and fill[9].all() and not fill[5, 2]
    fill, n = tiles(R.graph(1, 41, kind="chain", band=40))
    assert n == 55


def test_exports_in_header():
    h = open(os.path.join(ROOT, "include", "rover_fe.h")).read()
    for name in ("rfe_essential_graph", "rfe_essential_graph_dev"):
        assert re.search(r"\bint %s\(rfe_ctx\* ctx, rfe_essential_graph_params params" % name, h), name
    for macro, val in (("RFE_EG_MAX_KF", R.MAX_KF), ("RFE_EG_MAX_EDGES", R.MAX_EDGES), ("RFE_EG_MAX_ITERATIONS", R.MAX_ITERATIONS)):
        assert re.search(r"#define %s %d\b" % (macro, val), h), macro
    assert "#define RFE_EG_MAX_POINTS (1 << 20)" in h
    src = open(os.path.join(ROOT, "rover-slam_amd", "csrc", "rfe_internal.h")).read()
    assert "EG_TILE_V = %d, EG_TILE = %d" % (R.TILE_V, R.TILE) in src


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_drop_in_compiles(tmp_path):
    """include/rfe/essential_graph.h over the driver's stand-ins, as the reference builds: -std=c++14 -Wall -Werror"""
    DD.build(tmp_path, "essential_graph_driver", link=False)
