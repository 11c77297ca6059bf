"""CPU: the place-recognition checkers held against DBoW3's and KeyFrameDatabase's OWN C++.  tests/golden/ref_bow_*.npz record what the
reference's function bodies compute (oracle/ref_classic cuts Vocabulary::transform / fromStream / toStream, DescManip::distance, the
fronts of DetectNBestCandidates_sp / DetectRelocalizationCandidates out of a checkout, compiles BowVector.cpp, FeatureVector.cpp,
ScoringObject.cpp and quicklz.c whole, behind a stand-in for the few OpenCV names; tools/gen_ref_golden.py --only bow records).  Here the
numpy restatement tests/bow_ref.py -- what tests/test_gpu_bow.py holds the kernels to -- and the library's stream reader are compared with
those recordings; tests/test_gpu_ref_bow.py does the HIP kernels.  float64 outputs are compared as uint64 views, the stored (float) score
as uint32.  The live tests re-run the harness when oracle/_ref/ exists (it needs the checkout).

Two documented departures, and how they are scoped here:
* a leaf above depth L - levelsup: the reference never writes *nid and files the feature under an uninitialised node id, the project
  files it under the leaf's own id.  Whether a case can meet that is decided FROM THE TREE (ref_bow_cases.fv_defined) and must agree with
  what was recorded; only the BowVector, the words and the weights of such a case are compared, and the harness's nid where it was written.
* a connected keyframe: DetectNBestCandidates_sp resets its counter to 0 at every hit and so leaves 1, the library reports the true
  count.  `common` is compared for the entries the reference put in lKFsSharingWords; for a connected one only "not scored, not in the
  maximum" (the maximum, the gate and both counts are compared whole)."""
import numpy as np
import pytest

import bow_ref as B
import ref_bow_cases as BC
import ref_classic_cases as RC
from oracle.ref_classic import client as R

live = pytest.mark.skipif(not R.usable_bow(), reason="oracle/_ref/ref_bow is not built, or its Rover-SLAM checkout is absent "
                                                     "(__graft_entry__.build() builds it when the checkout is there)")


def u64(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def same64(a, b):
    return np.asarray(a).shape == np.asarray(b).shape and np.array_equal(u64(a), u64(b))


def check_transform(v, feats, levelsup, rec, fv_kind):
    """one restatement-shaped result (bow_ref.transform's keys) against one recording"""
    def check(got):
        assert np.array_equal(got["word"], rec["word"]) and same64(got["weight"], rec["weight"])
        assert np.array_equal(got["bow_word"], rec["bow_word"]), (got["bow_word"][:8], rec["bow_word"][:8])
        assert same64(got["bow_value"], rec["bow_value"]), np.argwhere(u64(got["bow_value"]) != u64(rec["bow_value"]))[:8].ravel()
        written = rec["nid"] >= 0
        assert np.array_equal(got["node"][written], rec["nid"][written])
        leaf = v["words"][got["word"]]                                      # the project's choice where the reference wrote nothing
        assert np.array_equal(got["node"][~written], leaf[~written])
        assert written.all() == fv_kind
        if fv_kind:
            for k in ("fv_node", "fv_offsets", "fv_feat"):
                assert got[k].dtype == rec[k].dtype and np.array_equal(got[k], rec[k]), k
        else:
            assert "fv_node" not in rec
    return check


# ---------------------------------------------------------------- transform
@pytest.mark.parametrize("name", BC.VOCABS)
def test_transform_restatement_equals_dbow3(name):
    z, v, cases = BC.load_vocab(name)
    assert len(cases) == len(z["census"]) and [str(k) for k in z["census_keys"]] == list(BC.TRANSFORM_CENSUS)
    for i, feats, levelsup in cases:
        fv_kind = BC.fv_defined(v, levelsup)
        assert fv_kind == bool(z["fv_recorded"][i]), (name, i, "the tree and the recording disagree about which kind of fixture this is")
        check_transform(v, feats, levelsup, BC.recorded(z, i), fv_kind)(B.transform(v, feats, levelsup))
        assert BC.transform_census(v, feats, levelsup) == z["census"][i].tolist(), "the census changed: regenerate (tools/gen_ref_golden.py --only bow)"
    assert (name == "irregular") == (not z["fv_recorded"].all())            # only the irregular tree has BowVector-only cases


def test_transform_fixtures_are_not_vacuous():
    total, seen_n, seen_w = np.zeros(4, np.int64), set(), set()
    for name in BC.VOCABS:
        z, v, cases = BC.load_vocab(name)
        assert v["scoring"] == B.L1_NORM
        total += z["census"].sum(axis=0)
        seen_w.add(v["weighting"])
        ups = {u for _, _, u in cases}
        seen_n |= {len(f) for _, f, _ in cases}
        assert v["D"] <= 32 or max(len(f) for _, f, _ in cases) <= 257
        if name in ("k2L4D8", "k3L3D24", "k5L3D32", "k6L3D256", "k10L2D32"):
            assert z["census"][:, 0].sum() >= 10, (name, "no descent tie decided by order")
            assert {0, 1, v["L"] - 1, v["L"], v["L"] + 1} >= ups and len(ups) >= 4 and v["L"] in ups and 0 in ups, (name, ups)
            assert z["census"][:, 2].sum() >= 1 and z["census"][:, 3].sum() >= 1, name
            assert (v["k"], v["L"], v["D"]) == tuple(int(x) for x in name.replace("k", "").replace("L", " ").replace("D", " ").split())
    assert (total >= 1).all() and seen_w == {B.TF_IDF, B.TF, B.IDF, B.BINARY} and seen_n >= set(BC.SIZES)
    # arbitrary bytes in one vocabulary, 0/1 bytes at D = 256
    assert BC.load_vocab("k6L3D256")[1]["desc"].max() == 1 and BC.load_vocab("k10L2D32")[1]["desc"].max() > 1
    # every feature stopped: an empty BowVector; the 700-term chain: not 700 * w, nor a pairwise sum
    z, v, cases = BC.load_vocab("stopped")
    assert len(cases[0][1]) == 64 and len(z["c0_bow_word"]) == 0 and len(z["c0_fv_node"]) == 0 and (z["c0_weight"] == 0).all()
    z, v, cases = BC.load_vocab("oneword")
    w = float(v["weight"][v["words"][0]])
    chain = 0.0
    for _ in range(700):
        chain += w
    assert len(cases[0][1]) == 701 and z["c0_bow_value"][0] == chain / (chain + 0.3)
    assert chain != 700 * w and chain != float(np.sum(np.full(700, w)))
    # the irregular tree: leaves at different depths, and a feature that ends on the shallow one
    z, v, cases = BC.load_vocab("irregular")
    assert len(set(BC.leaf_depths(v).tolist())) > 1 and (z["c0_nid"] == -1).any() and (z["c0_nid"] >= 0).any()


# ---------------------------------------------------------------- the stream reader and writer
def read(tmp_path, data):
    from rover_slam_amd import capi
    p = tmp_path / "voc.dbow3"
    p.write_bytes(bytes(data))
    return capi.read_bow_vocab(str(p))


def same_tree(got, v):
    for k in ("k", "L", "weighting", "scoring", "n_nodes", "D"):
        assert got[k] == v[k], k
    for k in B.VOCAB_ARRAYS:
        a, b = (got[k][1:], v[k][1:]) if k in ("parent", "desc") else (got[k], v[k])     # the root has neither parent nor descriptor
        assert a.dtype == b.dtype and a.shape == b.shape, k
        assert np.array_equal(u64(a), u64(b)) if k == "weight" else np.array_equal(a, b), k


@pytest.mark.parametrize("name", BC.VOCABS)
def test_reader_equals_voc_dump(tmp_path, name):
    """rfe_k_bow_vocab_read on the stream DBoW3's toStream wrote == what DBoW3's fromStream holds, field for field, children order included"""
    z, v, _ = BC.load_vocab(name)
    got = read(tmp_path, z["stream"])
    same_tree(got, v)
    assert v["n_words"] == int((got["word_id"] >= 0).sum()) and np.array_equal(np.nonzero(got["word_id"] >= 0)[0][np.argsort(got["word_id"][got["word_id"] >= 0])], v["words"])


def test_children_are_not_in_id_order_somewhere():
    """what keeps the test above from passing with a reader that sorts children by id, and with word ids taken from the leaf order"""
    for name in ("k3L3D24", "k5L3D32"):
        v = BC.load_vocab(name)[1]
        unsorted = sum(not np.array_equal(BC.kids(v, p), np.sort(BC.kids(v, p))) for p in range(v["n_nodes"]))
        assert unsorted >= 5, name
    v = BC.load_vocab("k3L3D24")[1]
    leaves = np.nonzero(v["word_id"] >= 0)[0]
    assert not np.array_equal(v["word_id"][leaves], np.arange(len(leaves)))


def test_compressed_stream_is_refused(tmp_path):
    from rover_slam_amd import capi
    z = RC.load("bow_oneword")
    assert z["stream_compressed"][8] == 1 and z["stream"][8] == 0 and not np.array_equal(z["stream"], z["stream_compressed"])
    with pytest.raises(capi.RfeError, match=r"error -4: .*compressed"):      # RFE_ERR_IO
        read(tmp_path, z["stream_compressed"])
    assert read(tmp_path, z["stream"])["n_nodes"] == 3


def test_our_writer_and_dbow3_rewrite_load_the_same_tree(tmp_path):
    """bow_ref.stream_bytes writes parent by parent, Vocabulary::toStream in the order of its stack: other bytes, the same tree"""
    differ = 0
    for name in BC.VOCABS:
        z, v, _ = BC.load_vocab(name)
        ours = B.stream_bytes(v)
        theirs = z["stream"].tobytes()
        assert len(ours) == len(theirs)
        same_tree(read(tmp_path, ours), v)
        same_tree(read(tmp_path, theirs), v)
        first = lambda s: [int.from_bytes(s[o:o + 4], "little") for o in node_offsets(s, v)]   # noqa: E731
        differ += first(ours) != first(theirs)
        assert sorted(first(ours)) == sorted(first(theirs)) == list(range(1, v["n_nodes"]))
    assert differ >= 3


def node_offsets(s, v):
    """byte offsets of the node records' ids in an uncompressed stream"""
    return [13 + 16 + i * (28 + v["D"]) for i in range(v["n_nodes"] - 1)]


# ---------------------------------------------------------------- scores and the database
def test_score_restatement_equals_l1scoring():
    z = RC.load("bow_kfdb")
    s, _ = BC.unpack_script(z, "grow")
    nonzero = 0
    for (a, b), ref in zip(z["score_pairs"].tolist(), z["score_ref"]):
        got = B.l1_score(*s["bows"][a], *s["bows"][b])
        assert u64(got) == u64(ref), (a, b, got, ref)
        nonzero += ref > 0
    assert nonzero >= 10 and len(s["bows"][603][0]) == 0


def check_query(r, ref, q, ex):
    """one library-shaped query result (common, scored, score f64, stats) against row q of a kfdb recording"""
    early, mx, mn, n_sharing, n_scored = (int(x) for x in ref["stats"][q])
    E = len(ex)
    sharing, words, scored = ref["sharing"][q][:E].astype(bool), ref["words"][q][:E], ref["scored"][q][:E]
    assert r["stats"].tolist() == [mx, mn, n_sharing, n_scored], (q, r["stats"], ref["stats"][q])
    assert early == (n_sharing == 0)
    assert np.array_equal((r["common"] > 0) & (ex == 0), sharing)
    assert np.array_equal(r["common"][sharing], words[sharing])
    assert (r["common"][(ex == 0) & ~sharing] == 0).all()
    assert np.array_equal(r["scored"], scored) and not r["scored"][ex == 1].any()
    if n_sharing:
        assert r["common"][sharing].max() == mx                              # no connected entry is in the maximum
    on = scored.astype(bool)
    assert np.array_equal(u64(r["score"][on]), u64(ref["score64"][q][:E][on]))
    assert np.array_equal(r["score"][on].astype(np.float32).view(np.uint32), ref["score"][q][:E][on].view(np.uint32))
    return on


@pytest.mark.parametrize("name", ["empty", "one", "grow", "gate"])
def test_database_rule_equals_keyframedatabase(name):
    z = RC.load("bow_kfdb")
    s, ref = BC.unpack_script(z, name)
    n = 0
    for q, op, entries, (qw, qx), ex in BC.replay(s):
        keep = np.full((len(entries),), -9.5)
        r = B.db_query(entries, qw, qx, ex, keep)
        on = check_query(r, ref, q, ex)
        assert (r["score"][~on] == -9.5).all() and (ref["score"][q][len(entries):] == np.float32(-9.5)).all()
        n += 1
    assert n == len(ref["stats"]) == len(s["connected"])
    assert BC.kfdb_census(s) == z[name + "_census"].tolist(), "the census changed: regenerate (tools/gen_ref_golden.py --only bow)"


def test_database_fixtures_are_not_vacuous():
    z = RC.load("bow_kfdb")
    assert [str(k) for k in z["census_keys"]] == list(BC.KFDB_CENSUS) and [str(k) for k in z["scripts"]] == ["empty", "one", "grow", "gate"]
    total = sum(z[f"{n}_census"] for n in ("empty", "one", "grow", "gate"))
    assert (total >= 1).all(), dict(zip(BC.KFDB_CENSUS, total.tolist()))
    gate = dict(zip(BC.KFDB_CENSUS, z["gate_census"].tolist()))
    assert gate["entry_at_gate"] >= 8 and gate["entry_one_above_gate"] >= 8 and gate["excluded_would_set_max"] == len(BC.GATE_MAXIMA)
    s, ref = BC.unpack_script(z, "gate")
    maxima = ref["stats"][:, 1].tolist()
    assert set(BC.GATE_MAXIMA) <= set(maxima) and sum(m % 5 == 0 for m in maxima) >= 4 and sum(m % 5 != 0 for m in maxima) >= 6
    for mx, mn in ref["stats"][:, 1:3].tolist():
        assert mn == int(np.float32(mx) * np.float32(0.8))                  # the recorded gate is the float product, truncated
    assert any(mn != int(round(mx * 0.8)) for mx, mn in ref["stats"][:, 1:3].tolist())   # and rounding would be told apart
    # a connected keyframe keeps the reference's counter at 1 however many words it shares: why `common` is not compared there
    ex = [c[0] for c in s["connected"][::2]]
    assert all(ref["words"][2 * g][e] == 1 and not ref["sharing"][2 * g][e] for g, e in enumerate(ex))
    s, ref = BC.unpack_script(z, "grow")
    adds = np.cumsum([op == BC.ADD for op, _ in s["ops"]])
    at_query = [int(adds[i]) for i, (op, _) in enumerate(s["ops"]) if op >= BC.QUERY_SP]
    assert at_query[:3] == [255, 256, 257] and at_query[-1] == 600
    lens = {len(w) for w, _ in s["bows"][:600]}
    assert {1, 63, 64, 65, 4096} <= lens
    nq = {len(s["bows"][a][0]) for op, a in s["ops"] if op >= BC.QUERY_SP}
    assert {0, 1, 4096} <= nq
    assert ref["stats"][-1].tolist()[0] == 1 and len(s["connected"][-1]) >= 1      # every sharing entry connected: the early return
    assert any(len(c) == 0 for c in s["connected"]) and any(0 < len(c) < 100 for c in s["connected"])


# ---------------------------------------------------------------- live: the harness itself
@live
def test_live_harness_reproduces_every_recording():
    """fixtures cannot go stale: the compiled reference gives today what was recorded, and reads back its own compressed stream"""
    for name in BC.VOCABS:
        z, v, cases = BC.load_vocab(name)
        stream = z["stream"].tobytes()
        d = R.voc_dump(stream)
        same_tree(d, v)
        assert np.array_equal(d["words"], v["words"])
        assert R.voc_write(stream, False) == stream
        for i, feats, levelsup in cases:
            r, rec = R.transform(stream, feats, levelsup), BC.recorded(z, i)
            for k, a in rec.items():
                assert a.dtype == r[k].dtype and np.array_equal(a.view(np.uint8), r[k].view(np.uint8)), (name, i, k)
    z = RC.load("bow_oneword")
    assert R.voc_write(z["stream"].tobytes(), True) == z["stream_compressed"].tobytes()
    same_tree(R.voc_dump(z["stream_compressed"].tobytes()), BC.dump_dict(z))
    z = RC.load("bow_kfdb")
    for name in ("empty", "one", "grow", "gate"):
        s, ref = BC.unpack_script(z, name)
        r = R.kfdb(s["n_words"], s["ops"], s["bows"], s["connected"])
        for k in BC.KFDB_OUT:
            assert np.array_equal(r[k].view(np.uint8), ref[k].view(np.uint8)), (name, k)
    s, _ = BC.unpack_script(z, "grow")
    for (a, b), ref in zip(z["score_pairs"].tolist(), z["score_ref"]):
        assert u64(R.score(*s["bows"][a], *s["bows"][b])) == u64(ref)


@live
def test_live_sources_give_the_recorded_inputs():
    """the seeded generators still make the recorded inputs (so --check style regeneration can give identical bytes)"""
    for name in BC.VOCABS:
        z, v, _ = BC.load_vocab(name)
        src, pools, cases = BC.source(name)
        assert R.voc_write(B.stream_bytes(src), False) == z["stream"].tobytes(), name
        for p, a in pools.items():
            assert np.array_equal(a, z["pool_" + p]), (name, p)
        assert [[list(pools).index(p), n, u] for p, n, u in cases] == z["cases"].tolist()


@live
def test_live_sweep():
    """fresh seeded cases: DBoW3 == restatement on trees, features and database scripts that are in no fixture"""
    for seed in range(6):
        rng = np.random.default_rng(900 + seed)
        k, L, D = int(rng.integers(2, 7)), int(rng.integers(1, 4)), int(rng.choice([8, 24, 32, 64]))
        bits01 = bool(seed % 2)
        v = BC.nested_vocab(k, L, D, 910 + seed, seed % 4, bits01, stop_every=int(rng.integers(0, 6)))
        pairs = BC.plant_ties(v, 920 + seed, bits01)
        BC.shuffle_children(v, 930 + seed)
        stream = R.voc_write(B.stream_bytes(v), False)
        d = R.voc_dump(stream)
        same_tree(d, v)
        v["words"] = d["words"]
        feats = BC.make_pool(v, pairs, 300, 940 + seed, bits01)
        for levelsup in (0, 1, L, L + 1):
            rec = R.transform(stream, feats, levelsup)
            check_transform(v, feats, levelsup, rec, True)(B.transform(v, feats, levelsup))


@live
def test_live_extractor_fails_on_drift(tmp_path):
    """a checkout whose lines moved is refused, not compiled: the ranges must be the ones include/rover_fe.h cites"""
    import shutil
    from oracle.ref_classic import build_ref
    ref = tmp_path / "ref"
    for name, (fname, *_r) in build_ref._spec_bow().items():
        dst = ref / fname
        dst.parent.mkdir(parents=True, exist_ok=True)
        shutil.copyfile(build_ref.ref_dir() + "/" + fname, dst)
    assert len(build_ref.extract_bow(str(ref), str(tmp_path / "out"))) == 19      # the copy as it is: accepted
    for victim in ("Thirdparty/DBoW3/src/Vocabulary.cpp", "src/KeyFrameDatabase.cc", "Thirdparty/DBoW3/src/ScoringObject.cpp"):
        f = ref / victim
        kept = f.read_bytes()
        f.write_bytes(b"// one more line\n" + kept)
        with pytest.raises(build_ref.Drift, match=victim.split("/")[-1]):
            build_ref.extract_bow(str(ref), str(tmp_path / "out2"))
        f.write_bytes(kept)
