"""CPU: tests/bow_ref.py (the restatement the GPU tests compare with) against a literal per-feature transcription of the reference's loops --
a dict filled the way BowVector::addWeight / addIfNotExist and FeatureVector::addFeature fill their maps, Python float chains, and the
merge loop of L1Scoring::score -- and the library's reader of DBoW3's binary stream (no device needed) against the writer."""
import numpy as np
import pytest

import bow_ref as B


# ---------------------------------------------------------------- the literal transcription
def distance(a, b):
    return sum(bin(int(x) ^ int(y)).count("1") for x, y in zip(a, b))


def literal_descend(v, feature, levelsup):
    kids = lambda i: v["children"][v["child_offsets"][i]:v["child_offsets"][i + 1]]   # noqa: E731
    nid_level = v["L"] - levelsup
    nid = 0 if nid_level <= 0 else None
    final_id, current_level = 0, 0
    while len(kids(final_id)):
        current_level += 1
        best_d = float("inf")
        for c in kids(final_id):
            d = distance(feature, v["desc"][c])
            if d < best_d:
                best_d, final_id = d, int(c)
        if current_level == nid_level:
            nid = final_id
    if nid is None:
        nid = final_id                                # the reference leaves *nid unwritten here
    return int(v["word_id"][final_id]), nid, float(v["weight"][final_id])


def literal_transform(v, feats, levelsup):
    bow, fv, per = {}, {}, []
    for i, f in enumerate(feats):
        word, nid, w = literal_descend(v, f, levelsup)
        per.append((word, nid, w))
        if w > 0:
            if v["weighting"] in (B.TF_IDF, B.TF):
                bow[word] = bow[word] + w if word in bow else w
            elif word not in bow:
                bow[word] = w
            fv.setdefault(nid, []).append(i)
    norm = 0.0
    for word in sorted(bow):
        norm += abs(bow[word])
    if norm > 0.0:
        for word in bow:
            bow[word] /= norm
    return per, sorted(bow.items()), sorted(fv.items())


def literal_score(v1, v2):
    """L1Scoring::score on two sorted (word, value) lists; lower_bound is a linear scan here"""
    i, j, score = 0, 0, 0.0
    while i < len(v1) and j < len(v2):
        if v1[i][0] == v2[j][0]:
            vi, wi = v1[i][1], v2[j][1]
            score += abs(vi - wi) - abs(vi) - abs(wi)
            i += 1; j += 1
        elif v1[i][0] < v2[j][0]:
            while i < len(v1) and v1[i][0] < v2[j][0]:
                i += 1
        else:
            while j < len(v2) and v2[j][0] < v1[i][0]:
                j += 1
    return -score / 2.0


def check_transform(v, feats, levelsup):
    r = B.transform(v, feats, levelsup)
    per, bow, fv = literal_transform(v, feats, levelsup)
    assert [(int(a), int(b), float(c)) for a, b, c in zip(r["word"], r["node"], r["weight"])] == per
    assert [(int(w), float(x)) for w, x in zip(r["bow_word"], r["bow_value"])] == bow          # float equality: bit-equal but for the sign of zero
    got_fv = [(int(n), [int(f) for f in r["fv_feat"][r["fv_offsets"][i]:r["fv_offsets"][i + 1]]]) for i, n in enumerate(r["fv_node"])]
    assert got_fv == fv
    assert len(r["fv_offsets"]) == len(r["fv_node"]) + 1 and r["fv_offsets"][-1] == len(r["fv_feat"])
    for k in B.KEYS:
        assert r[k].dtype == B.DTYPES[k], k
    return r


@pytest.mark.parametrize("weighting", [B.TF_IDF, B.TF, B.IDF, B.BINARY])
def test_restatement_matches_the_literal_loops(weighting):
    rng = np.random.default_rng(5 + weighting)
    v = B.make_vocab(4, 3, 32, seed=3, weighting=weighting, bits01=False, stop_every=5)
    feats = B.random_desc(rng, (150, 32), False)
    feats[:40] = v["desc"][rng.integers(1, v["n_nodes"], 40)]             # features equal to node descriptors: many share a word
    for levelsup in (0, 1, 3, 4):
        r = check_transform(v, feats, levelsup)
    assert len(r["bow_word"]) < (r["weight"] > 0).sum()                   # some word has several features
    assert (r["weight"] == 0).any()


def test_sequential_sum_differs_from_a_tree_sum():
    """what the exact GPU comparison pins: 700 equal non-dyadic weights added one after the other are not 700 * w, nor numpy's pairwise sum"""
    v, feats, w = B.one_word_case()
    r = check_transform(v, feats, 0)
    chain = 0.0
    for _ in range(700):
        chain += w
    assert r["bow_value"][0] == chain / (chain + 0.3)
    assert chain != 700 * w and chain != float(np.sum(np.full(700, w)))


def test_irregular_tree_and_nid_decision():
    v = B.irregular_vocab()
    feats = np.array([[0] * 8, [1] * 8, [1, 1, 1, 1, 0, 0, 0, 0], [1, 1, 1, 1, 1, 1, 0, 0]], np.uint8)
    for levelsup in (0, 1, 2, 3, 4):
        r = check_transform(v, feats, levelsup)
        assert r["node"][0] == (0 if levelsup >= 3 else 1)                # the depth-1 leaf stands for itself above the root level
    r0 = B.transform(v, feats, 0)
    assert r0["word"][0] == v["word_id"][1] and r0["node"][1] != 1 and r0["node"][2] == 1     # feature 2 ties between nodes 1 and 2


def test_scores_and_database_front():
    rng = np.random.default_rng(9)
    entries = []
    for e in range(40):
        w = np.sort(rng.choice(300, rng.integers(0, 120), replace=False)).astype(np.int32)
        x = rng.random(len(w)); x = x / x.sum() if len(w) else x
        entries.append((w, x))
    entries[7] = None
    qw, qx = entries[3]
    r = B.db_query(entries, qw, qx, exclude=np.arange(40) == 3, score=np.full(40, -5.0))
    assert r["common"][7] == 0 and r["common"][3] == len(qw) and not r["scored"][3]
    mx = max(r["common"][e] for e in range(40) if e != 3)
    assert r["stats"][0] == mx and r["stats"][1] == int(np.float32(mx) * np.float32(0.8))
    for e in range(40):
        if r["scored"][e]:
            assert r["score"][e] == literal_score(list(zip(qw, qx)), list(zip(*entries[e])))
        else:
            assert r["score"][e] == -5.0
    assert 0 < r["stats"][3] == r["scored"].sum() < r["stats"][2]
    assert B.l1_score(qw, qx, qw, qx) == literal_score(list(zip(qw, qx)), list(zip(qw, qx)))
    assert abs(B.l1_score(qw, qx, qw, qx) - 1.0) < 1e-12


# ---------------------------------------------------------------- the stream reader (host code of the library; no device)
def read(tmp_path, data):
    from rover_slam_amd import capi
    p = tmp_path / "voc.dbow3"
    p.write_bytes(data)
    return capi.read_bow_vocab(str(p))


def test_reader_returns_what_the_writer_wrote(tmp_path):
    for v in (B.make_vocab(10, 3, 256, seed=1), B.make_vocab(3, 2, 32, seed=2, weighting=B.IDF, bits01=False, stop_every=4), B.irregular_vocab()):
        got = read(tmp_path, B.stream_bytes(v))
        for k in ("k", "L", "weighting", "scoring", "n_nodes", "D"):
            assert got[k] == v[k], k
        for k in B.VOCAB_ARRAYS:
            a, b = (got[k][1:], v[k][1:]) if k in ("parent", "desc") else (got[k], v[k])     # the root has neither parent nor descriptor
            assert a.dtype == b.dtype and np.array_equal(a, b), k


def test_reader_refusals(tmp_path):
    from rover_slam_amd import capi
    v = B.make_vocab(3, 2, 32, seed=2)
    good = B.stream_bytes(v)
    with pytest.raises(capi.RfeError, match="compressed"):
        read(tmp_path, B.stream_bytes(v, compressed=1))
    for cut in (4, 12, 20, 29, 60, len(good) // 2, len(good) - 9, len(good) - 1):
        with pytest.raises(capi.RfeError, match="truncated|magic|more than the file"):
            read(tmp_path, good[:cut])
    with pytest.raises(capi.RfeError, match="more than the file can hold"):
        read(tmp_path, B.stream_bytes(v, nnodes=1 << 23))
    with pytest.raises(capi.RfeError, match="nnodes outside"):
        read(tmp_path, B.stream_bytes(v, nnodes=0xFFFFFFFF))
    with pytest.raises(capi.RfeError, match="not CV_8U"):
        read(tmp_path, B.stream_bytes(v, node_type=5))
    with pytest.raises(capi.RfeError, match="magic"):
        read(tmp_path, b"\0" * 64)
    with pytest.raises(capi.RfeError, match="cannot"):
        capi.read_bow_vocab(str(tmp_path / "missing.dbow3"))
    # a word table that names a node outside the tree, and a node id met twice
    bad = bytearray(good); bad[-4:] = (10 ** 6).to_bytes(4, "little")
    with pytest.raises(capi.RfeError, match="out of range"):
        read(tmp_path, bytes(bad))
    rec = 13 + 16
    bad = bytearray(good); bad[rec + 28 + 32:rec + 28 + 32 + 4] = bad[rec:rec + 4]
    with pytest.raises(capi.RfeError, match="occurs twice"):
        read(tmp_path, bytes(bad))
    assert read(tmp_path, good)["n_nodes"] == v["n_nodes"]                # and the same bytes untouched are taken
