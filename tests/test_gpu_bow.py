"""GPU: ComputeBoW3 and the keyframe database's scores on the device (rfe_bow_transform / _dev, rfe_bow_db_*) against the
restatement tests/bow_ref.py.  Every comparison is exact: np.array_equal on every output, float64 values bit for bit, in host and device
form, with sentinels behind the counts."""
import functools

import numpy as np
import pytest

import bow_ref as B

pytestmark = pytest.mark.gpu
SENT = {np.dtype(np.int32): -77, np.dtype(np.float64): -123.25, np.dtype(np.uint8): 201}


@pytest.fixture(scope="module")
def ctx():
    from rover_slam_amd import capi            # not at import time: collection must not load the library in front of the modules that load torch
    c = capi.Context(0)
    yield c
    c.close()


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def same(got, ref):
    for k in B.KEYS:
        assert got[k].dtype == ref[k].dtype == B.DTYPES[k] and got[k].shape == ref[k].shape, (k, got[k].shape, ref[k].shape)
        a, b = (bits(got[k]), bits(ref[k])) if B.DTYPES[k] == np.float64 else (got[k], ref[k])
        assert np.array_equal(a, b), (k, np.argwhere(a != b)[:8].ravel(), got[k][:4], ref[k][:4])


def transform_dev(ctx, vocab, desc, levelsup):
    """rfe_bow_transform_dev on an uploaded copy of desc, every output preset to a sentinel; returns the host form's dict and checks that
    nothing behind the counts was written"""
    N = len(desc)
    n1 = max(N, 1)
    sizes = {"word": n1, "node": n1, "weight": n1, "bow_n": 1, "bow_word": n1, "bow_value": n1, "fv_n": 1, "fv_node": n1, "fv_offsets": n1 + 1,
             "fv_feat": n1}
    dt = dict(B.DTYPES, bow_n=np.int32, fv_n=np.int32)
    out = {k: ctx.alloc(n * np.dtype(dt[k]).itemsize).upload(np.full((n,), SENT[np.dtype(dt[k])], dt[k])) for k, n in sizes.items()}
    d = ctx.alloc(max(desc.nbytes, 16))
    if desc.nbytes:
        d.upload(desc)
    try:
        ctx.bow_transform_dev(vocab, N, levelsup, **{k: out[k] for k in sizes}, **{"desc_f32" if desc.dtype == np.float32 else "desc_u8": d})
        ctx.synchronize()
        raw = {k: out[k].download((n,), dt[k]) for k, n in sizes.items()}
    finally:
        for b in list(out.values()) + [d]:
            b.free()
    nb, nf = int(raw["bow_n"][0]), int(raw["fv_n"][0])
    assert 0 <= nb <= N and 0 <= nf <= N
    kept = int(raw["fv_offsets"][nf])
    cut = {"word": N, "node": N, "weight": N, "bow_word": nb, "bow_value": nb, "fv_node": nf, "fv_offsets": nf + 1, "fv_feat": kept}
    for k, n in cut.items():
        assert (raw[k][n:] == SENT[np.dtype(dt[k])]).all(), f"{k} written past {n}"
    return {k: raw[k][:n] for k, n in cut.items()}


def check(ctx, v, desc, levelsup=0, vocab=None):
    """host and device form against the restatement; desc float32 [N,256] or uint8 [N,D]"""
    from rover_slam_amd import capi
    own = vocab is None
    vocab = capi.BowVocab(ctx, v) if own else vocab
    try:
        ref = B.transform(v, B.binarize(desc) if desc.dtype == np.float32 else desc, levelsup)
        same(ctx.bow_transform(vocab, desc, levelsup), ref)
        same(transform_dev(ctx, vocab, desc, levelsup), ref)
    finally:
        if own:
            vocab.close()
    return ref


@functools.lru_cache(maxsize=None)
def big_vocab():
    return B.make_vocab(10, 3, 256, seed=1, stop_every=7)


@functools.lru_cache(maxsize=None)
def big_desc():
    """4096 SuperPoint-like float descriptors: a quarter lies near a node of the vocabulary, and zeros, negative zeros and NaNs are planted"""
    rng = np.random.default_rng(2)
    v = big_vocab()
    d = rng.standard_normal((4096, 256)).astype(np.float32)
    near = rng.integers(0, 4096, 1024)
    d[near] = (v["desc"][rng.integers(1, v["n_nodes"], 1024)].astype(np.float32) * 2 - 1) * np.abs(d[near])
    d[rng.integers(0, 4096, 3000), rng.integers(0, 256, 3000)] = 0.0
    d[rng.integers(0, 4096, 3000), rng.integers(0, 256, 3000)] = -0.0
    d[rng.integers(0, 4096, 3000), rng.integers(0, 256, 3000)] = np.nan
    d[0, :3] = (0.0, -0.0, np.nan)
    return d


# ---------------------------------------------------------------- 1. transform
def test_hand_written_case(ctx):
    """k = 3, L = 2, D = 8, five features, every number worked out by hand"""
    b = B.TreeBuilder(3, 2, 8)
    n1, n2, n3 = b.add(0, [0, 0, 0, 0, 0, 0, 0, 0]), b.add(0, [1, 1, 1, 1, 0, 0, 0, 0]), b.add(0, [1, 1, 1, 1, 1, 1, 1, 1])
    leaves = [(n1, [0, 0, 0, 0, 0, 0, 0, 0], 1.5), (n1, [0, 0, 0, 0, 0, 0, 1, 1], 0.0), (n1, [0, 0, 0, 0, 1, 1, 0, 0], 0.25),
              (n2, [1, 1, 1, 1, 0, 0, 0, 0], 2.0), (n2, [1, 1, 1, 1, 0, 0, 1, 1], 0.75), (n2, [1, 1, 1, 1, 1, 1, 0, 0], 1.0),
              (n3, [1, 1, 1, 1, 1, 1, 1, 1], 0.5), (n3, [1, 1, 1, 1, 1, 1, 0, 0], 3.0), (n3, [0, 0, 1, 1, 1, 1, 1, 1], 1.25)]
    for p, d, w in leaves:
        b.add(p, d, w)
    v = b.finish()
    feats = np.array([[0, 0, 0, 0, 0, 0, 0, 1],      # node 1 (1 / 5 / 7); leaves 4 and 5 both at 1: the first, word 0
                      [0, 0, 0, 0, 0, 0, 1, 1],      # node 1, leaf 5 at 0: word 1, a stop word
                      [1, 1, 1, 1, 0, 0, 1, 1],      # nodes 2 and 3 both at 2: node 2; leaf 8 at 0: word 4
                      [1, 1, 1, 1, 1, 1, 1, 1],      # node 3, leaf 10: word 6
                      [0, 0, 0, 0, 0, 0, 0, 0]], np.uint8)   # node 1, leaf 4: word 0
    from rover_slam_amd import capi
    vocab = capi.BowVocab(ctx, v)
    assert (vocab.k, vocab.L, vocab.n_nodes, vocab.n_words, vocab.D, vocab.depth) == (3, 2, 13, 9, 8, 2)
    for got in (ctx.bow_transform(vocab, feats, 1), transform_dev(ctx, vocab, feats, 1)):
        assert got["word"].tolist() == [0, 1, 4, 6, 0] and got["node"].tolist() == [1, 1, 2, 3, 1]
        assert got["weight"].tolist() == [1.5, 0.0, 0.75, 0.5, 1.5]
        assert got["bow_word"].tolist() == [0, 4, 6]
        assert got["bow_value"].tolist() == [(1.5 + 1.5) / 4.25, 0.75 / 4.25, 0.5 / 4.25]
        assert got["fv_node"].tolist() == [1, 2, 3] and got["fv_offsets"].tolist() == [0, 2, 3, 4] and got["fv_feat"].tolist() == [0, 4, 2, 3]
    assert ctx.bow_transform(vocab, feats, 0)["node"].tolist() == [4, 5, 8, 10, 4]
    assert ctx.bow_transform(vocab, feats, 2)["node"].tolist() == [0] * 5
    same(ctx.bow_transform(vocab, feats, 1), B.transform(v, feats, 1))
    vocab.close()


@pytest.mark.parametrize("N", [1, 63, 65, 1100, 4096])
def test_superpoint_descriptors_f32_and_u8(ctx, N):
    from rover_slam_amd import capi
    v, d = big_vocab(), big_desc()[:N]
    vocab = capi.BowVocab(ctx, v)
    ref = check(ctx, v, d, 1, vocab)                                                    # f32: zeros, negative zeros and NaNs are 0 bits
    same(transform_dev(ctx, vocab, B.binarize(d), 1), ref)                              # u8
    same(ctx.bow_transform(vocab, B.binarize(d), 1), ref)
    if N >= 1100:
        assert len(ref["bow_word"]) < (ref["weight"] > 0).sum() and (ref["weight"] == 0).any() and len(ref["fv_node"]) > 50
    # the same call twice on the same ctx gives the same bits
    same(transform_dev(ctx, vocab, d, 1), ref)
    vocab.close()


def test_arbitrary_bytes_d32(ctx):
    rng = np.random.default_rng(4)
    v = B.make_vocab(5, 3, 32, seed=6, bits01=False, stop_every=9)
    feats = B.random_desc(rng, (300, 32), False)
    feats[:100] = v["desc"][rng.integers(1, v["n_nodes"], 100)] ^ (rng.random((100, 32)) < 0.05).astype(np.uint8)
    ref = check(ctx, v, feats, 0)
    assert len(ref["bow_word"]) < (ref["weight"] > 0).sum()
    check(ctx, B.make_vocab(3, 2, 24, seed=8, bits01=False), B.random_desc(rng, (70, 24), False), 1)     # D = 24: the last 16-byte piece is half full


def test_ties_keep_the_first_child_and_exact_hits(ctx):
    rng = np.random.default_rng(12)
    v = B.make_vocab(4, 2, 32, seed=13, bits01=False)
    kids = lambda i: v["children"][v["child_offsets"][i]:v["child_offsets"][i + 1]]   # noqa: E731
    a, b = kids(0)[1], kids(0)[3]
    v["desc"][b] = v["desc"][a]                                       # two children of the root alike: the earlier one is taken
    la, lb = kids(a)[0], kids(a)[2]
    v["desc"][la] = v["desc"][lb] = v["desc"][a]                      # and two leaves under it, both equal to their parent
    feats = np.concatenate([v["desc"][[a, la, kids(b)[1]]], v["desc"][1:], B.random_desc(rng, (40, 32), False)])
    ref = check(ctx, v, feats, 1)
    assert ref["node"][0] == a and ref["word"][0] == v["word_id"][la] and ref["word"][1] == v["word_id"][la]
    # every feature equal to a root child's descriptor takes that child, or its earlier twin
    for c in kids(0):
        assert ref["node"][3 + c - 1] == (a if c == b else c)


@pytest.mark.parametrize("levelsup", [0, 1, 2, 3, 4])
def test_irregular_tree(ctx, levelsup):
    v = B.irregular_vocab()
    feats = np.array([[0] * 8, [1] * 8, [1, 1, 1, 1, 0, 0, 0, 0], [1, 1, 1, 1, 1, 1, 0, 0], [0, 1, 1, 1, 1, 1, 1, 1], [0, 0, 0, 0, 0, 0, 0, 1]], np.uint8)
    ref = check(ctx, v, feats, levelsup)
    assert ref["node"][0] == (0 if levelsup >= 3 else 1)              # the depth-1 leaf: its own id wherever depth L - levelsup lies below it


def test_stop_words_and_everything_stopped(ctx):
    rng = np.random.default_rng(20)
    v = B.make_vocab(4, 2, 32, seed=21, stop_every=2)
    feats = B.random_desc(rng, (200, 32), True)
    ref = check(ctx, v, feats, 0)
    assert 0 < (ref["weight"] == 0).sum() < 200
    v["weight"][:] = 0.0
    ref = check(ctx, v, feats, 0)
    assert len(ref["bow_word"]) == 0 and len(ref["fv_node"]) == 0 and ref["fv_offsets"].tolist() == [0] and len(ref["fv_feat"]) == 0
    ref = check(ctx, v, feats[:0], 0)                                 # N == 0
    assert len(ref["word"]) == 0 and ref["fv_offsets"].tolist() == [0]


def test_long_chain_on_one_word(ctx):
    v, feats, w = B.one_word_case()
    ref = check(ctx, v, feats, 0)
    chain = 0.0
    for _ in range(700):
        chain += w
    assert ref["bow_value"][0] == chain / (chain + 0.3) and chain != 700 * w
    ref = check(ctx, v, np.zeros((4096, 8), np.uint8), 0)             # the longest run there can be: one thread adds 4096 weights
    assert len(ref["bow_word"]) == 1 and ref["bow_value"][0] == 1.0 and ref["fv_offsets"].tolist() == [0, 4096]


@pytest.mark.parametrize("weighting", [B.TF_IDF, B.TF, B.IDF, B.BINARY])
def test_weightings(ctx, weighting):
    rng = np.random.default_rng(30 + weighting)
    v = B.make_vocab(3, 3, 64, seed=31, weighting=weighting, stop_every=6)
    if weighting == B.IDF:
        assert len(set(v["weight"].tolist())) > 10
    feats = B.random_desc(rng, (500, 64), True)
    ref = check(ctx, v, feats, 2)
    assert len(ref["bow_word"]) < (ref["weight"] > 0).sum()


def test_refusals(ctx):
    from rover_slam_amd import capi
    v = B.make_vocab(3, 2, 32, seed=40)
    vocab = capi.BowVocab(ctx, v)
    with pytest.raises(capi.RfeError, match="N outside"):
        ctx.bow_transform(vocab, np.zeros((4097, 32), np.uint8))
    with pytest.raises(capi.RfeError, match="D = 256"):
        ctx.bow_transform(vocab, np.zeros((4, 256), np.float32))
    vocab.close()

    def refused(match, **kw):
        bad = {k: (a.copy() if isinstance(a, np.ndarray) else a) for k, a in v.items()}
        for k, f in kw.items():
            bad[k] = f(bad[k]) if callable(f) else f
        with pytest.raises(capi.RfeError, match=match):
            capi.BowVocab(ctx, bad)

    def put(i, x):
        def f(a):
            a[i] = x
            return a
        return f
    refused("L1_NORM", scoring=1)
    refused("multiple of 8", D=12)
    refused("multiple of 8", D=264)
    refused("out of range", children=put(2, 13))
    refused("out of range", children=put(2, 0))
    refused("two parents", children=put(2, int(v["children"][5])))
    refused("no word id", word_id=put(12, -1))
    refused("disagrees", parent=put(5, 2))
    # nodes 4 and 5 as each other's only child: neither hangs on the root any more
    loop = B.TreeBuilder(2, 2, 8)
    for p in (0, 0, 1, 1):
        loop.add(p, np.zeros(8, np.uint8), 1.0)
    lv = loop.finish()
    lv["child_offsets"] = np.array([0, 2, 2, 2, 3, 4], np.int32); lv["children"] = np.array([1, 2, 4, 3], np.int32)
    lv["parent"] = np.array([-1, 0, 0, 4, 3], np.int32); lv["word_id"] = np.arange(5, dtype=np.int32)
    with pytest.raises(capi.RfeError, match="cannot be reached"):
        capi.BowVocab(ctx, lv)


def test_vocabulary_from_a_stream_file(ctx, tmp_path):
    from rover_slam_amd import capi
    v = B.make_vocab(4, 2, 32, seed=50, bits01=False)
    p = tmp_path / "voc.dbow3"
    p.write_bytes(B.stream_bytes(v))
    vocab = capi.BowVocab(ctx, path=str(p))
    feats = B.random_desc(np.random.default_rng(51), (90, 32), False)
    check(ctx, v, feats, 1, vocab)
    vocab.close()
    p.write_bytes(B.stream_bytes(v, compressed=1))
    with pytest.raises(capi.RfeError, match="uncompressed"):
        capi.BowVocab(ctx, path=str(p))


# ---------------------------------------------------------------- 2. the keyframe database
def random_entries(rng, E, n_words=3000, max_len=1024):
    out = []
    for e in range(E):
        n = int(rng.integers(0, max_len + 1))
        w = np.sort(rng.choice(n_words, n, replace=False)).astype(np.int32)
        x = rng.random(n) + 1e-3
        out.append((w, x / B.sequential_sum(x) if n else x))
    return out


def db_same(got, ref):
    assert np.array_equal(got["stats"], ref["stats"]), (got["stats"], ref["stats"])
    for k in ("common", "scored"):
        assert got[k].dtype == ref[k].dtype and np.array_equal(got[k], ref[k]), (k, np.argwhere(got[k] != ref[k])[:8].ravel())
    assert np.array_equal(bits(got["score"]), bits(ref["score"])), np.argwhere(bits(got["score"]) != bits(ref["score"]))[:8].ravel()


def query_dev(ctx, db, qw, qx, exclude, score):
    E = len(db)
    up = lambda a, dt: ctx.alloc(max(np.asarray(a).size, 1) * np.dtype(dt).itemsize + 8).upload(np.ascontiguousarray(a, dt))   # noqa: E731
    bufs = {"w": up(qw, np.int32), "x": up(qx, np.float64), "common": up(np.full((E + 1,), -77), np.int32), "scored": up(np.full((E + 1,), 201), np.uint8),
            "score": up(np.r_[score, -123.25], np.float64), "stats": up(np.full((4,), -77), np.int32)}
    if exclude is not None:
        bufs["ex"] = up(exclude, np.uint8)
    try:
        db.query_dev(bufs["w"], bufs["x"], len(qw), bufs["common"], bufs["scored"], bufs["score"], bufs["stats"], exclude=bufs.get("ex"))
        ctx.synchronize()
        got = {"common": bufs["common"].download((E + 1,), np.int32), "scored": bufs["scored"].download((E + 1,), np.uint8),
               "score": bufs["score"].download((E + 1,), np.float64), "stats": bufs["stats"].download((4,), np.int32)}
    finally:
        for b in bufs.values():
            b.free()
    assert got["common"][E] == -77 and got["scored"][E] == 201 and got["score"][E] == -123.25      # nothing past the last entry id
    return {k: (a[:E] if k != "stats" else a) for k, a in got.items()}


def db_check(ctx, db, entries, qw, qx, exclude=None):
    score = np.full((len(entries),), -9.5)
    ref = B.db_query(entries, qw, qx, exclude, score)
    db_same(db.query(qw, qx, exclude, score), ref)
    db_same(query_dev(ctx, db, qw, qx, exclude, score), ref)
    return ref


@pytest.mark.parametrize("E", [0, 1, 65, 1000])
def test_database_sizes(ctx, E):
    """0..1024 words per entry; 1000 entries pass both initial capacities (65536 words, 256 entries); adds in host and device form"""
    from rover_slam_amd import capi
    rng = np.random.default_rng(60 + E)
    entries = random_entries(rng, E)
    db = capi.BowDatabase(ctx)
    for e, (w, x) in enumerate(entries):
        if e % 3 == 2 and len(w):
            bw, bx = ctx.alloc(w.nbytes).upload(w), ctx.alloc(x.nbytes).upload(x)
            assert db.add_dev(bw, bx, len(w)) == e
            ctx.synchronize(); bw.free(); bx.free()
        else:
            assert db.add(w, x) == e
    assert len(db) == E
    qw, qx = random_entries(rng, 1, max_len=900)[0]
    ref = db_check(ctx, db, entries, qw, qx)
    if E >= 65:
        assert 0 < ref["stats"][3] < ref["stats"][2]
        # a query equal to an entry: every word is common, the score is that of a vector with itself
        big = int(np.argmax([len(w) for w, _ in entries]))
        ref = db_check(ctx, db, entries, *entries[big])
        assert ref["stats"][0] == len(entries[big][0]) and ref["scored"][big] and abs(ref["score"][big] - 1.0) < 1e-12
        # an add after a query, an erased entry, and the entry with the largest count excluded
        entries.append(entries[big]); assert db.add(*entries[big]) == E
        db.erase(5); entries[5] = None
        ex = np.zeros((E + 1,), np.uint8); ex[big] = 1
        ref = db_check(ctx, db, entries, *entries[E], exclude=ex)
        assert ref["common"][5] == 0 and ref["common"][big] == ref["stats"][0] and not ref["scored"][big] and ref["scored"][E]
        ex[E] = 1
        ref = db_check(ctx, db, entries, *entries[E], exclude=ex)
        assert ref["stats"][0] < ref["common"][big]
    db.clear()
    assert len(db) == 0
    db_check(ctx, db, [], qw, qx)
    assert db.add(qw, qx) == 0
    db_check(ctx, db, [(qw, qx)], qw, qx)
    db.close()


def test_database_planted_counts(ctx):
    """max_common = 100, so min_common = (int)(100 * 0.8f) = 80: the entry with 80 common words is not scored, the one with 81 is"""
    from rover_slam_amd import capi
    rng = np.random.default_rng(70)
    qw = np.arange(0, 200, 2, dtype=np.int32); qx = rng.random(100); qx /= B.sequential_sum(qx)
    entries = []
    for c in (100, 80, 81, 79, 0, 1):
        w = np.sort(np.r_[qw[rng.choice(100, c, replace=False)], 1 + 2 * rng.choice(400, 50, replace=False)]).astype(np.int32)
        x = rng.random(len(w)); entries.append((w, x / B.sequential_sum(x)))
    db = capi.BowDatabase(ctx)
    for w, x in entries:
        db.add(w, x)
    ref = db_check(ctx, db, entries, qw, qx)
    assert ref["common"].tolist() == [100, 80, 81, 79, 0, 1] and ref["stats"].tolist() == [100, 80, 5, 2] and ref["scored"].tolist() == [1, 0, 1, 0, 0, 0]
    # the largest excluded: max_common = 81, min_common = 64
    ref = db_check(ctx, db, entries, qw, qx, exclude=np.array([1, 0, 0, 0, 0, 0], np.uint8))
    assert ref["stats"].tolist() == [81, 64, 4, 3] and ref["scored"].tolist() == [0, 1, 1, 1, 0, 0]
    # a query that shares no word with anybody: nothing is scored, the scores stay as they were
    ref = db_check(ctx, db, entries, np.array([100001, 100003], np.int32), np.array([0.5, 0.5]))
    assert ref["stats"].tolist() == [0, 0, 0, 0] and (ref["score"] == -9.5).all()
    ref = db_check(ctx, db, entries, qw[:0], qx[:0])
    assert ref["stats"].tolist() == [0, 0, 0, 0]
    db.close()


def test_transform_feeds_the_database(ctx):
    """the device path end to end: descriptors -> BoW vectors -> entries -> scores, nothing but the counts read back in between"""
    from rover_slam_amd import capi
    v = big_vocab()
    vocab, db = capi.BowVocab(ctx, v), capi.BowDatabase(ctx)
    rng = np.random.default_rng(80)
    frames = [big_desc()[rng.permutation(4096)[:600]] for _ in range(6)]
    frames.append(frames[2][::-1].copy())                               # the same features in another order
    entries = []
    for d in frames[:6]:
        r = ctx.bow_transform(vocab, d, 1)
        entries.append((r["bow_word"], r["bow_value"]))
        db.add(r["bow_word"], r["bow_value"])
    q = ctx.bow_transform(vocab, frames[6], 1)
    ref = db_check(ctx, db, entries, q["bow_word"], q["bow_value"])
    assert np.array_equal(q["bow_word"], entries[2][0]) and ref["scored"][2] and ref["score"][2] == ref["score"].max() > 0.99
    db.close(); vocab.close()
