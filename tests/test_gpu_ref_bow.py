"""GPU: the place-recognition kernels (rfe_bow_vocab_load, rfe_bow_transform / _dev, rfe_bow_db_*) against what DBoW3's and
KeyFrameDatabase's OWN C++ computed, as recorded in tests/golden/ref_bow_*.npz (tools/gen_ref_golden.py --only bow; tests/test_ref_bow.py
holds the numpy restatement to the same recordings and says how the two documented departures -- the unwritten *nid, the connected
keyframe's counter -- are scoped).  Fixtures only: neither the reference checkout nor oracle/_ref/ is needed.  Every comparison is exact:
np.array_equal, float64 on the bit patterns, the (float) score on its 32 bits; outputs are preset to sentinels and checked behind the
counts."""
import contextlib

import numpy as np
import pytest

import bow_ref as B
import ref_bow_cases as BC
import ref_classic_cases as RC
import test_gpu_bow as T
import test_ref_bow as TR

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from rover_slam_amd import capi            # not at import time: collection must not load the library in front of the modules that load torch
    c = capi.Context(0)
    yield c
    c.close()


@contextlib.contextmanager
def loaded(ctx, tmp_path, stream):
    """the vocabulary of a recorded stream; closed on the way out, pass or fail, so that it never outlives the ctx it hangs on"""
    from rover_slam_amd import capi
    p = tmp_path / "voc.dbow3"
    p.write_bytes(bytes(stream))
    vocab = capi.BowVocab(ctx, path=str(p))
    try:
        yield vocab
    finally:
        vocab.close()


def transform_host(ctx, vocab, desc, levelsup):
    """rfe_bow_transform on host arrays preset to sentinels; checks that nothing behind the counts was written"""
    from rover_slam_amd import capi
    N, n1 = len(desc), max(len(desc), 1)
    sizes = {"word": n1, "node": n1, "weight": n1, "bow_n": 1, "bow_word": n1, "bow_value": n1, "fv_n": 1, "fv_node": n1, "fv_offsets": n1 + 1,
             "fv_feat": n1}
    dt = dict(B.DTYPES, bow_n=np.int32, fv_n=np.int32)
    o = {k: np.full((n,), T.SENT[np.dtype(dt[k])], dt[k]) for k, n in sizes.items()}
    d = np.ascontiguousarray(desc)
    f32, u8 = (d.ctypes.data, None) if d.dtype == np.float32 else (None, d.ctypes.data)
    ctx._chk(capi.lib.rfe_bow_transform(ctx.h, vocab.h, f32, u8, N, int(levelsup), *[o[k].ctypes.data for k in sizes]))
    nb, nf = int(o["bow_n"][0]), int(o["fv_n"][0])
    assert 0 <= nb <= N and 0 <= nf <= N
    cut = {"word": N, "node": N, "weight": N, "bow_word": nb, "bow_value": nb, "fv_node": nf, "fv_offsets": nf + 1, "fv_feat": int(o["fv_offsets"][nf])}
    for k, n in cut.items():
        assert (o[k][n:] == T.SENT[np.dtype(dt[k])]).all(), f"{k} written past {n}"
    return {k: o[k][:n] for k, n in cut.items()}


# ---------------------------------------------------------------- load
@pytest.mark.parametrize("name", BC.VOCABS)
def test_load_recorded_stream(ctx, tmp_path, name):
    z, v, _ = BC.load_vocab(name)
    with loaded(ctx, tmp_path, z["stream"]) as vocab:
        got = (vocab.k, vocab.L, vocab.n_nodes, vocab.n_words, vocab.D, vocab.weighting, vocab.scoring, vocab.depth)
    assert got == (v["k"], v["L"], v["n_nodes"], v["n_words"], v["D"], v["weighting"], v["scoring"], int(BC.leaf_depths(v).max())), got


def test_compressed_stream_is_refused(ctx, tmp_path):
    from rover_slam_amd import capi
    z = RC.load("bow_oneword")
    with pytest.raises(capi.RfeError, match=r"error -4: .*compressed"):      # RFE_ERR_IO
        with loaded(ctx, tmp_path, z["stream_compressed"]):
            pass


# ---------------------------------------------------------------- transform
@pytest.mark.parametrize("name", BC.VOCABS)
def test_transform_u8(ctx, tmp_path, name):
    z, v, cases = BC.load_vocab(name)
    with loaded(ctx, tmp_path, z["stream"]) as vocab:
        for i, feats, levelsup in cases:
            check = TR.check_transform(v, feats, levelsup, BC.recorded(z, i), BC.fv_defined(v, levelsup))
            check(transform_host(ctx, vocab, feats, levelsup))
            check(T.transform_dev(ctx, vocab, feats, levelsup))


def floats_of(bits, seed):
    """float32 descriptors that binarize to `bits`: a 1 from positive values down to the smallest denormal, a 0 from 0.0, -0.0, negative
    values, a negative denormal and NaN"""
    rng = np.random.default_rng(seed)
    one = np.array([1.0, 0.37, 3e38, 1.1754944e-38, 1e-45], np.float32)
    zero = np.array([0.0, -0.0, -1.0, -1e-45, np.nan, -np.inf], np.float32)
    f = np.where(bits > 0, one[rng.integers(0, len(one), bits.shape)], zero[rng.integers(0, len(zero), bits.shape)]).astype(np.float32)
    if f.size:
        k = min(3, f.shape[0])
        f[:k, :6] = np.where(bits[:k, :6] > 0, np.float32(1e-45), np.array([0.0, -0.0, np.nan, -1e-45, -0.0, np.nan], np.float32))
    with np.errstate(invalid="ignore"):
        assert np.array_equal((f > 0).astype(np.uint8), bits)
    return f


def test_transform_f32_entry(ctx, tmp_path):
    z, v, cases = BC.load_vocab("k6L3D256")
    planted = 0
    with loaded(ctx, tmp_path, z["stream"]) as vocab:
        for i, feats, levelsup in cases:
            f = floats_of(feats, 300 + i)
            planted += int(np.isnan(f).sum() > 0 and (np.signbit(f) & (f == 0)).sum() > 0 and ((f != 0) & (np.abs(f) < 1e-38)).sum() > 0)
            check = TR.check_transform(v, feats, levelsup, BC.recorded(z, i), True)
            check(transform_host(ctx, vocab, f, levelsup))
            check(T.transform_dev(ctx, vocab, f, levelsup))
    assert planted >= len(cases) - 1                                         # all but N = 0 hold a NaN, a negative zero and a denormal


# ---------------------------------------------------------------- the keyframe database
@pytest.mark.parametrize("name", ["empty", "one", "grow", "gate"])
def test_database_replays_the_recorded_script(ctx, name):
    from rover_slam_amd import capi
    s, ref = BC.unpack_script(RC.load("bow_kfdb"), name)
    db = capi.BowDatabase(ctx)
    try:                                                             # closed pass or fail: a database must not outlive its ctx
        added, q = 0, 0
        replay = BC.replay(s)
        for op, arg in s["ops"]:
            if op == BC.ADD:
                w, x = s["bows"][arg]
                if added % 3 == 2:
                    bw, bx = ctx.alloc(w.nbytes).upload(w), ctx.alloc(x.nbytes).upload(x)
                    assert db.add_dev(bw, bx, len(w)) == added
                    ctx.synchronize(); bw.free(); bx.free()
                else:
                    assert db.add(w, x) == added
                added += 1
            elif op == BC.ERASE:
                db.erase(arg)
            else:
                rq, _, entries, (qw, qx), ex = next(replay)
                assert rq == q and len(db) == len(entries) == added
                keep = np.full((added,), -9.5)
                for got in (db.query(qw, qx, ex if op == BC.QUERY_SP else None, keep), T.query_dev(ctx, db, qw, qx, ex if op == BC.QUERY_SP else None, keep)):
                    assert got["common"].dtype == np.int32 and got["scored"].dtype == np.uint8 and got["score"].dtype == np.float64
                    on = TR.check_query(got, ref, q, ex)
                    assert (got["score"][~on] == -9.5).all()                     # not written where not scored
                q += 1
    finally:
        db.close()
    assert q == len(ref["stats"]) and added == ref["sharing"].shape[1]
