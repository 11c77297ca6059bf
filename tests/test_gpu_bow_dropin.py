"""GPU: the drop-ins of include/rfe/bow.h (ComputeBoW3_rfe, AddKeyFrame_rfe, ScoreKeyFrames_rfe) over mock DBoW3 classes and plain std::map
(tests/cpp/bow_driver.cpp, -std=c++14 -Wall -Werror) against the restatement tests/bow_ref.py: the two maps bit for bit, and the
(entry, (float)score) list of the two Detect... functions."""
import shutil

import numpy as np
import pytest

import bow_ref as B
import dropin_driver as DD

pytestmark = pytest.mark.gpu


def write_case(path, v, frames, levelsup, exclude):
    f32 = frames[0].dtype == np.float32
    with open(path, "wb") as f:
        np.array([v["k"], v["L"], v["weighting"], v["scoring"], v["n_nodes"], v["D"], int(f32), levelsup, len(frames)], np.int32).tofile(f)
        for k, dt in (("parent", np.int32), ("child_offsets", np.int32), ("children", np.int32), ("desc", np.uint8), ("weight", np.float64),
                      ("word_id", np.int32)):
            np.ascontiguousarray(v[k], dt).tofile(f)
        for d in frames:
            np.array([len(d)], np.int32).tofile(f)
            np.ascontiguousarray(d).tofile(f)
        np.array([len(exclude)], np.int32).tofile(f)
        np.ascontiguousarray(exclude, np.uint8).tofile(f)


def read_out(path):
    raw = np.fromfile(path, np.uint8)
    o = 0

    def take(n, dt):
        nonlocal o
        a = raw[o:o + n * np.dtype(dt).itemsize].view(dt); o += a.nbytes
        return a
    out = {"status": int(take(1, np.int32)[0])}
    nb = int(take(1, np.int32)[0])
    out["bow_word"], out["bow_value"] = take(nb, np.int32), take(nb, np.float64)
    out["fv"] = []
    for _ in range(int(take(1, np.int32)[0])):
        node, cnt = (int(x) for x in take(2, np.int32))
        out["fv"].append((node, take(cnt, np.int32).tolist()))
    out["agree"] = int(take(1, np.int32)[0])
    ns = int(take(1, np.int32)[0])
    rec = take(2 * max(ns, 0), np.int32).reshape(-1, 2)
    out["entries"], out["scores"] = rec[:, 0].copy(), rec[:, 1].copy().view(np.float32)
    out["n_scored"], out["stats"] = ns, take(4, np.int32)
    assert o == len(raw)
    return out


def run_and_compare(exe, tmp_path, v, frames, levelsup, exclude, stream=None):
    write_case(str(tmp_path / "case.bin"), v, frames, levelsup, exclude)
    DD.run(exe, str(tmp_path / "case.bin"), str(tmp_path / "out.bin"), *([stream] if stream else []))
    got = read_out(str(tmp_path / "out.bin"))
    u8 = [B.binarize(d) if d.dtype == np.float32 else d for d in frames]
    ref = B.transform(v, u8[0], levelsup)
    assert got["status"] == len(ref["bow_word"]) and got["agree"] == 1
    assert np.array_equal(got["bow_word"], ref["bow_word"]) and np.array_equal(got["bow_value"].view(np.uint64), ref["bow_value"].view(np.uint64))
    ref_fv = [(int(n), ref["fv_feat"][ref["fv_offsets"][i]:ref["fv_offsets"][i + 1]].tolist()) for i, n in enumerate(ref["fv_node"])]
    assert got["fv"] == ref_fv
    entries = []
    for d in u8[1:]:
        t = B.transform(v, d, levelsup)
        entries.append((t["bow_word"], t["bow_value"]))
    q = B.db_query(entries, ref["bow_word"], ref["bow_value"], exclude if len(exclude) else None)
    assert np.array_equal(got["stats"], q["stats"]) and got["n_scored"] == q["stats"][3]
    assert np.array_equal(got["entries"], np.nonzero(q["scored"])[0])
    assert np.array_equal(got["scores"].view(np.uint32), q["score"][q["scored"] > 0].astype(np.float32).view(np.uint32))
    return ref, q


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_drop_in_bow_and_scores(tmp_path):
    exe = DD.build(tmp_path, "bow_driver")
    rng = np.random.default_rng(3)
    # SuperPoint-like float descriptors, D = 256, the vocabulary handed over as arrays
    v = B.make_vocab(6, 3, 256, seed=4, stop_every=11)
    pool = rng.standard_normal((1500, 256)).astype(np.float32)
    pool[rng.integers(0, 1500, 200), rng.integers(0, 256, 200)] = np.nan
    frames = [pool[rng.permutation(1500)[:rng.integers(200, 500)]] for _ in range(9)]
    frames.append(frames[0][::-1].copy())                                # keyframe 8: the query's features in another order
    frames.append(pool[:0])                                              # keyframe 9: no features at all
    exclude = np.zeros((len(frames) - 1,), np.uint8); exclude[3] = 1
    ref, q = run_and_compare(exe, tmp_path, v, frames, 1, exclude)
    assert len(ref["bow_word"]) > 50 and q["scored"][8] and q["common"][9] == 0 and 0 < q["stats"][3] < len(frames) - 1
    # byte descriptors of D = 32, the vocabulary loaded from a DBoW3 stream file, nothing excluded
    v = B.make_vocab(4, 3, 32, seed=5, weighting=B.IDF, bits01=False)
    stream = tmp_path / "voc.dbow3"
    stream.write_bytes(B.stream_bytes(v))
    pool = B.random_desc(rng, (600, 32), False)
    frames = [pool[rng.permutation(600)[:rng.integers(50, 300)]] for _ in range(6)]
    run_and_compare(exe, tmp_path, v, frames, 0, np.zeros((0,), np.uint8), stream=str(stream))
