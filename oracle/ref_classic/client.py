"""Python side of oracle/_ref/ref_classic and oracle/_ref/ref_bow (built by build_ref.py): one child process per call, raw arrays through
two temporary files.  ref_classic runs the classic stages' bodies (stereo, geometry, distance, distinctive, normkp, binarize); ref_bow
is a second stand-alone program (ref_bow_main.cc, no Python in the process) around DBoW3's and KeyFrameDatabase's own bodies:
voc_dump / voc_write (Vocabulary::fromStream, toStream), transform (Vocabulary::transform), score (L1Scoring::score), kfdb
(KeyFrameDatabase::add / erase and the fronts of DetectNBestCandidates_sp / DetectRelocalizationCandidates).
Test and fixture-generation infrastructure only; nothing here runs on a GPU machine."""
import os
import struct
import subprocess
import tempfile

import numpy as np

from . import build_ref

_CODES = {np.dtype(np.uint8): 0, np.dtype(np.int32): 1, np.dtype(np.float32): 2, np.dtype(np.float64): 3}
_DTYPES = {v: k for k, v in _CODES.items()}


class RefError(RuntimeError):
    pass


def binary(sanitized=False, program="ref_classic"):
    return os.path.join(build_ref.OUT, program + ("_san" if sanitized else ""))


def usable(sanitized=False, program="ref_classic"):
    """the harness exists AND the checkout it was cut from is present (a leftover build without its source is not trusted)"""
    return os.path.isfile(binary(sanitized, program)) and build_ref.available()


def usable_bow(sanitized=False):
    return usable(sanitized, "ref_bow")


def _write(path, arrays):
    with open(path, "wb") as f:
        f.write(struct.pack("<i", len(arrays)))
        for a in arrays:
            a = np.ascontiguousarray(a)
            f.write(struct.pack("<iq", _CODES[a.dtype], a.size))
            f.write(a.tobytes())


def _read(path):
    with open(path, "rb") as f:
        raw = f.read()
    (count,), pos, out = struct.unpack_from("<i", raw, 0), 4, []
    for _ in range(count):
        code, n = struct.unpack_from("<iq", raw, pos)
        pos += 12
        dt = _DTYPES[code]
        out.append(np.frombuffer(raw, dt, n, pos).copy())
        pos += n * dt.itemsize
    return out


def run(op, arrays, sanitized=False, timeout=600, program="ref_classic"):
    exe = binary(sanitized, program)
    if not os.path.isfile(exe):
        raise RefError(f"{exe} is not built (python oracle/ref_classic/build_ref.py)")
    with tempfile.TemporaryDirectory() as d:
        fin, fout = os.path.join(d, "in"), os.path.join(d, "out")
        _write(fin, arrays)
        r = subprocess.run([exe, op, fin, fout], stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, timeout=timeout)
        if r.returncode != 0:
            raise RefError(f"{program} {op} ended with {r.returncode}: {r.stderr.decode(errors='replace')[-2000:]}")
        return _read(fout)


def _f(a, shape=None):
    a = np.ascontiguousarray(a, np.float32)
    return a if shape is None else a.reshape(shape)


def stereo(img_l, img_r, k_l, oct_l, k_r, oct_r, d_l, d_r, mb, mbf, nlevels=1, scale_factor=1.2, sanitized=False):
    """Frame::ComputeStereoMatches on level-0 images; returns (mvuRight [N], mvDepth [N])"""
    il, ir = np.ascontiguousarray(img_l, np.uint8), np.ascontiguousarray(img_r, np.uint8)
    H, W = il.shape
    kl, kr = _f(k_l, (-1, 2)), _f(k_r, (-1, 2))
    pi = np.array([H, W, nlevels, len(kl), len(kr)], np.int32)
    pf = np.array([mb, mbf, scale_factor], np.float32)
    u, z = run("stereo", [pi, pf, il, ir, kl, np.ascontiguousarray(oct_l, np.int32), kr, np.ascontiguousarray(oct_r, np.int32),
                          _f(d_l, (-1, 256)), _f(d_r, (-1, 256))], sanitized)
    return u, z


def geometry(H, W, nlevels, scale_factor, nfeatures=1000, sanitized=False):
    """SPextractor's constructor and ComputePyramid's level sizes: dict scale, inv, level_w, level_h, fpl"""
    s, inv, lw, lh, fpl = run("geometry", [np.array([H, W, nlevels, nfeatures], np.int32), np.array([scale_factor], np.float32)], sanitized)
    return {"scale": s, "inv": inv, "level_w": lw, "level_h": lh, "fpl": fpl}


def distance(a, b, sanitized=False):
    a, b = _f(a, (-1, 256)), _f(b, (-1, 256))
    return run("distance", [a, b], sanitized)[0].reshape(len(a), len(b))


def distinctive(desc, offsets, sanitized=False):
    return run("distinctive", [_f(desc, (-1, 256)), np.ascontiguousarray(offsets, np.int32)], sanitized)[0]


def normalize_keypoints(kpts, h, w, sanitized=False):
    k = _f(kpts, (-1, 2))
    return run("normkp", [k, np.array([h, w], np.int32)], sanitized)[0].reshape(-1, 2)


def binarize(desc, sanitized=False):
    d = _f(desc, (-1, 256))
    return run("binarize", [d], sanitized)[0].reshape(-1, 256)


# ---------------------------------------------------------------- ref_bow: DBoW3 and KeyFrameDatabase
def _i(a):
    return np.ascontiguousarray(a, np.int32).reshape(-1)


def _stream(data):
    return np.frombuffer(bytes(data), np.uint8)


def voc_dump(stream, sanitized=False):
    """Vocabulary::fromStream of the bytes, then the tree as the reference holds it: a dict with k, L, scoring, weighting, n_nodes, n_words,
    D and parent, child_offsets, children (in m_nodes[i].children's order), desc [n_nodes, D] (row 0 zeros), weight f64, word_id (-1 for a
    node with children), words [n_words] = the node of every word"""
    hdr, parent, off, children, cols, desc, weight, word_id, words = run("voc_dump", [_stream(stream)], sanitized, program="ref_bow")
    k, L, scoring, weighting, n, nw = (int(v) for v in hdr)
    D = int(cols[1]) if n > 1 else 0
    if not (cols[0] == 0 and (cols[1:] == D).all()):
        raise RefError("voc_dump: descriptors of different widths")
    full = np.zeros((n, D), np.uint8)
    full[1:] = desc.reshape(n - 1, D)
    return {"k": k, "L": L, "scoring": scoring, "weighting": weighting, "n_nodes": n, "n_words": nw, "D": D, "parent": parent,
            "child_offsets": off, "children": children, "desc": full, "weight": weight, "word_id": word_id, "words": words}


def voc_write(stream, compressed=False, sanitized=False):
    """fromStream, then the bytes Vocabulary::toStream(out, compressed) writes"""
    return run("voc_write", [_stream(stream), np.array([int(compressed)], np.int32)], sanitized, program="ref_bow")[0].tobytes()


BOW_KEYS = ("word", "nid", "weight", "bow_word", "bow_value", "fv_node", "fv_offsets", "fv_feat")


def transform(stream, feats, levelsup, sanitized=False):
    """Vocabulary::transform(features, v, fv, levelsup) on uint8 [N,D] features; a dict of BOW_KEYS.  nid == -1 marks a descent that never
    wrote *nid: the FeatureVector of such a case is filed under an uninitialised node id and must not be used."""
    f = np.ascontiguousarray(feats, np.uint8)
    out = run("transform", [_stream(stream), f.reshape(-1), np.array([f.shape[0], f.shape[1], levelsup], np.int32)], sanitized, program="ref_bow")
    return dict(zip(BOW_KEYS, out))


def score(w1, v1, w2, v2, sanitized=False):
    """L1Scoring::score of two BowVectors (ascending words), as float64"""
    f = lambda a: np.ascontiguousarray(a, np.float64).reshape(-1)   # noqa: E731
    return run("score", [_i(w1), f(v1), _i(w2), f(v2)], sanitized, program="ref_bow")[0][0]


KFDB_ADD, KFDB_ERASE, KFDB_QUERY_SP, KFDB_QUERY_RELOC = 0, 1, 2, 3
KFDB_KEYS = ("sharing", "words", "scored", "score", "score64", "stats")


def kfdb(n_words, ops, bows, connected, sanitized=False):
    """A script over KeyFrameDatabase: ops = [(KFDB_*, arg)], bows = [(word, value)], connected = one list of keyframe indices per query.
    Returns a dict of KFDB_KEYS, per query x keyframe (E = number of adds): sharing (in lKFsSharingWords), words (the common-word counter as
    the reference leaves it; -1 untouched), scored, score (the stored float; -9.5 not scored), score64 (the double it was made from);
    stats [n_queries, 5] = returned early, maxCommonWords, minCommonWords, len(lKFsSharingWords), len(lScoreAndMatch)."""
    ops = np.ascontiguousarray(ops, np.int32).reshape(-1, 2)
    boff = np.zeros((len(bows) + 1,), np.int32); boff[1:] = np.cumsum([len(w) for w, _ in bows])
    bw = np.concatenate([_i(w) for w, _ in bows]) if bows else np.zeros((0,), np.int32)
    bx = np.concatenate([np.ascontiguousarray(x, np.float64).reshape(-1) for _, x in bows]) if bows else np.zeros((0,), np.float64)
    coff = np.zeros((len(connected) + 1,), np.int32); coff[1:] = np.cumsum([len(c) for c in connected])
    cc = np.concatenate([_i(c) for c in connected]) if connected else np.zeros((0,), np.int32)
    out = run("kfdb", [np.array([n_words], np.int32), ops.reshape(-1), boff, bw.astype(np.int32), bx, coff, cc.astype(np.int32)], sanitized,
              program="ref_bow")
    E, Q = int((ops[:, 0] == KFDB_ADD).sum()), len(connected)
    r = dict(zip(KFDB_KEYS, out))
    for k in KFDB_KEYS[:-1]:
        r[k] = r[k].reshape(Q, E)
    r["stats"] = r["stats"].reshape(Q, 5)
    return r
