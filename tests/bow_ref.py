"""The contract of DESIGN.md 6h restated in numpy: DBoW3::Vocabulary::transform (descent, BowVector, FeatureVector, L1 normalisation),
L1Scoring::score and the front of KeyFrameDatabase::DetectNBestCandidates / DetectRelocalizationCandidates; a seeded synthetic-vocabulary
generator; a writer of DBoW3's uncompressed binary stream.  Sort-based and vectorised; every float64 sum is taken strictly left to right
(np.add.accumulate adds one element after the other) in the order the reference's loops have.  tests/test_bow_ref.py holds this file to a
literal per-feature transcription."""
import struct

import numpy as np

TF_IDF, TF, IDF, BINARY = 0, 1, 2, 3
L1_NORM = 0
MAGIC = 88877711233
POPCOUNT = np.array([bin(i).count("1") for i in range(256)], np.int32)
VOCAB_ARRAYS = ("parent", "child_offsets", "children", "desc", "weight", "word_id")


# ---------------------------------------------------------------- vocabularies
class TreeBuilder:
    """nodes in the order they are added (the root is node 0); a node's children keep the order of their adds"""

    def __init__(self, k, L, D, weighting=TF_IDF, scoring=L1_NORM):
        self.k, self.L, self.D, self.weighting, self.scoring = k, L, D, weighting, scoring
        self.parent, self.desc, self.weight = [-1], [np.zeros((D,), np.uint8)], [0.0]

    def add(self, parent, desc, weight=0.0):
        self.parent.append(parent); self.desc.append(np.asarray(desc, np.uint8).reshape(self.D)); self.weight.append(float(weight))
        return len(self.parent) - 1

    def finish(self):
        n = len(self.parent)
        parent = np.array(self.parent, np.int32)
        kids = [[] for _ in range(n)]
        for i in range(1, n):
            kids[parent[i]].append(i)
        off = np.zeros((n + 1,), np.int32)
        off[1:] = np.cumsum([len(c) for c in kids])
        children = np.array([c for cs in kids for c in cs], np.int32)
        word_id = np.full((n,), -1, np.int32)
        leaves = [i for i in range(n) if not kids[i]]
        word_id[leaves] = np.arange(len(leaves), dtype=np.int32)
        return {"k": self.k, "L": self.L, "weighting": self.weighting, "scoring": self.scoring, "n_nodes": n, "D": self.D, "parent": parent,
                "child_offsets": off, "children": children, "desc": np.stack(self.desc), "weight": np.array(self.weight, np.float64),
                "word_id": word_id}


def random_desc(rng, shape, bits01):
    return rng.integers(0, 2, shape, dtype=np.uint8) if bits01 else rng.integers(0, 256, shape, dtype=np.uint8)


def idf_weights(rng, n):
    """what a trained vocabulary holds: log(N / N_i), non-dyadic doubles"""
    return np.log(rng.integers(1000, 2000, n) / rng.integers(1, 900, n))


def make_vocab(k, L, D, seed, weighting=TF_IDF, bits01=True, stop_every=0):
    """a full k-ary tree of depth L, breadth first; stop_every > 0: every stop_every-th word has weight 0"""
    rng = np.random.default_rng(seed)
    b = TreeBuilder(k, L, D, weighting)
    level = [0]
    for depth in range(1, L + 1):
        nxt = []
        for p in level:
            for _ in range(k):
                nxt.append(b.add(p, random_desc(rng, (D,), bits01)))
        level = nxt
    w = idf_weights(rng, len(level))
    if weighting in (TF, BINARY):
        w[:] = 1.0
    if stop_every:
        w[::stop_every] = 0.0
    for i, node in enumerate(level):
        b.weight[node] = float(w[i])
    return b.finish()


def irregular_vocab():
    """k = 2, L = 3: node 1 is a leaf at depth 1, node 2 carries a full subtree down to depth 3"""
    b = TreeBuilder(2, 3, 8)
    z, o = np.zeros(8, np.uint8), np.ones(8, np.uint8)
    b.add(0, z, 0.7)
    n2 = b.add(0, o)
    a, c = b.add(n2, [1, 1, 1, 1, 0, 0, 0, 0]), b.add(n2, o)
    for p, d in ((a, [1, 1, 1, 1, 0, 0, 0, 0]), (a, [1, 1, 1, 1, 1, 1, 0, 0]), (c, o), (c, [0, 1, 1, 1, 1, 1, 1, 1])):
        b.add(p, d, 0.1 + 0.2 * len(b.parent))
    return b.finish()


def one_word_case():
    """700 features on one word of a non-dyadic idf and one on another: a sum taken as a tree differs from the chain in the last bit"""
    b = TreeBuilder(2, 1, 8)
    w = float(np.log(1000.0 / 7.0))
    b.add(0, np.zeros(8, np.uint8), w); b.add(0, np.full(8, 255, np.uint8), 0.3)
    feats = np.zeros((701, 8), np.uint8); feats[700] = 255
    return b.finish(), feats, w


# ---------------------------------------------------------------- transform
def binarize(desc_f32):
    """Frame::binarize_descriptors: byte = value > 0 (a NaN gives 0)"""
    with np.errstate(invalid="ignore"):
        return (np.asarray(desc_f32, np.float32) > 0).astype(np.uint8)


def descend(v, feats, levelsup=0):
    """per feature: word id, node at depth L - levelsup, weight.  Children are scanned in stored order, a strict < keeps the first minimum."""
    feats = np.ascontiguousarray(feats, np.uint8)
    N = len(feats)
    off, children, desc = v["child_offsets"], v["children"], v["desc"]
    nid_level = v["L"] - levelsup
    cur = np.zeros((N,), np.int64)
    nid = np.full((N,), 0 if nid_level <= 0 else -1, np.int64)
    level = 0
    while True:
        nkids = off[cur + 1] - off[cur]
        act = np.nonzero(nkids > 0)[0]
        if len(act) == 0:
            break
        level += 1
        best = np.full((len(act),), np.iinfo(np.int64).max, np.int64)
        best_id = cur[act].copy()
        for j in range(int(nkids[act].max())):
            has = nkids[act] > j
            ids = children[off[cur[act[has]]] + j]
            d = POPCOUNT[feats[act[has]] ^ desc[ids]].sum(axis=1)
            better = d < best[has]
            hb = np.nonzero(has)[0][better]
            best[hb] = d[better]; best_id[hb] = ids[better]
        cur[act] = best_id
        if level == nid_level:
            nid[act] = best_id
    nid = np.where(nid < 0, cur, nid)           # a leaf above depth L - levelsup: the leaf's own node id
    return v["word_id"][cur].astype(np.int32), nid.astype(np.int32), v["weight"][cur].astype(np.float64)


def sequential_sum(x):
    """x[0] + x[1] + ... one after the other in float64"""
    x = np.asarray(x, np.float64)
    return float(np.add.accumulate(x)[-1]) if len(x) else 0.0


def transform(v, feats, levelsup=0):
    """Vocabulary::transform(features, v, fv, levelsup) with L1 scoring.  feats: uint8 [N,D]."""
    word, node, weight = descend(v, feats, levelsup)
    kept = np.nonzero(weight > 0)[0]
    out = {"word": word, "node": node, "weight": weight}
    # BowVector: (word, feature) order; a word's weights added in feature order (TF_IDF, TF) or the first kept (IDF, BINARY)
    order = kept[np.lexsort((kept, word[kept]))]
    ws = word[order]
    heads = np.nonzero(np.r_[True, ws[1:] != ws[:-1]])[0] if len(order) else np.zeros((0,), np.int64)
    lens = np.diff(np.r_[heads, len(order)])
    vals = weight[order[heads]].copy()
    if v["weighting"] in (TF_IDF, TF):
        for r in range(1, int(lens.max()) if len(lens) else 0):
            m = lens > r
            vals[m] = vals[m] + weight[order[heads[m] + r]]
    norm = sequential_sum(np.abs(vals))
    if norm > 0:
        vals = vals / norm
    out["bow_word"], out["bow_value"] = ws[heads].astype(np.int32), vals
    # FeatureVector: (node, feature) order
    order = kept[np.lexsort((kept, node[kept]))]
    ns = node[order]
    heads = np.nonzero(np.r_[True, ns[1:] != ns[:-1]])[0] if len(order) else np.zeros((0,), np.int64)
    out["fv_node"] = ns[heads].astype(np.int32)
    out["fv_offsets"] = np.r_[heads, len(order)].astype(np.int32)
    out["fv_feat"] = order.astype(np.int32)
    return out


KEYS = ("word", "node", "weight", "bow_word", "bow_value", "fv_node", "fv_offsets", "fv_feat")
DTYPES = {"word": np.int32, "node": np.int32, "weight": np.float64, "bow_word": np.int32, "bow_value": np.float64, "fv_node": np.int32,
          "fv_offsets": np.int32, "fv_feat": np.int32}


# ---------------------------------------------------------------- scores
def l1_score(w1, v1, w2, v2):
    """L1Scoring::score of two BowVectors (ascending words): the common words' terms added in ascending word order, then -sum / 2"""
    _, i1, i2 = np.intersect1d(w1, w2, assume_unique=True, return_indices=True)
    vi, wi = np.asarray(v1, np.float64)[i1], np.asarray(v2, np.float64)[i2]
    return -sequential_sum(np.abs(vi - wi) - np.abs(vi) - np.abs(wi)) / 2.0


def db_query(entries, q_word, q_value, exclude=None, score=None):
    """entries: per entry id (word, value) or None once erased.  score: the array the scores go into (kept where an entry is not scored)."""
    E = len(entries)
    common = np.zeros((E,), np.int32)
    for e, ent in enumerate(entries):
        if ent is not None:
            common[e] = len(np.intersect1d(q_word, ent[0], assume_unique=True))
    ex = np.zeros((E,), bool) if exclude is None else np.asarray(exclude).astype(bool)
    sharing = (common > 0) & ~ex
    max_common = int(common[sharing].max()) if sharing.any() else 0
    min_common = int(np.float32(max_common) * np.float32(0.8))           # int minCommonWords = maxCommonWords * 0.8f
    scored = (common > min_common) & ~ex
    out = np.zeros((E,), np.float64) if score is None else np.array(score, np.float64)
    for e in np.nonzero(scored)[0]:
        out[e] = l1_score(q_word, q_value, entries[e][0], entries[e][1])
    return {"common": common, "scored": scored.astype(np.uint8), "score": out,
            "stats": np.array([max_common, min_common, int(sharing.sum()), int(scored.sum())], np.int32)}


# ---------------------------------------------------------------- DBoW3's binary stream
def stream_bytes(v, compressed=0, node_type=0, nnodes=None):
    """Vocabulary::toStream(str, false): the nodes parent by parent, every parent's children in their stored order (the reader appends a
    node to its parent's children as it meets it).  compressed / node_type / nnodes: what the header and the node records claim."""
    n = v["n_nodes"]
    out = [struct.pack("<QBI", MAGIC, compressed, n if nnodes is None else nnodes), struct.pack("<iiii", v["k"], v["L"], v["scoring"], v["weighting"])]
    elem = {0: 1, 5: 4}[node_type]                                       # CV_8U, CV_32F
    for p in range(n):
        for c in v["children"][v["child_offsets"][p]:v["child_offsets"][p + 1]]:
            out.append(struct.pack("<IId", int(c), p, float(v["weight"][c])))
            out.append(struct.pack("<iii", v["D"] // elem, 1, node_type))
            out.append(v["desc"][c].tobytes())
    leaves = np.nonzero(v["word_id"] >= 0)[0]
    out.append(struct.pack("<I", len(leaves)))
    for node in leaves:
        out.append(struct.pack("<II", int(v["word_id"][node]), int(node)))
    return b"".join(out)
