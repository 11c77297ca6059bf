"""Inputs and bookkeeping of the place-recognition fixtures tests/golden/ref_bow_*.npz (tools/gen_ref_golden.py records them from
oracle/_ref/ref_bow, DBoW3's and KeyFrameDatabase's own C++; tests/test_ref_bow.py and tests/test_gpu_ref_bow.py read them).  Only inputs
are made here -- seeded vocabularies with planted distance ties, feature pools, database scripts -- and the census that says the fixtures
exercise what they are for.  Every recorded OUTPUT comes from the harness."""
import numpy as np

import bow_ref as B
import ref_classic_cases as RC

SIZES = (0, 1, 3, 4, 5, 63, 64, 65, 257, 1025, 4096)        # either side of: 4 features per wave, 64 per workgroup, 2 sorted positions per thread
VOCABS = ("k2L4D8", "k3L3D24", "k5L3D32", "k6L3D256", "k10L2D32", "irregular", "stopped", "oneword")
BOW_OUT = ("word", "nid", "weight", "bow_word", "bow_value", "fv_node", "fv_offsets", "fv_feat")
TRANSFORM_CENSUS = ("descent_tie_decided_by_order", "stopped_feature", "multi_feature_word", "nid_level_le_0")
KFDB_CENSUS = ("entry_at_gate", "entry_one_above_gate", "excluded_would_set_max", "erased_entry", "returned_early", "max_multiple_of_5",
               "max_other")
ADD, ERASE, QUERY_SP, QUERY_RELOC = 0, 1, 2, 3


# ---------------------------------------------------------------- vocabularies
def flip(rng, row, nbits, bits01):
    """row with nbits distinct positions changed: a 0/1 byte toggled, or one bit of an arbitrary byte"""
    row = row.copy()
    D = len(row)
    if bits01:
        row[rng.choice(D, nbits, replace=False)] ^= 1
    else:
        for p in rng.choice(D * 8, nbits, replace=False):
            row[p // 8] ^= np.uint8(1 << (p % 8))
    return row


def nested_vocab(k, L, D, seed, weighting, bits01, stop_every=0):
    """a full k-ary tree whose children are their parent with a few positions changed (fewer at each depth), so that a feature near a
    leaf is carried down to it"""
    rng = np.random.default_rng(seed)
    b = B.TreeBuilder(k, L, D, weighting)
    units = D if bits01 else D * 8
    level = [(0, None)]
    for depth in range(1, L + 1):
        nxt = []
        for p, row in level:
            for _ in range(k):
                d = B.random_desc(rng, (D,), bits01) if row is None else flip(rng, row, max(2, units // (3 * 2 ** (depth - 1))), bits01)
                nxt.append((b.add(p, d), d))
        level = nxt
    w = B.idf_weights(rng, len(level))
    if weighting in (B.TF, B.BINARY):
        w[:] = 1.0
    if stop_every:
        w[::stop_every] = 0.0
    for i, (node, _) in enumerate(level):
        b.weight[node] = float(w[i])
    return b.finish()


def kids(v, i):
    return v["children"][v["child_offsets"][i]:v["child_offsets"][i + 1]]


def plant_ties(v, seed, bits01):
    """under every third parent: a later sibling becomes a copy of an earlier one, or the earlier one with 2t positions changed (a
    feature with t of those changed is then equally far from both).  Returns [(earlier, later, changed positions or None)]."""
    rng = np.random.default_rng(seed)
    pairs = []
    parents = [i for i in range(v["n_nodes"]) if len(kids(v, i)) >= 2]
    for n, p in enumerate(parents):
        if n % 3:
            continue
        c = kids(v, p)
        i, j = sorted(rng.choice(len(c), 2, replace=False))
        if n % 2:
            v["desc"][c[j]] = v["desc"][c[i]]
            pairs.append((int(c[i]), int(c[j]), None))
        else:
            t = int(rng.integers(1, 3))
            pos = rng.choice(v["D"] * (1 if bits01 else 8), 2 * t, replace=False)
            row = v["desc"][c[i]].copy()
            for q in pos:
                row[q if bits01 else q // 8] ^= np.uint8(1 if bits01 else 1 << (q % 8))
            v["desc"][c[j]] = row
            pairs.append((int(c[i]), int(c[j]), pos))
    return pairs


def shuffle_children(v, seed):
    """every parent's children in a seeded order that is not the ascending one (what a reader that sorts by id would lose)"""
    rng = np.random.default_rng(seed)
    for p in range(v["n_nodes"]):
        a, b = v["child_offsets"][p], v["child_offsets"][p + 1]
        if b - a >= 2:
            seg = v["children"][a:b].copy()
            while np.array_equal(seg, np.sort(seg)):
                seg = rng.permutation(seg)
            v["children"][a:b] = seg


def permute_word_ids(v, seed):
    leaves = np.nonzero(v["word_id"] >= 0)[0]
    v["word_id"][leaves] = np.random.default_rng(seed).permutation(len(leaves)).astype(np.int32)


def make_pool(v, pairs, n, seed, bits01):
    """n features: near leaves, exact copies of nodes, halfway between the planted sibling pairs, and random ones, shuffled"""
    rng = np.random.default_rng(seed)
    D = v["D"]
    leaves = np.nonzero(v["word_id"] >= 0)[0]
    out = np.zeros((n, D), np.uint8)
    for r in range(n):
        kind = r % 10
        if kind < 5:
            out[r] = flip(rng, v["desc"][rng.choice(leaves)], int(rng.integers(0, 3)), bits01)
        elif kind < 7:
            out[r] = v["desc"][rng.integers(1, v["n_nodes"])]
        elif kind < 9 and pairs:
            a, _, pos = pairs[rng.integers(0, len(pairs))]
            row = v["desc"][a].copy()
            if pos is not None:
                for q in pos[:len(pos) // 2]:
                    row[q if bits01 else q // 8] ^= np.uint8(1 if bits01 else 1 << (q % 8))
            else:                                        # a's twin holds the same row: a leaf below a, reached through that tie
                sub = a
                while len(kids(v, sub)):
                    sub = kids(v, sub)[rng.integers(0, len(kids(v, sub)))]
                row = v["desc"][sub].copy()
            out[r] = row
        else:
            out[r] = B.random_desc(rng, (D,), bits01)
    return out[rng.permutation(n)]


def cycle_cases(pool, sizes, L, start=0):
    ups = (0, 1, L - 1, L, L + 1)
    return [(pool, n, ups[(start + i) % 5]) for i, n in enumerate(sizes)]


def source(name):
    """(vocabulary in the project's dict form, {pool name: uint8 [n, D]}, [(pool name, N, levelsup)]) of one fixture"""
    if name == "k2L4D8":
        v = nested_vocab(2, 4, 8, 101, B.TF_IDF, False)
        pools = {"mix": make_pool(v, plant_ties(v, 102, False), 4096, 103, False)}
        cases = cycle_cases("mix", SIZES, 4) + [("mix", 65, u) for u in (0, 1, 3, 4, 5)]
    elif name == "k3L3D24":
        v = nested_vocab(3, 3, 24, 111, B.IDF, False, stop_every=7)
        pairs = plant_ties(v, 112, False)
        shuffle_children(v, 113); permute_word_ids(v, 114)
        pools = {"mix": make_pool(v, pairs, 4096, 115, False)}
        cases = cycle_cases("mix", (5, 65, 257, 1025, 4096), 3, 1) + [("mix", 64, u) for u in (0, 2, 3)]
    elif name == "k5L3D32":
        v = nested_vocab(5, 3, 32, 121, B.TF, True)
        pairs = plant_ties(v, 122, True)
        shuffle_children(v, 123)
        pools = {"mix": make_pool(v, pairs, 4096, 125, True)}
        cases = cycle_cases("mix", (1, 64, 1025, 4096), 3, 2)
    elif name == "k6L3D256":
        v = nested_vocab(6, 3, 256, 131, B.TF_IDF, True, stop_every=5)
        pools = {"mix": make_pool(v, plant_ties(v, 132, True), 257, 135, True)}
        cases = cycle_cases("mix", SIZES[:9], 3) + [("mix", 65, u) for u in (0, 1, 2, 3, 4)]
    elif name == "k10L2D32":
        v = nested_vocab(10, 2, 32, 141, B.BINARY, False, stop_every=9)
        pools = {"mix": make_pool(v, plant_ties(v, 142, False), 4096, 145, False)}
        cases = [("mix", 4, 0), ("mix", 63, 1), ("mix", 257, 2), ("mix", 1025, 3), ("mix", 4096, 1)]
    elif name == "irregular":
        v = B.irregular_vocab()
        rng = np.random.default_rng(151)
        hand = np.array([[0] * 8, [1] * 8, [1, 1, 1, 1, 0, 0, 0, 0], [1, 1, 1, 1, 1, 1, 0, 0], [0, 1, 1, 1, 1, 1, 1, 1], [0, 0, 0, 0, 0, 0, 0, 1]], np.uint8)
        pools = {"mix": np.concatenate([hand, B.random_desc(rng, (59, 8), True)])}
        cases = [("mix", 6, u) for u in range(5)] + [("mix", 65, u) for u in range(5)]
    elif name == "stopped":
        v = nested_vocab(4, 2, 32, 161, B.TF_IDF, True, stop_every=2)
        pool = make_pool(v, plant_ties(v, 162, True), 2000, 165, True)
        w = B.descend(v, pool, 0)[2]                     # orders the INPUT only: the stopped features first
        pools = {"mix": np.concatenate([pool[w == 0][:64], pool[w > 0][:193]])}
        assert len(pools["mix"]) == 257
        cases = [("mix", 64, 0), ("mix", 63, 1), ("mix", 257, 1), ("mix", 65, 2)]
    elif name == "oneword":
        v, chain, _ = B.one_word_case()
        pools = {"chain": chain, "zeros": np.zeros((4096, 8), np.uint8)}
        cases = [("chain", 701, 0), ("chain", 700, 1), ("zeros", 4096, 0), ("zeros", 1025, 2)]
    else:
        raise KeyError(name)
    return v, pools, cases


# ---------------------------------------------------------------- what a tree and a case are
def leaf_depths(v):
    depth = np.zeros((v["n_nodes"],), np.int32)
    order = [0]
    for p in order:
        for c in kids(v, p):
            depth[c] = depth[p] + 1
            order.append(int(c))
    return depth[v["word_id"] >= 0]


def fv_defined(v, levelsup):
    """from the tree alone: every descent writes *nid (no leaf above depth L - levelsup), or nid_level <= 0"""
    nid_level = v["L"] - levelsup
    return bool(nid_level <= 0 or leaf_depths(v).min() >= nid_level)


def transform_census(v, feats, levelsup):
    """counts of TRANSFORM_CENSUS on one case, by a descent of its own (all children's distances at every step)"""
    feats = np.ascontiguousarray(feats, np.uint8)
    cur = np.zeros((len(feats),), np.int64)
    ties = np.zeros((len(feats),), bool)
    while True:
        nk = v["child_offsets"][cur + 1] - v["child_offsets"][cur]
        act = np.nonzero(nk > 0)[0]
        if not len(act):
            break
        for i in act:
            c = kids(v, cur[i])
            d = B.POPCOUNT[feats[i][None, :] ^ v["desc"][c]].sum(axis=1)
            first = int(np.argmin(d))
            ties[i] |= (d == d[first]).sum() > 1
            cur[i] = c[first]
    w, word = v["weight"][cur], v["word_id"][cur]
    kept = word[w > 0]
    return [int(ties.sum()), int((w == 0).sum()), int(len(kept) - len(np.unique(kept))), int(len(feats) if v["L"] - levelsup <= 0 else 0)]


def dump_dict(z):
    """the recorded voc_dump as the project's vocabulary dict"""
    k, L, scoring, weighting, n, nw, D = (int(x) for x in z["dump_hdr"])
    v = {"k": k, "L": L, "scoring": scoring, "weighting": weighting, "n_nodes": n, "n_words": nw, "D": D}
    for key in B.VOCAB_ARRAYS:
        v[key] = z["dump_" + key]
    v["words"] = z["dump_words"]
    return v


def load_vocab(name):
    """(recorded fixture arrays, vocabulary dict of the recorded dump, [(case index, features, levelsup)])"""
    z = RC.load("bow_" + name)
    v = dump_dict(z)
    pools = [str(p) for p in z["pools"]]
    cases = [(i, z["pool_" + pools[p]][:n], int(u)) for i, (p, n, u) in enumerate(z["cases"].tolist())]
    return z, v, cases


def recorded(z, i):
    return {k: z[f"c{i}_{k}"] for k in BOW_OUT if f"c{i}_{k}" in z}


# ---------------------------------------------------------------- database scripts
def unit(rng, n):
    x = rng.random(n) + 1e-3
    return x / B.sequential_sum(x) if n else x


def script_empty():
    rng = np.random.default_rng(201)
    big = np.sort(rng.choice(6000, 4096, replace=False)).astype(np.int32)
    bows = [(np.array([17], np.int32), np.array([1.0])), (big, unit(rng, 4096))]
    return {"name": "empty", "n_words": 6000, "bows": bows, "ops": [(QUERY_SP, 0), (QUERY_RELOC, 1), (QUERY_SP, 1)], "connected": [[], [], []]}


def script_one():
    rng = np.random.default_rng(211)
    w = np.sort(rng.choice(500, 63, replace=False)).astype(np.int32)
    q = np.sort(np.r_[w[rng.choice(63, 10, replace=False)], 500 + rng.choice(100, 30, replace=False)]).astype(np.int32)
    bows = [(w, unit(rng, 63)), (q, unit(rng, 40)), (w[:1], np.array([1.0]))]
    ops = [(ADD, 0), (QUERY_SP, 1), (QUERY_RELOC, 1), (QUERY_SP, 1), (QUERY_SP, 2), (ERASE, 0), (QUERY_SP, 1), (QUERY_RELOC, 2)]
    return {"name": "one", "n_words": 600, "bows": bows, "ops": ops, "connected": [[], [], [0], [], [], []]}


def script_grow():
    """255, 256, 257 and 600 entries (the store's first doubling lies between), entries of 1 / 63 / 64 / 65 / 4096 words, queries of 1 and
    4096 words, connected sets empty / partial / holding the entry with the largest count, erased entries"""
    rng = np.random.default_rng(221)
    hot = rng.choice(6000, 400, replace=False)

    def entry(n):
        n_hot = min(n, int(rng.integers(0, min(n, 120) + 1)))
        rest = np.setdiff1d(np.arange(6000), hot)
        w = np.sort(np.r_[rng.choice(hot, n_hot, replace=False), rng.choice(rest, n - n_hot, replace=False)]).astype(np.int32)
        return w, unit(rng, n)
    lens = [1, 63, 64, 65] * 3 + [4096] + [int(x) for x in rng.integers(1, 71, 600 - 13)]
    lens = [lens[i] for i in rng.permutation(600)]
    bows = [entry(n) for n in lens]
    q200 = (np.sort(rng.choice(hot, 200, replace=False)).astype(np.int32), unit(rng, 200))
    q4096 = entry(4096)
    q1 = (np.array([int(np.sort(hot)[3])], np.int32), np.array([1.0]))
    q0 = (np.zeros((0,), np.int32), np.zeros((0,)))
    bows += [q200, q4096, q1, q0]
    Q200, Q4096, Q1, Q0 = 600, 601, 602, 603

    def top(qw, upto, k):
        common = np.array([len(np.intersect1d(qw, bows[e][0], assume_unique=True)) for e in range(upto)])
        return [int(e) for e in np.argsort(-common, kind="stable")[:k]]
    ops = [(ADD, e) for e in range(255)] + [(QUERY_SP, Q200)]; conn = [[]]
    ops += [(ADD, 255), (QUERY_RELOC, Q200)]; conn += [[]]
    ops += [(ADD, 256), (QUERY_SP, Q200)]; conn += [top(q200[0], 257, 1) + [3, 200]]          # the largest count is connected
    ops += [(ADD, e) for e in range(257, 600)]
    gone = list(dict.fromkeys(top(q200[0], 600, 2) + [int(e) for e in rng.choice(600, 18, replace=False)]))
    ops += [(ERASE, e) for e in gone]
    ops += [(QUERY_SP, Q4096), (QUERY_RELOC, Q1), (QUERY_SP, Q1), (QUERY_SP, Q0), (QUERY_SP, Q200), (QUERY_RELOC, Q4096)]
    conn += [[int(e) for e in rng.choice(600, 40, replace=False)], [], [], [], top(q200[0], 600, 6), []]
    sharing1 = [e for e in range(600) if e not in gone and q1[0][0] in bows[e][0]]
    ops += [(QUERY_SP, Q1)]; conn += [sharing1]                                                # all sharing entries connected
    return {"name": "grow", "n_words": 6000, "bows": bows, "ops": ops, "connected": conn}


GATE_MAXIMA = (5, 10, 100, 7, 13, 64, 99, 101, 1, 255)


def script_gate():
    """per maximum M a word range of its own: entries with M, (int)(M * 0.8f) and (int)(M * 0.8f) + 1 of the query's words, and one with M + 3
    that is connected (it would have set the maximum); asked through both fronts (DetectRelocalizationCandidates excludes nobody)"""
    rng = np.random.default_rng(231)
    bows, ops, queries, conn = [], [], [], []
    for g, M in enumerate(GATE_MAXIMA):
        base = g * 1000
        qw = base + np.sort(rng.choice(600, M + 3, replace=False)).astype(np.int32)
        gate = int(np.float32(M) * np.float32(0.8))
        first = len(bows)
        for c in (M, gate, gate + 1, M + 3, max(gate - 1, 0)):
            if c > M + 3:
                continue
            own = base + 600 + rng.choice(400, 5, replace=False)
            sel = qw[:M][rng.choice(M, c, replace=False)] if c <= M else qw
            w = np.sort(np.r_[sel, own]).astype(np.int32)
            bows.append((w, unit(rng, len(w))))
        queries.append((g, (qw, unit(rng, M + 3)), first + 3))
    E = len(bows)
    ops = [(ADD, e) for e in range(E)]
    for g, q, excluded in queries:
        bows.append(q)
        ops += [(QUERY_SP, len(bows) - 1), (QUERY_RELOC, len(bows) - 1)]
        conn += [[excluded], []]
    return {"name": "gate", "n_words": 1000 * len(GATE_MAXIMA), "bows": bows, "ops": ops, "connected": conn}


def kfdb_scripts():
    return [script_empty(), script_one(), script_grow(), script_gate()]


KFDB_OUT = ("sharing", "words", "scored", "score", "score64", "stats")


def pack_script(s):
    boff = np.zeros((len(s["bows"]) + 1,), np.int32); boff[1:] = np.cumsum([len(w) for w, _ in s["bows"]])
    coff = np.zeros((len(s["connected"]) + 1,), np.int32); coff[1:] = np.cumsum([len(c) for c in s["connected"]])
    cat = lambda xs, dt: np.concatenate([np.asarray(x, dt).reshape(-1) for x in xs]) if xs else np.zeros((0,), dt)   # noqa: E731
    return {"n_words": np.array([s["n_words"]], np.int32), "ops": np.array(s["ops"], np.int32).reshape(-1, 2), "bow_off": boff,
            "bow_word": cat([w for w, _ in s["bows"]], np.int32), "bow_value": cat([x for _, x in s["bows"]], np.float64), "conn_off": coff,
            "conn": cat(s["connected"], np.int32)}


def unpack_script(z, name):
    g = lambda k: z[f"{name}_{k}"]   # noqa: E731
    boff, coff = g("bow_off"), g("conn_off")
    bows = [(g("bow_word")[boff[i]:boff[i + 1]], g("bow_value")[boff[i]:boff[i + 1]]) for i in range(len(boff) - 1)]
    conn = [g("conn")[coff[i]:coff[i + 1]].tolist() for i in range(len(coff) - 1)]
    s = {"name": name, "n_words": int(g("n_words")[0]), "bows": bows, "ops": [tuple(o) for o in g("ops").tolist()], "connected": conn}
    return s, {k: g(k) for k in KFDB_OUT}


def replay(s):
    """the script as a database would see it: yields (query index, op, entries so far [(word, value) or None], query bow, exclude u8 [E])"""
    entries, q = [], 0
    for op, arg in s["ops"]:
        if op == ADD:
            entries.append(s["bows"][arg])
        elif op == ERASE:
            entries[arg] = None
        else:
            ex = np.zeros((len(entries),), np.uint8)
            if op == QUERY_SP:
                ex[s["connected"][q]] = 1
            yield q, op, list(entries), s["bows"][arg], ex
            q += 1


def kfdb_census(s):
    """counts of KFDB_CENSUS over the script's queries, from the restatement (tests/bow_ref.py)"""
    c = dict.fromkeys(KFDB_CENSUS, 0)
    for _, _, entries, (qw, qx), ex in replay(s):
        r = B.db_query(entries, qw, qx, ex)
        mx, mn, n_sharing, _ = (int(x) for x in r["stats"])
        sharing = (r["common"] > 0) & (ex == 0)
        c["entry_at_gate"] += int((sharing & (r["common"] == mn)).sum())
        c["entry_one_above_gate"] += int((sharing & (r["common"] == mn + 1)).sum())
        c["excluded_would_set_max"] += int(((ex == 1) & (r["common"] > mx)).sum())
        c["erased_entry"] += sum(e is None for e in entries)
        c["returned_early"] += int(n_sharing == 0)
        c["max_multiple_of_5"] += int(mx > 0 and mx % 5 == 0)
        c["max_other"] += int(mx % 5 != 0)
    return [c[k] for k in KFDB_CENSUS]
