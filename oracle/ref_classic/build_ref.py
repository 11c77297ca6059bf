"""Recipe of oracle/_ref/: cut the classic (model-free) function bodies out of a Rover-SLAM checkout, verbatim, and compile them
behind the stand-in headers of this directory into the command-line program oracle/_ref/ref_classic (+ ref_classic_san with host
AddressSanitizer / UBSan when the toolchain has them); and, for place recognition, DBoW3's and KeyFrameDatabase's bodies into
oracle/_ref/ref_bow (+ ref_bow_san): ranges of Vocabulary.cpp, DescManip.cpp and KeyFrameDatabase.cc, the files BowVector.cpp,
FeatureVector.cpp, ScoringObject.cpp and quicklz.c whole, DBoW3's own headers from the checkout's include path.  Nothing this writes is
committed: oracle/_ref/ is ignored by git.

The checkout is taken from $ROVER_SLAM_REF (default /root/reference).  Every range found by signature / anchor and brace matching must
be the one include/rover_fe.h cites; on drift the recipe fails loudly rather than compile something else.

    python oracle/ref_classic/build_ref.py          # build; prints one line
"""
import os
import re
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(ROOT, "oracle", "_ref")
DEFAULT_REF = "/root/reference"
CXXFLAGS = ["-std=c++14", "-O2", "-ffp-contract=off", "-fno-fast-math", "-D_GLIBCXX_ASSERTIONS", "-w"]
SANFLAGS = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]


class Drift(RuntimeError):
    pass


def ref_dir():
    return os.environ.get("ROVER_SLAM_REF", DEFAULT_REF)


def available():
    return os.path.isfile(os.path.join(ref_dir(), "src", "Frame.cc"))


def _code_mask(text):
    """per character: True where the character is code (not inside a comment, string or character literal)"""
    mask = [True] * len(text)
    i, n = 0, len(text)
    while i < n:
        c = text[i]
        if text.startswith("//", i):
            j = text.find("\n", i)
            j = n if j < 0 else j
            while j > 0 and j < n and text[j - 1] == "\\":      # line comment continued by a trailing backslash
                j = text.find("\n", j + 1)
                j = n if j < 0 else j
        elif text.startswith("/*", i):
            j = text.find("*/", i + 2)
            j = n if j < 0 else j + 2
        elif c in "\"'":
            j = i + 1
            while j < n and text[j] != c:
                j += 2 if text[j] == "\\" else 1
            j += 1
        else:
            i += 1
            continue
        for k in range(i, min(j, n)):
            mask[k] = False
        i = j
    return mask


def _line_of(text, pos):
    return text.count("\n", 0, pos) + 1


def _find_code(text, mask, needle, start=0, end=None):
    """first occurrence of `needle` that starts in code"""
    end = len(text) if end is None else end
    pos = text.find(needle, start, end)
    while pos >= 0 and not mask[pos]:
        pos = text.find(needle, pos + 1, end)
    if pos < 0:
        raise Drift(f"anchor not found: {needle!r}")
    return pos


def _body(text, mask, signature, at=None):
    """(position of the signature, position of the brace that closes its body); at: the signature's position when already known"""
    sig = _find_code(text, mask, signature) if at is None else at
    depth, i = 0, sig
    while i < len(text):
        if mask[i]:
            if text[i] == ";" and depth == 0:
                raise Drift(f"{signature!r} is a declaration, not a definition")
            if text[i] == "{":
                depth += 1
            elif text[i] == "}":
                depth -= 1
                if depth == 0:
                    return sig, i
        i += 1
    raise Drift(f"unbalanced braces after {signature!r}")


def _lines(text, first, last):
    return "".join(text.splitlines(keepends=True)[first - 1:last])


def _function(text, mask, signature):
    sig, close = _body(text, mask, signature)
    return _line_of(text, sig), _line_of(text, close)


def _between(text, mask, a, b, lo, hi):
    """lines from the one holding anchor a to the last non-blank line before the one holding anchor b (both inside [lo, hi])"""
    pa = _find_code(text, mask, a, lo, hi)
    pb = _find_code(text, mask, b, pa, hi)
    first, last = _line_of(text, pa), _line_of(text, pb) - 1
    rows = text.splitlines()
    while last > first and not rows[last - 1].strip():
        last -= 1
    return first, last


# name -> (file, expected first line, expected last line, finder)
def _spec():
    def fn(sig):
        return lambda t, m: _function(t, m, sig)

    def ctor_scales(t, m):
        lo, hi = _body(t, m, "SPextractor::SPextractor(")
        return _between(t, m, "mvScaleFactor.resize(nlevels)", "mvImagePyramid.resize(nlevels)", lo, hi)

    def ctor_fpl(t, m):
        lo, hi = _body(t, m, "SPextractor::SPextractor(")
        return _line_of(t, _find_code(t, m, "mnFeaturesPerLevel.resize(nlevels)", lo, hi)), _line_of(t, hi)

    def level_size(t, m):
        lo, hi = _body(t, m, "void SPextractor::ComputePyramid(")
        pa = _find_code(t, m, "float scale = mvInvScaleFactor[level]", lo, hi)
        pb = _find_code(t, m, "Size sz(", pa, hi)
        return _line_of(t, pa), _line_of(t, pb)

    def thresholds(t, m):
        pa = _find_code(t, m, "const float SPmatcher::TH_HIGH")
        pb = _find_code(t, m, "const float SPmatcher::TH_LOW")
        return min(_line_of(t, pa), _line_of(t, pb)), max(_line_of(t, pa), _line_of(t, pb))

    return {
        "frame_stereo": ("src/Frame.cc", 1159, 1446, fn("void Frame::ComputeStereoMatches()")),
        "frame_binarize": ("src/Frame.cc", 1034, 1043, fn("void Frame::binarize_descriptors()")),
        "mappoint_distinctive": ("src/MapPoint.cc", 438, 530, fn("void MapPoint::ComputeDistinctiveDescriptors()")),
        "spmatcher_distance": ("src/Matchers/SPmatcher.cc", 2184, 2189, fn("float SPmatcher::DescriptorDistance_sp(")),
        "spmatcher_th": ("src/Matchers/SPmatcher.cc", 13, 14, thresholds),
        "transform_normkp": ("src/Matchers/transform.cpp", 19, 32, fn("std::vector<cv::Point2f> NormalizeKeypoints(")),
        "spx_scales": ("src/Extractors/SPextractor.cc", 109, 129, ctor_scales),
        "spx_fpl": ("src/Extractors/SPextractor.cc", 133, 146, ctor_fpl),
        "spx_levelsize": ("src/Extractors/SPextractor.cc", 691, 692, level_size),
    }


def _enclosing_close(text, mask, pos, levels):
    """position of the brace that closes the `levels`-th block around pos"""
    depth = 0
    for i in range(pos, len(text)):
        if mask[i]:
            if text[i] == "{":
                depth += 1
            elif text[i] == "}":
                depth -= 1
                if depth == -levels:
                    return i
    raise Drift("unbalanced braces behind an anchor")


DBOW3 = "Thirdparty/DBoW3/src/"
BOW_WHOLE = ("BowVector.cpp", "FeatureVector.cpp", "ScoringObject.cpp", "quicklz.c")     # compiled from the checkout as they are


# place recognition; the BowVector / FeatureVector / ScoringObject entries lie in files that are compiled whole (BOW_WHOLE): their
# ranges are cut too, but only to hold them to the citations
def _spec_bow():
    def fn(sig):
        return lambda t, m: _function(t, m, sig)

    def fn_at(prefix, anchor):
        """the function whose signature starts with `prefix` on a line before the one that holds `anchor`"""
        def find(t, m):
            pa = _find_code(t, m, anchor)
            sig = t.rfind(prefix, 0, pa)
            if sig < 0 or not m[sig]:
                raise Drift(f"no {prefix!r} in front of {anchor!r}")
            return _line_of(t, sig), _line_of(t, _body(t, m, prefix, at=sig)[1])
        return find

    def front(sig):
        """from the first declaration of the body to the end of the loop that fills lScoreAndMatch"""
        def find(t, m):
            lo, hi = _body(t, m, sig)
            pa = _find_code(t, m, "list<KeyFrame *> lKFsSharingWords;", lo, hi)
            pb = _find_code(t, m, "lScoreAndMatch.push_back(make_pair(si, pKFi));", pa, hi)
            return _line_of(t, pa), _line_of(t, _enclosing_close(t, m, pb, 2))
        return find

    voc, dm, kf = DBOW3 + "Vocabulary.cpp", DBOW3 + "DescManip.cpp", "src/KeyFrameDatabase.cc"
    return {
        "voc_ctor": (voc, 10, 16, fn("Vocabulary::Vocabulary")),
        "voc_scoring": (voc, 48, 80, fn("void Vocabulary::createScoringObject()")),
        "voc_dtor": (voc, 112, 115, fn("Vocabulary::~Vocabulary()")),
        "voc_transform": (voc, 752, 818, fn_at("void Vocabulary::transform(", "BowVector &v, FeatureVector &fv, int levelsup) const")),
        "voc_transform1": (voc, 836, 874, fn_at("void Vocabulary::transform(", "WordId &word_id, WordValue &weight, NodeId *nid, int levelsup) const")),
        "voc_tostream": (voc, 1180, 1257, fn("void Vocabulary::toStream(")),
        "voc_fromstream": (voc, 1335, 1406, fn("void Vocabulary::fromStream(")),
        "descmanip_distance": (dm, 92, 130, fn("double DescManip::distance(")),
        "descmanip_tostream": (dm, 249, 258, fn("void DescManip::toStream(")),
        "descmanip_fromstream": (dm, 260, 267, fn("void DescManip::fromStream(")),
        "bowvector_addweight": (DBOW3 + "BowVector.cpp", 34, 46, fn("void BowVector::addWeight(")),
        "bowvector_addifnotexist": (DBOW3 + "BowVector.cpp", 50, 58, fn("void BowVector::addIfNotExist(")),
        "bowvector_normalize": (DBOW3 + "BowVector.cpp", 62, 84, fn("void BowVector::normalize(")),
        "featurevector_addfeature": (DBOW3 + "FeatureVector.cpp", 31, 45, fn("void FeatureVector::addFeature(")),
        "scoring_l1": (DBOW3 + "ScoringObject.cpp", 23, 68, fn("double L1Scoring::score(")),
        "kfdb_add": (kf, 44, 54, fn("void KeyFrameDatabase::add(KeyFrame *pKF)")),
        "kfdb_erase": (kf, 65, 85, fn("void KeyFrameDatabase::erase(KeyFrame *pKF)")),
        "kfdb_nbest_sp": (kf, 661, 739, front("void KeyFrameDatabase::DetectNBestCandidates_sp(")),
        "kfdb_reloc": (kf, 1047, 1099, front("vector<KeyFrame *> KeyFrameDatabase::DetectRelocalizationCandidates(")),
    }


def _cited(header, fname, first, last):
    """include/rover_fe.h cites `<file>:<first>-<last>` (a bare `:<first>-<last>` counts after the file was named)"""
    base = os.path.basename(fname)
    return f"{base}:{first}-{last}" in header or (base in header and re.search(rf"[ (,]:{first}-{last}\b", header) is not None)


def extract(ref=None, out=None, spec=None):
    """cut every range of `spec` (default: the classic stages), check it, write <out>/<name>.inc; returns {name: (file, first, last)}"""
    ref = ref or ref_dir()
    out = out or OUT
    with open(os.path.join(ROOT, "include", "rover_fe.h"), encoding="utf-8") as f:
        header = f.read()
    os.makedirs(out, exist_ok=True)
    found = {}
    for name, (fname, e_first, e_last, finder) in (spec or _spec()).items():
        with open(os.path.join(ref, fname), encoding="utf-8", errors="surrogateescape") as f:
            text = f.read()
        first, last = finder(text, _code_mask(text))
        if (first, last) != (e_first, e_last):
            raise Drift(f"{fname}: {name} found at lines {first}-{last}, include/rover_fe.h cites {e_first}-{e_last}")
        if not _cited(header, fname, first, last):
            raise Drift(f"include/rover_fe.h does not cite {fname}:{first}-{last}")
        with open(os.path.join(out, name + ".inc"), "w", encoding="utf-8", errors="surrogateescape") as f:
            f.write(_lines(text, first, last))
        found[name] = (fname, first, last)
    return found


def compile_(out=None):
    out = out or OUT
    base = ["g++"] + CXXFLAGS + ["-I" + HERE, "-I" + out, os.path.join(HERE, "ref_main.cc")]
    subprocess.check_call(base + ["-o", os.path.join(out, "ref_classic"), "-pthread"])
    san = os.path.join(out, "ref_classic_san")
    r = subprocess.run(base + SANFLAGS + ["-o", san, "-pthread"], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    if r.returncode != 0 and os.path.exists(san):
        os.remove(san)
    return r.returncode == 0


def extract_bow(ref=None, out=None):
    return extract(ref, out, _spec_bow())


def compile_bow(ref=None, out=None):
    ref, out = ref or ref_dir(), out or OUT
    src = os.path.join(ref, DBOW3)
    cc = ["gcc", "-O2", "-w", "-c", os.path.join(src, "quicklz.c"), "-o", os.path.join(out, "quicklz.o")]
    subprocess.check_call(cc)
    base = ["g++"] + CXXFLAGS + ["-I" + HERE, "-I" + out, "-I" + src, os.path.join(HERE, "ref_bow_main.cc")] \
        + [os.path.join(src, f) for f in BOW_WHOLE if f.endswith(".cpp")] + [os.path.join(out, "quicklz.o")]
    subprocess.check_call(base + ["-o", os.path.join(out, "ref_bow"), "-pthread"])
    san = os.path.join(out, "ref_bow_san")
    r = subprocess.run(base + SANFLAGS + ["-o", san, "-pthread"], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    if r.returncode != 0 and os.path.exists(san):
        os.remove(san)
    return r.returncode == 0


def build():
    """True when oracle/_ref/ref_classic and ref_bow were built; False (one line said) when there is no checkout"""
    if not available():
        print(f"oracle/_ref: no Rover-SLAM checkout at {ref_dir()} (set ROVER_SLAM_REF); reference harness not built, live tests will skip")
        return False
    found = extract()
    san = compile_()
    bow = extract_bow()
    san_bow = compile_bow()
    print(f"oracle/_ref: {len(found)} + {len(bow)} ranges cut from {ref_dir()}, ref_classic and ref_bow built"
          + (" (+ sanitizer builds)" if san and san_bow else " (no sanitizer build)" if not (san or san_bow) else " (one sanitizer build)"))
    return True


if __name__ == "__main__":
    try:
        build()
    except Drift as e:
        sys.exit(f"oracle/ref_classic: REFERENCE DRIFT: {e}")
