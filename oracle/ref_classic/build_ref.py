"""Recipe of oracle/_ref/: cut the classic (model-free) function bodies out of a Rover-SLAM checkout, verbatim, and compile them
behind the stand-in headers of this directory into the command-line program oracle/_ref/ref_classic (+ ref_classic_san with host
AddressSanitizer / UBSan when the toolchain has them).  Nothing this writes is committed: oracle/_ref/ is ignored by git.

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


def _body(text, mask, signature):
    """(position of the signature, position of the brace that closes its body)"""
    sig = _find_code(text, mask, signature)
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


def _cited(header, fname, first, last):
    """include/rover_fe.h cites `<file>:<first>-<last>` (a bare `:<first>-<last>` counts after the file was named)"""
    base = os.path.basename(fname)
    return f"{base}:{first}-{last}" in header or (base in header and re.search(rf"[ (,]:{first}-{last}\b", header) is not None)


def extract(ref=None, out=None):
    """cut every range, check it, write <out>/<name>.inc; returns {name: (file, first, last)}"""
    ref = ref or ref_dir()
    out = out or OUT
    with open(os.path.join(ROOT, "include", "rover_fe.h"), encoding="utf-8") as f:
        header = f.read()
    os.makedirs(out, exist_ok=True)
    found = {}
    for name, (fname, e_first, e_last, finder) in _spec().items():
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


def build():
    """True when oracle/_ref/ref_classic was built; False (one line said) when there is no checkout"""
    if not available():
        print(f"oracle/_ref: no Rover-SLAM checkout at {ref_dir()} (set ROVER_SLAM_REF); reference harness not built, live tests will skip")
        return False
    found = extract()
    san = compile_()
    print(f"oracle/_ref: {len(found)} ranges cut from {ref_dir()}, ref_classic built" + (" (+ sanitizer build)" if san else " (no sanitizer build)"))
    return True


if __name__ == "__main__":
    try:
        build()
    except Drift as e:
        sys.exit(f"oracle/ref_classic: REFERENCE DRIFT: {e}")
