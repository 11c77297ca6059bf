#!/usr/bin/env python3
"""Sensitivity of the reference fixtures: each plausible misreading of Frame::ComputeStereoMatches / SPextractor is applied to an
IN-MEMORY copy of tests/stereo_pyramid_ref.py (the file is not touched) and the fixture tests of tests/test_ref_classic.py are run
against it; every mutation must make at least one of them fail.  Prints the table of profiles/ref_classic.md.

    python tools/mutate_ref_classic.py            # all mutations, one child process each
"""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CAND = "(minr <= row) & (row <= maxr) & (oR >= l - 1) & (oR <= l + 1) & (kR[:, 0] >= minU)"
MUTATIONS = {
    "row band from the LEFT keypoint's octave": (
        CAND, "(np.floor((kR[:, 1] - f32(2.0) * scale[l]).astype(np.float32)) <= row) & (row <= np.ceil((kR[:, 1] + f32(2.0) * scale[l]).astype(np.float32)))"
              " & (oR >= l - 1) & (oR <= l + 1) & (kR[:, 0] >= minU)"),
    "octave gate +-2": (CAND, "(minr <= row) & (row <= maxr) & (oR >= l - 2) & (oR <= l + 2) & (kR[:, 0] >= minU)"),
    "round half to even": ("    x = float(x)\n    return int(np.floor(x + 0.5)) if x >= 0 else -int(np.floor(-x + 0.5))",
                           "    return int(np.rint(np.float32(x)))"),
    "last minimum among tied descriptors": ("                if d < best:\n", "                if d <= best:\n"),
    "median at (n-1)/2": ("v[len(v) // 2][0]", "v[(len(v) - 1) // 2][0]"),
    "cut with > instead of >=": ("            if not (f32(d) < th):\n", "            if f32(d) > th:\n"),
    "level size from X / s": ("        h[l] = int(np.rint(f32(f32(H) * inv)))\n        w[l] = int(np.rint(f32(f32(W) * inv)))\n",
                              "        h[l] = int(np.rint(f32(H) / sc))\n        w[l] = int(np.rint(f32(W) / sc))\n"),
    "disparity < 0 in the clamp": ("            if disp <= 0:\n", "            if disp < 0:\n"),
}


def run_one(name):
    sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
    import pytest
    import stereo_pyramid_ref as SR
    old, new = MUTATIONS[name]
    with open(SR.__file__) as f:
        src = f.read()
    assert src.count(old) >= 1, f"mutation site not found: {name}"
    exec(compile(src.replace(old, new), SR.__file__, "exec"), SR.__dict__)
    return pytest.main([os.path.join(ROOT, "tests", "test_ref_classic.py"), "-q", "-p", "no:cacheprovider", "-rf", "--tb=no",
                        "-k", "test_stereo_fixture or test_geometry"])


def main():
    if len(sys.argv) == 3 and sys.argv[1] == "--one":
        sys.exit(run_one(sys.argv[2]))
    print("| mutation of the restatement | fixture tests that fail |\n|---|---|")
    ok = True
    for name in MUTATIONS:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", name], capture_output=True, text=True, cwd=ROOT)
        failed = [ln.split(" - ")[0].replace("FAILED tests/test_ref_classic.py::", "") for ln in r.stdout.splitlines() if ln.startswith("FAILED")]
        ok = ok and len(failed) > 0
        print(f"| {name} | {len(failed)}: {', '.join(failed) if failed else 'NONE -- the fixtures do not see it'} |")
    base = subprocess.run([sys.executable, "-m", "pytest", os.path.join(ROOT, "tests", "test_ref_classic.py"), "-q", "-p", "no:cacheprovider",
                           "-k", "test_stereo_fixture or test_geometry"], capture_output=True, text=True, cwd=ROOT)
    print(f"| (none) | {'0' if base.returncode == 0 else 'UNMUTATED RUN FAILS'} |")
    sys.exit(0 if ok and base.returncode == 0 else 1)


if __name__ == "__main__":
    main()
