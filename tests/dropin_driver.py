"""Builds and runs the C++ drivers of tests/cpp against the drop-in headers of include/ and librover_fe.so: the one compiler command the
driver tests share, as the reference builds (-std=c++14, CMakeLists.txt:12) with -Wall -Werror."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "rover-slam_amd")


def build(tmp_path, name, macros=(), link=True):
    """tests/cpp/<name>.cpp with -D<macro> for every macro -> tmp_path/<name> (link=False: <name>.o only); returns the path"""
    out = str(tmp_path / (name if link else name + ".o"))
    cmd = ["g++", "-std=c++14", "-O1", "-Wall", "-Werror", *("-D" + m for m in macros), "-I" + os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "cpp", name + ".cpp"), "-o", out]
    cmd += ["-L" + LIB, "-lrover_fe", "-L/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath," + LIB, "-Wl,-rpath,/opt/rocm/lib"] if link else ["-c"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    return out


def run(exe, *args, **kw):
    """the completed process of exe with args (env, cwd, ... as subprocess.run takes them); it must exit 0"""
    r = subprocess.run([exe, *(str(a) for a in args)], capture_output=True, text=True, **kw)
    assert r.returncode == 0, r.stdout + r.stderr
    return r
