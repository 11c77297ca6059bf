"""CPU: the C-ABI library loads and exports every symbol include/rover_fe.h declares; the drop-in C++
headers compile and link against it; without a GPU every entry point fails loudly (no CPU fallback)."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import dropin_driver as DD

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared_symbols():
    text = open(os.path.join(ROOT, "include", "rover_fe.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(rfe_[a-z0-9_]+)\s*\(", text)))


def test_library_exports_every_declared_symbol():
    from rover_slam_amd import capi
    syms = _declared_symbols()
    assert len(syms) >= 25
    for s in syms:
        assert hasattr(capi.lib, s), f"librover_fe.so does not export {s}"
    assert set(capi.EXPORTS) == set(syms)
    assert capi.lib.rfe_weight_count(1) == 1300865 and capi.lib.rfe_weight_count(2) == 11321153
    assert b"gfx950" in capi.lib.rfe_version()


def test_no_cpu_fallback_without_gpu():
    import torch
    if torch.cuda.device_count() > 0:
        pytest.skip("GPU present")
    from rover_slam_amd import capi
    with pytest.raises(capi.RfeError) as e:
        capi.Context(0)
    assert "no HIP device" in str(e.value) or "hip" in str(e.value).lower()
    # NULL ctx is rejected, not dereferenced
    assert capi.lib.rfe_synchronize(None) < 0


def test_weight_container_roundtrip(tmp_path):
    from rover_slam_amd import weights as Wt
    blob = Wt.make_superpoint(seed=3)
    p = str(tmp_path / "sp.rfew")
    Wt.save(p, blob, 1)
    back, kind = Wt.load(p)
    assert kind == 1 and np.array_equal(back, blob)
    assert Wt.SP_COUNT == 1300865 and Wt.LG_COUNT == 11321153
    # the manifest is the canonical layout: contiguous, complete
    man, n = Wt.lg_manifest()
    off = 0
    for _, o, shape in man:
        assert o == off
        off += int(np.prod(shape))
    assert off == n


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_shim_headers_compile_and_link(tmp_path):
    """include/Extractors/SPextractor.h, include/Matchers/SPmatcher.h, include/SuperPoint.h and
    include/super_glue.h build without OpenCV / onnxruntime and link against librover_fe.so."""
    assert os.path.exists(DD.build(tmp_path, "shim_driver"))


# the drivers of tests/cpp that document NO_DEVICE, with the macros each is built with
NO_DEVICE = "without arguments: compile / link check only"
NO_DEVICE_DRIVERS = [("projection_search_driver", ()), ("sim3_search_driver", ()), ("local_points_driver", ()),
                     ("local_points_driver", ("RFE_SP_PYRAMID=1",)), ("triangulation_driver", ()), ("pose_opt_driver", ()),
                     ("sim3_solver_driver", ()), ("bow_driver", ())]


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
@pytest.mark.parametrize("name,macros", NO_DEVICE_DRIVERS, ids=["-".join((n,) + m) for n, m in NO_DEVICE_DRIVERS])
def test_drop_in_driver_compiles_links_and_runs_without_arguments(tmp_path, name, macros):
    """every drop-in header of include/rfe with its driver, -std=c++14 -Wall -Werror; the run without arguments touches no device"""
    DD.run(DD.build(tmp_path, name, macros))


def test_every_driver_with_a_no_device_run_is_listed():
    cpp = os.path.join(ROOT, "tests", "cpp")
    documented = {f[:-4] for f in os.listdir(cpp) if f.endswith(".cpp") and NO_DEVICE in open(os.path.join(cpp, f)).read()}
    assert documented == {name for name, _ in NO_DEVICE_DRIVERS}


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_spmatcher_in_tree_mode_cxx14(tmp_path):
    """-DRFE_WITH_ROVER_SLAM: include/Matchers/SPmatcher.h only DECLARES (full member list of the reference class) and a
    reference-style SPmatcher.cc -- out-of-line constants, constructor and MatchingPoints_onnx bodies written against
    Ort::Value (rfe/ort_compat) -- compiles against it with -std=c++14 -Wall -Werror; the constants are defined exactly
    once (no C++17 inline variables in the header) and the object links against librover_fe.so."""
    stubs = os.path.join(ROOT, "tests", "cpp", "rover_slam_stubs")
    obj = str(tmp_path / "bodies.o")
    cmd = ["g++", "-std=c++14", "-O1", "-Wall", "-Werror", "-DRFE_WITH_ROVER_SLAM", "-I" + os.path.join(ROOT, "include"),
           "-I" + os.path.join(ROOT, "include", "rfe", "ort_compat"), "-I" + stubs, "-c", os.path.join(stubs, "onnx_matcher_bodies.cc"), "-o", obj]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    nm = subprocess.run(["nm", "-C", obj], capture_output=True, text=True).stdout
    for sym in ("ORB_SLAM3::SPmatcher::TH_HIGH", "ORB_SLAM3::SPmatcher::TH_LOW", "ORB_SLAM3::SPmatcher::HISTO_LENGTH"):
        defs = [l for l in nm.splitlines() if l.endswith(sym) and l.split()[-2] in "RDrdB"]
        assert len(defs) == 1, (sym, nm)
    main = tmp_path / "main.cc"
    main.write_text("int rfe_in_tree_probe();\nint main() { return rfe_in_tree_probe() == 31 ? 0 : 1; }\n")
    exe = str(tmp_path / "probe")
    r = subprocess.run(["g++", "-std=c++14", str(main), obj, "-o", exe, "-L" + os.path.join(ROOT, "rover-slam_amd"), "-lrover_fe",
                        "-L/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath," + os.path.join(ROOT, "rover-slam_amd"), "-Wl,-rpath,/opt/rocm/lib"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    # the stand-alone header, and the rfe drop-ins with rfe/dropin_detail.h, in a second translation unit next to the first: no duplicate
    # definitions in C++14 either
    for i in (1, 2):
        (tmp_path / f"tu{i}.cc").write_text('#include "Matchers/SPmatcher.h"\n#include "rfe/projection_search.h"\n#include "rfe/local_points_search.h"\n#include "rfe/sim3_search.h"\n'
                                            '#include "rfe/triangulation.h"\n#include "rfe/pose_optimization.h"\n#include "rfe/sim3_solver.h"\n'
                                            'float tu%d() { return ORB_SLAM3::SPmatcher::TH_HIGH; }\n' % i)
    (tmp_path / "tumain.cc").write_text("float tu1(); float tu2(); int main() { return tu1() == tu2() ? 0 : 1; }\n")
    r = subprocess.run(["g++", "-std=c++14", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(tmp_path / "tu1.cc"), str(tmp_path / "tu2.cc"),
                        str(tmp_path / "tumain.cc"), "-o", str(tmp_path / "tu"), "-L" + os.path.join(ROOT, "rover-slam_amd"), "-lrover_fe",
                        "-L/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath," + os.path.join(ROOT, "rover-slam_amd"), "-Wl,-rpath,/opt/rocm/lib"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
