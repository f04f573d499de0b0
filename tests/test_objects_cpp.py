"""The C++ mirrors of the objects, spaces and get calls (CPU, host leg): GetObjects, BlobObject<T>,
GetSpaces and Get of include/storm_blocks.hpp compile with -Wall -Wextra -Werror and get objects
back from a store the program builds itself: by typed IDs, by the results of GetObjectIDs read in
place, by the roots GetSpaces hands out, and by Get from the singularity (tests/cpp/get_test.cpp)."""
import os
import subprocess

from tests.conftest import ROOT


def test_cpp_mirror_gets_objects_on_the_host_leg():
    from storm_amd import build as b
    out = os.path.join(ROOT, "tests", "cpp", "build", "get_test")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    libdir = os.path.dirname(b.LIB)
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "get_test.cpp"), "-o", out, "-L", libdir, "-lstormck",
                    f"-Wl,-rpath,{libdir}"], check=True)
    r = subprocess.run([out], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stderr
