"""No GPU: every header under csrc/ stands alone.  For each one a translation unit that holds nothing but its #include is
compiled for gfx950 (syntax only, with the flags csrc/build.py builds the library with), so a header that leans on what its
includer happened to define before it — as octav_tail.hpp once did, included in the middle of octav_tail_host.hip — does not
compile.  The headers without HIP in them (the host planning, its error text, the numbers it shares with the kernels, the MX
element formats) must also pass the host compiler alone."""
import glob
import os
import shutil
import subprocess
from concurrent.futures import ThreadPoolExecutor

import pytest

from dipoorlet_amd.csrc import build as hipbuild

CSRC = os.path.dirname(os.path.abspath(hipbuild.__file__))
HEADERS = sorted(os.path.basename(p) for p in glob.glob(os.path.join(CSRC, "*.hpp")))
HOST_ONLY = ("host_plan.hpp", "host_error.hpp", "octav_geometry.hpp", "mx_format.hpp")


def _compile(job):
    """job = (key, command prefix, source suffix, directory) -> (key, return code, compiler output)"""
    key, cmd, suffix, d = job
    src = os.path.join(d, key.replace(".", "_").replace(":", "_") + suffix)
    with open(src, "w") as f:
        f.write('#include "%s"\n' % os.path.join(CSRC, key.split(":")[1]))
    r = subprocess.run(cmd + [src], capture_output=True, text=True)
    return key, r.returncode, r.stdout + r.stderr


@pytest.fixture(scope="module")
def compiled(tmp_path_factory):
    """Every compilation of this module, once, in one pool of 8."""
    d = str(tmp_path_factory.mktemp("csrc_headers"))
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "a host C++ compiler is needed"
    hip = [hipbuild.hipcc_path(), "--offload-arch=gfx950", "-std=c++17", "-ffp-contract=off", "-fsyntax-only"]
    host = [cxx, "-std=c++17", "-fsyntax-only"]
    jobs = [("hip:" + h, hip, ".hip", d) for h in HEADERS] + [("host:" + h, host, ".cpp", d) for h in HOST_ONLY]
    with ThreadPoolExecutor(max_workers=8) as pool:
        return {key: (rc, out) for key, rc, out in pool.map(_compile, jobs)}


def test_the_header_list_is_what_build_py_watches():
    """csrc/build.py rebuilds the library when a header changes: its list must name every header there is."""
    watched = {os.path.basename(p) for p in hipbuild.HDR if os.path.dirname(os.path.abspath(p)) == CSRC}
    assert watched == set(HEADERS)
    assert set(HOST_ONLY) <= set(HEADERS)


@pytest.mark.parametrize("header", HEADERS)
def test_header_compiles_as_first_include_for_gfx950(compiled, header):
    rc, out = compiled["hip:" + header]
    assert rc == 0, out


@pytest.mark.parametrize("header", HOST_ONLY)
def test_header_compiles_with_the_host_compiler_alone(compiled, header):
    rc, out = compiled["host:" + header]
    assert rc == 0, out
