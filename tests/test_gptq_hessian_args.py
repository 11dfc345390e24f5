"""CPU: --gptq_hessian's parser default and refusal, the places that declare the C ABI of the device Hessian, and its host-only
plan header (csrc/gptq_hessian_plan.hpp) built by the host compiler alone into a program of its own, under the address and
undefined-behaviour sanitizers, that checks the row split over a sweep of (rows, K)."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PLAN_MAIN = r"""
#include <stdio.h>
#include "gptq_hessian_plan.hpp"
#define CHECK(c) do { if (!(c)) { printf("rows %lld k %lld: %s\n", (long long)rows, (long long)k, #c); return 1; } } while (0)
int main() {
    const int64_t ks[] = {1, 63, 64, 65, 200, 576, 768, 2048, 4608, 16384};
    const int64_t rs[] = {1, 31, 32, 33, 1023, 1024, 2047, 2048, 4096, 12608, 65536, 200704, 1000003, 802816 * 4, kGhMaxRows};
    for (int64_t k : ks)
        for (int64_t rows : rs) {
            const GhPlan p = gh_plan(k, rows), again = gh_plan(k, rows);
            CHECK(p.splits == again.splits && p.range_rows == again.range_rows && p.bytes == again.bytes);      // (rows, K) alone
            CHECK(p.splits >= 1 && p.range_rows % 32 == 0 && p.range_rows > 0);
            CHECK(p.tiles == (uint64_t)p.nt * (p.nt + 1) / 2 && (int64_t)p.nt * 64 >= k && ((int64_t)p.nt - 1) * 64 < k);
            uint64_t next = 0;                                            // every row exactly once, ranges on multiples of 32
            for (uint32_t s = 0; s < p.splits; ++s) {
                CHECK(p.begin(s) == next && p.begin(s) % 32 == 0 && p.end(s) > p.begin(s) && p.end(s) - p.begin(s) <= p.range_rows);
                next = p.end(s);
            }
            CHECK(next == (uint64_t)rows);
            CHECK(p.bytes == (p.splits > 1 ? (uint64_t)p.splits * p.tiles * 4096 * 8 : 0));
            CHECK(p.splits == 1 || rows / p.splits >= 1024);        // the floor on a range's rows
        }
    int64_t rows = 4096, k = 64;
    CHECK(gh_plan(k, rows).splits >= 4);
    double h = 0.0;
    float x = 0.0f;
    dpl_gptq_hessian_geom g = {2, 3, 9, 8, 3, 3, 1, 1, 1, 1, 1, 1, 1, 1};
    CHECK(gh_check(&x, &g, 27, 2 * 9 * 8, &h, nullptr, 0) == 0);
    CHECK(gh_check(&x, &g, 28, 2 * 9 * 8, &h, nullptr, 0) == -2 && gh_check(&x, &g, 27, 2 * 9 * 8 + 1, &h, nullptr, 0) == -2);
    g.kh = 12;      // the window no longer fits: 9 + 2 < 12
    CHECK(gh_check(&x, &g, 3 * 12 * 3, 0, &h, nullptr, 0) == -2);
    CHECK(gh_check(&x, nullptr, 0, 1, &h, nullptr, 0) == -2 && gh_check(&x, nullptr, 16385, 1, &h, nullptr, 0) == -2);
    CHECK(gh_check(nullptr, nullptr, 64, 1, &h, nullptr, 0) == -2 && gh_check(&x, nullptr, 64, 4096, &h, &h, 8) == -2);
    CHECK(gh_check(&x, nullptr, 64, 0, &h, nullptr, 0) == 0);
    printf("ok\n");
    return 0;
}
"""


def test_flag_default_refusal_and_abi():
    from dipoorlet_amd import _hip
    from dipoorlet_amd.__main__ import build_parser, check_args
    base = ["-M", "m.onnx", "-I", "in", "-N", "1", "-D", "ocp_fp8", "-A", "minmax"]
    assert build_parser().parse_args(base).gptq_hessian == "blas"
    check_args(build_parser().parse_args(base + ["--gptq", "--gptq_hessian", "device", "--gptq_factor", "device"]))
    check_args(build_parser().parse_args(base + ["--mx", "mxfp4", "--mx_gptq", "--gptq_hessian", "device"]))
    with pytest.raises(ValueError, match="--gptq_hessian device needs --gptq or --mx_gptq"):
        check_args(build_parser().parse_args(base + ["--gptq_hessian", "device"]))
    header = open(os.path.join(ROOT, "include", "dipoorlet_hip.h")).read()
    assert "added under 37" in header
    for name, n_args in (("dpl_gptq_hessian_workspace", 2), ("dpl_gptq_hessian", 8)):
        decl = re.search(r"^\w+ " + name + r"\(([^;]*)\);", header, re.M | re.S)
        assert decl is not None and len(decl.group(1).split(",")) == n_args == len(_hip.SIGNATURES[name][1]), name
    fields = re.search(r"typedef struct dpl_gptq_hessian_geom \{(.*?)\}", header, re.S).group(1)
    assert re.findall(r"(\w+)[,;]", fields) == [f[0] for f in _hip.GptqHessianGeom._fields_]


def test_plan_header_with_the_host_compiler_alone(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "a host C++ compiler is needed"
    src, exe = tmp_path / "plan_main.cpp", tmp_path / "plan_main"
    src.write_text(PLAN_MAIN)
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-Wno-unused-function", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "dipoorlet_amd", "csrc"), "-o", str(exe), str(src)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr
