"""CPU: `--smooth_search`'s flag, refusals and selection rule, dpl_mx_smooth_err's declaration, its argument check in a stand-alone
program under the address and undefined-behaviour sanitizers, and apply_smooth with a per-site mapping."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import smooth_model as M
from dipoorlet_amd import _hip
from dipoorlet_amd.__main__ import build_parser, check_args
from dipoorlet_amd.weight_transform.smooth import apply_smooth, choose_candidate, find_smooth_sites

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN = float("nan")
CHECK_MAIN = r"""
#include <stdio.h>
#include <string.h>
#include "mx_plan.hpp"
#define CHECK(c) do { if (!(c)) { printf("line %d: %s (%s)\n", __LINE__, #c, g_err); return 1; } } while (0)
int main() {
    alignas(16) float f[8] = {0};
    double d = 0.0;  int rc = 7; MxTiles t; bool vec = false;      // call(elem, x, w, s, n_cand, m, n, k, ref, part)
    auto call = [&](int32_t e, const float* x, const float* w, const float* s, uint64_t nc, uint64_t m, uint64_t n, uint64_t k, const float* ref,
                    const double* part) { return mx_smooth_check(rc, t, vec, e, x, w, s, nc, m, n, k, ref, part); };
    CHECK(call(DPL_MX_E2M3, nullptr, f, f, 0, 1, 1, 1, f, &d) && rc == -2 && strstr(g_err, "elem must be"));           // elem first
    CHECK(call(DPL_MX_E2M1, nullptr, f, f, 0, 1, 1, 1, f, &d) && rc == 0 && call(DPL_MX_E4M3, f, f, f, 65, 1, 0, 1, f, &d) && rc == 0);
    CHECK(call(DPL_MX_E2M1, nullptr, f, f, 65, 1ull << 31, 1, 1, f, &d) && rc == -2 && strstr(g_err, "must not be null"));
    CHECK(call(DPL_MX_E2M1, f, f, f, 65, 1ull << 31, 1, 1, f, &d) && rc == -2 && strstr(g_err, "[1, 2^31)"));
    CHECK(call(DPL_MX_E2M1, f, f, f, 65, 1, 1, 1, f, &d) && rc == -2 && strstr(g_err, "n_cand must be in [1, 64]"));
    CHECK(call(DPL_MX_E2M1, f, f, f, 64, 0x7FFFFFFFull, 0x7FFFFFFFull, 4, f, &d) && rc == -2 && strstr(g_err, "tensor too large"));
    CHECK(!call(DPL_MX_E4M3, f, f, f, 12, 65, 130, 4, f, &d) && rc == 0 && vec && t.tiles_m == 2 && t.tiles_n == 3 && t.blocks == 72);
    CHECK(!call(DPL_MX_E4M3, f, f, f, 1, 64, 64, 6, f, &d) && !vec && t.blocks == 1);                                    // k % 4
    CHECK(!call(DPL_MX_E4M3, f + 1, f, f, 1, 1, 1, 4, f, &d) && !vec && !call(DPL_MX_E4M3, f, f + 2, f, 1, 1, 1, 4, f, &d) && !vec);      // alignment alone
    CHECK(!call(DPL_MX_E4M3, f, f, f + 3, 1, 1, 1, 4, f, &d) && !vec && !call(DPL_MX_E4M3, f, f, f + 4, 1, 1, 1, 4, f + 1, &d) && vec);
    printf("ok\n");
    return 0;
}
"""
BASE = ["-M", "m.onnx", "-I", "d", "-N", "4", "-A", "minmax", "-D", "ocp_fp8"]


def test_parser_default_and_flag():
    args = build_parser().parse_args(BASE + ["--smooth", "--smooth_search", "--mx", "mxfp4"])
    assert build_parser().parse_args(BASE).smooth_search is False and args.smooth_search is True
    check_args(args)


@pytest.mark.parametrize("extra,words", [(["--mx", "mxfp4"], "needs --smooth"), (["--smooth"], "needs --mx"),
                                         (["--smooth", "--mx", "mxfp6_e2m3"], "not supported with --mx mxfp6_e2m3")])
def test_refusals(extra, words):
    with pytest.raises(ValueError, match=re.escape(words)):
        check_args(build_parser().parse_args(BASE + ["--smooth_search"] + extra))


@pytest.mark.parametrize("errs,want", [([3.0, 1.0, 2.0], 1), ([2.0, 1.0, 1.0, 5.0], 1), ([NAN, 4.0, 3.0, NAN, 3.0], 2), ([1.0, NAN], 0),
                                       ([NAN, NAN, NAN], None), ([0.5] * 12, 0)])
def test_the_smallest_wins_the_earliest_of_equals_a_nan_never(errs, want):
    assert choose_candidate(errs) == want


def test_argument_check_with_the_host_compiler_alone(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    src, exe = tmp_path / "check_main.cpp", tmp_path / "check_main"
    src.write_text(CHECK_MAIN)
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-Wno-unused-function", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "dipoorlet_amd", "csrc"), "-o", str(exe), str(src)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr


def test_header_declares_the_symbol_with_the_binding_arity():
    with open(os.path.join(ROOT, "include", "dipoorlet_hip.h")) as f:
        decl = re.search(r"\bint dpl_mx_smooth_err\(([^)]*)\);", f.read())
    assert decl is not None and "added under 37" in open(os.path.join(ROOT, "dipoorlet_amd", "csrc", "mx_smooth_kernels.hip")).read()
    assert len(decl.group(1).split(",")) == len(_hip.SIGNATURES["dpl_mx_smooth_err"][1]) == 11 and _hip.ABI_VERSION == 37


def test_apply_smooth_takes_a_per_site_mapping():
    g = M.mini_vit()
    sites = find_smooth_sites(g)
    rng = np.random.default_rng(2)
    stats = {s.tensor: (1.0 + 9.0 * rng.random(s.channels)).astype(np.float32) for s in sites}
    alone, folded = sites[1], sites[2]
    got, scales = apply_smooth(g, sites, stats, {**{s.tensor: 0.5 for s in sites}, alone.tensor: None, folded.tensor: 0.3})
    want, want_scales = apply_smooth(g, [folded], stats, 0.3)
    for name in (alone.gamma, alone.beta) + tuple(r.weight for r in alone.readers):
        assert np.asarray(got.get_initializer(name)).tobytes() == np.asarray(g.get_initializer(name)).tobytes()
    for name in (folded.gamma, folded.beta) + tuple(r.weight for r in folded.readers):
        assert np.asarray(got.get_initializer(name)).tobytes() == np.asarray(want.get_initializer(name)).tobytes()
    assert np.array_equal(scales[folded.tensor], want_scales[folded.tensor]) and np.array_equal(scales[alone.tensor], np.ones(alone.channels, np.float32))
