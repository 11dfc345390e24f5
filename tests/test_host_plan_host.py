"""No GPU: csrc/host_plan.hpp — the HOST planning of the C ABI, every table the streaming kernels index with — compiled by the
host compiler into a stand-alone program (tests/host_plan_host.cpp, with the address, leak and undefined-behaviour sanitizers),
which must end clean, equal the shipped library byte for byte on the same inputs, and satisfy what tests/host_plan_checks.py
states.  The library is called on the CPU through the _hip wrappers: none of these entry points touches a device.  Its plan's
tables stay inside it (only dpl_octav_plan_upload reads them), so the program's copies are held to the library's builders, to
dpl_octav_list_cap and to the offsets of the library's bound jobs."""
import ctypes as C
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import host_plan_checks as K
from dipoorlet_amd import _hip
from dipoorlet_amd.csrc import build as hipbuild

HERE = os.path.dirname(os.path.abspath(__file__))
BASE = 1 << 40
CALLS = [(call, fb) for call in (0, 8, 9, 16) for fb in (0, 1)]          # the jobs host_plan_host.cpp binds, in its order
ITEM = np.dtype([("offset", "<u8"), ("count", "<u4"), ("seg", "<u4"), ("slot", "<u4"), ("reserved", "<u4")])


def _cases(cap):
    """(spans, n_tensors — 0: no plan —, n_blocks, chunk_elems)"""
    for spans, nb in K.balanced_sets():
        yield spans, 0, nb, 1 << 20
    for spans in K.slice_sets(cap):
        yield spans, len(spans), 64, 1 << 20
    big = 5 * 10 ** 9                                                     # shares above 2^32 - 1024; far too large for a plan
    yield [(0, 0, big, 0)], 1, 1, 0xFFFFFC00
    yield [(0, 64, big, 0), (1, 0, 1000, 1)], 0, 7, 1 << 30
    for nb in (1, 7, 4099):                                               # fewer aligned pieces than blocks
        yield [(0, 0, 3000, 0), (1, 16, 1, 1), (2, 0, 2048, 2)], 3, nb, 1024
    yield [(0, 0, 0, 0), (1, 0, 5000, 1), (2, 8, 777, 2)], 3, 7, 2048     # zero-count spans: first, last, all of them
    yield [(0, 0, 5000, 0), (1, 8, 777, 1), (2, 0, 0, 2)], 1, 7, 2048
    yield [(0, 0, 0, 0), (1, 0, 0, 1)], 2, 7, 2048
    yield [(i, 4 * i, n, i) for i, n in enumerate([1, 3, 20480, 20481, cap, cap + 1, 3 * cap + 5, 64 * cap])], 4, 512, 1 << 20
    yield [(0, 0, 1000, 0), (1, 0, 65 * cap, 1)], 2, 64, 1 << 20          # 65 slices: refused
    yield [], 0, 7, 1024                                                  # n_spans = 0
    yield [(0, 0, 5000, 0), (1, 16, 1024, 1)], 2, 2, 1000                 # chunk_elems not a multiple of 1024


class _Records:
    def __init__(self, raw):
        self.raw, self.at = raw, 0

    def take(self):
        n, = struct.unpack_from("<Q", self.raw, self.at)
        out = self.raw[self.at + 8:self.at + 8 + n]
        self.at += 8 + (n + 7) // 8 * 8
        assert len(out) == n
        return out

    def i64(self):
        return struct.unpack("<q", self.take())[0]

    def items(self):
        return np.frombuffer(self.take(), ITEM)

    def arr(self, dt):
        return np.frombuffer(self.take(), dt).tolist()


def _tuples(a, reserved=False):
    f = ("seg", "offset", "count", "slot") + (("reserved",) if reserved else ())
    return list(zip(*(a[k].tolist() for k in f))) if len(a) else []


@pytest.fixture(scope="module")
def program_output(tmp_path_factory):
    hipbuild.build()
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "a host C++ compiler is needed"
    d = tmp_path_factory.mktemp("hostplan")
    exe = str(d / "host_plan_host")
    subprocess.run([cxx, "-O1", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(HERE, "host_plan_host.cpp"), "-o", exe], check=True)
    cases = list(_cases(_hip.lib().dpl_octav_slice_cap()))
    words = [len(cases)]
    for spans, T, nb, chunk in cases:
        words += [len(spans), T, nb, chunk] + [w for seg, off, cnt, slot in spans for w in (seg, off, cnt, slot)]
    words += [len(K.SIX_STATES)] + [w for s in K.SIX_STATES for w in s]
    np.array(words, np.uint64).tofile(d / "in.u64")
    r = subprocess.run([exe, str(d / "in.u64"), str(d / "out.bin")], capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "", r.stderr               # clean: no sanitizer report, no leak
    return cases, _Records(open(d / "out.bin", "rb").read())


def _plan(L, R, spans, T, nb, cap, slices, ps, items, bb):
    arr, ns = _hip._span_array(spans)
    plan = L.dpl_octav_plan_create(C.addressof(arr), ns, T, nb)
    assert bool(plan) == bool(R.i64())
    if not plan:
        assert R.take() == L.dpl_last_error() and b"slices" in L.dpl_last_error()
        return
    try:
        z = _hip.OctavWorkspaceSizes()
        assert L.dpl_octav_plan_sizes(plan, C.byref(z)) == 0
        assert R.take() == bytes(z)
        elems = [sp[2] for sp in spans]
        K.check_plan_sizes(z, elems, T, cap, L.dpl_octav_list_cap)
        offs = R.arr("<u8")
        # the eight tables: what the builders made of the same spans, the spans themselves, the list regions, the pair order
        assert R.take() == slices.tobytes() and R.arr("<u4") == ps
        assert R.take() == bytes(arr)[:24 * ns]
        base, full = K.list_regions(elems, cap, L.dpl_octav_list_cap)
        assert R.arr("<u8") == base and R.arr("<u8") == full
        assert R.arr("<u4") == sorted(range(ns), key=lambda i: (-elems[i], i))
        assert R.take() == items.tobytes() and R.arr("<u4") == bb
        sizes = [24 * max(len(slices), 1), 8 * ns, 24 * ns, 8 * (ns + 1), 8 * (ns + 1), 4 * ns, 24 * max(len(items), 1), 4 * (nb + 1)]
        assert offs[0] == 0 and offs[8] == z.tables_bytes
        assert all(offs[k + 1] == offs[k] + (sizes[k] + 255) // 256 * 256 for k in range(8))   # 256-byte table offsets, no overlap
        for call, fb in CALLS:
            addr = (BASE, BASE + (1 << 30), BASE + (2 << 30), BASE + (3 << 30), BASE + (4 << 30), BASE + (5 << 30),
                    BASE + (7 << 30) if fb else None, BASE + (6 << 30))
            job = _hip.OctavOnereadJob()
            assert L.dpl_octav_plan_bind(plan, *addr, call, call & 1, 20, C.byref(job)) == 0
            theirs = R.take()
            assert theirs == bytes(job)
            for j in (job, _hip.OctavOnereadJob.from_buffer_copy(theirs)):
                K.check_job(j, z, addr, call, call & 1, 20)
                assert [getattr(j, f) - BASE for f in K.TABLE_FIELDS] == offs[:8]
    finally:
        L.dpl_octav_plan_destroy(plan)


def test_host_build_of_the_planning_equals_the_library(program_output):
    cases, R = program_output
    L = _hip.lib()
    cap = L.dpl_octav_slice_cap()
    seen = set()
    for spans, T, nb, chunk in cases:
        # dpl_build_work_items
        n = R.i64()
        if chunk % 1024:
            with pytest.raises(_hip.DipoorletHipError):
                _hip.build_work_items(spans, chunk)
            assert n == -2 and R.take() == L.dpl_last_error() and b"1024" in L.dpl_last_error()
            assert R.take() == b""
            seen.add("chunk")
        else:
            arr, n_lib = _hip.build_work_items(spans, chunk)
            got = R.items()
            assert n == n_lib == len(got) and got.tobytes() == bytes(arr)[:24 * n]
            K.check_work_items(spans, chunk, _tuples(got))
        # dpl_build_balanced_items
        arr, n_lib, bb_lib = _hip.build_balanced_items(spans, nb)
        n, items, bb = R.i64(), R.items(), R.arr("<u4")
        assert n == n_lib == len(items) and items.tobytes() == bytes(arr)[:24 * n] and bb == list(bb_lib)
        K.check_balanced(spans, nb, _tuples(items), bb)
        if n and int(items["count"].max()) == 0xFFFFFC00:
            seen.add("share above 2^32 - 1024")
        if n < nb:
            seen.add("fewer pieces than blocks")
        # dpl_build_octav_slices
        n = R.i64()
        lib = _hip.build_octav_slices(spans)
        if lib is None:
            assert n == -3 and R.take() == L.dpl_last_error() and b"slices" in L.dpl_last_error()
            assert R.take() == b"" and not any(R.arr("<u4"))
            slices = ps = None
            seen.add("refused")
        else:
            slices, ps = R.items(), R.arr("<u4")
            assert n == lib[1] == len(slices) and slices.tobytes() == bytes(lib[0])[:24 * n] and ps == list(lib[2])[:2 * len(spans)]
            if [sp[3] for sp in spans] == list(range(len(spans))):
                K.check_slices(spans, cap, _tuples(slices, True), ps)
            if spans and n == 0:
                seen.add("all empty")
        if T:
            _plan(L, R, spans, T, nb, cap, slices, ps, items, bb)
    assert seen == {"chunk", "share above 2^32 - 1024", "fewer pieces than blocks", "refused", "all empty"}
    # dpl_octav_fallback_layout: the six states of test_octav_fallback_layout_host; a null argument fails with its message
    want = K.fallback_layout(K.SIX_STATES)
    st = (_hip.OctavState * (len(K.SIX_STATES) + 1))()
    for i, (mode, done, elems) in enumerate(K.SIX_STATES):
        st[i].mode, st[i].done, st[i].n_elems = mode, done, elems
    base = np.full(len(want), 99, np.uint64)
    assert L.dpl_octav_fallback_layout(C.addressof(st), len(K.SIX_STATES), base.ctypes.data) == want[-1] == R.i64() == 1024 + 64
    assert R.arr("<u8") == want == base.tolist()
    assert L.dpl_octav_fallback_layout(None, 6, base.ctypes.data) == R.i64() == -2 and R.take() == L.dpl_last_error()
    assert R.at == len(R.raw)
