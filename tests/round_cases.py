"""Shared by tests/test_round_oracle_golden.py (CPU: pins oracle/round_oracle.py to torch autograd) and the GPU tests of
csrc/round_kernels.hip (tests/test_round_parity.py, tests/test_sparse_quant.py): comparison helpers, the layouts that
take the kernels' grid-stride loops round a second time, and the small rows with one NaN / ±inf in them."""
import numpy as np

F32 = np.float32
NAN, INF = F32(np.nan), F32(np.inf)


def same_f32(got, want):
    """fp32 bit for bit, except that any NaN equals any NaN and -0.0 equals +0.0 (tests/test_hip_parity._same_f32)."""
    got, want = np.asarray(got, F32), np.asarray(want, F32)
    assert got.shape == want.shape, (got.shape, want.shape)
    return (got.view(np.uint32) == want.view(np.uint32)) | (np.isnan(got) & np.isnan(want)) | ((got == 0) & (want == 0))


def assert_bits(got, want, what=""):
    ok = same_f32(got, want)
    if not ok.all():
        bad = np.argwhere(~ok.reshape(-1))[:4, 0]
        raise AssertionError(f"{what}: {int((~ok).sum())} of {ok.size} differ, first at {bad.tolist()}: got "
                             f"{np.asarray(got).reshape(-1)[bad].tolist()} want {np.asarray(want).reshape(-1)[bad].tolist()}")


def assert_close_specials(got, want, rtol, atol, what=""):
    """NaN, +inf and -inf exactly where `want` has them and nowhere else; every finite value within rtol / atol."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    for f in (np.isnan, np.isposinf, np.isneginf):
        assert np.array_equal(f(got), f(want)), (what, f.__name__, np.argwhere(f(got) != f(want))[:4].tolist())
    fin = np.isfinite(want)
    np.testing.assert_allclose(got[fin], want[fin], rtol=rtol, atol=atol, err_msg=what)


def ulp_distance(a, b):
    """Distance in fp32 representation steps (finite values only; ±0 are one point)."""
    def key(x):
        i = np.asarray(x, F32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)
    return np.abs(key(a) - key(b))


# (name, shape, per_channel): every grid-stride loop of the round / sparse kernels (4096 workgroups of 256 threads) takes a
# second trip for n > 2^20; channel = idx / inner with inner a power of two, odd, one, and n itself
LAYOUTS = (("pt_2p20-1", (2 ** 20 - 1,), False), ("pt_2p20", (2 ** 20,), False), ("pt_2p20+1", (2 ** 20 + 1,), False),
           ("pc_512x512x3x3", (512, 512, 3, 3), True), ("pc_1000x2048", (1000, 2048), True),
           ("pc_257x4099", (257, 4099), True), ("pc_inner1", (2 ** 20 + 77, 1), True))

_LAYOUT_CACHE = {}


def layout_data(name):
    """Host inputs of one layout, generated once per process: weights N(0, 0.1) with one in a thousand set to zero (an exact
    multiple of the scale: alpha_init puts it on the kink of the rectified sigmoid), scale = amax / 100 or amax / 160 so
    that every other channel clamps, an upstream gradient, a 0 / 1 prune mask and a 'trained' round mask (alpha_init + N(0, 2))."""
    if name in _LAYOUT_CACHE:
        return _LAYOUT_CACHE[name]
    from oracle import round_oracle as ro
    _, shape, pc = next(r for r in LAYOUTS if r[0] == name)
    rng = np.random.default_rng(sum(shape) + len(shape))
    w = (rng.standard_normal(shape) * 0.1).astype(F32)
    w.reshape(-1)[rng.integers(0, w.size, w.size // 1000)] = 0
    if pc and shape[-1] == 1 and len(shape) == 2:        # one weight per channel: a scale of its own, never zero
        scale = ((np.abs(w.reshape(-1)) + F32(0.01)) / F32(37.5)).astype(F32)
    elif pc:
        # the channel's extreme at 100 steps (even channels: nothing clamps) or at 160 (odd: the tails clamp at ±127)
        scale = (np.abs(w).reshape(shape[0], -1).max(1) / np.where(np.arange(shape[0]) % 2, F32(160), F32(100))).astype(F32)
    else:
        scale = (np.abs(w).max(keepdims=True).reshape(1) / F32(100)).astype(F32)
    d = {"shape": shape, "pc": pc, "w": w, "scale": scale, "qmin": np.full_like(scale, -127), "qmax": np.full_like(scale, 127),
         "G": rng.standard_normal(shape).astype(F32), "G2": rng.standard_normal(shape).astype(F32),
         "G3": rng.standard_normal(shape).astype(F32), "prune": (rng.random(shape) < 0.5).astype(F32)}
    d["wfloor"], d["alpha0"] = ro.alpha_init(w, scale)
    d["trained"] = (d["alpha0"] + rng.standard_normal(shape).astype(F32) * F32(2)).astype(F32)
    _LAYOUT_CACHE[name] = d
    return d


def kink(mask):
    """Elements whose rectified sigmoid sits on a corner of the clamp: the raw value (zeta - gamma) * sigmoid(a) + gamma,
    evaluated in fp64 from the fp32 mask with the fp32 constants, within 16 * 2^-23 of 0 or of 1.  There one ulp of expf
    decides between dh = 0 and dh ~ 0.0917, on the reference's hardware as much as here."""
    a = np.asarray(mask, F32).astype(np.float64)
    with np.errstate(over="ignore"):
        raw = float(F32(1.1 - -0.1)) / (1.0 + np.exp(-a)) + float(F32(-0.1))
    tol = 16 * 2.0 ** -23
    return (np.abs(raw) <= tol) | (np.abs(raw - 1.0) <= tol)


# ---- rows with one special value: [2, 8] arrays, per-channel power-of-two scales; each case puts ONE NaN / +inf / -inf at
# element (1, 3) of one input.  test_round_oracle_golden.py pins the oracle on exactly these rows against torch autograd.
SPECIAL_AT = (1, 3)
SPECIAL_VALUES = (("nan", NAN), ("+inf", INF), ("-inf", -INF))


def special_base():
    rng = np.random.default_rng(77)
    scale = np.array([2.0 ** -7, 2.0 ** -6], F32)
    w = (rng.standard_normal((2, 8)) * 0.3).astype(F32)
    w[0, 0], w[1, 0] = 1.5, -3.0                       # clamps at +127 / -127 (w / scale = 192 / -192)
    return {"w": w, "scale": scale, "qmin": np.full(2, -127, F32), "qmax": np.full(2, 127, F32),
            "mask": (rng.standard_normal((2, 8)) * 2).astype(F32), "G": rng.standard_normal((2, 8)).astype(F32),
            "prune": (rng.random((2, 8)) < 0.6).astype(F32), "z": rng.standard_normal((2, 8)).astype(F32),
            "t": rng.standard_normal((2, 8)).astype(F32), "x": (rng.standard_normal((2, 8)) * 3).astype(F32),
            "r": rng.random((2, 8)).astype(F32)}


def special_cases(fields):
    """[(id, dict)]: the base row, then one special value in one of `fields` at a time."""
    out = [("base", special_base())]
    for f in fields:
        for name, v in SPECIAL_VALUES:
            d = special_base()
            d[f][SPECIAL_AT] = v
            # the prune mask drops nothing at the special element, and the ReLU row has it on the side it would hide
            d["prune"][SPECIAL_AT] = 1
            out.append((f"{f}={name}", d))
    return out
