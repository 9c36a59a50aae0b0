"""Shared by test_fft_cases.py (host) and test_fft_engines_gpu.py (device):
the extended-precision references of the native transforms (csrc/nft_fft.hip),
a normwise error bound derived from the transform lengths, the per-item error
measure, the launch labels a plain ``hartley`` call has to leave in a
LaunchProfile, and the case tables: one case per kernel instantiation, tile
tail and launch configuration of the two engines, each naming the regime it
has to be in.  Not a test module."""
import math
import zlib
from collections import namedtuple

import numpy as np

U64 = 2.0 ** -53     # unit roundoff, float64
U32 = 2.0 ** -24     # unit roundoff, float32
LD = np.longdouble

POW2 = tuple(1 << p for p in range(3, 15))      # 8 .. 16384
ROWS_N = POW2[:11]                              # engine-v2 row passes: 8 .. 8192
STRIDED_N = POW2[:7]                            # engine-v2 strided passes: 8 .. 512
FOURSTEP_N = POW2[7:]                           # four-step first axis: 1024 .. 16384
TILE_VALUES = 16                                # values per thread of an engine-v2 tile


# ------------------------------------------------------------------ references
def ref_fft(x, axes, inverse=False):
    """Unnormalised DFT over ``axes`` in extended precision (complex256);
    inverse=True is the unnormalised backward transform."""
    import scipy.fft
    x = np.asarray(x)
    z = x.astype(np.clongdouble if np.iscomplexobj(x) else LD)
    axes = tuple(axes)
    if not axes:
        return z.astype(np.clongdouble)
    if inverse:
        return np.conj(scipy.fft.fftn(np.conj(z), axes=axes))
    return scipy.fft.fftn(z, axes=axes)


def ref_hartley(x, axes, convention=0):
    """Re F + s Im F in extended precision: s = +1 for convention 0 (the
    reference's default), s = -1 for convention 1 (canonical)."""
    f = ref_fft(x, axes)
    return f.real + f.imag if convention == 0 else f.real - f.imag


# ------------------------------------------------------------------ error bound
def direct_dft(n):
    """make_plan's rule (csrc/nft_fft.hip): radices 8, 4, 2, 3, 5, 7 in that
    order; what is left over, or no stage at all, means a direct DFT."""
    m, stages = n, 0
    for r in (8, 4, 2, 3, 5, 7):
        while m % r == 0:
            m, stages = m // r, stages + 1
    return m != 1 or stages == 0


def unit_roundoff(dtype):
    """dtype: "f64" / "f32" or a real or complex numpy dtype"""
    if dtype in ("f64", "f32"):
        return U64 if dtype == "f64" else U32
    return U64 if np.dtype(dtype) in (np.dtype(np.float64), np.dtype(np.complex128)) else U32


def bound(shape, axes, dtype):
    """Normwise relative error bound of one item (one independent transform):
    u (2 + sum_a 8 ceil(log2 N_a)) over the factored axes -- Higham's
    log2(N) growth of an FFT with correctly rounded twiddles, with room for the
    mixed radices, the pair split and the scale -- plus u (N_a + 8) for every
    direct-DFT axis, the normwise worst case of an N-term inner product."""
    c = 2.0
    for a in set(int(a) % len(shape) for a in axes):
        n = int(shape[a])
        c += n + 8 if direct_dft(n) else 8 * math.ceil(math.log2(n))
    return unit_roundoff(dtype) * c


def item_errors(out, ref, item_axes):
    """l2 error of every item of the batch over that item's own l2 norm
    (extended precision); item_axes are the axes one item spans."""
    out = np.asarray(out)
    ref = np.asarray(ref)
    assert out.shape == ref.shape, (out.shape, ref.shape)
    ax = tuple(sorted(set(int(a) % max(ref.ndim, 1) for a in item_axes)))
    d = out.astype(np.clongdouble if np.iscomplexobj(ref) or np.iscomplexobj(out) else LD) - ref
    num = np.sqrt(np.sum(np.abs(d) ** 2, axis=ax))
    den = np.sqrt(np.sum(np.abs(ref) ** 2, axis=ax))
    tiny = np.finfo(np.float64).tiny
    return np.asarray(num / np.maximum(den, tiny), dtype=np.float64).ravel()


def mirror(a, axes):
    """a(-k) over ``axes``: every transformed coordinate negated modulo its length."""
    axes = tuple(axes)
    if not axes:
        return a
    return np.roll(np.flip(a, axes), 1, axes)


# ------------------------------------------------------------------ launch labels
def rows_supported(n):
    return n in ROWS_N


def strided_supported(n):
    return n in STRIDED_N


def fourstep_supported(n):
    return n in FOURSTEP_N


def expected_labels(shape, axes):
    """LaunchProfile labels of a plain ``hartley`` call: the three predicates
    of csrc/fast_dispatch.hpp plus "the half axis is the last dimension".
    The generic engine places no marks."""
    nd = len(shape)
    ax = sorted(set(int(a) % nd for a in axes)) if nd else []
    m = len(ax)
    if m == 0 or ax[-1] != nd - 1 or not rows_supported(shape[-1]):
        return []
    if m == 1:
        return ["fft_h1d"]
    if not all(strided_supported(shape[a]) for a in ax[1:-1]):
        return []
    n0 = shape[ax[0]]
    if strided_supported(n0):
        return ["fft_r2c"] + ["fft_c2c"] * (m - 2) + ["fft_unpack"]
    if fourstep_supported(n0):
        return ["fft_r2c"] + ["fft_c2c"] * (m - 1) + ["fft_unpack"]
    return []


# ------------------------------------------------------------------ tile geometry of engine v2
def nt_rows(n):
    return 256 if n <= 2048 else (512 if n == 4096 else 1024)


def nt_strided(n):
    return 256 if n <= 128 else (512 if n == 256 else 1024)


def pair_lines_per_tile(n):
    """pair lines (two real rows each) of one row-pass tile"""
    return nt_rows(n) * TILE_VALUES // n


def lines_per_tile_strided(n):
    return nt_strided(n) * TILE_VALUES // n


def half_ext(n):
    """complex extent of the half spectrum along a last axis of length n"""
    return (n // 2 + 1 + 7) // 8 * 8


# ------------------------------------------------------------------ cases
# op: "hartley" or "c2c"; dtype: "f64" / "f32" (complex128 / complex64 for c2c)
# regime: dict(engine=..., nt=..., tail=..., plus the numbers the sanity test checks)
Case = namedtuple("Case", "id group op shape axes dtype convention scale regime")

DTYPES = ("f64", "f32")


def np_dtype(c):
    return np.float64 if c.dtype == "f64" else np.float32


def case_input(c, shape=None):
    """the case's input, already rounded to the device dtype (float64 array
    holding float32 values for f32 cases); complex for c2c"""
    shape = tuple(c.shape if shape is None else shape)
    key = f"{c.op}{shape}{c.axes}".encode()
    rng = np.random.default_rng(zlib.crc32(key))
    x = rng.standard_normal(shape)
    if c.op == "c2c":
        x = x + 1j * rng.standard_normal(shape)
        return x.astype(np.complex128 if c.dtype == "f64" else np.complex64)
    return x.astype(np_dtype(c))


_REF = {}


def case_fft(c, shape=None, inverse=False):
    """extended-precision DFT of the case's input, computed once per (input,
    axes, direction) and shared by the conventions and tests that need it;
    read-only"""
    shape = tuple(c.shape if shape is None else shape)
    key = (c.op, shape, c.axes, c.dtype, inverse)
    if key not in _REF:
        f = ref_fft(case_input(c, shape), c.axes, inverse=inverse)
        f.setflags(write=False)
        _REF[key] = f
    return _REF[key]


def case_ref(c, shape=None, inverse=False, scale=None):
    """scale * reference output of the case in extended precision"""
    f = case_fft(c, shape, inverse)
    s = LD(c.scale if scale is None else scale)
    if c.op == "c2c":
        return s * f
    return s * (f.real + f.imag if c.convention == 0 else f.real - f.imag)


def scipy_same_precision(c, shape=None):
    """scipy's transform of the case in the case's own precision"""
    import scipy.fft
    x = case_input(c, shape)
    f = scipy.fft.fftn(x, axes=c.axes) if c.axes else x.astype(np.complex128 if c.dtype == "f64" else np.complex64)
    s = np_dtype(c)(c.scale)
    if c.op == "c2c":
        return s * f
    return s * (f.real + f.imag if c.convention == 0 else f.real - f.imag)


def _v2(nt, tail, **kw):
    return dict(engine="v2", nt=nt, tail=tail, **kw)


def _gen(nt, tail, **kw):
    return dict(engine="generic", nt=nt, tail=tail, **kw)


def _conv_tag(cv):
    return "nc" if cv == 0 else "c"


def cases_a():
    """v2 row H1D: two tiles, the second partial, the last pair a single row"""
    out = []
    for n in ROWS_N:
        lp = pair_lines_per_tile(n)
        rows = 2 * lp + 3
        for dt in DTYPES:
            for cv in (0, 1):
                out.append(Case(f"a-h1d-rows{n}-{dt}-{_conv_tag(cv)}", "a", "hartley", (rows, n), (1,), dt, cv, 0.3,
                                _v2(nt_rows(n), "second tile partial, last pair one row", kinds=("H1D",), rows_n=n,
                                    pair_lines=(rows + 1) // 2, tile=lp, real_rows=rows)))
    return out


def cases_b():
    """v2 R2C rows of every length and strided UNPACK of every length, with an
    untransformed leading axis"""
    out = []
    for n in ROWS_N:
        for dt in DTYPES:
            for cv in (0, 1):
                out.append(Case(f"b-r2c-rows{n}-{dt}-{_conv_tag(cv)}", "b", "hartley", (3, 8, n), (1, 2), dt, cv, 1.0,
                                _v2(nt_rows(n), "unpack tiles partial, untransformed outer axis",
                                    kinds=("R2C", "UNPACK"), rows_n=n, strided_n=8, lines=half_ext(n),
                                    tile=lines_per_tile_strided(8))))
    for m in STRIDED_N:
        for dt in DTYPES:
            for cv in (0, 1):
                out.append(Case(f"b-unpack-strided{m}-{dt}-{_conv_tag(cv)}", "b", "hartley", (3, m, 8), (1, 2), dt, cv,
                                1.0, _v2(nt_strided(m), "unpack tiles partial, untransformed outer axis",
                                         kinds=("R2C", "UNPACK"), rows_n=8, strided_n=m, lines=half_ext(8),
                                         tile=lines_per_tile_strided(m))))
    return out


def cases_c():
    """v2 middle-axis strided C2C of every length"""
    out = []
    for m in STRIDED_N:
        for dt in DTYPES:
            out.append(Case(f"c-c2c-strided{m}-{dt}", "c", "hartley", (8, m, 8), (0, 1, 2), dt, 0, 1.0,
                            _v2(nt_strided(m), "middle tiles partial", kinds=("R2C", "C2C", "UNPACK"), rows_n=8,
                                strided_n=m, lines=half_ext(8), tile=lines_per_tile_strided(m))))
    for dt in DTYPES:
        out.append(Case(f"c-c2c-4d-{dt}", "c", "hartley", (8, 16, 8, 32), (0, 1, 2, 3), dt, 0, 1.0,
                        _v2(256, "two middle axes", kinds=("R2C", "C2C", "C2C", "UNPACK"), rows_n=32, strided_n=16,
                            lines=8 * half_ext(32), tile=lines_per_tile_strided(16))))
    return out


def fourstep_split(n):
    p = n.bit_length() - 1
    n2 = 1 << (p // 2)
    return n // n2, n2


def cases_d():
    """four-step first axis: strided C2C of length N1 with the post-twiddle,
    then strided UNPACK of length N2 writing k = m + N1 x and its mirror"""
    out = []
    for n0 in FOURSTEP_N:
        n1, n2 = fourstep_split(n0)
        for shape, axes, tag in (((n0, 8), (0, 1), "2d"), ((3, n0, 8), (1, 2), "batch3")):
            for dt in DTYPES:
                for cv in (0, 1):
                    out.append(Case(f"d-fourstep{n0}-{tag}-{dt}-{_conv_tag(cv)}", "d", "hartley", shape, axes, dt, cv,
                                    0.3, _v2(nt_strided(n2), "four-step mirror index, scale != 1",
                                             kinds=("R2C", "C2C", "UNPACK"), rows_n=8, fourstep_n=n0, n1=n1, n2=n2)))
    return out


PERSIST_TILE_REALS = 8192      # real values of one R2C row tile at 256 threads


def persist_batch(n, ncu):
    """smallest leading batch of (B, 8, n) whose R2C row pass has at least
    8 ncu + 3 tiles (B items are 4 B pair lines; a tile holds 4096 / n of them)"""
    lp = pair_lines_per_tile(n)
    want = 8 * ncu + 3
    return -(-((want - 1) * lp + 1) // 4)


def persist_tiles(batch, n):
    return -(-4 * batch // pair_lines_per_tile(n))


def cases_e(ncu=256):
    """persistent R2C loop: more tiles than the grid of 8 workgroups per CU,
    so the prefetched second iteration runs.  At n = 64 the batch gives exactly
    8 ncu + 3 tiles, the last one partial; at n = 2048 an item is two whole
    tiles, so the count is even: 8 ncu + 4."""
    out = []
    for n, dt in ((2048, "f32"), (64, "f32"), (2048, "f64")):
        b = persist_batch(n, ncu)
        out.append(Case(f"e-persist-rows{n}-{dt}", "e", "hartley", (b, 8, n), (1, 2), dt, 0, 1.0,
                        _v2(256, "second loop iteration", kinds=("R2C", "UNPACK"), rows_n=n, strided_n=8,
                            grid=8 * ncu, ntiles=persist_tiles(b, n), tile=pair_lines_per_tile(n),
                            host_shape=(16, 8, n))))
    return out


def cases_f():
    """generic engine: odd extents of the pair modes, length-1 and empty axes,
    a half axis that is not last"""
    table = [
        ((16, 3), (0,), 1.0, "strided pair, odd inner extent", dict(odd=3)),
        ((4, 6, 5), (0, 1), 1.0, "strided pair, odd inner extent", dict(odd=5)),
        ((5, 12, 7), (1,), 1.0, "strided pair, odd inner extent", dict(odd=7)),
        ((6, 10, 3), (0, 1), 1.0, "strided pair, odd inner extent", dict(odd=3)),
        ((7, 30), (1,), 1.0, "rows pair, odd row count", dict(odd=7)),
        ((64, 1), (0, 1), 1.0, "length-1 axis", dict(one=1)),
        ((1, 64), (0, 1), 1.0, "length-1 axis", dict(one=0)),
        ((5, 7), (), 2.0, "no axes", dict()),
        ((6, 9, 4, 5), (0, 1), 1.0, "half axis not last, negated by the unpack", dict(half=1)),
    ]
    out = []
    for shape, axes, scale, tail, extra in table:
        name = "x".join(map(str, shape)) + "-ax" + "".join(map(str, axes))
        for dt in DTYPES:
            for cv in (0, 1):
                out.append(Case(f"f-{name}-{dt}-{_conv_tag(cv)}", "f", "hartley", shape, axes, dt, cv, scale,
                                _gen(256, tail, **extra)))
    return out


# generic-engine launch configurations of the plan cases: (length, dtypes,
# threads, dynamic LDS bytes of a (3, n) complex128 / complex64 row pass,
# factored or direct).  Recorded from the dispatch's choice; the GPU tests do
# not depend on these numbers, the sanity test checks their arithmetic.
PLAN_LENGTHS = [
    # n, dtypes, NT, lds c128, lds c64, kind
    (210, DTYPES, 256, 13552, 6832, "every radix"),
    (3000, DTYPES, 256, 48040, 24040, "NT 256"),
    (4800, DTYPES, 512, 76840, 38440, "NT 512"),
    (6000, DTYPES, 512, 96040, 48040, "NT 512"),
    (8192, DTYPES, 512, 131112, 65576, "NT 512, power of two"),
    (10000, DTYPES, 1024, 160040, 80040, "NT 1024"),
    (10080, DTYPES, 1024, 161320, 80680, "NT 1024, every radix"),
    (251, DTYPES, 256, 16176, 8144, "direct"),
    (1021, DTYPES, 256, 65456, 32784, "direct"),
    (2310, DTYPES, 256, 37000, 18520, "direct"),
    (4099, DTYPES, 512, 65624, 32832, "direct"),
    (12288, ("f32",), 1024, None, 98344, "fp32 only"),
    (14336, ("f32",), 1024, None, 114728, "fp32 only"),
    (16384, ("f32",), 1024, None, 131112, "fp32 only"),
]
LDS_OPT_IN = 65536     # dynamic LDS above this needs the per-kernel opt-in
LDS_MAX = 163840


def cases_g():
    """generic engine plans: every thread count, LDS up to the ceiling, direct DFTs"""
    out = []
    for n, dts, nt, l64, l32, kind in PLAN_LENGTHS:
        for dt in dts:
            lds = l64 if dt == "f64" else l32
            reg = _gen(nt, kind, n=n, lds=lds, direct=kind == "direct")
            if n not in ROWS_N:   # (3, 8192) is an engine-v2 row pass; see g-hartley-8192x6
                out.append(Case(f"g-hartley-{n}-{dt}", "g", "hartley", (3, n), (1,), dt, 0, 1.0, reg))
            out.append(Case(f"g-c2c-{n}-{dt}", "g", "c2c", (3, n), (1,), dt, 0, 1.0, reg))
    for dt in DTYPES:
        out.append(Case(f"g-hartley-8192x6-{dt}", "g", "hartley", (8192, 6), (0,), dt, 0, 1.0,
                        _gen(512, "strided pair H1D", n=8192, lds=131128 if dt == "f64" else 65584, direct=False)))
        out.append(Case(f"g-c2c-strided2048x3-{dt}", "g", "c2c", (2048, 3), (0,), dt, 0, 1.0,
                        _gen(256, "strided C2C, odd inner extent", n=2048, lds=32824 if dt == "f64" else 32848,
                             direct=False)))
        out.append(Case(f"g-hartley-6000x6-{dt}", "g", "hartley", (6000, 6), (0, 1), dt, 0, 1.0,
                        _gen(512, "strided UNPACK", n=6000, lds=96056 if dt == "f64" else 48048, direct=False)))
        out.append(Case(f"g-c2c-6000x6-{dt}", "g", "c2c", (6000, 6), (0, 1), dt, 0, 1.0,
                        _gen(512, "strided C2C", n=6000, lds=96056 if dt == "f64" else 48048, direct=False)))
    return out


# refusals: (id, op, shape, axes, dtype, the length the message has to name)
REFUSALS = [
    ("h-10240-f64-hartley", "hartley", (2, 10240), (1,), "f64", 10240),
    ("h-10240-f64-c2c", "c2c", (2, 10240), (1,), "f64", 10240),
    ("h-16411-f64-hartley", "hartley", (2, 16411), (1,), "f64", 16411),
    ("h-16411-f32-hartley", "hartley", (2, 16411), (1,), "f32", 16411),
    ("h-16411-f64-c2c", "c2c", (2, 16411), (1,), "f64", 16411),
    ("h-16411-f32-c2c", "c2c", (2, 16411), (1,), "f32", 16411),
    ("h-16384x6-f64-hartley", "hartley", (16384, 6), (0,), "f64", 16384),
]


def all_cases(ncu=256):
    return cases_a() + cases_b() + cases_c() + cases_d() + cases_e(ncu) + cases_f() + cases_g()


def instantiations():
    """every engine-v2 instantiation reachable from nft_hartley:
    (tiling, kind, length, dtype)"""
    out = []
    for dt in DTYPES:
        for n in ROWS_N:
            out += [("rows", "H1D", n, dt), ("rows", "R2C", n, dt)]
        for n in STRIDED_N:
            out += [("strided", "C2C", n, dt), ("strided", "UNPACK", n, dt)]
        for n in FOURSTEP_N:
            out.append(("fourstep", "C2C+UNPACK", n, dt))
    return out


def case_instantiations(c):
    """the engine-v2 instantiations case c launches"""
    r = c.regime
    if r["engine"] != "v2":
        return set()
    out = set()
    kinds = r["kinds"]
    if "H1D" in kinds:
        out.add(("rows", "H1D", r["rows_n"], c.dtype))
    if "R2C" in kinds:
        out.add(("rows", "R2C", r["rows_n"], c.dtype))
    if "fourstep_n" in r:
        out.add(("fourstep", "C2C+UNPACK", r["fourstep_n"], c.dtype))
        out.add(("strided", "C2C", r["n1"], c.dtype))
        out.add(("strided", "UNPACK", r["n2"], c.dtype))
        return out
    ax = sorted(c.axes)
    if "UNPACK" in kinds:
        out.add(("strided", "UNPACK", c.shape[ax[0]], c.dtype))
    for a in ax[1:-1]:
        out.add(("strided", "C2C", c.shape[a], c.dtype))
    return out


def instantiation_table(ncu=256):
    """instantiation -> id of the first case that launches it"""
    first = {}
    for c in all_cases(ncu):
        for inst in sorted(case_instantiations(c)):
            first.setdefault(inst, c.id)
    return [(inst, first.get(inst)) for inst in instantiations()]
