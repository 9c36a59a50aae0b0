"""Host checks of tests/fft_cases.py: the extended-precision references
reproduce the reference project's own outputs (tests/golden/dispatch.npz),
scipy's same-precision transforms stay inside the derived bound on every case
(so the reference alone passes it), and the case tables' own arithmetic holds."""
import numpy as np
import pytest

import fft_cases as fc
from conftest import golden

G = golden("dispatch.npz")
NC = int(G["ncases"])
CASES = fc.all_cases()


def _rel(a, b):
    return float(np.linalg.norm((a - b).ravel()) / max(np.linalg.norm(np.asarray(b).ravel()), 1e-300))


# ------------------------------------------------------------------ references against the fixture
@pytest.mark.parametrize("i", range(NC))
def test_ref_reproduces_golden(i):
    x = G[f"c{i}_x"]
    z = G[f"c{i}_z"]
    axes = tuple(int(a) for a in G[f"c{i}_axes"])
    assert _rel(fc.ref_hartley(x, axes, 0), G[f"c{i}_h_nc"]) < 1e-14
    assert _rel(fc.ref_hartley(x, axes, 1), G[f"c{i}_h_c"]) < 1e-14
    assert _rel(fc.ref_fft(z, axes), G[f"c{i}_fft"]) < 1e-14
    ntot = int(np.prod([z.shape[a] for a in axes]))
    assert _rel(fc.ref_fft(z, axes, inverse=True) / ntot, G[f"c{i}_ifft"]) < 1e-14
    # the fixture's float32 output, against the reference of the rounded input
    x32 = x.astype(np.float32)
    e = fc.item_errors(G[f"c{i}_h32_nc"], fc.ref_hartley(x32, axes, 0), range(x.ndim))
    assert e.max() <= fc.bound(x.shape, axes, "f32")


def test_ref_dtypes():
    x = np.arange(12.).reshape(3, 4)
    assert fc.ref_fft(x, (1,)).dtype == np.clongdouble
    assert fc.ref_hartley(x, (0, 1), 1).dtype == np.longdouble
    assert fc.ref_fft(x, ()).dtype == np.clongdouble
    # a real even sequence has a real spectrum: both conventions agree
    ev = np.array([1., 2., 3., 2.])
    assert np.array_equal(fc.ref_hartley(ev, (0,), 0), fc.ref_hartley(ev, (0,), 1))
    # H(-k) of convention 0 is H(k) of convention 1
    y = np.random.default_rng(0).standard_normal((5, 6))
    assert _rel(fc.mirror(fc.ref_hartley(y, (0, 1), 0), (0, 1)), fc.ref_hartley(y, (0, 1), 1)) < 1e-18


# ------------------------------------------------------------------ bound, errors, labels
def test_bound_values():
    assert fc.bound((3, 8192), (1,), "f64") == fc.U64 * (2 + 8 * 13)
    assert fc.bound((7, 1021), (1,), np.float64) == fc.U64 * (2 + 1021 + 8)
    assert fc.bound((5, 16384, 8), (1, 2), np.complex64) == fc.U32 * (2 + 8 * 14 + 8 * 3)
    assert fc.bound((4, 6), (), "f32") == fc.U32 * 2
    assert fc.bound((4, 6), (-1, 1), "f64") == fc.U64 * (2 + 8 * 3)   # a repeated axis counts once


def test_direct_dft_rule():
    assert [n for n in (1, 11, 19, 46, 251, 1021, 2310, 4099, 16411) if not fc.direct_dft(n)] == []
    assert [n for n in (2, 7, 21, 210, 3000, 4800, 6000, 8192, 10000, 10080, 12288, 14336, 16384)
            if fc.direct_dft(n)] == []


def test_item_errors_do_not_dilute():
    rng = np.random.default_rng(1)
    ref = rng.standard_normal((1000, 64)).astype(np.longdouble)
    out = np.array(ref, dtype=np.float64)
    out[617] *= 1 + 1e-10
    e = fc.item_errors(out, ref, (1,))
    assert e.shape == (1000,)
    assert int(np.argmax(e)) == 617 and 0.9e-10 < e[617] < 1.1e-10
    assert np.delete(e, 617).max() <= fc.U64
    # one Frobenius norm over the batch hides the bad line by sqrt(1000)
    assert _rel(out, ref) < e[617] / 30
    # items over the first axis; a zero item does not divide by zero
    z = np.zeros((4, 3))
    assert np.array_equal(fc.item_errors(z, z.astype(np.longdouble), (0,)), np.zeros(3))


@pytest.mark.parametrize("shape,axes,labels", [
    ((5, 64), (1,), ["fft_h1d"]),
    ((5, 8192), (1,), ["fft_h1d"]),
    ((5, 16384), (1,), []),
    ((64, 5), (0,), []),
    ((64, 64), (0, 1), ["fft_r2c", "fft_unpack"]),
    ((512, 8), (0, 1), ["fft_r2c", "fft_unpack"]),
    ((1024, 8), (0, 1), ["fft_r2c", "fft_c2c", "fft_unpack"]),
    ((16384, 8), (0, 1), ["fft_r2c", "fft_c2c", "fft_unpack"]),
    ((32768, 8), (0, 1), []),
    ((3, 2048, 8), (1, 2), ["fft_r2c", "fft_c2c", "fft_unpack"]),
    ((16, 16, 16), (0, 1, 2), ["fft_r2c", "fft_c2c", "fft_unpack"]),
    ((8, 16, 8, 32), (0, 1, 2, 3), ["fft_r2c", "fft_c2c", "fft_c2c", "fft_unpack"]),
    ((1024, 1024, 8), (0, 1, 2), []),        # only the first axis may be four-step
    ((8, 12, 10), (0, 2), []),
    ((6, 9, 4, 5), (0, 1), []),
    ((64, 64, 4), (0, 1), []),               # half axis not last
    ((4, 4), (0, 1), []),
    ((5, 7), (), []),
])
def test_expected_labels(shape, axes, labels):
    assert fc.expected_labels(shape, axes) == labels


# ------------------------------------------------------------------ the tables
def test_case_ids_unique_and_regimes_stated():
    ids = [c.id for c in CASES]
    assert len(ids) == len(set(ids))
    for c in CASES:
        assert c.regime["engine"] in ("v2", "generic") and c.regime["nt"] in (256, 512, 1024) and c.regime["tail"], c.id
        assert c.id.startswith(c.group + "-") and c.dtype in fc.DTYPES and c.op in ("hartley", "c2c"), c.id
        if c.op == "hartley":
            # the engine the case claims is the one the dispatch rules give it
            assert bool(fc.expected_labels(c.shape, c.axes)) == (c.regime["engine"] == "v2"), c.id
        assert int(np.prod(c.shape)) <= 10 ** 7 or c.group == "e", c.id


def test_every_v2_instantiation_has_a_case():
    table = fc.instantiation_table()
    assert len(table) == 2 * (2 * 11 + 2 * 7 + 5)
    assert [inst for inst, cid in table if cid is None] == []


def test_table_arithmetic():
    for c in fc.cases_a():
        r = c.regime
        assert r["tile"] * r["rows_n"] == r["nt"] * fc.TILE_VALUES, c.id
        # two tiles, the second short of real rows (of whole pair lines too, above two lines per tile)
        assert r["tile"] < r["pair_lines"] <= 2 * r["tile"] and r["real_rows"] < 4 * r["tile"], c.id
        assert r["real_rows"] % 2 == 1 and r["pair_lines"] == (r["real_rows"] + 1) // 2, c.id
    for c in fc.cases_b() + fc.cases_c():
        r = c.regime
        assert r["lines"] % r["tile"] != 0, c.id                          # partial last tile of the strided passes
        assert r["tile"] * r["strided_n"] == fc.nt_strided(r["strided_n"]) * fc.TILE_VALUES, c.id
        assert c.shape[-1] == r["rows_n"], c.id
    for c in fc.cases_b():
        assert sorted(c.axes)[0] == 1 and c.shape[0] == 3, c.id           # an untransformed outer axis
    for c in fc.cases_d():
        r = c.regime
        assert r["n1"] * r["n2"] == r["fourstep_n"] and r["n1"] >= r["n2"] and r["n1"] <= 2 * r["n2"], c.id
        assert fc.strided_supported(r["n1"]) and fc.strided_supported(r["n2"]), c.id
        assert c.shape[sorted(c.axes)[0]] == r["fourstep_n"] and c.scale != 1.0, c.id
    for ncu in (256, 304, 64):
        for c in fc.cases_e(ncu):
            r = c.regime
            assert r["grid"] == 8 * ncu and r["ntiles"] >= r["grid"] + 3, c.id
            assert r["ntiles"] == -(-(c.shape[0] * 4) // r["tile"]), c.id
            assert r["tile"] * 2 * r["rows_n"] == fc.PERSIST_TILE_REALS, c.id
            # the smallest such batch: one item fewer falls short
            assert fc.persist_tiles(c.shape[0] - 1, r["rows_n"]) < r["grid"] + 3, c.id
            assert r["host_shape"][1:] == c.shape[1:], c.id
    for c in fc.cases_f():
        r = c.regime
        if "odd" in r:
            ax = sorted(c.axes)
            # the extent the pair mode pairs up: the rows before a last-axis line,
            # the flattened inner dims after the half axis otherwise
            h = ax[-1]
            ext = int(np.prod(c.shape[:h])) if h == len(c.shape) - 1 else int(np.prod(c.shape[h + 1:]))
            assert ext % 2 == 1 and ext == r["odd"], c.id
        if "one" in r:
            assert c.shape[r["one"]] == 1 and r["one"] in c.axes, c.id
        if "half" in r:
            assert sorted(c.axes)[-1] == r["half"] != len(c.shape) - 1, c.id
    seen_nt = set()
    for n, dts, nt, l64, l32, kind in fc.PLAN_LENGTHS:
        assert fc.direct_dft(n) == (kind == "direct"), n
        seen_nt.add(nt)
        for dt, lds in (("f64", l64), ("f32", l32)):
            if dt not in dts:
                assert lds is None, n
                continue
            es = 16 if dt == "f64" else 8
            # whole lines of n complex values plus the per-line table and the pad
            lines, rest = divmod(lds - 16, n * es + 24)
            assert rest == 0 and lines >= 1 and lds <= fc.LDS_MAX, (n, dt)
    assert seen_nt == {256, 512, 1024}
    big = [c.id for c in fc.cases_g() if c.regime["lds"] > fc.LDS_OPT_IN]
    assert {"g-c2c-4800-f64", "g-c2c-6000-f64", "g-c2c-10000-f64", "g-c2c-10080-f64", "g-c2c-16384-f32",
            "g-hartley-8192x6-f64", "g-hartley-6000x6-f64"} <= set(big)
    for cid, op, shape, axes, dt, n in fc.REFUSALS:
        assert n in shape and shape[axes[0]] == n, cid


# ------------------------------------------------------------------ scipy inside the bound
@pytest.mark.parametrize("c", CASES, ids=[c.id for c in CASES])
def test_scipy_inside_bound(c):
    shape = c.regime.get("host_shape", c.shape)   # the persistent-loop cases with a short batch
    item_axes = c.axes
    b = fc.bound(shape, c.axes, c.dtype)
    e = fc.item_errors(fc.scipy_same_precision(c, shape), fc.case_ref(c, shape), item_axes)
    assert e.max() <= b, (e.max(), b)
    if c.op == "c2c":
        import scipy.fft
        n = int(np.prod([shape[a] for a in c.axes]))
        z = fc.case_input(c, shape)
        inv = scipy.fft.ifftn(z, axes=c.axes)
        e = fc.item_errors(inv, fc.case_ref(c, shape, inverse=True, scale=1.0 / n), item_axes)
        assert e.max() <= b, (e.max(), b)
