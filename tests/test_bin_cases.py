"""CPU: the conditions test_bin_kernels_gpu.py relies on, asserted from the data
of tests/bin_cases.py.

Regimes: at every chunk size the kernels of csrc/nft_cf.hip use, the layouts
hold a long (> 64) and a short bin that start in one chunk and end in a later
one, a chunk that owns no bin, and (at 2048) a chunk with more than 512 bins.

Reference self-checks: the exact references against np.bincount, against
each other and against their longdouble twins within n * u * sum|terms|.

Discrimination: each exact reference with one documented detail turned wrong
differs bitwise from the right one on the inputs of the GPU tests.
"""
import numpy as np
import pytest

import bin_cases as bc

F64, F32 = np.float64, np.float32


def _layout(name):
    pindex, nb = bc.layout(name)
    perm, offs = bc.csr(pindex, nb)
    return pindex, nb, perm, offs


# ------------------------------------------------------------------ regimes
def test_layout_sizes():
    want = {"A": (7643, 25), "B": (6161, 2500), "B2": (4096, 5000), "D": (7127, 120), "E": (10, 12)}
    for name in bc.LAYOUTS:
        pindex, nb, perm, offs = _layout(name)
        assert (len(pindex), nb) == want[name], name
        bc.assert_valid_csr(pindex, perm, offs, nb)


def test_chunk_sizes():
    assert bc.CHUNKS == (2048, 1024, 512, 256) and bc.LONGB == 64


@pytest.mark.parametrize("ch", bc.CHUNKS)
def test_regimes_per_chunk_size(ch):
    R = {name: bc.regime(name, ch) for name in bc.LAYOUTS}
    i = bc.CHUNKS.index(ch)
    # a long bin that starts in one chunk and ends in a later one
    assert R["A"]["long_straddlers"] == (1, 3, 5, 9)[i]
    assert R["D"]["long_straddlers"] == (1, 2, 7, 15)[i]
    # a short one
    assert R["D"]["short_straddlers"] == (2, 4, 6, 12)[i]
    assert R["B"]["short_straddlers"] >= 1
    # chunks that own no bin
    assert R["A"]["empty_chunks"] == (2, 4, 9, 20)[i]
    # a grid smaller than one chunk
    assert R["E"]["nchunks"] == 1 and R["E"]["npix"] < ch
    # npix an exact multiple of the chunk size; the last chunk owns the trailing empty bins
    assert R["B2"]["npix"] % ch == 0 and R["B2"]["trailing_empty"] >= 7
    if ch == 2048:
        assert R["B"]["max_bins_per_chunk"] == 846 and R["B2"]["max_bins_per_chunk"] > 512


def test_layout_a_lengths():
    r = bc.regime("A", 2048)
    assert r["n64"] == 3 and r["n65"] == 3 and r["max_len"] == 5000
    assert r["leading_empty"] == 2 and r["trailing_empty"] == 2
    ln = np.diff(_layout("A")[3])
    assert 63 in ln and 0 in ln[3:-3]          # 63 beside 64 / 65; an inner empty bin
    r = bc.regime("D", 2048)
    assert r["nlong"] > 10 and r["nbins"] - r["nlong"] > 10


@pytest.mark.parametrize("name", bc.LAYOUTS)
@pytest.mark.parametrize("ch", bc.CHUNKS)
def test_chunk_bins_is_its_definition(name, ch):
    from nifty_amd.operators.distributors import _chunk_bins
    pindex, nb, perm, offs = _layout(name)
    got = _chunk_bins(offs, nb, len(pindex), ch)
    assert got.dtype == np.int32
    np.testing.assert_array_equal(got, bc.chunk_bins_def(offs, nb, len(pindex), ch))


@pytest.mark.parametrize("name", bc.LAYOUTS)
def test_pixel_order_tables(name):
    pindex, nb, perm, offs = _layout(name)
    gpix, gslot = bc.pixel_order(perm, bc.CH_PLAIN)
    for j0 in range(0, len(perm), bc.CH_PLAIN):
        seg, gp, gs = perm[j0:j0 + bc.CH_PLAIN], gpix[j0:j0 + bc.CH_PLAIN], gslot[j0:j0 + bc.CH_PLAIN]
        assert np.all(np.diff(gp) > 0)
        assert np.array_equal(np.sort(gs), np.arange(len(seg)))
        assert np.array_equal(seg[gs], gp)          # slot of each entry in bin-sorted order


# ---------------------------------------------------- reference self-checks
def test_seq_is_the_running_sum():
    for dt in (F64, F32):
        v = bc.values((3, 300), dt, 2)
        assert bc._seq(v).dtype == dt
        np.testing.assert_array_equal(bc._seq(v), bc.seq_loop(v))
        np.testing.assert_array_equal(bc._seq(v, descending=True), bc.seq_loop(v[:, ::-1]))


@pytest.mark.parametrize("name", bc.LAYOUTS)
def test_scatter_seq_is_bincount(name):
    pindex, nb, perm, offs = _layout(name)
    x = bc.values((2, len(pindex), 3), F64, 21)
    got = bc.scatter_seq(x, perm, offs)
    for p in range(2):
        for q in range(3):
            np.testing.assert_array_equal(got[p, :, q], np.bincount(pindex, weights=x[p, :, q], minlength=nb))


@pytest.mark.parametrize("dt", [F64, F32])
@pytest.mark.parametrize("name", bc.LAYOUTS)
def test_scatter_references_within_bound(name, dt):
    pindex, nb, perm, offs = _layout(name)
    x = bc.values((2, len(pindex)), dt, 22)
    ref, n, sa = bc.scatter_ld(x[:, :, None], pindex, nb)
    bnd = bc.bound(n[None, :, None], sa, dt)
    worst = 0.
    for got in (bc.scatter_seq(x[:, :, None], perm, offs), bc.scatter_wave(x, perm, offs)[:, :, None]):
        assert got.dtype == dt
        err = np.abs(got.astype(np.longdouble) - ref)
        assert np.all(err <= bnd)
        worst = max(worst, float(np.max(err[bnd > 0] / bnd[bnd > 0])))
    print(name, dt.__name__, "worst error / bound", worst)
    # short bins of the wave sum are the sequential sum
    short = np.diff(offs) <= bc.LONGB
    np.testing.assert_array_equal(bc.scatter_wave(x, perm, offs)[:, short],
                                  bc.scatter_seq(x[:, :, None], perm, offs)[:, short, 0])


@pytest.mark.parametrize("shape", bc.FOLD_SHAPES)
def test_fold_full_is_bincount_on_the_canonical_cell(shape):
    """the image order (ascending s, axis 0 the MSB) is the ascending raveled
    index of the images"""
    w = bc.values((2,) + shape, F64, 23)
    got = bc.fold_full(w)
    cell = bc.canonical_cell(shape)
    nf = int(np.prod(bc.cell_shape(shape)))
    for p in range(2):
        np.testing.assert_array_equal(got[p].ravel(), np.bincount(cell, weights=w[p].ravel(), minlength=nf))


@pytest.mark.parametrize("dt", [F64, F32])
@pytest.mark.parametrize("shape", bc.FOLD_SHAPES)
def test_fold_references_within_bound(shape, dt):
    w = bc.values((2,) + shape, dt, 24)
    ref, n, sa = bc.fold_ld(w, shape)
    assert n.sum() == np.prod(shape)                      # every pixel is one image of one cell
    full = bc.fold_full(w)
    assert full.dtype == dt
    assert np.all(np.abs(full.astype(np.longdouble) - ref) <= bc.bound(n, sa, dt))
    # the half fold of the pair sums: the same cells' sums, any order
    H = bc.pair_sums(w)
    half = bc.fold_half(H, shape)
    assert half.dtype == dt and half.shape == full.shape
    assert np.all(np.abs(half.astype(np.longdouble) - ref) <= bc.bound(n, sa, dt))
    # and against its own twin on its own input
    refh, nh, sah = bc.fold_ld(H, shape, half=True)
    assert np.all(np.abs(half.astype(np.longdouble) - refh) <= bc.bound(nh, sah, dt))
    srt = bc.fold_half_sorted(H, shape)
    np.testing.assert_array_equal(srt.reshape(-1, 2).T, half.reshape(2, -1))


# ----------------------------------------------------------- discrimination
def _differs(a, b):
    return not np.array_equal(a, b)


@pytest.mark.parametrize("dt", [F64, F32])
def test_wrong_wave_sums_differ(dt):
    pindex, nb, perm, offs = _layout("A")
    ln = np.diff(offs)
    x = bc.values((1, len(pindex)), dt, 31)
    right = bc.scatter_wave(x, perm, offs)
    # threshold >= 64 instead of > 64: only bins of exactly 64 positions change (two orders of one bin may
    # round alike, so not every one has to)
    wrong = bc.scatter_wave(x, perm, offs, longb=bc.LONGB - 1)
    ch = right[0] != wrong[0]
    assert ch[ln == 64].any() and not ch[ln != 64].any()
    # threshold one too high: the bins of 65
    wrong = bc.scatter_wave(x, perm, offs, longb=bc.LONGB + 1)
    ch = right[0] != wrong[0]
    assert ch[ln == 65].any() and not ch[ln != 65].any()
    for kw in (dict(stride=63), dict(tree=bc.TREE[:-1]), dict(descending=True)):
        wrong = bc.scatter_wave(x, perm, offs, **kw)
        ch = right[0] != wrong[0]
        assert ch[ln > bc.LONGB].sum() >= 3, kw
        assert "descending" in kw or not ch[ln <= bc.LONGB].any(), kw
    # a wave sum is not the sequential sum
    seq = bc.scatter_seq(x[:, :, None], perm, offs)[:, :, 0]
    assert (seq[0] != right[0])[ln > bc.LONGB].sum() >= 3


@pytest.mark.parametrize("dt", [F64, F32])
@pytest.mark.parametrize("ch", bc.CHUNKS)
def test_dropped_tail_differs(ch, dt):
    """on every straddling bin, long and short, at every chunk size"""
    seen_long = seen_short = 0
    for name in ("A", "B", "D"):
        pindex, nb, perm, offs = _layout(name)
        x = bc.values((1, len(pindex)), dt, 32)
        r = bc.regime(name, ch)
        ch_ = bc.scatter_wave(x, perm, offs)[0] != bc.scatter_wave(x, perm, offs, drop_tail_ch=ch)[0]
        strad = np.concatenate([r["long_straddler_bins"], r["short_straddler_bins"]])
        assert ch_[strad].all() and ch_.sum() == len(strad), name
        seen_long += r["long_straddlers"]
        seen_short += r["short_straddlers"]
    assert seen_long >= 2 and seen_short >= 2


@pytest.mark.parametrize("dt", [F64, F32])
@pytest.mark.parametrize("name", ["A", "B2", "D", "E"])
def test_descending_sequential_sum_differs(name, dt):
    pindex, nb, perm, offs = _layout(name)
    x = bc.values((1, len(pindex), 1), dt, 33)
    assert _differs(bc.scatter_seq(x, perm, offs), bc.scatter_seq(x, perm, offs, descending=True))


# shapes with a cell of four images: two flipped axes of length >= 3
FOUR_FULL = [s for s in bc.FOLD_SHAPES if sum(n >= 3 for n in s) >= 2]
FOUR_HALF = [s for s in bc.FOLD_SHAPES if sum(n >= 3 for n in s[:-1]) >= 2]


def test_reversed_image_order_differs():
    """(a two-image sum is commutative: only cells of four or more images tell)"""
    assert len(FOUR_FULL) >= 6 and FOUR_HALF == [(3, 4, 5), (5, 6, 2)]
    for dt in (F64, F32):
        for shape in FOUR_FULL:
            w = bc.values((3,) + shape, dt, 34)
            assert _differs(bc.fold_full(w), bc.fold_full(w, reverse=True)), shape
        for shape in FOUR_HALF:
            H = bc.values((3,) + bc.half_shape(shape), dt, 35)
            assert _differs(bc.fold_half(H, shape), bc.fold_half(H, shape, reverse=True)), shape
            assert _differs(bc.fold_half_sorted(H, shape), bc.fold_half_sorted(H, shape, reverse=True)), shape


def test_forward_cpos_differs():
    for shape in bc.FOLD_SHAPES:
        nf = int(np.prod(bc.cell_shape(shape)))
        if nf < 3:
            continue        # every permutation of one or two cells is its own inverse
        cpos = bc.cell_perm(nf, 36)
        H = bc.values((2,) + bc.half_shape(shape), F64, 37)
        right = bc.fold_half_sorted(H, shape, cpos)
        assert _differs(right, bc.fold_half_sorted(H, shape, cpos, forward_cpos=True)), shape
        assert _differs(right, bc.fold_half_sorted(H, shape, None)), shape
        # the definition, element by element
        f = bc.fold_half(H, shape).reshape(2, -1)
        for c in range(0, nf, max(1, nf // 7)):
            for p in range(2):
                assert right[cpos[c] * 2 + p] == f[p, c]
