"""GPU: the public CSR entry points nft_spmv_csr, nft_spmv_scaled and
nft_csr_rowblocks (include/nifty_amd.h) against scipy CSR in float64 on the
same arrays.

Three kernels with row-length-dependent loop bounds:
  vector  one wave per row, four gathers per lane while j + 192 < hi, then a
          64-strided tail: row lengths around 64, 192, 256 and 448 (+ one lane)
          and a row of 1000; nrows % 4 != 0 (four rows per workgroup).
  thread  one thread per row (nnz / nrows < 32): 1003 rows of 0 .. 8 entries.
  stream  host-built row blocks (<= 256 rows, <= 2048 nonzeros, a longer row on
          its own): more than 256 consecutive short rows, a run that crosses
          the nonzero cap, one row of 5000, empty rows at both ends and inside.

Tolerance, per element (los_cases.bound64 / bound32): |got - ref| <=
2 (n_i + 4) 2^-53 (|A| |v|)_i, scales included, plus 2^-24 |ref| for fp32
storage (inputs cast first); an empty row gives exactly 0."""
import ctypes

import numpy as np
import pytest
import torch

import los_cases as lc

pytestmark = pytest.mark.gpu

DT = {"f64": torch.float64, "f32": torch.float32}
NCOLS = 777
VECTOR_ROWS = [0, 1, 63, 64, 65, 191, 192, 193, 255, 256, 257, 448, 449, 1000, 33]
STREAM_ROWS = ([0] * 3 + [1, 2, 3] * 100 + [0] * 5 + [100] * 40 + [0, 7, 0] + [5000] + [2, 9, 2048, 1, 2047, 2]
               + [0] * 4)


def _matrix(lens, seed):
    rng = np.random.default_rng(seed)
    indptr = np.r_[0, np.cumsum(lens)].astype(np.int64)
    nnz = int(indptr[-1])
    indices = rng.integers(0, NCOLS, nnz).astype(np.int32)
    weights = rng.random(nnz).astype(np.float32) - np.float32(0.3)
    return indptr, indices, weights


class Mat:
    def __init__(self, lens, seed, dev):
        import scipy.sparse
        self.indptr, self.indices, self.weights = _matrix(lens, seed)
        self.nrows, self.n = len(lens), np.asarray(lens)
        # copies: scipy may sort a row's indices in place; the kernels get the arrays as drawn
        # (unsorted, with repeated columns)
        self.A = scipy.sparse.csr_matrix((self.weights.astype(np.float64), self.indices.copy(), self.indptr.copy()),
                                         shape=(self.nrows, NCOLS))
        self.Aabs = abs(self.A)
        self.dev = dev
        self.d = tuple(torch.from_numpy(a).to(dev) for a in (self.indptr, self.indices, self.weights))
        rng = np.random.default_rng(seed + 1)
        self.x = rng.standard_normal(NCOLS)
        self.cs = (rng.random(NCOLS) + 0.5) * np.where(rng.random(NCOLS) < 0.5, -1., 1.)
        self.rs = (rng.random(self.nrows) + 0.5) * np.where(rng.random(self.nrows) < 0.5, -1., 1.)

    def up(self, a, dt):
        t = torch.from_numpy(np.ascontiguousarray(a)).to(dt).to(self.dev)
        return t, t.double().cpu().numpy()

    def check(self, y, xn, csn, rsn, scale, dt, what):
        v = xn if csn is None else csn * xn
        ref, mag = scale * (self.A @ v), abs(scale) * (self.Aabs @ np.abs(v))
        if rsn is not None:
            ref, mag = rsn * ref, np.abs(rsn) * mag
        g = y.double().cpu().numpy()
        assert not np.isnan(g).any(), f"{what}: unwritten output"
        bnd = lc.bound64(self.n, mag) if dt == torch.float64 else lc.bound32(self.n, mag, ref)
        err, pos = np.abs(g - ref), bnd > 0
        print(f"{what}: max err / bound {float((err[pos] / bnd[pos]).max()):.3e}")
        assert np.all(err[~pos] == 0.) and np.all(err <= bnd), what


@pytest.mark.parametrize("dtn", list(DT))
def test_spmv_csr_vector_kernel(dev, dtn):
    from nifty_amd import _native
    dt = DT[dtn]
    M = Mat(VECTOR_ROWS, 1, dev)
    assert M.nrows % 4 != 0 and M.indices.size // M.nrows >= 32
    x, xn = M.up(M.x, dt)
    y = torch.full((M.nrows,), float("nan"), dtype=dt, device=dev)
    _native.spmv_csr(*M.d, x, y, scale=1.5)
    M.check(y, xn, None, None, 1.5, dt, f"spmv_csr vector {dtn}")


@pytest.mark.parametrize("dtn", list(DT))
def test_spmv_csr_thread_kernel(dev, dtn):
    from nifty_amd import _native
    dt = DT[dtn]
    lens = np.random.default_rng(2).integers(0, 9, 1003)
    M = Mat(list(lens), 3, dev)
    assert M.indices.size // M.nrows < 32 and (lens == 0).any() and (lens == 8).any()
    x, xn = M.up(M.x, dt)
    y = torch.full((M.nrows,), float("nan"), dtype=dt, device=dev)
    _native.spmv_csr(*M.d, x, y, scale=-0.75)
    M.check(y, xn, None, None, -0.75, dt, f"spmv_csr thread {dtn}")


def test_csr_rowblocks_invariants(dev):
    from nifty_amd import _native
    M = Mat(STREAM_ROWS, 5, dev)
    rb = _native.csr_rowblocks(M.indptr)
    assert rb.dtype == np.int32 and rb[0] == 0 and rb[-1] == M.nrows and np.all(np.diff(rb) >= 1)
    rows, nnz = np.diff(rb), np.diff(M.indptr[rb])
    assert rows.max() == 256                       # the run of short rows fills a block by row count
    assert np.all(rows <= 256) and np.all((nnz <= 2048) | (rows == 1))
    long_row = STREAM_ROWS.index(5000)
    i = int(np.searchsorted(rb, long_row, side="right")) - 1
    assert rb[i] == long_row and rb[i + 1] == long_row + 1 and nnz[i] == 5000
    assert (nnz > 2048).sum() == 1 and ((nnz > 1900) & (rows > 1)).any()   # a block cut by the nonzero cap
    assert (nnz == 2048).any()                     # the cap itself is allowed


@pytest.mark.parametrize("blocks", ["rowblocks", "vector"])
@pytest.mark.parametrize("has_rs", [False, True], ids=["nors", "rs"])
@pytest.mark.parametrize("has_cs", [False, True], ids=["nocs", "cs"])
@pytest.mark.parametrize("dtn", list(DT))
def test_spmv_scaled(dev, dtn, has_cs, has_rs, blocks):
    from nifty_amd import _native
    dt = DT[dtn]
    M = Mat(STREAM_ROWS, 5, dev)
    rb = torch.from_numpy(_native.csr_rowblocks(M.indptr)).to(dev) if blocks == "rowblocks" else None
    x, xn = M.up(M.x, dt)
    cs, csn = M.up(M.cs, dt) if has_cs else (None, None)
    rs, rsn = M.up(M.rs, dt) if has_rs else (None, None)
    y = torch.full((M.nrows,), float("nan"), dtype=dt, device=dev)
    _native.spmv_scaled(*M.d, rb, x, y, colscale=cs, rowscale=rs, scale=1.25)
    M.check(y, xn, csn, rsn, 1.25, dt, f"spmv_scaled {blocks} {dtn} cs={has_cs} rs={has_rs}")


def test_spmv_argument_errors(dev):
    from nifty_amd import _native
    lib = _native.load()
    M = Mat(STREAM_ROWS, 5, dev)
    # nft_csr_rowblocks: a block array too small for the blocks needed
    blocks = np.empty(8, dtype=np.int32)
    nb = ctypes.c_int64(0)
    for cap in (4, 0):
        with pytest.raises(_native.NativeError):
            _native._check(lib.nft_csr_rowblocks(M.indptr.ctypes.data, M.nrows, blocks.ctypes.data, cap,
                                                 ctypes.byref(nb)))
    # a dtype code that is neither fp64 (0) nor fp32 (1): refused before any launch
    x, _ = M.up(M.x, torch.float64)
    y = torch.full((M.nrows,), float("nan"), dtype=torch.float64, device=dev)
    P = _native.ptr
    with pytest.raises(_native.NativeError, match="bad dtype"):
        _native._check(lib.nft_spmv_csr(P(M.d[0]), P(M.d[1]), P(M.d[2]), P(x), P(y), M.nrows, 7, 1.0,
                                        M.indices.size, _native.stream_ptr()))
    with pytest.raises(_native.NativeError, match="bad dtype"):
        _native._check(lib.nft_spmv_scaled(P(M.d[0]), P(M.d[1]), P(M.d[2]), None, 0, P(x), None, None, P(y),
                                           M.nrows, 7, 1.0, _native.stream_ptr()))
    torch.cuda.synchronize()
    assert torch.isnan(y).all(), "a rejected call wrote"
    # the Python binding refuses other dtypes itself
    with pytest.raises(TypeError):
        _native.spmv_csr(*M.d, x.half(), y.half())
