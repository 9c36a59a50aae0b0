"""Shared by test_bin_cases.py (host) and test_bin_kernels_gpu.py (device):
bin layouts, fold shapes and two references for every operation of
csrc/nft_cf.hip (power-bin gather, scatter and mirror fold).  Not a test
module; numpy only.

Exact references restate the summation order the kernels document, in the
kernel's storage type (np.float64 / np.float32 arithmetic from +0), so a
kernel is held to them bit for bit:

  gather            out[p, i, q] = in[p, pindex[i], q]
  scatter_seq       per (p, b, q) the running sum over perm[offs[b]:offs[b+1]]
                    in ascending position (fp64: np.bincount, the reference's
                    special_add_at)
  scatter_wave      bins of <= LONGB positions as scatter_seq; longer bins as
                    64 lane partials (lane l: positions a+l, a+l+64, ... in
                    that order) and the tree v[l] += v[l+off], off = 32 .. 1
  fold_full         a cell's images in ascending s, the bit of axis 0 the MSB;
                    an image counts where every flipped axis has q != 0 and
                    n - q != q
  fold_half         the same, flipping the first d-1 axes of the half grid
  fold_half_sorted  fold_half stored at out[(cpos[cell] | cell) * pre + p]

Every one takes keyword knobs whose defaults are the documented order;
test_bin_cases.py turns each knob to a wrong value and asserts that the result
changes bitwise, so a kernel wrong in that way cannot pass.

Order-free references (`*_ld`) sum in np.longdouble and return, per output,
the sum, the number of terms n and sum |terms|; `bound` is the element-wise
recursive-summation bound n * u * sum|terms|, valid for any order and tree.
"""
import numpy as np

LONGB = 64                      # bins above this are summed one wave each (nft_cf.hip: bin_scatter_chunk, bin_scatter_il)
LANES = 64
TREE = (32, 16, 8, 4, 2, 1)
CH_PLAIN = 2048                 # nft_bin_chunk(): BS_CH, csrc/nft_cf.hip
CH_IL = {2: 1024, 4: 512, 8: 256}   # nft_bin_scatter_il_chunk(pre): sil_chunk(), SIL_CH = 2048, csrc/nft_cf.hip
CHUNKS = (CH_PLAIN,) + tuple(CH_IL[p] for p in (2, 4, 8))
U = {np.dtype(np.float64): 2.0 ** -53, np.dtype(np.float32): 2.0 ** -24}

_SIZES_A = [0, 0, 1, 63, 64, 65, 100, 130, 0, 190, 255, 256, 257, 300, 64, 65, 5000, 0, 3, 700, 65, 64, 1, 0, 0]
LAYOUTS = ("A", "B", "B2", "D", "E")

FOLD_SHAPES = [(1,), (2,), (7,), (8,),
               (1, 5), (5, 1), (2, 2), (6, 7), (7, 6),
               (3, 4, 5), (4, 1, 6), (2, 2, 2), (1, 1, 1), (5, 6, 2),
               (3, 2050),       # half length 1026 > the first round of every row kernel (4 * 256; 2 * 256; 256)
               (70, 66)]        # 36 * 34 = 1224 cells: four full 256-thread blocks and a partial one


# ------------------------------------------------------------------ layouts
def layout(name):
    """name -> (pindex int64 (npix,), nbins)"""
    if name == "A":
        sizes = np.array(_SIZES_A)
        return np.random.default_rng(1).permutation(np.repeat(np.arange(len(sizes)), sizes)), len(sizes)
    if name == "B":
        return np.random.default_rng(3).integers(0, 2500 - 7, 3 * 2048 + 17), 2500
    if name == "B2":
        return np.random.default_rng(4).integers(0, 5000 - 7, 4096), 5000
    if name == "D":
        sizes = np.random.default_rng(5).integers(40, 91, 120)
        sizes[::17] = 0
        return np.random.default_rng(6).permutation(np.repeat(np.arange(120), sizes)), 120
    if name == "E":
        return np.random.default_rng(3).integers(0, 12 - 7, 10), 12
    raise KeyError(name)


def csr(pindex, nbins):
    """the stable bin -> pixel permutation and CSR offsets, as BinIndex builds them (int64)"""
    pindex = np.asarray(pindex).ravel()
    perm = np.argsort(pindex, kind="stable")
    offs = np.zeros(nbins + 1, dtype=np.int64)
    np.cumsum(np.bincount(pindex, minlength=nbins), out=offs[1:])
    return perm.astype(np.int64), offs


def assert_valid_csr(pindex, perm, offs, nbins):
    """what a kernel may assume of its index arrays (checked on the host before every launch)"""
    npix = len(pindex)
    assert len(offs) == nbins + 1 and offs[0] == 0 and offs[-1] == npix and np.all(np.diff(offs) >= 0)
    assert len(perm) == npix and np.array_equal(np.sort(perm), np.arange(npix))
    assert npix == 0 or (pindex.min() >= 0 and pindex.max() < nbins)
    assert np.array_equal(np.repeat(np.arange(nbins), np.diff(offs)), pindex[perm])
    for b in range(nbins):
        assert np.all(np.diff(perm[offs[b]:offs[b + 1]]) > 0)     # ascending pixels inside a bin


def chunk_bins_def(offs, nbins, npix, ch):
    """the chunk -> first bin table by its definition: entry c is the first bin
    whose start offset is >= c * ch, the last entry nbins"""
    nch = (npix + ch - 1) // ch
    cb = np.empty(nch + 1, dtype=np.int32)
    for c in range(nch + 1):
        b = 0
        while b < nbins and offs[b] < c * ch:
            b += 1
        cb[c] = b
    cb[-1] = nbins
    return cb


def pixel_order(perm, ch):
    """(gpix int32, gslot uint16) of nft_bin_scatter_ordered: per chunk of ch
    sorted positions, the chunk's perm entries in ascending pixel order and the
    bin-sorted slot of each inside its chunk"""
    npix = len(perm)
    gpix = np.empty(npix, dtype=np.int32)
    gslot = np.empty(npix, dtype=np.uint16)
    for j0 in range(0, npix, ch):
        seg = perm[j0:j0 + ch]
        o = np.argsort(seg, kind="stable")
        gpix[j0:j0 + len(seg)] = seg[o]
        gslot[j0:j0 + len(seg)] = o
    return gpix, gslot


def regime(name, ch):
    """what a layout holds at chunk size ch (from the data)"""
    pindex, nb = layout(name)
    _, offs = csr(pindex, nb)
    ln = np.diff(offs)
    ne = ln > 0
    first, last = offs[:-1] // ch, (offs[1:] - 1) // ch
    strad = ne & (first != last)
    cb = chunk_bins_def(offs, nb, len(pindex), ch)
    t = 0
    while t < nb and ln[nb - 1 - t] == 0:
        t += 1
    return dict(npix=len(pindex), nbins=nb, nchunks=len(cb) - 1,
                long_straddlers=int((strad & (ln > LONGB)).sum()),
                short_straddlers=int((strad & (ln <= LONGB)).sum()),
                long_straddler_bins=np.nonzero(strad & (ln > LONGB))[0],
                short_straddler_bins=np.nonzero(strad & (ln <= LONGB))[0],
                empty_chunks=int((np.diff(cb) == 0).sum()),
                max_bins_per_chunk=int(np.diff(cb).max()),
                n64=int((ln == 64).sum()), n65=int((ln == 65).sum()),
                nlong=int((ln > LONGB).sum()), max_len=int(ln.max()),
                trailing_empty=t, leading_empty=int(np.argmax(ne)) if ne.any() else nb)


def values(shape, dtype, seed):
    """test data in the storage type"""
    return np.random.default_rng(seed).standard_normal(shape).astype(dtype)


def cell_perm(nf, seed):
    """a permutation of the cells that is not its own inverse (nf >= 3), int32"""
    rng = np.random.default_rng(seed)
    p = rng.permutation(nf)
    while nf >= 3 and np.array_equal(p[p], np.arange(nf)):
        p = rng.permutation(nf)
    return p.astype(np.int32)


# --------------------------------------------------------- exact references
def _seq(v, descending=False):
    """running sum along the last axis from +0 in v's type"""
    if v.shape[-1] == 0:
        return np.zeros(v.shape[:-1], dtype=v.dtype)
    if descending:
        v = v[..., ::-1]
    return np.cumsum(v, axis=-1, dtype=v.dtype)[..., -1]


def seq_loop(v):
    """_seq written out (the self-check of the cumsum form)"""
    acc = np.zeros(v.shape[:-1], dtype=v.dtype)
    for j in range(v.shape[-1]):
        acc = acc + v[..., j]
    return acc


def gather(src, pindex, pre, nbins, post):
    return np.ascontiguousarray(src.reshape(pre, nbins, post)[:, pindex, :])


def scatter_seq(x, perm, offs, descending=False):
    """x (pre, npix, post) -> (pre, nbins, post)"""
    pre, npix, post = x.shape
    nb = len(offs) - 1
    out = np.zeros((pre, nb, post), dtype=x.dtype)
    xt = np.ascontiguousarray(np.moveaxis(x, 1, 2))            # (pre, post, npix)
    for b in range(nb):
        out[:, b, :] = _seq(xt[:, :, perm[offs[b]:offs[b + 1]]], descending)
    return out


def _wave(v, stride, tree):
    """v (pre, L): lane partials (lane l sums v[l], v[l + stride], ... in that
    order), then the shuffle tree; lane 0's value"""
    pre, L = v.shape
    part = np.zeros((pre, LANES), dtype=v.dtype)
    idx = np.arange(LANES)
    while idx[0] < L:
        m = idx < L
        part[:, m] = part[:, m] + v[:, idx[m]]
        idx = idx + stride
    for off in tree:
        part[:, :off] = part[:, :off] + part[:, off:2 * off]
    return part[:, 0]


def scatter_wave(x, perm, offs, longb=LONGB, stride=LANES, tree=TREE, descending=False, drop_tail_ch=None):
    """x (pre, npix) -> (pre, nbins): the folded and the interleaved scatter.
    drop_tail_ch (wrong on purpose): a bin loses what lies past the end of the
    chunk of drop_tail_ch positions it starts in."""
    pre, npix = x.shape
    nb = len(offs) - 1
    out = np.zeros((pre, nb), dtype=x.dtype)
    for b in range(nb):
        a, e = int(offs[b]), int(offs[b + 1])
        if drop_tail_ch is not None and e > a:
            e = min(e, (a // drop_tail_ch + 1) * drop_tail_ch)
        v = x[:, perm[a:e]]
        if offs[b + 1] - offs[b] > longb:
            out[:, b] = _wave(v[:, ::-1] if descending else v, stride, tree)
        else:
            out[:, b] = _seq(v, descending)
    return out


def half_shape(shape):
    return tuple(shape[:-1]) + (shape[-1] // 2 + 1,)


def cell_shape(shape):
    return tuple(n // 2 + 1 for n in shape)


def _images(shape, nflip):
    """(ok over the cell grid, index tuple into the source) per mirror image,
    in ascending s with the bit of axis 0 the most significant"""
    d = len(shape)
    q = np.indices(cell_shape(shape), sparse=True)
    out = []
    for s in range(1 << nflip):
        ok = np.ones(cell_shape(shape), dtype=bool)
        idx = []
        for a in range(d):
            if a < nflip and (s >> (nflip - 1 - a)) & 1:
                m = shape[a] - q[a]
                ok = ok & (q[a] != 0) & (m != q[a])
                idx.append(m % shape[a])           # q == 0: not an image (ok is False there)
            else:
                idx.append(q[a])
        out.append((ok, tuple(idx)))
    return out


def _fold(src, shape, nflip, reverse):
    acc = np.zeros(src.shape[:1] + cell_shape(shape), dtype=src.dtype)
    ims = _images(shape, nflip)
    for ok, idx in (ims[::-1] if reverse else ims):
        acc = np.where(ok, acc + src[(slice(None),) + idx], acc)
    return acc


def fold_full(w, reverse=False):
    """w (pre, *shape) -> (pre, *cell_shape)"""
    return _fold(w, w.shape[1:], w.ndim - 1, reverse)


def fold_half(H, shape, reverse=False):
    """H (pre, *half_shape(shape)): point-mirror pair sums -> (pre, *cell_shape)"""
    assert H.shape[1:] == half_shape(shape)
    return _fold(H, shape, len(shape) - 1, reverse)


def fold_half_sorted(H, shape, cpos=None, reverse=False, forward_cpos=False):
    """-> flat (nf * pre,): the fold of cell c, item p at (cpos[c] | c) * pre + p"""
    f = fold_half(H, shape, reverse)
    pre = f.shape[0]
    f = f.reshape(pre, -1)
    out = np.empty((f.shape[1], pre), dtype=f.dtype)
    if cpos is None:
        out[:] = f.T
    elif forward_cpos:
        out[:] = f.T[cpos]
    else:
        out[cpos] = f.T
    return out.ravel()


def pair_sums(w):
    """H = w + pointmirror(w) on the half grid, the self-mirror columns 0 (and
    n/2 for even n) holding the single value (what epi_out2_pairs stores)"""
    ax = tuple(range(1, w.ndim))
    mir = np.roll(np.flip(w, ax), 1, ax)
    n = w.shape[-1]
    H = np.ascontiguousarray((w + mir)[..., :n // 2 + 1])
    for c in [0] + ([n // 2] if n % 2 == 0 else []):
        H[..., c] = w[..., c]
    return H


def canonical_cell(shape):
    """per grid pixel the raveled index of its fundamental cell"""
    q = [np.minimum(i, n - i) for i, n in zip(np.indices(shape, sparse=True), shape)]
    return np.ravel_multi_index(np.broadcast_arrays(*q), cell_shape(shape)).ravel()


# ---------------------------------------------------- order-free references
def bound(n, sumabs, dtype):
    return np.asarray(n, dtype=np.longdouble) * np.longdouble(U[np.dtype(dtype)]) * sumabs


def scatter_ld(x, pindex, nbins):
    """x (pre, npix, post) -> (sum, n, sum|.|) of (pre, nbins, post), (nbins,), (pre, nbins, post)"""
    pre, npix, post = x.shape
    s = np.zeros((pre, nbins, post), dtype=np.longdouble)
    sa = np.zeros_like(s)
    xl = x.astype(np.longdouble)
    for p in range(pre):
        for q in range(post):
            np.add.at(s[p, :, q], pindex, xl[p, :, q])
            np.add.at(sa[p, :, q], pindex, np.abs(xl[p, :, q]))
    return s, np.bincount(pindex, minlength=nbins), sa


def fold_ld(src, shape, half=False):
    """-> (sum, n, sum|.|), each (pre, *cell_shape) / n (*cell_shape)"""
    s = np.zeros(src.shape[:1] + cell_shape(shape), dtype=np.longdouble)
    sa = np.zeros_like(s)
    n = np.zeros(cell_shape(shape), dtype=np.int64)
    sl = src.astype(np.longdouble)
    for ok, idx in _images(shape, len(shape) - (1 if half else 0)):
        v = sl[(slice(None),) + idx]
        s = np.where(ok, s + v, s)
        sa = np.where(ok, sa + np.abs(v), sa)
        n = n + ok
    return s, n, sa
