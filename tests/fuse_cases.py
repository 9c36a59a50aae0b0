"""Shared by test_fuse_cases.py (host) and test_fuse_engines_gpu.py (device):
the extended-precision reference of ``nft_hartley_fused`` (include/nifty_amd.h,
``nft_hartley_fuse``), an error bound derived from the operands, the launch
labels a fused call has to leave in a LaunchProfile, host restatements of the
kernel choices that labels do not show, the check every group's outputs have
to pass, and the case tables.  Companion of fft_cases.py; not a test module.

Semantics (flat item element j, item b):

    u    = (a ? a[j] : 1) x[b][j] + (b ? b[j] c[b][bin(j)] : 0)
    bin  = pro_index[j], or folded pro_index[cell(j)], cell = (min(k, n - k))_axis
    h    = scale Hartley(u)
    out  = (ea ? ea[j] : 1) h + (d ? shift d[b][j] : 0);   out2 = eb[j] h
    pair output: out2(row, c) + out2(-row, -c) on the half grid c <= n/2, the
                 single value in the columns c = 0 and c = n/2
    quad: per item sum_j h (ea h);  dir: x <- max(0, gamma / gprev) x + r first

Bound (``fused_bound``), unit roundoff u, per item in the l2 norm.  With
N the number of transformed elements of one line set (||Hartley|| = sqrt N):

    Bh   = fft_cases.bound ||h|| + |scale| sqrt(N) 3u || |a x| + |b c| ||
    out  : max|ea| Bh + 2u || |ea h| + |shift d| ||
    out2 : max|eb| Bh + 2u || eb h ||

u carries at most three roundings (two products, one sum; contraction to FMA
removes one), the transform its own normwise error on top of the exact
transform of the perturbed u; the epilogue two (product and cast of the shift,
sum).  Terms the issue's formula did not name, with their derivation:

* pair output: every full-grid element enters exactly one half-grid entry, so
  for the elementwise errors e of out2, sum (e_j + e_mj)^2 <= 2 sum e^2:
  sqrt(2) times the out2 bound, plus the one rounding of the pair sum,
  u || |t_j| + |t_mj| ||.
* dir cases: the reference forms h from the exact d'; the device from its
  stored d', which differs by at most 4u (|beta d| + |r|) (the element bound of
  test_cg_primitives_gpu.check_dir_row): Bh gains
  |scale| sqrt(N) 4u || |a| (|beta d| + |r|) ||.
* quad sums: Q = sum ea h^2 of the device's h = h_ref + dh is off by
  2 sum ea h dh <= 2 max|ea| ||h|| Bh to first order, one rounding u per
  stored product ea h, and the fp64 reduction in the form of
  test_cg_primitives_gpu (``red_bound``: (L + 25) 2^-53 sum|terms|, L = 38: a
  thread chains 2 x 8 values (its tile values and their mirrors), then 6
  shuffle steps and at most 16 waves; the tiles of an item are summed
  exactly on the host).

Inputs are uniform in +-[0.5, 1.5] (as the CG primitive tests): a single wrong,
missing or swapped element moves an output by O(1) against bounds of O(u)."""
import math
import zlib
from collections import namedtuple

import numpy as np

import fft_cases as fc

LD = fc.LD
SENT = 3.0e30                      # padding / untouched-slot sentinel (finite in fp32)
NS, GAMMA, GPREV, DONE = 16, 0, 1, 8      # CG scalar block (include/nifty_amd.h NFT_CG_*)
DIR_SHIFT = 0.7
# values per thread of an engine-v2 tile (fast::VPT, csrc/fft_fast.hpp; fft_cases.TILE_VALUES is the generic
# engine's 16, so its tile sizes are twice the real ones -- test_fuse_engines_gpu.py holds cg_blocks, which is
# built on this figure, against nft_hartley_cg_blocks on the device)
V2_VPT = 8
QUAD_CHAIN = 2 * V2_VPT + 6 + 16
PRO_ROWS_MAXH = (160 * 1024 - 4 * 8 * 8) // 64      # 2556, csrc/nft_fft.hip
NBINS = 37                         # random per-pixel bins of the unfolded cases

# spec keys -- pro: dict(a, b: None / "shared" / "item"; index: "pixel" / "fold";
# c: "single" / "inter" / "item"; xpad), epi: dict(a, b: None / "shared" /
# "item"; d: bool; shift; pairs; opad, dpad, o2pad), quad: dict(blk0, tail),
# dir: dict(done=item or None, neg=item or None, blk0, tail), env: dict
FCase = namedtuple("FCase", "id group dtype shape axes nb scale convention spec regime")


def np_dtype(c):
    return np.float64 if c.dtype == "f64" else np.float32


def grid_of(c):
    return tuple(c.shape[1:]) if c.nb else tuple(c.shape)


def items_of(c):
    return c.nb if c.nb else 1


def item_axes(c):
    """transform axes in the coordinates of one item"""
    return tuple(a - 1 for a in c.axes) if c.nb else tuple(c.axes)


def period(c):
    return int(np.prod(grid_of(c)))


def out2_period(c):
    g = grid_of(c)
    e = c.spec.get("epi") or {}
    return period(c) // g[-1] * (g[-1] // 2 + 1) if e.get("pairs") else period(c)


def row_tile(n):
    """pair lines (two real rows each) of one engine-v2 row-pass tile"""
    return fc.nt_rows(n) * V2_VPT // n


def strided_tile(n):
    """lines of one engine-v2 strided-pass tile"""
    return fc.nt_strided(n) * V2_VPT // n


def items_independent(c):
    """every item is transformed on lines of its own: engine v2 over more than
    one axis (its row pass pairs rows 2l, 2l + 1 of an item's even row count).
    The one-axis H1D pass and the generic engine pair rows or columns across
    the items of a batch, which mixes their rounding: there a batch of one
    agrees with the batch only to rounding."""
    return bool(c.nb) and len(item_axes(c)) >= 2 and bool(fc.expected_labels(c.shape, c.axes))


# ------------------------------------------------------------------ inputs
def _draw(rng, shape, dt):
    v = rng.uniform(0.5, 1.5, size=shape) * rng.choice([-1.0, 1.0], size=shape)
    return v.astype(dt)


def _padded(rng, k, n, pad, dt):
    a = np.full((k, n + pad), SENT, dt)
    a[:, :n] = _draw(rng, (k, n), dt)
    return a


def cell_index(grid):
    """flat index of cell(j) = (min(k, n - k))_a in the fundamental cell
    (n_a / 2 + 1 per axis, C order) for every element j of the grid"""
    idx = np.zeros(grid, np.int64)
    for a, n in enumerate(grid):
        k = np.arange(n)
        m = np.minimum(k, n - k).reshape([-1 if b == a else 1 for b in range(len(grid))])
        idx = idx * (n // 2 + 1) + m
    return idx


def kbins(grid):
    """|k| bins of a harmonic grid (mildly anisotropic, so that the axes'
    bins differ): (bin of every pixel, bin of every fundamental cell, nbins)"""
    kk = np.zeros(grid)
    for a, n in enumerate(grid):
        f = np.fft.fftfreq(n) * n
        kk = kk + (f.reshape([-1 if b == a else 1 for b in range(len(grid))]) * (1. + 0.1 * a)) ** 2
    uq, pidx = np.unique(np.round(np.sqrt(kk), 9), return_inverse=True)
    pidx = pidx.reshape(grid).astype(np.int32)
    fold = pidx[tuple(slice(0, n // 2 + 1) for n in grid)]
    return pidx, np.ascontiguousarray(fold), int(uq.size)


_INP = {}


def fused_inputs(c):
    """the case's operands, rounded to the device dtype; shared, read-only"""
    if c.id in _INP:
        return _INP[c.id]
    rng = np.random.default_rng(zlib.crc32(f"fuse{c.shape}{c.axes}{c.nb}{c.group}".encode()))
    dt, k, P, g = np_dtype(c), items_of(c), period(c), grid_of(c)
    pro, epi = c.spec.get("pro"), c.spec.get("epi")
    inp = {}
    if pro:
        inp["X"] = _padded(rng, k, P, pro.get("xpad", 0), dt)
        for key, name in (("a", "A"), ("b", "B")):
            if pro.get(key):
                inp[name] = _draw(rng, (k, P) if pro[key] == "item" else (P,), dt)
        if pro.get("b"):
            if pro["index"] == "fold":
                pidx, fold, nbins = kbins(g)
                inp["pidx"], inp["fidx"] = pidx.reshape(-1), fold.reshape(-1)
            else:
                nbins = NBINS
                inp["pidx"] = rng.integers(0, nbins, P).astype(np.int32)
            lay = pro.get("c", "single")
            inp["C"] = _draw(rng, {"single": (nbins,), "inter": (nbins, k), "item": (k, nbins)}[lay], dt)
    else:
        inp["X"] = _draw(rng, (k, P), dt)
    if epi:
        for key, name in (("a", "EA"), ("b", "EB")):
            if epi.get(key):
                inp[name] = _draw(rng, (k, P) if epi[key] == "item" else (P,), dt)
        if epi.get("d"):
            inp["D"] = _padded(rng, k, P, epi.get("dpad", 0), dt)
    dr = c.spec.get("dir")
    if dr:
        inp["R"] = _padded(rng, k, P, pro.get("xpad", 0), dt)
        sc = np.zeros((k, NS))
        for j in range(k):
            sc[j] = [2.0 + rng.uniform(), 3.0 + rng.uniform(), 4.0 + rng.uniform(), -11.0, -12.0, -13.0, 0.0, -14.0,
                     0.0, 5.0, 0.0, 0.0, -15.0, -16.0, -17.0, -18.0]
        if dr.get("done") is not None:
            sc[dr["done"], DONE] = 1.0
        if dr.get("neg") is not None:
            sc[dr["neg"], GAMMA] = -sc[dr["neg"], GAMMA]
        inp["SC"] = sc
    for v in inp.values():
        v.setflags(write=False)
    _INP[c.id] = inp
    return inp


def item_case(c, inp, j):
    """item j of a batched case as a batch of one: (case, inputs)"""
    spec = {k: (dict(v) if isinstance(v, dict) else v) for k, v in c.spec.items()}
    one = {}
    pro = spec.get("pro")
    for name, v in inp.items():
        if name in ("pidx", "fidx"):
            one[name] = v
        elif name == "C":
            lay = pro.get("c", "single")
            one[name] = np.ascontiguousarray(v[:, j:j + 1] if lay == "inter" else v[j:j + 1] if lay == "item" else v)
        elif v.ndim == 2 and v.shape[0] == c.nb:
            one[name] = np.ascontiguousarray(v[j:j + 1])
        else:
            one[name] = v
    if spec.get("dir"):
        d = spec["dir"]
        d["done"] = 0 if d.get("done") == j else None
        d["neg"] = 0 if d.get("neg") == j else None
    return c._replace(id=f"{c.id}-item{j}", nb=1, shape=(1,) + tuple(c.shape[1:]), spec=spec), one


# ------------------------------------------------------------------ reference
def _rows(v, k, P):
    """(k, P) extended-precision view of a shared (P,) or per-item (k, >= P) operand"""
    v = np.asarray(v)
    if v.ndim == 1:
        return np.broadcast_to(v[:P].astype(LD), (k, P))
    return v[:, :P].astype(LD)


def beta_of(sc):
    with np.errstate(all="ignore"):
        b = LD(sc[GAMMA]) / LD(sc[GPREV])
        b64 = np.float64(sc[GAMMA]) / np.float64(sc[GPREV])
    return b if b64 > 0.0 else LD(0.0)


def ref_fused(c, inp=None, defect=None):
    """every output of the case in np.longdouble, with the magnitudes the
    bound needs.  defect="mirror_bin": one element of the last item whose last
    coordinate lies past n/2 gathers the bin of the neighbour of its mirror
    cell (the case's sensitivity check)."""
    inp = fused_inputs(c) if inp is None else inp
    k, P, g, iax = items_of(c), period(c), grid_of(c), item_axes(c)
    pro, epi, dr = c.spec.get("pro"), c.spec.get("epi") or {}, c.spec.get("dir")
    ref = {}
    x = _rows(inp["X"], k, P)
    dmag = None
    if dr:
        x1, dmag = np.array(x), np.zeros((k, P), LD)
        for j in range(k):
            if inp["SC"][j, DONE] != 0.0:
                continue
            beta = beta_of(inp["SC"][j])
            r = inp["R"][j, :P].astype(LD)
            x1[j] = beta * x[j] + r
            dmag[j] = np.abs(beta * x[j]) + np.abs(r)
        ref["x1"], ref["x1_mag"] = x1, dmag
        ref["dd"] = np.array([DIR_SHIFT * np.sum(x1[j] ** 2) if inp["SC"][j, DONE] == 0.0 else LD(0) for j in range(k)])
        x = x1
    u, umag = x, np.abs(x)
    amax = np.ones(k, LD)
    if pro and pro.get("a"):
        a = _rows(inp["A"], k, P)
        u, umag = a * x, np.abs(a * x)
        if dmag is not None:
            dmag = np.abs(a) * dmag
    if pro and pro.get("b"):
        if pro["index"] == "fold":
            bins = inp["fidx"][cell_index(g).reshape(-1)]
        else:
            bins = inp["pidx"]
        bins = np.broadcast_to(bins.astype(np.int64), (k, P)).copy()
        if defect == "mirror_bin":
            n = g[-1]
            j = P - 1                               # last coordinate n - 1: mirror cell 1
            if pro["index"] == "fold":
                cell = cell_index(g).reshape(-1)[j] + 1          # the neighbour cell (n >= 4)
                assert n >= 4
                bins[k - 1, j] = inp["fidx"][cell]
            else:
                bins[k - 1, j] = (bins[k - 1, j] + 1) % NBINS
        lay = pro.get("c", "single")
        C = inp["C"].astype(LD)
        cv = np.stack([(C[bins[i], i] if lay == "inter" else C[i, bins[i]] if lay == "item" else C[bins[i]])
                       for i in range(k)])
        bc = _rows(inp["B"], k, P) * cv
        u, umag = u + bc, umag + np.abs(bc)
    ref["u"], ref["u_mag"], ref["dir_mag"] = u, umag, dmag
    full = tuple(a + 1 for a in iax)
    h = LD(c.scale) * fc.ref_hartley(u.reshape((k,) + g), full, c.convention)
    h = h.reshape(k, P)
    ref["h"] = h
    out, omag = h, np.abs(h)
    if epi.get("a"):
        ea = _rows(inp["EA"], k, P)
        out, omag = ea * h, np.abs(ea * h)
        amax = np.max(np.abs(ea), axis=1)
    if epi.get("d"):
        sd = LD(epi["shift"]) * _rows(inp["D"], k, P)
        out, omag = out + sd, omag + np.abs(sd)
    ref["out"], ref["out_mag"], ref["ea_max"] = out, omag, amax
    if epi.get("b"):
        eb = _rows(inp["EB"], k, P)
        t = eb * h
        ref["eb_max"] = np.max(np.abs(eb), axis=1)
        if epi.get("pairs"):
            assert len(iax) == len(g), "pair sums: the point mirror runs over every axis of the item"
            n, nh = g[-1], g[-1] // 2 + 1
            tg = t.reshape((k,) + g)
            tm = fc.mirror(tg, full)
            pair, pmag = tg[..., :nh] + tm[..., :nh], np.abs(tg[..., :nh]) + np.abs(tm[..., :nh])
            for col in (0, n // 2):
                pair[..., col], pmag[..., col] = tg[..., col], np.abs(tg[..., col])
            ref["out2"], ref["out2_mag"] = pair.reshape(k, -1), pmag.reshape(k, -1)
            ref["t_mag"] = np.abs(t)
        else:
            ref["out2"], ref["out2_mag"] = t, np.abs(t)
    if c.spec.get("quad"):
        ref["quad"] = np.sum(h * out, axis=1)
        ref["quad_abs"] = np.sum(np.abs(h * out), axis=1)
    return ref


# ------------------------------------------------------------------ bound
def _l2(v):
    return np.sqrt(np.sum(np.asarray(v, LD) ** 2, axis=-1))


def red_bound(sumabs, L, extra=25):
    """the reduction form of test_cg_primitives_gpu"""
    return (L + extra) * 2.0 ** -53 * sumabs


def fused_bound(c, ref):
    """per-item absolute bounds, dict(out, out2, quad) of (items,) arrays; see
    the module docstring"""
    u = fc.unit_roundoff(c.dtype)
    g, iax = grid_of(c), item_axes(c)
    epi = c.spec.get("epi") or {}
    n = float(np.prod([g[a] for a in iax])) if iax else 1.0
    bh = fc.bound(g, iax, c.dtype) * _l2(ref["h"]) + abs(c.scale) * math.sqrt(n) * 3 * u * _l2(ref["u_mag"])
    if ref.get("dir_mag") is not None:
        bh = bh + abs(c.scale) * math.sqrt(n) * 4 * u * _l2(ref["dir_mag"])
    b = dict(h=bh, out=ref["ea_max"] * bh + 2 * u * _l2(ref["out_mag"]))
    if "out2" in ref:
        if epi.get("pairs"):
            single = ref["eb_max"] * bh + 2 * u * _l2(ref["t_mag"])
            b["out2_single"] = single
            b["out2"] = math.sqrt(2.0) * single + u * _l2(ref["out2_mag"])
        else:
            b["out2"] = ref["eb_max"] * bh + 2 * u * _l2(ref["out2_mag"])
    if "quad" in ref:
        b["quad"] = (2 * ref["ea_max"] * _l2(ref["h"]) * bh + u * ref["quad_abs"]
                     + red_bound(ref["quad_abs"], QUAD_CHAIN) + 2.0 ** -53 * np.abs(ref["quad"]))
    return {k: np.asarray(v, np.float64) for k, v in b.items()}


# ------------------------------------------------------------------ regime predicates
def _env(c):
    return (c.spec.get("env") or {}).get("NFT_PRO_R2C")


def _v2_labels(shape, axes, pro, epi, quad):
    out = []
    for lab in fc.expected_labels(shape, axes):
        if lab == "fft_h1d" and (pro or epi):
            lab = "fft_h1d+fused"
        elif lab == "fft_r2c" and pro:
            lab = "fft_r2c+pro"
        elif lab == "fft_unpack" and (quad or epi):
            lab = "fft_unpack+quad" if quad else "fft_unpack+epi"
        out.append(lab)
    return out


def pro_r2c_applies(c):
    """pro_r2c_try (csrc/nft_pro_r2c.hip)"""
    pro, g = c.spec.get("pro") or {}, grid_of(c)
    mode = {None: 1, "0": 0, "2": 2}[_env(c)]
    if mode == 0 or not c.spec.get("dir") or len(g) != 2 or pro.get("a") == "item" or pro.get("b") != "shared":
        return False
    if not c.nb or tuple(c.axes) != (1, 2) or pro.get("index") != "fold":
        return False
    n0, n1 = g
    if n0 < 16 or (n0 // 2) % 8 != 0 or n1 not in (512, 1024, 2048, 4096):
        return False
    return not (mode == 1 and n1 > 1024)


def split_prologue(c):
    """hartley_fused_impl: the prologue runs as its own pass before the transform"""
    pro = c.spec.get("pro")
    if not pro or not (pro.get("a") or pro.get("b")):
        return False
    fold = pro.get("b") and pro.get("index") == "fold"
    dr = bool(c.spec.get("dir"))
    shared = pro.get("a") != "item" and pro.get("b") != "item"
    if not c.nb:
        return bool(fold)            # a single folded item runs as a batch of one
    return bool((shared or (fold and not dr)) and (c.nb > 1 or dr or fold))


def pro_kernel(c):
    """which stand-alone prologue kernel serves the case: "r2c", "rows", "fold",
    "batch", or None (in-pass / no prologue)"""
    if not split_prologue(c):
        return None
    pro, g = c.spec["pro"], grid_of(c)
    if pro_r2c_applies(c):
        return "r2c"
    if pro.get("b") and pro.get("index") == "fold":
        rows = len(g) >= 2 and g[-1] // 2 + 1 <= PRO_ROWS_MAXH      # nft_hartley_pro_rows
        return "rows" if rows and items_of(c) <= 8 else "fold"
    return "batch"


def nbm_class(nb):
    """register capacity class of launch_pro_rows / launch_pro_fold"""
    return 2 if nb <= 2 else 4 if nb <= 4 else 8


def per_item_ab(c):
    pro = c.spec.get("pro") or {}
    return pro.get("a") == "item" or pro.get("b") == "item"


def vector_gather(c):
    """c_elem == nb and c == 1 and nb even (and nb within the register class
    of the folded kernels)"""
    pro = c.spec.get("pro") or {}
    nb = items_of(c)
    return bool(pro.get("b")) and pro.get("c") == "inter" and nb % 2 == 0 and (pro_kernel(c) == "batch" or nb <= 8)


def cg_blocks(c):
    """nft_hartley_cg_blocks: tiles per item of the strided unpack pass"""
    g, iax = grid_of(c), item_axes(c)
    if not c.nb or len(iax) < 2 or iax != tuple(range(len(g))) or not fc.rows_supported(g[-1]):
        return 0
    if not all(fc.strided_supported(n) for n in g[1:-1]):
        return 0
    lines = int(np.prod(g[1:-1])) * fc.half_ext(g[-1])
    n0, m = g[0], 1
    if not fc.strided_supported(n0):
        if not fc.fourstep_supported(n0):
            return 0
        m, n0 = fc.fourstep_split(n0)
    lt = strided_tile(n0)
    return m * -(-lines // lt)


def bgroup_applies(c):
    """fast_dispatch.hpp: the XCD regrouping of tiles"""
    epi = c.spec.get("epi") or {}
    if not c.spec.get("quad") or c.nb <= 1 or epi.get("a") != "shared":
        return False
    t = cg_blocks(c)
    return t > 0 and (t * c.nb) % (8 * c.nb) == 0


def expected_fused_labels(c):
    pro, epi, quad = c.spec.get("pro"), c.spec.get("epi") or {}, bool(c.spec.get("quad"))
    has_epi = bool(epi.get("a") or epi.get("d") or epi.get("b"))
    shape, axes = tuple(c.shape), tuple(c.axes)
    kern = pro_kernel(c)
    if kern is None:
        return _v2_labels(shape, axes, bool(pro), has_epi, quad)
    if not c.nb:
        shape, axes = (1,) + shape, tuple(a + 1 for a in axes)
    rest = _v2_labels(shape, axes, False, has_epi, quad)
    if kern == "r2c":
        assert rest[:1] == ["fft_r2c"]
        return ["pro_r2c+dir"] + rest[1:]
    if kern == "batch":
        return ["pro_batch"] + rest
    return ["pro_fold+dir" if c.spec.get("dir") else "pro_fold"] + rest


# ------------------------------------------------------------------ the check
def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int64 if a.dtype == np.float64 else np.int32)


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(_bits(a), _bits(b))


def cast_ref(c, ref):
    """the reference rounded to the device dtype in the layout of a device
    result: dict(out (k, P + opad), out2, quad (k, blk0 + tiles + tail)),
    padding and unused slots at the sentinel"""
    dt, k, P = np_dtype(c), items_of(c), period(c)
    epi, quad = c.spec.get("epi") or {}, c.spec.get("quad")
    got = {}
    o = np.full((k, P + epi.get("opad", 0)), SENT, dt)
    o[:, :P] = ref["out"].astype(dt)
    got["out"] = o
    if "out2" in ref:
        P2 = out2_period(c)
        o2 = np.full((k, P2 + epi.get("o2pad", 0)), SENT, dt)
        o2[:, :P2] = ref["out2"].astype(dt)
        got["out2"] = o2
    if quad:
        t = cg_blocks(c)
        q = np.full((k, quad["blk0"] + t + quad["tail"]), SENT, np.float64)
        # the item's sum in its last tile's slot, the other tiles empty
        q[:, quad["blk0"]:quad["blk0"] + t] = 0.0
        q[:, quad["blk0"] + t - 1] = ref["quad"].astype(np.float64)
        got["quad"] = q
    return got


def check_case(c, ref, got):
    """asserts every output of ``got`` (device layout, see cast_ref) against
    the reference under fused_bound, padding and unused slots bit-exact;
    returns {output: largest error / bound}"""
    k, P = items_of(c), period(c)
    epi, quad = c.spec.get("epi") or {}, c.spec.get("quad")
    b = fused_bound(c, ref)
    ratios = {}
    sent = np.array(SENT, np_dtype(c))

    def normwise(name, arr, n):
        assert arr.shape[0] == k and arr.shape[1] >= n, (c.id, name, arr.shape)
        assert np.all(arr[:, n:] == sent), (c.id, name, "padding written")
        assert np.all(np.isfinite(arr[:, :n])), (c.id, name, "not finite")
        e = _l2(arr[:, :n].astype(LD) - ref[name])
        r = np.asarray(e / b[name], np.float64)
        ratios[name] = float(r.max())
        assert np.all(e <= b[name]), (c.id, name, "item", int(np.argmax(r)), float(r.max()))

    normwise("out", got["out"], P)
    if "out2" in ref:
        P2 = out2_period(c)
        normwise("out2", got["out2"], P2)
        if epi.get("pairs"):
            n = grid_of(c)[-1]
            cols = [0, n // 2]
            d = got["out2"][:, :P2].astype(LD) - ref["out2"]
            e = _l2(d.reshape(k, -1, n // 2 + 1)[:, :, cols].reshape(k, -1))
            assert np.all(e <= b["out2_single"]), (c.id, "self-mirror columns", float(np.max(e / b["out2_single"])))
    if quad:
        t, q = cg_blocks(c), got["quad"]
        lo, hi = quad["blk0"], quad["blk0"] + t
        assert q.shape == (k, hi + quad["tail"]), (c.id, q.shape)
        assert np.all(q[:, :lo] == SENT) and np.all(q[:, hi:] == SENT), (c.id, "quad slots outside the tiles written")
        assert np.all(np.isfinite(q[:, lo:hi])), (c.id, "a quad slot of the tile range is unwritten or not finite")
        s = np.array([math.fsum(q[j, lo:hi].tolist()) for j in range(k)])
        e = np.abs(s.astype(LD) - ref["quad"])
        ratios["quad"] = float(np.max(e / b["quad"]))
        assert np.all(e <= b["quad"]), (c.id, "quad", ratios["quad"])
    return ratios


# ------------------------------------------------------------------ defects of the sensitivity check
def _mirror_flat(c, j):
    g, iax = grid_of(c), item_axes(c)
    co = list(np.unravel_index(j, g))
    for a in iax:
        co[a] = (-co[a]) % g[a]
    return int(np.ravel_multi_index(co, g))


def apply_defect(c, ref, name):
    """a device-layout result with one defect; None where the defect has no
    meaning for the case"""
    k, P = items_of(c), period(c)
    epi, quad = c.spec.get("epi") or {}, c.spec.get("quad")
    pro = c.spec.get("pro") or {}
    if name == "mirror_bin":
        if pro.get("b"):
            return cast_ref(c, ref_fused(c, defect="mirror_bin"))
        got = cast_ref(c, ref)             # no gather: one output element taken from its mirror cell
        j = P - 1 - (grid_of(c)[-1] // 4)
        assert _mirror_flat(c, j) != j
        got["out"][k - 1, j] = got["out"][k - 1, _mirror_flat(c, j)]
        return got
    got = cast_ref(c, ref)
    if name == "swap_items":
        if k < 2:
            return None
        got["out"][[0, 1], :P] = got["out"][[1, 0], :P]
        return got
    if name == "tail_row":
        n = grid_of(c)[-1]
        got["out"][k - 1, P - n:P] = SENT
        return got
    if name == "nyquist_twice":
        if not epi.get("pairs"):
            return None
        n = grid_of(c)[-1]
        v = got["out2"][:, :out2_period(c)].reshape(k, -1, n // 2 + 1)
        v[:, :, n // 2] *= 2
        return got
    if name == "quad_slot":
        if not quad:
            return None
        hi = quad["blk0"] + cg_blocks(c)
        got["quad"][k - 1, hi] = got["quad"][k - 1, hi - 1]
        got["quad"][k - 1, hi - 1] = SENT
        return got
    raise KeyError(name)


DEFECTS = ("mirror_bin", "swap_items", "tail_row", "nyquist_twice", "quad_slot")


# ------------------------------------------------------------------ cases
DTYPES = fc.DTYPES


def _pro(a=None, b=None, index="pixel", c="single", xpad=0):
    return dict(a=a, b=b, index=index, c=c, xpad=xpad)


def _epi(a=None, d=False, shift=0.0, b=None, pairs=False, opad=0, dpad=0, o2pad=0):
    return dict(a=a, d=d, shift=shift, b=b, pairs=pairs, opad=opad, dpad=dpad, o2pad=o2pad)


PRO_SETS = {"x": _pro(), "ax": _pro(a="shared"), "axbc": _pro(a="shared", b="shared")}
EPI_SETS = {"ea": _epi(a="shared"), "ead": _epi(a="shared", d=True, shift=0.7), "eb": _epi(b="shared"),
            "all": _epi(a="shared", d=True, shift=0.7, b="shared")}


def cases_a():
    """in-pass prologue of the R2C row pass: a single transform with a
    per-pixel index, every row length, a short strided first axis; and a
    three-axis case whose 12 pair lines leave the second row tile (8 pair
    lines at rows of 256) partial"""
    out = []
    for n in fc.ROWS_N:
        for ops, pro in PRO_SETS.items():
            for dt in DTYPES:
                out.append(FCase(f"a-r2c{n}-{ops}-{dt}", "a", dt, (8, n), (0, 1), 0, 0.3, 0, dict(pro=pro),
                                 dict(rows_n=n, pair_lines=4, tile=row_tile(n))))
    for dt in DTYPES:
        out.append(FCase(f"a-r2c256-3d-tail-{dt}", "a", dt, (3, 8, 256), (1, 2), 0, 0.3, 1, dict(pro=PRO_SETS["axbc"]),
                         dict(rows_n=256, pair_lines=12, tile=row_tile(256), partial=True)))
    return out


def cases_b():
    """fft_h1d+fused: prologue and epilogue in the one row pass; more than
    one tile, the last one partial where a tile holds more than two pair
    lines, the last pair a single row"""
    out = []
    for n in fc.ROWS_N:
        lp = row_tile(n)
        rows = 2 * lp + 3
        for dt in DTYPES:
            out.append(FCase(f"b-h1d{n}-{dt}", "b", dt, (rows, n), (1,), 0, 0.3, 0,
                             dict(pro=PRO_SETS["axbc"], epi=EPI_SETS["all"]),
                             dict(rows_n=n, real_rows=rows, pair_lines=(rows + 1) // 2, tile=lp)))
    return out


def _unpack_regime(n0, lines):
    m, n = (1, n0) if fc.strided_supported(n0) else fc.fourstep_split(n0)
    lt = strided_tile(n)
    return dict(first_n=n0, lines=lines, tile=lt, tiles=m * -(-lines // lt), partial=lines % lt != 0)


def cases_c():
    """strided unpack epilogue: every strided and four-step first axis, a last
    axis of 8 or 16 (every unpack tile partial), every operand set; batched
    with padded out / d / out2 rows, shared and per-item ea / eb"""
    out = []
    for i, n0 in enumerate(fc.STRIDED_N + fc.FOURSTEP_N):
        n = n0 if fc.strided_supported(n0) else fc.fourstep_split(n0)[1]
        last = 16 if i % 2 == 1 and strided_tile(n) > 16 else 8      # 256 and 128 x 128: 16 lines fill the tile
        for ops, epi in EPI_SETS.items():
            for dt in DTYPES:
                out.append(FCase(f"c-unpack{n0}x{last}-{ops}-{dt}", "c", dt, (n0, last), (0, 1), 0, 0.3, i % 2,
                                 dict(epi=epi), _unpack_regime(n0, fc.half_ext(last))))
    for n0 in (64, 1024):
        for item in (False, True):
            m = "item" if item else "shared"
            epi = _epi(a=m, d=True, shift=0.7, b=m, opad=5, dpad=3, o2pad=7)
            for dt in DTYPES:
                out.append(FCase(f"c-unpack{n0}x8-batch3-{m}-{dt}", "c", dt, (3, n0, 8), (1, 2), 3, 0.3, 0,
                                 dict(epi=epi), dict(_unpack_regime(n0, fc.half_ext(8)), batched=True)))
    return out


# (shape, ea per item, bgroup)
QUAD_GEOS = [
    ((1, 64, 64), False, False),
    ((1, 1024, 8), False, False),
    ((2, 1024, 8), False, True),
    ((3, 64, 64, 8), False, True),
    ((8, 2048, 8), False, True),
    ((2, 64, 64), False, False),
    ((3, 16, 16, 16), False, False),
    ((8, 64, 16), False, False),
    ((2, 1024, 8), True, False),
]
PAIR_GEOS = [(0, (64, 64)), (1, (2048, 16)), (2, (1024, 8)), (3, (16, 16, 16)), (8, (64, 16))]


def cases_d():
    """the quadratic-form partials on both sides of the tile regrouping, and
    the point-mirror pair sums, on strided and four-step first axes"""
    out = []
    for shape, item, bg in QUAD_GEOS:
        nb = shape[0]
        name = "x".join(map(str, shape)) + ("-item" if item else "")
        for dt in DTYPES:
            out.append(FCase(f"d-quad-{name}-{dt}", "d", dt, shape, tuple(range(1, len(shape))), nb,
                             1.0 / math.sqrt(np.prod(shape[1:])), 0,
                             dict(epi=_epi(a="item" if item else "shared", opad=3), quad=dict(blk0=2, tail=3)),
                             dict(kind="quad", bgroup=bg)))
    for nb, grid in PAIR_GEOS:
        shape = ((nb,) if nb else ()) + grid
        ax = tuple(range(1 if nb else 0, len(shape)))
        name = "x".join(map(str, shape))
        for dt in DTYPES:
            out.append(FCase(f"d-pairs-{name}-{dt}", "d", dt, shape, ax, nb, 1.0 / math.sqrt(np.prod(grid)), 0,
                             dict(epi=_epi(a="shared", d=True, shift=0.7, b="shared", pairs=True,
                                           opad=3 if nb else 0, dpad=0, o2pad=5 if nb else 0)),
                             dict(kind="pairs")))
    return out


POW2_GRIDS = {1: (64,), 2: (16, 16), 3: (8, 8, 8)}
ODD_GRIDS = {1: (15,), 2: (15, 20), 3: (9, 8, 7)}
LONG_GRIDS = {2: (8, 8192), 3: (2, 2, 8192)}      # last axis past the row-staged prologue's LDS


def _e_case(tag, grid, nb, per_item, lay, kern, dt, index="fold"):
    m = "item" if per_item else "shared"
    shape = (nb,) + grid
    name = "x".join(map(str, grid))
    return FCase(f"e-{tag}-{name}-nb{nb}-{m}-{lay}-{dt}", "e", dt, shape, tuple(range(1, len(shape))), nb, 0.7, 0,
                 dict(pro=_pro(a=m, b=m, index=index, c=lay, xpad=64)),
                 dict(kernel=kern, D=len(grid), NBM=nbm_class(nb), PI=per_item))


def cases_e():
    """the stand-alone prologue passes: pro_batch, pro_fold (D = 1, nb > 8, a
    last axis too long for the row staging) and pro_rows; x rows 64 elements
    longer than the item"""
    out = []
    for dt in DTYPES:
        for grid in ((32, 32), ODD_GRIDS[2]):
            for nb in (2, 3):
                for lay in ("inter", "item"):
                    out.append(_e_case("batch", grid, nb, False, lay, "batch", dt, index="pixel"))
        for i, (nb, per_item) in enumerate(((2, False), (2, True), (3, False), (3, True), (5, False), (5, True),
                                            (9, False))):
            for grid in (POW2_GRIDS[1], ODD_GRIDS[1]):
                out.append(_e_case("fold1d", grid, nb, per_item, "inter" if i % 2 == 0 else "item", "fold", dt))
        for D in (2, 3):
            for nb, per_item in ((9, False), (11, True), (9, True), (11, False)):
                for grid in (POW2_GRIDS[D], ODD_GRIDS[D]):
                    out.append(_e_case("foldnb", grid, nb, per_item, "inter" if nb == 9 else "item", "fold", dt))
            for nb in (2, 3):
                for per_item in (False, True):
                    out.append(_e_case("foldlong", LONG_GRIDS[D], nb, per_item, "inter", "fold", dt))
            for nb in (1, 2, 3, 4, 5, 8):
                for per_item in (False, True):
                    for grid in (POW2_GRIDS[D], ODD_GRIDS[D]):
                        out.append(_e_case("rows", grid, nb, per_item, "inter" if per_item else "item", "rows", dt))
    return out


# (n1, n0, nb, NFT_PRO_R2C)
PRO_R2C_GEOS = [(512, 16, 1, None), (512, 32, 8, None), (1024, 16, 3, None), (1024, 32, 1, None),
                (2048, 16, 3, "2"), (2048, 32, 1, "2"), (4096, 16, 8, "2"), (4096, 32, 3, "2")]


def cases_f():
    """pro_r2c+dir: the direction-carrying prologue fused with the R2C pass"""
    out = []
    for n1, n0, nb, env in PRO_R2C_GEOS:
        for dt in DTYPES:
            dr = dict(done=1 if nb >= 3 else None, neg=2 if nb >= 3 else None, blk0=3, tail=7)
            out.append(FCase(f"f-pror2c-{nb}x{n0}x{n1}-{dt}", "f", dt, (nb, n0, n1), (1, 2), nb,
                             1.0 / math.sqrt(n0 * n1), 0,
                             dict(pro=_pro(a="shared", b="shared", index="fold", c="inter", xpad=64), dir=dr,
                                  env={"NFT_PRO_R2C": env} if env else {}),
                             dict(rows_n=n1, n0=n0)))
    return out


GROUPS = dict(a=cases_a, b=cases_b, c=cases_c, d=cases_d, e=cases_e, f=cases_f)


def all_cases():
    return [c for g in GROUPS.values() for c in g()]


def pro_instantiations():
    """every (kernel, D, NBM, PI) launch_pro_rows / launch_pro_fold can launch"""
    out = {("rows", D, nbm, pi) for D in (2, 3) for nbm in (2, 4, 8) for pi in (False, True)}
    out |= {("fold", D, nbm, pi) for D in (1, 2, 3) for nbm in (2, 4, 8) for pi in (False, True)}
    return out
