"""The device CG state machine of csrc/nft_blas.hip against a plain reference.

Every entry point is called through the C ABI (as fused_cg.py calls it) and
compared with a numpy restatement in ``np.longdouble`` of the formulas in
include/nifty_amd.h, i.e. the vector algebra of NIFTy's
ConjugateGradient.__call__:

    alpha = gamma / curv                      (guarded, see ``_ref_update``)
    x' = x - alpha d ;  r' = r - alpha (q + shift d)
    gamma' = r'.r' ; xr = x'.r' ; xb = x'.b
    d' = max(0, gamma / gprev) d + r
    r = (ax + shift x) - b                    (residual refresh)

Bounds (derived, none is fitted to output).  u = 2^-53 for fp64 storage and
2^-24 for fp32.

* element-wise: ``4 u (|x| + |alpha d|)`` and ``4 u (|r| + |alpha| (|q| +
  |shift d|))``.  To first order x' carries the cast of alpha to the storage
  type, the product and the subtraction (3 u).  r' carries ``u (|r| + A)``
  from the subtraction, ``3 u A`` from the cast of alpha, the product with
  it and the inner sum, and ``2 u |alpha shift d|`` from the cast of the
  shift and its product, with ``A = |alpha| (|q| + |shift d|)``: within the
  bound while ``2 |alpha shift d| <= 3 |r|``, which ``alpha shift <= 0.5``
  guarantees for these inputs (|r| >= 0.5, |d| <= 1.5); the tests keep
  alpha <= 0.5 with shift 0.7.  Contraction to FMA only removes roundings.
  The direction and the residual have at most four error sources on any
  term, hence the same form.
* reductions: ``(L + 25) 2^-53 sum|terms|`` with L the serial chain per thread
  (ceil(n / (blocks 256))), against the exact sum (``math.fsum`` over error-
  free products) of the values the device stored; the reference's own
  rounding (half an ulp of the sum; 2^-58 sum|terms| where long vectors are
  summed pairwise in longdouble instead) is added.

Inputs are uniform in +-[0.5, 1.5], so one dropped or double-counted element
moves a sum by >= 0.25: ``_assert_sensitive`` checks for every reduction
that the reference without its first, its last or its median element lies
outside the bound.
"""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

LD = np.longdouble
NS = 16
GAMMA, GPREV, CURV, ALPHA, XR, XB, FLAG, DD, DONE, ITER, AUTO, LAZY = range(12)
RED_NT, RED_MAXBLOCKS = 256, 1024
CAP = 2048 * RED_MAXBLOCKS      # 2 097 152: the 1024-block cap exactly
SMALL_N = [1, 255, 256, 257, 2047, 2048, 2049]
LARGE_N = [CAP, CAP + 1, 2 * CAP + 17]
SENT = 3.0e30                   # padding / untouched-slot sentinel (finite in fp32)
NP = {0: np.float64, 1: np.float32}
U = {0: 2.0 ** -53, 1: 2.0 ** -24}
SHIFT = 0.7
OK, ERR_ARG = 0, -1


def red_blocks(n):
    return int(min(max((n + RED_NT * 8 - 1) // (RED_NT * 8), 1), RED_MAXBLOCKS))


def chain(n, nb):
    return -(-n // (nb * RED_NT))


# ------------------------------------------------------------------ helpers
def _draw(rng, shape, dt):
    v = rng.uniform(0.5, 1.5, size=shape) * rng.choice([-1.0, 1.0], size=shape)
    return v.astype(NP[dt])


def _rows(rng, nrhs, n, vs, dt):
    a = np.full((nrhs, vs), SENT, NP[dt])
    a[:, :n] = _draw(rng, (nrhs, n), dt)
    return a


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int64 if a.dtype == np.float64 else np.int32)


def _same(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _two_prod(a, b):
    """a * b = p + e exactly (Dekker / Veltkamp), float64 arrays"""
    p = a * b
    c = 134217729.0

    def split(v):
        t = v * c
        h = t - (t - v)
        return h, v - h
    ah, al = split(a)
    bh, bl = split(b)
    e = ((ah * bh - p) + ah * bl + al * bh) + al * bl
    return p, e


def exact_dot(a, b, drop=None):
    """(sum a_i b_i, sum |a_i b_i|, the reference's own error bound), the
    stored values taken exactly.  drop: an index to leave out."""
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    if drop is not None:
        a = np.delete(a, drop)
        b = np.delete(b, drop)
    if a.size == 0:
        return 0.0, 0.0, 0.0
    if a.size <= 1 << 16 or np.finfo(LD).nmant < 63:
        p, e = _two_prod(a, b)
        s = math.fsum(p.tolist() + e.tolist())
        sa = math.fsum(np.abs(p).tolist())
        return s, sa, 2.0 ** -53 * abs(s)
    # long vectors: longdouble products (2^-64 each) summed pairwise by numpy
    # (depth < 64): relative to sum|terms| below 2^-58
    t = a.astype(LD) * b.astype(LD)
    sa = float(np.sum(np.abs(t)))
    s = float(np.sum(t))
    return s, sa, 2.0 ** -58 * sa + 2.0 ** -53 * abs(s)


def red_bound(sumabs, L, extra=25):
    return (L + extra) * 2.0 ** -53 * sumabs


def assert_reduction(dev, a, b, Lc, what, scale=1.0):
    """|dev - scale * sum a b| within the reduction bound, and the bound is
    sharp enough to see one missing element"""
    s, sa, eref = exact_dot(a, b)
    if np.isnan(s):
        assert np.isnan(dev), what
        return
    bound = abs(scale) * (red_bound(sa, Lc) + eref)
    assert abs(dev - scale * s) <= bound, (what, dev, scale * s, abs(dev - scale * s), bound)
    if sa == 0.0:
        return      # every term is zero (the guard table's r = 0 rows): the sum is exactly 0
    _assert_sensitive(a, b, Lc, what)


def _assert_sensitive(a, b, Lc, what):
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    if a.size == 0:
        return
    t = np.abs(a * b)
    mid = int(np.argpartition(t, a.size // 2)[a.size // 2])
    if a.size > 1 << 16:
        # a missing element moves the sum by |term|: compare that directly
        sa = float(np.sum(t.astype(LD)))
        bound = red_bound(sa, Lc) + 2.0 ** -57 * sa
        for i in (0, a.size - 1, mid):
            assert t[i] > bound, (what, "bound blind to element", i, t[i], bound)
        return
    s, sa, eref = exact_dot(a, b)
    bound = red_bound(sa, Lc) + eref
    for i in {0, a.size - 1, mid}:
        s1, _, _ = exact_dot(a, b, drop=i)
        assert abs(s1 - s) > bound, (what, "bound blind to element", i, abs(s1 - s), bound)


@pytest.fixture(scope="module")
def nat(dev):
    from nifty_amd import _native
    _native.load()
    return _native


class Lib:
    """thin caller: numpy in, device buffers held, numpy out"""

    def __init__(self, nat, dev):
        self.nat, self.lib, self.dev = nat, nat.load(), dev
        self.P, self.s = nat.ptr, nat.stream_ptr

    def up(self, a):
        return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(self.dev)

    def ws(self, n, nrhs):
        """reduce workspace with a sentinel tail (nothing may write past it)"""
        need = nrhs * 3 * red_blocks(n)
        assert self.lib.nft_reduce_workspace(n) == 3 * red_blocks(n) * 8
        return torch.full((need + 8,), SENT, dtype=torch.float64, device=self.dev), need

    @staticmethod
    def down(t):
        torch.cuda.synchronize()
        return t.cpu().numpy()


@pytest.fixture(scope="module")
def L(nat, dev):
    return Lib(nat, dev)


def _sc_block(rng, **kw):
    """a scalar block with recognisable values in every slot"""
    sc = np.array([2.0 + rng.uniform(), 3.0 + rng.uniform(), 4.0 + rng.uniform(), -11.0, -12.0, -13.0, 0.0, -14.0,
                   0.0, 5.0, 0.0, 0.0, -15.0, -16.0, -17.0, -18.0])
    for k, v in kw.items():
        sc[globals()[k]] = v
    return sc


# ------------------------------------------------------------------ update
def _alpha64(sc):
    with np.errstate(all="ignore"):
        return np.float64(sc[GAMMA]) / np.float64(sc[CURV])


def _guard_ok(sc):
    curv, alpha = sc[CURV], _alpha64(sc)
    return bool(curv == curv and curv != 0.0 and alpha >= 0.0 and alpha == alpha)


def _ref_update(x, r, d, q, shift, sc):
    """longdouble x', r' and the error bounds' magnitudes for a step that applies"""
    with np.errstate(all="ignore"):
        al = LD(sc[GAMMA]) / LD(sc[CURV])
        xl, rl, dl, ql = (v.astype(LD) for v in (x, r, d, q))
        xn = xl - al * dl
        rn = rl - al * (ql + LD(shift) * dl)
        mx = np.abs(xl) + np.abs(al * dl)
        mr = np.abs(rl) + np.abs(al) * (np.abs(ql) + np.abs(LD(shift) * dl))
    return xn, rn, mx, mr


def check_update_row(dt, n, Lc, x0, r0, d, q, b, shift, sc0, x1, r1, sc1, what):
    """one right-hand side of nft_cg_update*: vectors are whole rows (length
    vstride), b may be None"""
    u = U[dt]
    assert _same(x1[n:], x0[n:]) and _same(r1[n:], r0[n:]), (what, "padding written")
    if sc0[DONE] != 0.0:
        assert _same(sc1, sc0), (what, "DONE row's scalars changed", sc0, sc1)
        assert _same(x1, x0) and _same(r1, r0), (what, "DONE row moved")
        return
    ok = _guard_ok(sc0)
    a64 = _alpha64(sc0)
    exp = sc0.copy()
    exp[ALPHA] = a64
    exp[FLAG] = 0.0 if ok else 1.0
    exp[ITER] = sc0[ITER] + 1.0
    if ok:
        exp[GPREV] = sc0[GAMMA]
    # ALPHA: a correctly rounded fp64 division
    assert (np.isnan(a64) and np.isnan(sc1[ALPHA])) or sc1[ALPHA] == a64, (what, sc1[ALPHA], a64)
    if not ok:
        assert _same(x1, x0) and _same(r1, r0), (what, "guarded step moved x or r")
        exp[DONE] = 2.0
        for k in range(NS):
            if k != ALPHA:
                assert _bits(sc1[k:k + 1])[0] == _bits(exp[k:k + 1])[0], (what, "scalar", k, sc1[k], exp[k])
        return
    xn, rn, mx, mr = _ref_update(x0[:n], r0[:n], d[:n], q[:n], shift, sc0)
    fin = np.isfinite(rn.astype(np.float64))
    ex = np.abs(x1[:n].astype(LD) - xn)
    er = np.abs(r1[:n].astype(LD) - rn)
    assert np.all(ex <= 4 * u * mx), (what, "x", float(np.max(ex / mx)) / u)
    assert np.all(er[fin] <= 4 * u * mr[fin]), (what, "r", float(np.max(er[fin] / mr[fin])) / u)
    assert np.all(np.isnan(r1[:n][~fin])), (what, "NaN of r lost")
    assert_reduction(sc1[GAMMA], r1[:n], r1[:n], Lc, what + " GAMMA")
    assert_reduction(sc1[XR], x1[:n], r1[:n], Lc, what + " XR")
    if b is None:
        assert sc1[XB] == 0.0, (what, "XB without b", sc1[XB])
    else:
        assert_reduction(sc1[XB], x1[:n], b[:n], Lc, what + " XB")
    g1 = sc1[GAMMA]
    exp[DONE] = 2.0 if (sc0[AUTO] != 0.0 and not g1 > 0.0) else 0.0
    for k in (GPREV, CURV, FLAG, DD, DONE, ITER, AUTO, LAZY, 12, 13, 14, 15):
        assert _bits(sc1[k:k + 1])[0] == _bits(exp[k:k + 1])[0], (what, "scalar", k, sc1[k], exp[k])


def run_update(L, dt, n, vs, X, R, D, Q, B, shift, SC, single=False):
    """nft_cg_update_batched on host arrays (nrhs, vs); returns x', r', sc'.
    single: one call per right-hand side instead of the batched one."""
    nrhs = X.shape[0]
    x, r, d, q, b, sc = (L.up(v) for v in (X, R, D, Q, B, SC))
    ws, need = L.ws(n, nrhs)
    P = L.P
    if single:
        for j in range(nrhs):
            st = L.lib.nft_cg_update_batched(P(x[j]), P(r[j]), P(d[j]), P(q[j]), P(b[j] if b is not None else None),
                                             n, vs, 1, dt, shift, P(sc[j]), P(ws), L.s())
            assert st == OK
    else:
        st = L.lib.nft_cg_update_batched(P(x), P(r), P(d), P(q), P(b), n, vs, nrhs, dt, shift, P(sc), P(ws), L.s())
        assert st == OK
    wsh = L.down(ws)
    assert np.all(wsh[need:] == SENT), "workspace overrun"
    return L.down(x), L.down(r), L.down(sc)


def _update_scalars(rng, nrhs):
    """row 0 live; further rows cycle through DONE, a tripped guard and AUTO"""
    SC = np.stack([_sc_block(rng) for _ in range(nrhs)])
    for j in range(nrhs):
        SC[j, CURV] = SC[j, GAMMA] * rng.uniform(2.0, 4.0)      # alpha in (0.25, 0.5]
        kind = j % 4
        if kind == 1:
            SC[j, DONE] = 1.0
        elif kind == 2:
            SC[j, CURV] = -SC[j, CURV]
        elif kind == 3:
            SC[j, AUTO] = 1.0
    return SC


@pytest.mark.parametrize("dt", [0, 1])
@pytest.mark.parametrize("n", SMALL_N)
def test_update_small(L, dt, n):
    """nft_cg_update_batched: x', r', scalars and sums against the reference;
    padding kept; every right-hand side bitwise its single call"""
    rng = np.random.default_rng(1000 + n)
    for vs in (n, n + 37):
        for with_b in (True, False):
            for nrhs in (1, 3, 8):
                X, R, D, Q, Bv = (_rows(rng, nrhs, n, vs, dt) for _ in range(5))
                B = Bv if with_b else None
                SC = _update_scalars(rng, nrhs)
                x1, r1, sc1 = run_update(L, dt, n, vs, X, R, D, Q, B, SHIFT, SC)
                for j in range(nrhs):
                    check_update_row(dt, n, chain(n, red_blocks(n)), X[j], R[j], D[j], Q[j],
                                     None if B is None else B[j], SHIFT, SC[j], x1[j], r1[j], sc1[j],
                                     f"n={n} vs={vs} b={with_b} rhs {j}/{nrhs}")
                if nrhs > 1:
                    x2, r2, sc2 = run_update(L, dt, n, vs, X, R, D, Q, B, SHIFT, SC, single=True)
                    assert _same(x1, x2) and _same(r1, r2) and _same(sc1, sc2), "batched != single calls"


@pytest.mark.parametrize("dt", [0, 1])
@pytest.mark.parametrize("n", LARGE_N)
def test_update_large(L, dt, n):
    """the 1024-block cap and the grid-stride passes beyond it"""
    rng = np.random.default_rng(2000 + n % 1000)
    nrhs, vs = 2, n + 37
    X, R, D, Q, B = (_rows(rng, nrhs, n, vs, dt) for _ in range(5))
    SC = _update_scalars(rng, nrhs)
    SC[1, DONE] = 0.0
    x1, r1, sc1 = run_update(L, dt, n, vs, X, R, D, Q, B, SHIFT, SC)
    for j in range(nrhs):
        check_update_row(dt, n, chain(n, red_blocks(n)), X[j], R[j], D[j], Q[j], B[j], SHIFT, SC[j], x1[j], r1[j],
                         sc1[j], f"n={n} rhs {j}")


GUARD_ROWS = [
    ("live", {}),
    ("DONE=1", dict(DONE=1.0)),
    ("DONE=2", dict(DONE=2.0)),
    ("curv=+0", dict(CURV=0.0)),
    ("curv=-0", dict(CURV=-0.0)),
    ("curv=NaN", dict(CURV=float("nan"))),
    ("curv<0", dict(CURV=-3.5)),
    ("gamma=NaN", dict(GAMMA=float("nan"))),
    ("curv=+inf", dict(CURV=float("inf"))),
    ("gamma=0 AUTO=0", dict(GAMMA=0.0)),
    ("gamma=0 AUTO=1", dict(GAMMA=0.0, AUTO=1.0)),
    ("AUTO=1 r=0", dict(GAMMA=0.0, AUTO=1.0)),
    ("AUTO=0 r=0", dict(GAMMA=0.0)),
    ("AUTO=1 NaN in r", dict(AUTO=1.0)),
]


def guard_scalars(rng, rows):
    SC = []
    for name, kw in rows:
        sc = _sc_block(rng)
        sc[CURV] = sc[GAMMA] * 3.0
        for k, v in kw.items():
            sc[globals()[k]] = v
        SC.append(sc)
    return np.stack(SC)


def guard_expect(name, sc0, sc1):
    """the state machine's verdict per table row, spelled out"""
    if name.startswith("DONE"):
        return
    tripped = name in ("curv=+0", "curv=-0", "curv=NaN", "curv<0", "gamma=NaN")
    assert sc1[FLAG] == (1.0 if tripped else 0.0), name
    assert sc1[ITER] == sc0[ITER] + 1.0, name
    frozen = tripped or name in ("AUTO=1 r=0", "AUTO=1 NaN in r")
    assert sc1[DONE] == (2.0 if frozen else 0.0), (name, sc1[DONE])
    if name == "AUTO=1 NaN in r":
        assert np.isnan(sc1[GAMMA])
    if name in ("AUTO=1 r=0", "AUTO=0 r=0"):
        assert sc1[GAMMA] == 0.0
    if name == "curv=+inf":
        assert sc1[ALPHA] == 0.0


@pytest.mark.parametrize("dt", [0, 1])
def test_update_guard_table(L, dt):
    """one batched launch over 8 right-hand sides with the guard table's first
    eight scalar blocks, a second over the remaining six"""
    n, vs = 2049, 2049 + 37
    rng = np.random.default_rng(7)
    for rows in (GUARD_ROWS[:8], GUARD_ROWS[8:]):
        nrhs = len(rows)
        X, R, D, Q, B = (_rows(rng, nrhs, n, vs, dt) for _ in range(5))
        for j, (name, _) in enumerate(rows):
            if name.endswith("r=0"):
                R[j, :n] = 0.0
            if name.endswith("NaN in r"):
                R[j, n // 2] = np.nan
        SC = guard_scalars(rng, rows)
        x1, r1, sc1 = run_update(L, dt, n, vs, X, R, D, Q, B, SHIFT, SC)
        for j, (name, _) in enumerate(rows):
            check_update_row(dt, n, chain(n, red_blocks(n)), X[j], R[j], D[j], Q[j], B[j], SHIFT, SC[j], x1[j], r1[j],
                             sc1[j], name)
            guard_expect(name, SC[j], sc1[j])
        x2, r2, sc2 = run_update(L, dt, n, vs, X, R, D, Q, B, SHIFT, SC, single=True)
        assert _same(x1, x2) and _same(r1, r2) and _same(sc1, sc2), "batched != single calls"


# ------------------------------------------------------------------ dot / curv
@pytest.mark.parametrize("dt", [0, 1])
@pytest.mark.parametrize("n", [0] + SMALL_N + LARGE_N)
def test_dot_batched(L, dt, n):
    rng = np.random.default_rng(3000 + n % 1000)
    for vs in ((n, n + 37) if n <= 2049 else (n + 37,)):
        for nrhs, ostride in (((1, 1), (3, 16), (8, 1)) if n <= 2049 else ((2, 16),)):
            A, B = (_rows(rng, nrhs, n, max(vs, 1), dt) for _ in range(2))
            a, b = L.up(A), L.up(B)
            out = torch.full((nrhs, ostride), SENT, dtype=torch.float64, device=L.dev)
            ws, need = L.ws(n, nrhs)
            assert L.lib.nft_dot_batched(L.P(a), L.P(b), n, max(vs, 1), nrhs, dt, L.P(out), ostride, L.P(ws),
                                         L.s()) == OK
            o, w = L.down(out), L.down(ws)
            assert np.all(w[need:] == SENT)
            assert np.all(o[:, 1:] == SENT)
            for j in range(nrhs):
                if n == 0:
                    assert o[j, 0] == 0.0
                else:
                    assert_reduction(o[j, 0], A[j, :n], B[j, :n], chain(n, red_blocks(n)), f"dot n={n} rhs {j}")
            if nrhs > 1:
                for j in range(nrhs):
                    o1 = torch.full((1,), SENT, dtype=torch.float64, device=L.dev)
                    assert L.lib.nft_dot_batched(L.P(a[j]), L.P(b[j]), n, max(vs, 1), 1, dt, L.P(o1), 1, L.P(ws),
                                                 L.s()) == OK
                    assert _same(L.down(o1), o[j, :1])


@pytest.mark.parametrize("dt", [0, 1])
@pytest.mark.parametrize("n", SMALL_N)
def test_curv_batched(L, dt, n):
    """CURV = d.(q + shift d): q + shift d is formed in the storage type (two
    roundings and, for fp32, the cast of the shift: 3 u on each term) and
    then summed like every other reduction"""
    rng = np.random.default_rng(3500 + n)
    nrhs, vs = 3, n + 37
    D, Q = (_rows(rng, nrhs, n, vs, dt) for _ in range(2))
    SC = np.stack([_sc_block(rng) for _ in range(nrhs)])
    d, q, sc = L.up(D), L.up(Q), L.up(SC)
    ws, need = L.ws(n, nrhs)
    assert L.lib.nft_cg_curv_batched(L.P(d), L.P(q), n, vs, nrhs, dt, SHIFT, L.P(sc), L.P(ws), L.s()) == OK
    sc1 = L.down(sc)
    for j in range(nrhs):
        dl, ql = D[j, :n].astype(LD), Q[j, :n].astype(LD)
        t = dl * (ql + LD(SHIFT) * dl)
        mag = np.abs(dl) * (np.abs(ql) + np.abs(LD(SHIFT) * dl))
        ref = float(np.sum(t))
        sa = float(np.sum(mag))
        bound = red_bound(sa, chain(n, red_blocks(n))) + 3 * U[dt] * sa + 2.0 ** -58 * sa
        assert abs(sc1[j, CURV] - ref) <= bound, (n, j, sc1[j, CURV], ref, bound)
        assert float(np.median(np.abs(t))) > bound, "bound blind to one element"
        exp = SC[j].copy()
        exp[CURV] = sc1[j, CURV]
        assert _same(sc1[j], exp)


# ------------------------------------------------------------------ direction
def _dir_scalars(rng, nrhs):
    """row 0 live with beta > 0; then DONE, gamma/gprev NaN (0/0), negative,
    live again"""
    SC = np.stack([_sc_block(rng) for _ in range(nrhs)])
    for j in range(nrhs):
        kind = j % 5
        if kind == 1:
            SC[j, DONE] = 1.0
        elif kind == 2:
            SC[j, GAMMA] = SC[j, GPREV] = 0.0
        elif kind == 3:
            SC[j, GAMMA] = -SC[j, GAMMA]
        elif kind == 4:
            SC[j, DONE] = 2.0
    return SC


def _beta(sc):
    with np.errstate(all="ignore"):
        b = LD(sc[GAMMA]) / LD(sc[GPREV])
        b64 = np.float64(sc[GAMMA]) / np.float64(sc[GPREV])
    return b if b64 > 0.0 else LD(0.0)


def check_dir_row(dt, n, d0, r, sc, d1, what):
    assert _same(d1[n:], d0[n:]), (what, "padding written")
    if sc[DONE] != 0.0:
        assert _same(d1, d0), (what, "DONE row's direction changed")
        return
    beta = _beta(sc)
    ref = beta * d0[:n].astype(LD) + r[:n].astype(LD)
    mag = np.abs(beta * d0[:n].astype(LD)) + np.abs(r[:n].astype(LD))
    err = np.abs(d1[:n].astype(LD) - ref)
    assert np.all(err <= 4 * U[dt] * mag), (what, float(np.max(err / mag)) / U[dt])
    if beta == 0:
        # the clamp: d' = 0 d + r is r exactly (|d| finite)
        assert np.array_equal(d1[:n], r[:n]), what


def run_dirs(L, dt, n, vs, D, R, SC, shift, single=False):
    """direction, direction_dd (partials with a sentinel tail) on the same
    input: returns d'(plain), d'(dd), partials (nrhs, pstride), nb"""
    nrhs = D.shape[0]
    P = L.P
    nb = int(L.lib.nft_cg_dd_blocks(n))
    assert nb == red_blocks(n)
    pstride = nb + 3
    r, sc = L.up(R), L.up(SC)
    da, db = L.up(D), L.up(D)
    part = torch.full((nrhs, pstride), SENT, dtype=torch.float64, device=L.dev)
    if single:
        for j in range(nrhs):
            assert L.lib.nft_cg_direction_batched(P(da[j]), P(r[j]), n, vs, 1, dt, P(sc[j]), L.s()) == OK
            assert L.lib.nft_cg_direction_dd_batched(P(db[j]), P(r[j]), n, vs, 1, dt, P(sc[j]), shift, P(part[j]),
                                                     pstride, L.s()) == OK
    else:
        assert L.lib.nft_cg_direction_batched(P(da), P(r), n, vs, nrhs, dt, P(sc), L.s()) == OK
        assert L.lib.nft_cg_direction_dd_batched(P(db), P(r), n, vs, nrhs, dt, P(sc), shift, P(part), pstride,
                                                 L.s()) == OK
    folded = torch.full((nrhs, 2), SENT, dtype=torch.float64, device=L.dev)
    pc = part[:, :nb].contiguous()
    assert L.lib.nft_fold_partials(P(pc), nb, nrhs, P(folded), 2, L.s()) == OK
    assert _same(L.down(sc), SC), "direction wrote the scalars"
    return L.down(da), L.down(db), L.down(part), L.down(folded), nb


def check_dirs(L, dt, n, vs, nrhs, rng, batch_check):
    D, R = (_rows(rng, nrhs, n, vs, dt) for _ in range(2))
    SC = _dir_scalars(rng, nrhs)
    da, db, part, folded, nb = run_dirs(L, dt, n, vs, D, R, SC, SHIFT)
    assert _same(da, db), "direction and direction_dd disagree"
    assert np.all(part[:, nb:] == SENT), "partials past nb written"
    assert np.all(folded[:, 1] == SENT)
    for j in range(nrhs):
        what = f"dir n={n} vs={vs} rhs {j}/{nrhs}"
        check_dir_row(dt, n, D[j], R[j], SC[j], da[j], what)
        if SC[j, DONE] != 0.0:
            assert np.all(part[j, :nb] == 0.0), (what, "DONE row's partials")
            assert folded[j, 0] == 0.0
        else:
            # one more rounding (shift * block sum) than the plain reductions,
            # inside the constant's slack: fold_wide's chain is 1 + 6 + 16
            assert_reduction(folded[j, 0], db[j, :n], db[j, :n], chain(n, nb), what + " d.d", scale=SHIFT)
    if batch_check and nrhs > 1:
        da2, db2, part2, _, _ = run_dirs(L, dt, n, vs, D, R, SC, SHIFT, single=True)
        assert _same(da, da2) and _same(db, db2) and _same(part, part2), "batched != single calls"


@pytest.mark.parametrize("dt", [0, 1])
@pytest.mark.parametrize("n", SMALL_N)
def test_direction_small(L, dt, n):
    rng = np.random.default_rng(4000 + n)
    for vs in (n, n + 37):
        for nrhs in (1, 3, 8):
            check_dirs(L, dt, n, vs, nrhs, rng, True)


@pytest.mark.parametrize("dt", [0, 1])
@pytest.mark.parametrize("n", LARGE_N)
def test_direction_large(L, dt, n):
    """past cg_dir_kernel's 8192 x 256 cap (2 097 152) and red_blocks' cap"""
    rng = np.random.default_rng(4500 + n % 1000)
    D, R = (_rows(rng, 2, n, n + 37, dt) for _ in range(2))
    SC = _dir_scalars(rng, 2)
    SC[1, DONE] = 0.0
    SC[1, GAMMA] = -1.0
    da, db, part, folded, nb = run_dirs(L, dt, n, n + 37, D, R, SC, SHIFT)
    assert _same(da, db)
    assert np.all(part[:, nb:] == SENT)
    for j in range(2):
        check_dir_row(dt, n, D[j], R[j], SC[j], da[j], f"dir n={n} rhs {j}")
        assert_reduction(folded[j, 0], db[j, :n], db[j, :n], chain(n, nb), f"d.d n={n} rhs {j}", scale=SHIFT)


@pytest.mark.parametrize("dt", [0, 1])
@pytest.mark.parametrize("n1,n2,gap", [(1, 1, 0), (257, 2049, 5), (2049, 255, 0), (4097, 2048, 3)])
def test_direction_dd2_is_two_dd(L, dt, n1, n2, gap):
    """nft_cg_direction_dd2_batched: bitwise two dd calls, in d and in every
    partial slot; argument checks"""
    rng = np.random.default_rng(4700 + n1)
    nrhs, o2 = 5, n1 + gap
    vs = o2 + n2 + 11
    nb1, nb2 = red_blocks(n1), red_blocks(n2)
    poff2 = nb1 + 2
    pstride = poff2 + nb2 + 1
    D = _rows(rng, nrhs, vs, vs, dt)
    R = _rows(rng, nrhs, vs, vs, dt)
    SC = _dir_scalars(rng, nrhs)
    P = L.P
    r, sc = L.up(R), L.up(SC)
    d2, dd = L.up(D), L.up(D)
    p2 = torch.full((nrhs, pstride), SENT, dtype=torch.float64, device=L.dev)
    pd = torch.full((nrhs, pstride), SENT, dtype=torch.float64, device=L.dev)
    assert L.lib.nft_cg_direction_dd2_batched(P(d2), P(r), n1, o2, n2, vs, nrhs, dt, P(sc), SHIFT, P(p2), poff2,
                                              pstride, L.s()) == OK
    assert L.lib.nft_cg_direction_dd_batched(P(dd), P(r), n1, vs, nrhs, dt, P(sc), SHIFT, P(pd), pstride,
                                             L.s()) == OK
    assert L.lib.nft_cg_direction_dd_batched(P(dd[0, o2:]), P(r[0, o2:]), n2, vs, nrhs, dt, P(sc), SHIFT,
                                             P(pd[0, poff2:]), pstride, L.s()) == OK
    a, b, pa, pb = L.down(d2), L.down(dd), L.down(p2), L.down(pd)
    assert _same(a, b) and _same(pa, pb)
    keep = np.ones(vs, bool)
    keep[:n1] = False
    keep[o2:o2 + n2] = False
    assert _same(a[:, keep], D[:, keep]), "elements outside both ranges written"
    slots = np.ones(pstride, bool)
    slots[:nb1] = False
    slots[poff2:poff2 + nb2] = False
    assert np.all(pa[:, slots] == SENT)
    for j in range(nrhs):
        check_dir_row(dt, n1, D[j, :o2], R[j, :o2], SC[j], a[j, :o2], f"dd2 range 1 rhs {j}")
        check_dir_row(dt, n2, D[j, o2:], R[j, o2:], SC[j], a[j, o2:], f"dd2 range 2 rhs {j}")
    bad = [dict(o2=n1 - 1), dict(poff2=nb1 - 1), dict(pstride=poff2 + nb2 - 1), dict(n2=0), dict(dt=2)]
    for kw in bad:
        a_ = dict(n1=n1, o2=o2, n2=n2, poff2=poff2, pstride=pstride, dt=dt)
        a_.update(kw)
        st = L.lib.nft_cg_direction_dd2_batched(P(d2), P(r), a_["n1"], a_["o2"], a_["n2"], vs, nrhs, a_["dt"], P(sc),
                                                SHIFT, P(p2), a_["poff2"], a_["pstride"], L.s())
        assert st == ERR_ARG, kw
    assert L.lib.nft_cg_direction_dd_batched(P(dd), P(r), n1, vs, nrhs, dt, P(sc), SHIFT, P(pd), nb1 - 1,
                                             L.s()) == ERR_ARG
    assert _same(L.down(d2), a), "a rejected call wrote"


# ------------------------------------------------------------------ segments
@pytest.mark.parametrize("dt", [0, 1])
@pytest.mark.parametrize("n1,n2,gap", [(1, 257, 0), (2049, 255, 7), (4097, 2048, 0)])
def test_update_segments(L, dt, n1, n2, gap):
    """nft_cg_update_seg_batched / seg2 with nbtot > nb and blk0 > 0: seg2 is
    bitwise two seg calls, slots outside the written ranges keep a sentinel,
    nft_cg_finalize_batched over the assembled partials gives the reference
    scalars; the argument checks reject"""
    rng = np.random.default_rng(5000 + n1)
    nrhs, o2 = 8, n1 + gap
    vs = o2 + n2 + 13
    nb1, nb2 = red_blocks(n1), red_blocks(n2)
    blk1, blk2 = nb2 + 2, 1            # the second range's slots first
    nbtot = blk1 + nb1 + 2
    X, R, D, Q = (_rows(rng, nrhs, vs, vs, dt) for _ in range(4))
    SC = guard_scalars(rng, GUARD_ROWS[:8])
    P = L.P
    d, q, sc = L.up(D), L.up(Q), L.up(SC)

    def fresh():
        return L.up(X), L.up(R), torch.full((nrhs, 3, nbtot), SENT, dtype=torch.float64, device=L.dev)
    xa, ra, pa = fresh()
    assert L.lib.nft_cg_update_seg2_batched(P(xa), P(ra), P(d), P(q), n1, blk1, o2, n2, blk2, vs, nrhs, dt, SHIFT,
                                            P(sc), P(pa), nbtot, L.s()) == OK
    xb, rb, pb = fresh()
    assert L.lib.nft_cg_update_seg_batched(P(xb), P(rb), P(d), P(q), None, n1, vs, nrhs, dt, SHIFT, P(sc), P(pb),
                                           nbtot, blk1, L.s()) == OK
    assert L.lib.nft_cg_update_seg_batched(P(xb[0, o2:]), P(rb[0, o2:]), P(d[0, o2:]), P(q[0, o2:]), None, n2, vs,
                                           nrhs, dt, SHIFT, P(sc), P(pb), nbtot, blk2, L.s()) == OK
    x1, r1, p1 = L.down(xa), L.down(ra), L.down(pa)
    assert _same(x1, L.down(xb)) and _same(r1, L.down(rb)) and _same(p1, L.down(pb)), "seg2 != two seg calls"
    assert _same(L.down(sc), SC), "segment update wrote the scalars"
    slots = np.ones(nbtot, bool)
    slots[blk1:blk1 + nb1] = False
    slots[blk2:blk2 + nb2] = False
    assert np.all(p1[:, :, slots] == SENT), "partial slots outside the ranges written"
    assert np.all(p1[:, :, ~slots] != SENT)
    # the other segments of a real solve fill the remaining slots; here zeros
    pa[:, :, torch.from_numpy(slots).to(L.dev)] = 0.0
    assert L.lib.nft_cg_finalize_batched(P(pa), nbtot, nrhs, P(sc), L.s()) == OK
    sc1 = L.down(sc)
    keep = np.ones(vs, bool)
    keep[:n1] = False
    keep[o2:o2 + n2] = False
    assert _same(x1[:, keep], X[:, keep]) and _same(r1[:, keep], R[:, keep]), "elements outside the ranges written"
    for j, (name, _) in enumerate(GUARD_ROWS[:8]):
        # both ranges as one vector: element-wise per element, sums over both
        # (chain: the longer of the two, and the fold's ceil(nbtot / 256) = 1
        # is inside the constant as for nft_cg_update_batched)
        sel = ~keep
        n = int(sel.sum())

        def cat(v):
            return np.concatenate([v[j, sel], v[j, keep]])
        check_update_row(dt, n, max(chain(n1, nb1), chain(n2, nb2)), cat(X), cat(R), cat(D), cat(Q), None, SHIFT,
                         SC[j], cat(x1), cat(r1), sc1[j], "seg " + name)
        guard_expect(name, SC[j], sc1[j])
    xc, rc, pc = fresh()
    seg2_bad = [dict(o2=n1 - 1), dict(blk1=nbtot - nb1 + 1), dict(blk2=nbtot - nb2 + 1), dict(blk2=blk1),
                dict(blk2=blk1 + nb1 - 1), dict(blk1=-1), dict(n1=0), dict(dt=2)]
    for kw in seg2_bad:
        a_ = dict(n1=n1, blk1=blk1, o2=o2, n2=n2, blk2=blk2, dt=dt)
        a_.update(kw)
        st = L.lib.nft_cg_update_seg2_batched(P(xc), P(rc), P(d), P(q), a_["n1"], a_["blk1"], a_["o2"], a_["n2"],
                                              a_["blk2"], vs, nrhs, a_["dt"], SHIFT, P(sc), P(pc), nbtot, L.s())
        assert st == ERR_ARG, kw
    for blk0 in (-1, nbtot - nb1 + 1):
        assert L.lib.nft_cg_update_seg_batched(P(xc), P(rc), P(d), P(q), None, n1, vs, nrhs, dt, SHIFT, P(sc),
                                               P(pc), nbtot, blk0, L.s()) == ERR_ARG
    assert L.lib.nft_cg_update_seg_batched(P(xc), P(rc), P(d), P(q), None, n1, vs, nrhs, 2, SHIFT, P(sc), P(pc),
                                           nbtot, blk1, L.s()) == ERR_ARG
    assert _same(L.down(xc), X) and _same(L.down(rc), R) and np.all(L.down(pc) == SENT), "a rejected call wrote"


# ------------------------------------------------------------------ residual
def run_residual(L, dt, n, vs, R, AX, X, B, SC, single=False):
    nrhs = R.shape[0]
    P = L.P
    r, ax, x, b, sc = (L.up(v) for v in (R, AX, X, B, SC))
    ws, need = L.ws(n, nrhs)
    if single:
        for j in range(nrhs):
            assert L.lib.nft_cg_residual_batched(P(r[j]), P(ax[j]), P(x[j]), P(b[j] if b is not None else None), n,
                                                 vs, 1, dt, SHIFT, P(sc[j]), P(ws), L.s()) == OK
    else:
        assert L.lib.nft_cg_residual_batched(P(r), P(ax), P(x), P(b), n, vs, nrhs, dt, SHIFT, P(sc), P(ws),
                                             L.s()) == OK
    assert np.all(L.down(ws)[need:] == SENT)
    return L.down(r), L.down(sc)


def check_residual(L, dt, n, vs, nrhs, with_b, rng, batch_check):
    R, AX, X, Bv = (_rows(rng, nrhs, n, vs, dt) for _ in range(4))
    B = Bv if with_b else None
    SC = np.stack([_sc_block(rng) for _ in range(nrhs)])
    for j in range(nrhs):
        if j % 3 == 1:
            SC[j, DONE] = 1.0 + (j % 2)
    r1, sc1 = run_residual(L, dt, n, vs, R, AX, X, B, SC)
    for j in range(nrhs):
        what = f"residual n={n} vs={vs} b={with_b} rhs {j}/{nrhs}"
        assert _same(r1[j, n:], R[j, n:]), (what, "padding written")
        if SC[j, DONE] != 0.0:
            assert _same(r1[j], R[j]) and _same(sc1[j], SC[j]), (what, "DONE row changed")
            continue
        axl, xl = AX[j, :n].astype(LD), X[j, :n].astype(LD)
        bl = B[j, :n].astype(LD) if with_b else LD(0.0)
        ref = (axl + LD(SHIFT) * xl) - bl
        mag = np.abs(axl) + np.abs(LD(SHIFT) * xl) + np.abs(bl)
        err = np.abs(r1[j, :n].astype(LD) - ref)
        assert np.all(err <= 4 * U[dt] * mag), (what, float(np.max(err / mag)) / U[dt])
        Lc = chain(n, red_blocks(n))
        assert_reduction(sc1[j, GAMMA], r1[j, :n], r1[j, :n], Lc, what + " GAMMA")
        assert_reduction(sc1[j, XR], X[j, :n], r1[j, :n], Lc, what + " XR")
        if with_b:
            assert_reduction(sc1[j, XB], X[j, :n], B[j, :n], Lc, what + " XB")
        else:
            assert sc1[j, XB] == 0.0
        exp = SC[j].copy()
        exp[GPREV] = SC[j, GAMMA]
        for k in (GAMMA, XR, XB):
            exp[k] = sc1[j, k]
        assert _same(sc1[j], exp), (what, sc1[j], exp)
    if batch_check and nrhs > 1:
        r2, sc2 = run_residual(L, dt, n, vs, R, AX, X, B, SC, single=True)
        assert _same(r1, r2) and _same(sc1, sc2), "batched != single calls"


@pytest.mark.parametrize("dt", [0, 1])
@pytest.mark.parametrize("n", SMALL_N)
def test_residual_small(L, dt, n):
    rng = np.random.default_rng(6000 + n)
    for vs in (n, n + 37):
        for with_b in (True, False):
            for nrhs in (1, 3, 8):
                check_residual(L, dt, n, vs, nrhs, with_b, rng, True)


@pytest.mark.parametrize("dt", [0, 1])
@pytest.mark.parametrize("n", LARGE_N)
def test_residual_large(L, dt, n):
    check_residual(L, dt, n, n + 37, 2, True, np.random.default_rng(6500 + n % 1000), False)


# ------------------------------------------------------------------ fold
@pytest.mark.parametrize("nb", [1, 1023, 1024, 1025, 5000])
@pytest.mark.parametrize("ostride", [1, 16])
def test_fold_partials(L, nb, ostride):
    """fold_wide: thread-strided chain ceil(nb / 1024), 6 shuffles, 16 LDS
    terms -- inside the reduction bound's constant"""
    rng = np.random.default_rng(7000 + nb)
    nrhs = 3
    Pn = _draw(rng, (nrhs, nb), 0)
    part = L.up(Pn)
    out = torch.full((nrhs, ostride), SENT, dtype=torch.float64, device=L.dev)
    assert L.lib.nft_fold_partials(L.P(part), nb, nrhs, L.P(out), ostride, L.s()) == OK
    o = L.down(out)
    assert np.all(o[:, 1:] == SENT)
    ones = np.ones(nb)
    for j in range(nrhs):
        assert_reduction(o[j, 0], Pn[j], ones, -(-nb // 1024), f"fold nb={nb} rhs {j}")
    assert L.lib.nft_fold_partials(L.P(part), 0, nrhs, L.P(out), ostride, L.s()) == ERR_ARG
    assert L.lib.nft_fold_partials(L.P(part), nb, 0, L.P(out), ostride, L.s()) == ERR_ARG
    assert L.lib.nft_fold_partials(None, nb, nrhs, L.P(out), ostride, L.s()) == ERR_ARG


# ------------------------------------------------------------------ lazy flush
@pytest.mark.parametrize("dt", [0, 1])
@pytest.mark.parametrize("n", [1, 255, 257, 2049])
def test_lazy_flush(L, dt, n):
    """nft_cg_lazy_flush: x bitwise the m sequential update launches that
    skip the NaN steps, within m element-wise bounds of the reference; d the
    last slot, also for a row whose alphas are all NaN"""
    rng = np.random.default_rng(8000 + n)
    nrhs, nslot = 4, 5
    vs = n + 37
    ss = nrhs * vs + 29
    P = L.P
    nan = float("nan")
    AL = rng.uniform(0.25, 0.75, size=(nrhs, nslot))
    AL[1, :] = nan                  # never steps
    AL[2, 1] = AL[2, 3] = nan       # mixed
    AL[3, 2:] = nan                 # trips at step 2 and stays out
    X, D = (_rows(rng, nrhs, n, vs, dt) for _ in range(2))
    RING = np.full((nslot, ss), SENT, NP[dt])
    for t in range(nslot):
        RING[t, :nrhs * vs] = _rows(rng, nrhs, n, vs, dt).ravel()
    ring, al = L.up(RING), L.up(AL)
    zero = torch.zeros((nrhs, vs), dtype=ring.dtype, device=L.dev)
    for m in (0, 1, nslot):
        x, d = L.up(X), L.up(D)
        assert L.lib.nft_cg_lazy_flush(P(x), P(d), P(ring), ss, P(al), nslot, m, n, vs, nrhs, dt, L.s()) == OK
        x1, d1 = L.down(x), L.down(d)
        assert _same(x1[:, n:], X[:, n:]) and _same(d1[:, n:], D[:, n:]), "padding written"
        last = RING[m - 1, :nrhs * vs].reshape(nrhs, vs) if m else D
        assert _same(d1[:, :n], last[:, :n]), "d is not the last slot"
        # the same steps, one nft_cg_update_batched launch each
        xs = L.up(X)
        xl = X[:, :n].astype(LD)
        bound = np.zeros((nrhs, n), LD)
        for t in range(m):
            SC = np.stack([_sc_block(rng, CURV=1.0, GAMMA=(AL[j, t] if AL[j, t] == AL[j, t] else 1.0),
                                     DONE=(0.0 if AL[j, t] == AL[j, t] else 1.0)) for j in range(nrhs)])
            rs = torch.zeros((nrhs, vs), dtype=ring.dtype, device=L.dev)
            ws, _ = L.ws(n, nrhs)
            assert L.lib.nft_cg_update_batched(P(xs), P(rs), P(ring[t]), P(zero), None, n, vs, nrhs, dt, 0.0,
                                               P(L.up(SC)), P(ws), L.s()) == OK
            dl = RING[t, :nrhs * vs].reshape(nrhs, vs)[:, :n].astype(LD)
            for j in range(nrhs):
                if AL[j, t] == AL[j, t]:
                    # the device iterate is within `bound` of the reference's
                    bound[j] += 4 * U[dt] * (np.abs(xl[j]) + bound[j] + np.abs(LD(AL[j, t]) * dl[j]))
                    xl[j] = xl[j] - LD(AL[j, t]) * dl[j]
        assert _same(x1, L.down(xs)), f"flush of {m} steps != sequential updates"
        assert _same(x1[1], X[1]), "all-NaN row stepped"
        err = np.abs(x1[:, :n].astype(LD) - xl)
        assert np.all(err <= bound), float(np.max(err - bound))
    x, d = L.up(X), L.up(D)
    bad = [dict(m=nslot + 1), dict(vs=n - 1), dict(ss=nrhs * vs - 1), dict(dt=2), dict(m=-1), dict(nrhs=0)]
    for kw in bad:
        a_ = dict(m=1, vs=vs, ss=ss, dt=dt, nrhs=nrhs)
        a_.update(kw)
        st = L.lib.nft_cg_lazy_flush(P(x), P(d), P(ring), a_["ss"], P(al), nslot, a_["m"], n, a_["vs"], a_["nrhs"],
                                     a_["dt"], L.s())
        assert st == ERR_ARG, kw
    assert _same(L.down(x), X) and _same(L.down(d), D), "a rejected call wrote"
