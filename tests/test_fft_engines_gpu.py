"""Every kernel instantiation, tile tail and launch configuration of the two
transform engines (csrc/nft_fft.hip: engine v2 for power-of-two row / strided /
four-step passes, the generic pass_kernel for everything else and for
fft_c2c) against the extended-precision reference of tests/fft_cases.py.

Every comparison is per item (one independent transform of the batch) under
fft_cases.bound, which follows from the transform lengths and the number
format alone.  Every hartley call runs inside a LaunchProfile and has to leave
exactly the labels of the engine its case names, so a case cannot move to the
other engine unnoticed.

For information (never asserted) each test prints its error over the bound
and the ratio of its error to scipy's same-precision error on the same input;
with NFT_FFT_REPORT=<path> the per-group maxima are also written there as JSON.

Recorded on an MI355X when the file was added (largest error over the bound,
fp64 / fp32): a 0.097 / 0.097, b 0.031 / 0.026, c 0.022 / 0.022, d 0.021 /
0.020, e 0.021 / 0.028, f 0.051 / 0.054, g 0.031 / 0.029, h 0.045 / 0.045;
against scipy in the same precision 1.0 to 1.5 times its error, up to 6.3
times on the direct-DFT lengths (2310: a plain N-term sum per output).  The
generic engine's launches with more than 64 KB of dynamic LDS (up to 161,320 B
at 10080) succeed as they are."""
import json
import os

import numpy as np
import pytest
import torch

import fft_cases as fc

pytestmark = pytest.mark.gpu

REPORT = {}     # (group, dtype) -> [max error / bound, max error / scipy's error, cases]


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    rows = {f"{g}-{dt}": dict(err_over_bound=v[0], err_over_scipy=v[1], checks=v[2])
            for (g, dt), v in sorted(REPORT.items())}
    for k, v in rows.items():
        print(f"\n[fft-engines] {k}: max error/bound {v['err_over_bound']:.3g}, "
              f"max error/scipy {v['err_over_scipy']:.3g} ({v['checks']} checks)", end="")
    path = os.environ.get("NFT_FFT_REPORT")
    if path:
        with open(path, "w") as f:
            json.dump(rows, f, indent=1)


def _nat():
    from nifty_amd import _native as nat
    return nat


def _note(c, what, e, b, e_scipy=None):
    ratio = float(e / e_scipy) if e_scipy else float("nan")
    print(f"[fft-engines] {c.id} {what}: error {e:.3g} = {e / b:.3g} x bound, {ratio:.3g} x scipy")
    v = REPORT.setdefault((c.group, c.dtype), [0.0, 0.0, 0])
    v[0] = max(v[0], float(e / b))
    if e_scipy:
        v[1] = max(v[1], ratio)
    v[2] += 1


def _check(c, out, ref, what="", scipy_out=None):
    """max per-item error of out against ref under the case's bound"""
    b = fc.bound(c.shape, c.axes, c.dtype)
    e = fc.item_errors(out, ref, c.axes)
    es = float(fc.item_errors(scipy_out, ref, c.axes).max()) if scipy_out is not None else None
    _note(c, what, float(e.max()), b, es)
    assert e.max() <= b, (c.id, what, int(np.argmax(e)), float(e.max()), b)
    return e


def _hartley(c, dev, x=None, inplace=False):
    """the case's hartley call inside a LaunchProfile; the labels name the engine"""
    nat = _nat()
    t = torch.from_numpy(fc.case_input(c) if x is None else x).to(dev)
    with nat.LaunchProfile(capacity=16) as p:
        out = nat.hartley(t, c.axes, convention=c.convention, scale=c.scale, out=t if inplace else None)
    assert [label for label, _ in p.records] == fc.expected_labels(c.shape, c.axes), c.id
    assert out.dtype == (torch.float64 if c.dtype == "f64" else torch.float32) and tuple(out.shape) == c.shape
    return out.cpu().numpy()


def _ids(cases):
    return [c.id for c in cases]


# ------------------------------------------------------------------ a. v2 rows, H1D
@pytest.mark.parametrize("c", fc.cases_a(), ids=_ids(fc.cases_a()))
def test_a_rows_h1d(c, dev):
    out = _hartley(c, dev)
    e = _check(c, out, fc.case_ref(c), "out of place", fc.scipy_same_precision(c))
    assert e.shape == (c.shape[0],)
    # the last item is the single row of the last pair, in the partial tile
    assert e[-1] <= fc.bound(c.shape, c.axes, c.dtype)
    inp = _hartley(c, dev, inplace=True)
    assert np.array_equal(inp, out), c.id


# ------------------------------------------------------------------ b. v2 R2C rows, strided UNPACK
@pytest.mark.parametrize("c", fc.cases_b(), ids=_ids(fc.cases_b()))
def test_b_r2c_unpack(c, dev):
    _check(c, _hartley(c, dev), fc.case_ref(c), "", fc.scipy_same_precision(c))


# ------------------------------------------------------------------ c. v2 middle C2C
@pytest.mark.parametrize("c", fc.cases_c(), ids=_ids(fc.cases_c()))
def test_c_middle_c2c(c, dev):
    _check(c, _hartley(c, dev), fc.case_ref(c), "", fc.scipy_same_precision(c))


# ------------------------------------------------------------------ d. four-step
def _item_norm(a, axes):
    return np.sqrt(np.sum(np.abs(a) ** 2, axis=tuple(axes)))


@pytest.mark.parametrize("c", fc.cases_d(), ids=_ids(fc.cases_d()))
def test_d_fourstep(c, dev):
    out = _hartley(c, dev)
    ref = fc.case_ref(c)
    _check(c, out, ref, "out of place", fc.scipy_same_precision(c))
    b = fc.bound(c.shape, c.axes, c.dtype)
    n_item = int(np.prod([c.shape[a] for a in c.axes]))
    # one element (or one swapped pair) cannot hide in the item's l2 norm
    d = np.abs(out.astype(fc.LD) - ref)
    rms = _item_norm(ref, c.axes) / np.sqrt(fc.LD(n_item))
    worst = np.max(np.max(d, axis=c.axes) / rms)
    assert worst <= b * np.sqrt(n_item), (c.id, float(worst), b * np.sqrt(n_item))
    # every element with its mirror partner: the pair H(k), H(-k) is written
    # from one spectrum value F(k) as Re F +- s Im F (||H|| = ||F|| per item)
    f = fc.LD(c.scale) * fc.case_fft(c)
    s = 1 if c.convention == 0 else -1
    o = out.astype(fc.LD)
    om = fc.mirror(o, c.axes)
    fn = _item_norm(f, c.axes)
    e_re = _item_norm((o + om) / 2 - f.real, c.axes) / fn
    e_im = _item_norm((o - om) / 2 - s * f.imag, c.axes) / fn
    assert max(e_re.max(), e_im.max()) <= b, (c.id, float(e_re.max()), float(e_im.max()), b)
    inp = _hartley(c, dev, inplace=True)
    assert np.array_equal(inp, out), c.id


# ------------------------------------------------------------------ e. persistent R2C loop
def _chunked_errors(c, x, out, ref_dtype, chunk=64):
    """per-item errors of the whole batch, the reference formed chunk by chunk
    in ref_dtype; the same for scipy's transform in the case's own precision"""
    import scipy.fft
    e, es = [], []
    own = fc.np_dtype(c)
    for i0 in range(0, c.shape[0], chunk):
        xs = x[i0:i0 + chunk]
        f = scipy.fft.fftn(xs.astype(ref_dtype), axes=c.axes)
        ref = f.real + f.imag
        e.append(fc.item_errors(out[i0:i0 + chunk], ref, c.axes))
        g = scipy.fft.fftn(xs.astype(own), axes=c.axes)
        es.append(fc.item_errors(g.real + g.imag, ref, c.axes))
    return np.concatenate(e), np.concatenate(es)


@pytest.mark.parametrize("n,dt", [(2048, "f32"), (64, "f32"), (2048, "f64")])
def test_e_persistent_r2c(n, dt, dev):
    ncu = torch.cuda.get_device_properties(dev).multi_processor_count
    c, = [c for c in fc.cases_e(ncu) if c.regime["rows_n"] == n and c.dtype == dt]
    r = c.regime
    grid, ntiles, lp = r["grid"], r["ntiles"], r["tile"]
    assert ntiles > grid and ntiles - grid >= 3, (ntiles, grid)       # a second loop iteration
    assert ntiles == -(-(4 * c.shape[0]) // lp)
    x = fc.case_input(c)
    out = _hartley(c, dev, x=x)
    # float32: the float64 transform is the reference (its own error, u64 (2 + 8 log2 N) per axis,
    # is 2^-29 of the float32 bound); float64: extended precision
    e, es = _chunked_errors(c, x, out, np.float64 if dt == "f32" else fc.LD)
    b = fc.bound(c.shape, c.axes, c.dtype)
    _note(c, "all items", float(e.max()), b, float(es.max()))
    assert e.shape == (c.shape[0],)
    # item i is pair lines 4 i .. 4 i + 3; tile = pair line // lp
    first_tile = (4 * np.arange(c.shape[0])) // lp
    last_tile = (4 * np.arange(c.shape[0]) + 3) // lp
    head = last_tile < 3
    second = last_tile >= grid
    assert head.any() and second.any()
    assert e[head].max() <= b, ("first three tiles", float(e[head].max()), b)
    assert e[second].max() <= b, ("tiles of the second loop iteration", int(np.argmax(e * second)),
                                  float(e[second].max()), b)
    assert e[first_tile >= ntiles - 3].max() <= b, ("last three tiles", b)
    assert e.max() <= b, (int(np.argmax(e)), float(e.max()), b)


# ------------------------------------------------------------------ f. generic engine, tails and geometry
@pytest.mark.parametrize("c", fc.cases_f(), ids=_ids(fc.cases_f()))
def test_f_generic_tails(c, dev):
    out = _hartley(c, dev)
    _check(c, out, fc.case_ref(c), "out of place", fc.scipy_same_precision(c))
    inp = _hartley(c, dev, inplace=True)
    assert np.array_equal(inp, out), c.id


# ------------------------------------------------------------------ g. generic engine, plans
@pytest.mark.parametrize("c", fc.cases_g(), ids=_ids(fc.cases_g()))
def test_g_generic_plans(c, dev):
    nat = _nat()
    if c.op == "hartley":
        _check(c, _hartley(c, dev), fc.case_ref(c), "", fc.scipy_same_precision(c))
        return
    import scipy.fft
    x = fc.case_input(c)
    z = torch.from_numpy(x).to(dev)
    fwd = nat.fft_c2c(z, c.axes, forward=True)
    assert fwd.dtype == z.dtype
    _check(c, fwd.cpu().numpy(), fc.case_ref(c), "forward", fc.scipy_same_precision(c))
    n = int(np.prod([c.shape[a] for a in c.axes]))
    inv = nat.fft_c2c(z, c.axes, forward=False, scale=1.0 / n)
    _check(c, inv.cpu().numpy(), fc.case_ref(c, inverse=True, scale=1.0 / n), "inverse",
           scipy.fft.ifftn(x, axes=c.axes))
    assert np.array_equal(z.cpu().numpy(), x)        # out of place: the input is untouched


# ------------------------------------------------------------------ h. refusals
@pytest.mark.parametrize("cid,op,shape,axes,dt,n", fc.REFUSALS, ids=[r[0] for r in fc.REFUSALS])
def test_h_refusals(cid, op, shape, axes, dt, n, dev):
    nat = _nat()
    real = torch.float64 if dt == "f64" else torch.float32
    cplx = torch.complex128 if dt == "f64" else torch.complex64
    x = torch.ones(shape, dtype=real if op == "hartley" else cplx, device=dev)
    with pytest.raises(nat.NativeError, match=f"unsupported FFT length {n}"):
        if op == "hartley":
            nat.hartley(x, axes)
        else:
            nat.fft_c2c(x, axes)
    # the refusal is a host-side return before any launch: the next call is served
    c = fc.Case(f"{cid}-then-valid", "h", "hartley", (7, 30), (1,), dt, 0, 1.0, dict(engine="generic"))
    _check(c, _hartley(c, dev), fc.case_ref(c), "after the refusal", fc.scipy_same_precision(c))
    z = fc.Case(f"{cid}-then-valid-c2c", "h", "c2c", (3, 210), (1,), dt, 0, 1.0, dict(engine="generic"))
    out = nat.fft_c2c(torch.from_numpy(fc.case_input(z)).to(dev), z.axes)
    _check(z, out.cpu().numpy(), fc.case_ref(z), "after the refusal", fc.scipy_same_precision(z))
