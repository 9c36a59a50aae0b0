"""The fused prologue / epilogue passes of ``nft_hartley_fused`` against the
extended-precision reference of tests/fuse_cases.py: the in-pass prologue of
the R2C row pass (a), the one-pass H1D with both (b), the strided and
four-step unpack epilogue (c), its pair sums and quadratic-form partials on
both sides of the tile regrouping (d), the stand-alone prologue kernels
pro_batch / pro_fold / pro_rows in every instantiation (e) and the
direction-carrying prologue fused with the R2C pass (f).

Every call runs inside a LaunchProfile and has to leave exactly
``fuse_cases.expected_fused_labels``.  Outputs are held per item under
``fuse_cases.fused_bound`` (derived from the operands and the number format),
padding and unused partial slots bit-exact, inputs unchanged.  The bitwise
promises of the kernel comments are asserted where both sides can be
reached: folded == per-pixel gather, item j of a batch == a batch of one,
the quad pass's ``out`` == the plain epilogue's.

For information (never asserted) each test prints its error over the bound;
with NFT_FUSE_REPORT=<path> the per-group maxima are written there as JSON.

Recorded on an MI355X when the file was added (largest error over the bound,
fp64 / fp32; cases per precision): a 0.032 / 0.030 (34), b 0.030 / 0.033
(11), c 0.026 / 0.024 (52), d 0.017 / 0.017 (14), e 0.054 / 0.049 (94),
f 0.021 / 0.020 (8).  Every bitwise assertion held; no kernel defect was
found.  The 426 tests take 5 s (the 274 of test_fft_engines_gpu.py: 7 s).

A batch of one is compared bit for bit only where the engine transforms
each item on lines of its own (``fuse_cases.items_independent``): the H1D
pass and the generic engine pair rows across the items of a batch, so there
the two agree to rounding only (observed, and inherent in a pair transform).
"""
import json
import math
import os
import time

import numpy as np
import pytest
import torch

import fuse_cases as fu
import test_cg_primitives_gpu as prim

pytestmark = pytest.mark.gpu

REPORT = {}     # (group, dtype) -> [max error / bound, checks]
TT = {"f64": torch.float64, "f32": torch.float32}
DT = {"f64": 0, "f32": 1}


@pytest.fixture(scope="module", autouse=True)
def _report():
    t0 = time.perf_counter()
    yield
    rows = {f"{g}-{dt}": dict(err_over_bound=v[0], checks=v[1]) for (g, dt), v in sorted(REPORT.items())}
    for k, v in rows.items():
        print(f"\n[fuse-engines] {k}: max error/bound {v['err_over_bound']:.3g} ({v['checks']} checks)", end="")
    print(f"\n[fuse-engines] wall time {time.perf_counter() - t0:.1f} s", end="")
    path = os.environ.get("NFT_FUSE_REPORT")
    if path:
        with open(path, "w") as f:
            json.dump(rows, f, indent=1)


def _nat():
    from nifty_amd import _native as nat
    return nat


def _note(c, ratios):
    print(f"[fuse-engines] {c.id}: " + ", ".join(f"{k} {v:.3g} x bound" for k, v in ratios.items()))
    v = REPORT.setdefault((c.group, c.dtype), [0.0, 0])
    v[0] = max([v[0]] + [float(r) for r in ratios.values()])
    v[1] += len(ratios)


def _ids(cases):
    return [c.id for c in cases]


def _run(c, inp, dev, pixel=False, quad=True, labels=True):
    """the case's nft_hartley_fused call inside a LaunchProfile.  pixel: the
    per-pixel index in place of the folded one; quad=False: the same call
    without the quadratic-form partials.  Returns the outputs in the layout
    of fuse_cases.cast_ref (plus x1 / dpart of a dir case) after checking the
    labels and that no input operand changed."""
    nat = _nat()
    T = TT[c.dtype]
    k, P = fu.items_of(c), fu.period(c)
    pro, epi, dr = c.spec.get("pro"), c.spec.get("epi"), c.spec.get("dir")
    qd = c.spec.get("quad") if quad else None
    dv = {name: torch.from_numpy(np.array(v)).to(dev) for name, v in inp.items()}
    batch = dict(period=P) if c.nb else None
    kw = {}
    if pro:
        p = dict(x=dv["X"][0])
        if c.nb:
            batch["x"] = dv["X"].shape[1]
        for key, name in (("a", "A"), ("b", "B")):
            if pro.get(key):
                p[key] = dv[name]
                if pro[key] == "item":
                    batch[key] = P
        if pro.get("b"):
            fold = pro["index"] == "fold" and not pixel
            p.update(c=dv["C"], index=dv["fidx"] if fold else dv["pidx"], fold=fold)
            if c.nb:
                lay = pro["c"]
                assert lay in ("inter", "item")
                batch.update(dict(c=1, c_elem=k) if lay == "inter" else dict(c=dv["C"].shape[1]))
        if dr:
            nbd = nat.hartley_dir_blocks(fu.grid_of(c))
            dpart = torch.full((k, dr["blk0"] + nbd + dr["tail"]), fu.SENT, dtype=torch.float64, device=dev)
            p["dir"] = dict(r=dv["R"][0], sc=dv["SC"], part=dpart, pstride=dpart.shape[1], shift=fu.DIR_SHIFT,
                            blk0=dr["blk0"])
        kw["pro"] = p
    else:
        kw["x"] = dv["X"].reshape(c.shape)
    out = torch.full((k, P + (epi or {}).get("opad", 0)), fu.SENT, dtype=T, device=dev)
    out2 = None
    if epi:
        e = dict(shift=epi["shift"], pairs=epi["pairs"])
        if c.nb:
            batch["out"] = out.shape[1]
        for key, name in (("a", "EA"), ("b", "EB")):
            if epi.get(key):
                e[key] = dv[name]
                if epi[key] == "item":
                    batch["e" + key] = P
        if epi.get("d"):
            e["d"] = dv["D"][0]
            if c.nb:
                batch["d"] = dv["D"].shape[1]
        if epi.get("b"):
            out2 = torch.full((k, fu.out2_period(c) + epi["o2pad"]), fu.SENT, dtype=T, device=dev)
            e["out2"] = out2[0]
            if c.nb:
                batch["out2"] = out2.shape[1]
        kw["epi"] = e
    qpart = None
    if qd:
        tiles = nat.hartley_cg_blocks(c.shape, c.axes, T)
        assert tiles == fu.cg_blocks(c) > 0, (c.id, tiles, fu.cg_blocks(c))
        qpart = torch.full((k, qd["blk0"] + tiles + qd["tail"]), fu.SENT, dtype=torch.float64, device=dev)
        kw["quad"] = dict(part=qpart, pstride=qpart.shape[1], blk0=qd["blk0"])
    with nat.LaunchProfile(capacity=16) as prof:
        nat.hartley_fused(out[0], c.axes, c.scale, convention=c.convention, shape=c.shape, batch=batch, **kw)
    torch.cuda.synchronize()
    if labels:
        assert [lab for lab, _ in prof.records] == fu.expected_fused_labels(c), c.id
    got = dict(out=out.cpu().numpy())
    if out2 is not None:
        got["out2"] = out2.cpu().numpy()
    if qpart is not None:
        got["quad"] = qpart.cpu().numpy()
    for name, v in inp.items():
        if name == "X" and dr:
            got["x1"] = dv["X"].cpu().numpy()
            continue
        after = dv[name].cpu().numpy()
        assert after.dtype == v.dtype and np.array_equal(after.view(np.uint8), np.asarray(v).view(np.uint8)), \
            (c.id, name, "input operand changed")
    if dr:
        got["dpart"] = dpart.cpu().numpy()
    return got


def _check(c, got, ref=None):
    ref = fu.ref_fused(c) if ref is None else ref
    ratios = fu.check_case(c, ref, got)
    _note(c, ratios)
    return ref


def _item_is_batch_of_one(c, inp, got, dev, j, keys=("out", "out2", "quad", "x1", "dpart")):
    c1, inp1 = fu.item_case(c, inp, j)
    one = _run(c1, inp1, dev, labels=False)
    for key in keys:
        if key in got:
            assert fu.same(one[key][0], got[key][j]), (c.id, key, "item", j, "differs from a batch of one")


# ------------------------------------------------------------------ a. in-pass prologue, R2C rows
@pytest.mark.parametrize("c", fu.cases_a(), ids=_ids(fu.cases_a()))
def test_a_r2c_prologue(c, dev):
    _check(c, _run(c, fu.fused_inputs(c), dev))


# ------------------------------------------------------------------ b. H1D, prologue + epilogue
@pytest.mark.parametrize("c", fu.cases_b(), ids=_ids(fu.cases_b()))
def test_b_h1d_fused(c, dev):
    _check(c, _run(c, fu.fused_inputs(c), dev))


# ------------------------------------------------------------------ c. strided unpack epilogue
@pytest.mark.parametrize("c", fu.cases_c(), ids=_ids(fu.cases_c()))
def test_c_unpack_epilogue(c, dev):
    inp = fu.fused_inputs(c)
    got = _run(c, inp, dev)
    _check(c, got)
    if c.nb:
        _item_is_batch_of_one(c, inp, got, dev, c.nb - 1)


# ------------------------------------------------------------------ d. pair sums, quad partials
@pytest.mark.parametrize("c", fu.cases_d(), ids=_ids(fu.cases_d()))
def test_d_pairs_quad(c, dev):
    inp = fu.fused_inputs(c)
    got = _run(c, inp, dev)
    _check(c, got)
    if c.spec.get("quad"):
        assert fu.bgroup_applies(c) == c.regime["bgroup"]
        plain = _run(c, inp, dev, quad=False, labels=False)
        assert fu.same(plain["out"], got["out"]), (c.id, "the quad pass's out differs from the plain epilogue's")
    if c.nb > 1:
        _item_is_batch_of_one(c, inp, got, dev, c.nb - 1)


# ------------------------------------------------------------------ e. stand-alone prologue passes
@pytest.mark.parametrize("c", fu.cases_e(), ids=_ids(fu.cases_e()))
def test_e_prologue_passes(c, dev):
    nat = _nat()
    inp = fu.fused_inputs(c)
    assert fu.pro_kernel(c) == c.regime["kernel"]
    if c.regime["kernel"] != "batch":
        g = fu.grid_of(c)
        assert bool(nat.hartley_pro_rows(g)) == (len(g) >= 2 and g[-1] // 2 + 1 <= fu.PRO_ROWS_MAXH)
    got = _run(c, inp, dev)
    _check(c, got)
    if c.spec["pro"]["index"] == "fold":
        pix = _run(c, inp, dev, pixel=True, labels=False)
        assert fu.same(pix["out"], got["out"]), (c.id, "folded gather differs from the per-pixel gather")
    if fu.items_independent(c):
        _item_is_batch_of_one(c, inp, got, dev, c.nb - 1)


# ------------------------------------------------------------------ f. pro_r2c + dir
def _dir_chain(grid):
    """serial chain of a d.d partial (tests/test_cg_carried_kernels_gpu.py)"""
    return 2 ** (len(grid) - 1) * -(-grid[-1] // 64)


@pytest.mark.parametrize("c", fu.cases_f(), ids=_ids(fu.cases_f()))
def test_f_pro_r2c_dir(c, dev, monkeypatch):
    assert (prim.NS, prim.GAMMA, prim.GPREV, prim.DONE, prim.SENT) == (fu.NS, fu.GAMMA, fu.GPREV, fu.DONE, fu.SENT)
    env = c.spec["env"].get("NFT_PRO_R2C")
    if env is None:
        monkeypatch.delenv("NFT_PRO_R2C", raising=False)
    else:
        monkeypatch.setenv("NFT_PRO_R2C", env)
    nat = _nat()
    inp = fu.fused_inputs(c)
    got = _run(c, inp, dev)
    _check(c, got)
    k, P, g, dr = c.nb, fu.period(c), fu.grid_of(c), c.spec["dir"]
    nbd = nat.hartley_dir_blocks(g)
    assert nbd == g[0] // 2 + 1
    lo, hi = dr["blk0"], dr["blk0"] + nbd
    X, R, SC, x1, part = inp["X"], inp["R"], inp["SC"], got["x1"], got["dpart"]
    assert np.all(part[:, :lo] == fu.SENT) and np.all(part[:, hi:] == fu.SENT), "partials outside the block range"
    for j in range(k):
        what = f"{c.id} item {j}"
        prim.check_dir_row(DT[c.dtype], P, X[j], R[j], SC[j], x1[j], what)
        if SC[j, fu.DONE] != 0.0:
            assert np.all(part[j, lo:hi] == 0.0), (what, "DONE item's partials")
        else:
            dd = math.fsum(part[j, lo:hi].tolist())
            prim.assert_reduction(dd, x1[j, :P], x1[j, :P], _dir_chain(g), what + " d.d", scale=fu.DIR_SHIFT)
    _item_is_batch_of_one(c, inp, got, dev, k - 1)
