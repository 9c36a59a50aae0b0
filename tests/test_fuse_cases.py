"""Host checks of tests/fuse_cases.py: the extended-precision reference of the
fused transform agrees with an independent float64 composition (scipy.fft,
explicit loops for the mirror cell and the pair sums), the bound is positive
and the correctly rounded reference stays below a quarter of it on every
case, every case is in the regime its group names, the tables are complete,
and the check every group's device outputs go through rejects each of the
defects it is there to find."""
import numpy as np
import pytest

import fft_cases as fc
import fuse_cases as fu

CASES = fu.all_cases()
SMALL = [c for c in CASES if np.prod(c.shape) <= 1 << 14 and c.dtype == "f64"]


def _ids(cases):
    return [c.id for c in cases]


# ------------------------------------------------------------------ the reference against a plain composition
def _plain(c, inp):
    """float64, element by element where the semantics are index arithmetic"""
    import scipy.fft
    k, P, g, iax = fu.items_of(c), fu.period(c), fu.grid_of(c), fu.item_axes(c)
    pro, epi, dr = c.spec.get("pro"), c.spec.get("epi") or {}, c.spec.get("dir")
    res = dict(out=np.zeros((k, P)))
    for i in range(k):
        x = inp["X"][i, :P].astype(np.float64)
        if dr and inp["SC"][i, fu.DONE] == 0.0:
            beta = max(0.0, inp["SC"][i, fu.GAMMA] / inp["SC"][i, fu.GPREV])
            x = beta * x + inp["R"][i, :P]
        u = x.copy()
        if pro and pro.get("a"):
            u = u * (inp["A"][i] if pro["a"] == "item" else inp["A"])
        if pro and pro.get("b"):
            bv = inp["B"][i] if pro["b"] == "item" else inp["B"]
            half = [n // 2 + 1 for n in g]
            for j in range(P):
                if pro["index"] == "fold":
                    cell = 0
                    for a, kk in enumerate(np.unravel_index(j, g)):
                        cell = cell * half[a] + min(int(kk), g[a] - int(kk))
                    b = int(inp["fidx"][cell])
                else:
                    b = int(inp["pidx"][j])
                lay = pro["c"]
                cv = inp["C"][b, i] if lay == "inter" else inp["C"][i, b] if lay == "item" else inp["C"][b]
                u[j] += bv[j] * cv
        f = scipy.fft.fftn(u.reshape(g), axes=iax)
        h = c.scale * (f.real + f.imag if c.convention == 0 else f.real - f.imag).reshape(-1)
        o = h.copy()
        if epi.get("a"):
            o = o * (inp["EA"][i] if epi["a"] == "item" else inp["EA"])
        if epi.get("d"):
            o = o + epi["shift"] * inp["D"][i, :P]
        res["out"][i] = o
        if epi.get("b"):
            t = (h * (inp["EB"][i] if epi["b"] == "item" else inp["EB"])).reshape(g)
            if epi.get("pairs"):
                n, nh = g[-1], g[-1] // 2 + 1
                pr = np.zeros(g[:-1] + (nh,))
                for co in np.ndindex(*pr.shape):
                    mi = tuple((-q) % m for q, m in zip(co, g))
                    pr[co] = t[co] if co[-1] in (0, n // 2) else t[co] + t[mi]
                t = pr
            res.setdefault("out2", np.zeros((k, t.size)))[i] = t.reshape(-1)
        if c.spec.get("quad"):
            res.setdefault("quad", np.zeros(k))[i] = float(np.sum(h * o))
    return res


@pytest.mark.parametrize("c", SMALL, ids=_ids(SMALL))
def test_ref_against_plain_composition(c):
    inp = fu.fused_inputs(c)
    ref, plain = fu.ref_fused(c), _plain(c, inp)
    for key, v in plain.items():
        r = np.asarray(ref[key], np.float64)
        assert r.shape == v.shape, (key, r.shape, v.shape)
        assert np.linalg.norm(r - v) <= 1e-12 * max(np.linalg.norm(v), 1e-300), key
    if (c.spec.get("pro") or {}).get("index") == "fold":
        assert np.array_equal(inp["fidx"][fu.cell_index(fu.grid_of(c)).reshape(-1)], inp["pidx"])


def test_small_cases_cover_every_group():
    assert {c.group for c in SMALL} == set(fu.GROUPS)
    assert any((c.spec.get("epi") or {}).get("pairs") for c in SMALL)
    assert any(c.spec.get("quad") for c in SMALL) and any(c.spec.get("dir") for c in SMALL)
    assert any(len(fu.grid_of(c)) == 3 and (c.spec.get("pro") or {}).get("index") == "fold" for c in SMALL)


# ------------------------------------------------------------------ bound and condition of the inputs
@pytest.mark.parametrize("c", CASES, ids=_ids(CASES))
def test_bound_positive_and_reference_well_inside(c):
    ref = fu.ref_fused(c)
    b = fu.fused_bound(c, ref)
    for key, v in b.items():
        assert v.shape == (fu.items_of(c),) and np.all(v > 0) and np.all(np.isfinite(v)), key
    ratios = fu.check_case(c, ref, fu.cast_ref(c, ref))
    assert set(ratios) == {"out"} | ({"out2"} if "out2" in ref else set()) | ({"quad"} if "quad" in ref else set())
    assert max(ratios.values()) <= 0.25, ratios


# ------------------------------------------------------------------ regimes
def test_ids_unique():
    assert len({c.id for c in CASES}) == len(CASES)
    assert all(np.prod(fu.grid_of(c)) <= 1 << 18 for c in CASES if c.nb)
    assert all(np.prod(c.shape) <= 1 << 20 for c in CASES)


@pytest.mark.parametrize("c", fu.cases_a(), ids=_ids(fu.cases_a()))
def test_regime_a(c):
    r = c.regime
    assert fu.expected_fused_labels(c) == ["fft_r2c+pro", "fft_unpack"] and not c.nb
    assert fu.pro_kernel(c) is None and c.spec["pro"]["index"] == "pixel"
    assert c.shape[-1] == r["rows_n"] and r["pair_lines"] == int(np.prod(c.shape[:-1])) // 2
    if r.get("partial"):
        assert r["pair_lines"] > r["tile"] and r["pair_lines"] % r["tile"] != 0 and len(c.shape) == 3


@pytest.mark.parametrize("c", fu.cases_b(), ids=_ids(fu.cases_b()))
def test_regime_b(c):
    r = c.regime
    assert fu.expected_fused_labels(c) == ["fft_h1d+fused"]
    assert c.spec["pro"]["b"] and c.spec["epi"]["a"] and c.spec["epi"]["b"] and c.spec["epi"]["d"]
    assert r["real_rows"] % 2 == 1 and r["pair_lines"] == r["tile"] + 2
    # more than one tile, the last one partial (tiles of two pair lines: whole, ending in the single row)
    assert (r["pair_lines"] % r["tile"] != 0) == (r["tile"] > 2)


@pytest.mark.parametrize("c", fu.cases_c(), ids=_ids(fu.cases_c()))
def test_regime_c(c):
    r = c.regime
    n0 = fu.grid_of(c)[0]
    mid = ["fft_c2c"] if n0 in fc.FOURSTEP_N else []
    assert fu.expected_fused_labels(c) == ["fft_r2c"] + mid + ["fft_unpack+epi"]
    assert r["first_n"] == n0 and r["partial"] and fu.grid_of(c)[-1] in (8, 16)
    if r.get("batched"):
        e = c.spec["epi"]
        assert c.nb == 3 and e["opad"] and e["dpad"] and e["o2pad"] and fu.cg_blocks(c) == r["tiles"]


@pytest.mark.parametrize("c", fu.cases_d(), ids=_ids(fu.cases_d()))
def test_regime_d(c):
    labels = fu.expected_fused_labels(c)
    if c.regime["kind"] == "quad":
        assert labels[-1] == "fft_unpack+quad" and fu.cg_blocks(c) > 0
        assert fu.bgroup_applies(c) == c.regime["bgroup"]
    else:
        assert labels[-1] == "fft_unpack+epi" and c.spec["epi"]["pairs"] and not fu.bgroup_applies(c)
    assert labels[0] == "fft_r2c" and labels[1:-1] == ["fft_c2c"] * (len(labels) - 2)


def test_group_d_both_sides_of_the_regrouping():
    quad = [c for c in fu.cases_d() if c.regime["kind"] == "quad" and c.dtype == "f64"]
    assert sum(fu.bgroup_applies(c) for c in quad) >= 2
    assert sum(not fu.bgroup_applies(c) and c.nb > 1 for c in quad) >= 2
    assert {c.nb for c in quad} == {1, 2, 3, 8}
    assert {fu.grid_of(c)[0] in fc.FOURSTEP_N for c in fu.cases_d()} == {True, False}
    # a shared weight whose tile count is a multiple of 8, and the same geometry with per-item weights
    assert any(fu.cg_blocks(c) % 8 == 0 and not fu.bgroup_applies(c) and c.nb > 1 for c in quad)


@pytest.mark.parametrize("c", fu.cases_e(), ids=_ids(fu.cases_e()))
def test_regime_e(c):
    r = c.regime
    labels = fu.expected_fused_labels(c)
    assert fu.pro_kernel(c) == r["kernel"] and fu.nbm_class(c.nb) == r["NBM"] and fu.per_item_ab(c) == r["PI"]
    assert labels[0] == ("pro_batch" if r["kernel"] == "batch" else "pro_fold")
    assert labels[1:] == fc.expected_labels(c.shape, c.axes)
    assert c.spec["pro"]["xpad"] == 64
    g = fu.grid_of(c)
    if r["kernel"] == "rows":
        assert len(g) >= 2 and c.nb <= 8
    if r["kernel"] == "fold":
        assert len(g) == 1 or c.nb > 8 or g[-1] // 2 + 1 > fu.PRO_ROWS_MAXH
    assert fu.vector_gather(c) == (c.spec["pro"]["c"] == "inter" and c.nb % 2 == 0 and
                                   (c.nb <= 8 or r["kernel"] == "batch"))


@pytest.mark.parametrize("c", fu.cases_f(), ids=_ids(fu.cases_f()))
def test_regime_f(c):
    n0, n1 = fu.grid_of(c)
    assert fu.expected_fused_labels(c) == ["pro_r2c+dir", "fft_unpack"]
    assert (c.spec["env"].get("NFT_PRO_R2C") == "2") == (n1 > 1024)
    # without the switch the long rows take the row-staged prologue
    off = c._replace(spec=dict(c.spec, env={}))
    assert (fu.pro_kernel(off) == "r2c") == (n1 <= 1024)


# ------------------------------------------------------------------ completeness
def test_tables_complete():
    assert sorted({c.regime["rows_n"] for c in fu.cases_a()}) == list(fc.ROWS_N)
    for ops in fu.PRO_SETS:
        assert sorted(c.shape[-1] for c in fu.cases_a() if f"-{ops}-f32" in c.id) == list(fc.ROWS_N)
    assert sorted({c.regime["rows_n"] for c in fu.cases_b()}) == list(fc.ROWS_N)
    for ops in fu.EPI_SETS:
        firsts = sorted(c.regime["first_n"] for c in fu.cases_c() if f"-{ops}-f64" in c.id)
        assert firsts == list(fc.STRIDED_N + fc.FOURSTEP_N)
    for g in fu.GROUPS.values():
        cs = g()
        assert sorted(c.id[:-3] for c in cs if c.dtype == "f64") == sorted(c.id[:-3] for c in cs if c.dtype == "f32")


def test_group_e_reaches_every_prologue_instantiation():
    for dt in fu.DTYPES:
        have = {(c.regime["kernel"], c.regime["D"], c.regime["NBM"], c.regime["PI"])
                for c in fu.cases_e() if c.dtype == dt and c.regime["kernel"] != "batch"}
        assert have == fu.pro_instantiations()
    e = fu.cases_e()
    batch = [c for c in e if c.regime["kernel"] == "batch"]
    assert {(c.nb % 2, c.spec["pro"]["c"]) for c in batch} == {(0, "inter"), (1, "inter"), (0, "item"), (1, "item")}
    assert {fu.vector_gather(c) for c in batch} == {True, False}
    rows = [c for c in e if c.regime["kernel"] == "rows"]
    assert {(len(fu.grid_of(c)), c.nb, c.regime["PI"]) for c in rows} == \
        {(D, nb, pi) for D in (2, 3) for nb in (1, 2, 3, 4, 5, 8) for pi in (False, True)}
    fold = [c for c in e if c.regime["kernel"] == "fold"]
    assert {(len(fu.grid_of(c)), c.nb) for c in fold if c.nb > 8} >= {(D, nb) for D in (2, 3) for nb in (9, 11)}
    assert any(c.regime["PI"] and c.nb > 8 for c in fold)
    assert {any(n % 2 for n in fu.grid_of(c)) for c in rows} == {True, False}
    assert {fc.expected_labels(c.shape, c.axes) == [] for c in e} == {True, False}


def test_group_f_table():
    f = fu.cases_f()
    assert {fu.grid_of(c)[1] for c in f} == {512, 1024, 2048, 4096}
    assert {fu.grid_of(c)[0] for c in f} == {16, 32} and {c.nb for c in f} == {1, 3, 8}
    assert any(c.spec["dir"]["done"] is not None and c.spec["dir"]["neg"] is not None for c in f)
    c = next(c for c in f if c.spec["dir"]["neg"] is not None)
    inp = fu.fused_inputs(c)
    assert fu.beta_of(inp["SC"][c.spec["dir"]["neg"]]) == 0 and inp["SC"][c.spec["dir"]["done"], fu.DONE] != 0
    ref = fu.ref_fused(c)
    P = fu.period(c)
    assert np.array_equal(ref["x1"][c.spec["dir"]["neg"]], inp["R"][c.spec["dir"]["neg"], :P].astype(fu.LD))
    assert np.array_equal(ref["x1"][c.spec["dir"]["done"]], inp["X"][c.spec["dir"]["done"], :P].astype(fu.LD))


def test_cg_blocks_restatement():
    """tile counts of nft_hartley_cg_blocks, by hand"""
    mk = lambda shape: fu.FCase("t", "d", "f64", shape, tuple(range(1, len(shape))), shape[0], 1.0, 0, {}, {})
    assert fu.cg_blocks(mk((4, 64, 64))) == 2            # 40 lines, 32 per tile
    assert fu.cg_blocks(mk((4, 512, 1024))) == 33        # 520 lines, 16 per tile
    assert fu.cg_blocks(mk((2, 1024, 8))) == 32          # four-step 32 x 32: 32 x ceil(8 / 64)
    assert fu.cg_blocks(mk((2, 2048, 2048))) == 64 * 17  # four-step 64 x 32: 1032 lines, 64 per tile
    assert fu.cg_blocks(mk((3, 64, 64, 8))) == 16
    assert fu.cg_blocks(mk((3, 15, 20))) == 0


# ------------------------------------------------------------------ sensitivity
SENSITIVE = {
    "a": ["a-r2c64-axbc-f64", "a-r2c256-3d-tail-f32"],
    "b": ["b-h1d64-f64", "b-h1d8-f32"],
    "c": ["c-unpack64x8-batch3-shared-f64", "c-unpack1024x8-batch3-item-f32"],
    "d": ["d-pairs-8x64x16-f64", "d-pairs-64x64-f32", "d-quad-2x1024x8-f64", "d-quad-3x16x16x16-f32"],
    "e": ["e-rows-15x20-nb3-shared-item-f64", "e-foldnb-8x8x8-nb9-item-inter-f32",
          "e-batch-32x32-nb2-shared-inter-f64"],
    "f": ["f-pror2c-3x16x1024-f64", "f-pror2c-8x32x512-f32"],
}


@pytest.mark.parametrize("cid", [i for v in SENSITIVE.values() for i in v])
def test_check_rejects_defects(cid):
    c = next(c for c in CASES if c.id == cid)
    ref = fu.ref_fused(c)
    fu.check_case(c, ref, fu.cast_ref(c, ref))          # the unperturbed reference passes
    tried = []
    for name in fu.DEFECTS:
        got = fu.apply_defect(c, ref, name)
        if got is None:
            continue
        tried.append(name)
        with pytest.raises(AssertionError):
            fu.check_case(c, ref, got)
    assert "mirror_bin" in tried and "tail_row" in tried


def test_every_defect_is_tried_in_its_group():
    by_id = {c.id: c for c in CASES}
    assert set(SENSITIVE) == set(fu.GROUPS)
    seen = set()
    for g, ids in SENSITIVE.items():
        for cid in ids:
            c = by_id[cid]
            assert c.group == g
            for name in fu.DEFECTS:
                if name in ("swap_items",) and fu.items_of(c) < 2:
                    continue
                if name == "nyquist_twice" and not (c.spec.get("epi") or {}).get("pairs"):
                    continue
                if name == "quad_slot" and not c.spec.get("quad"):
                    continue
                seen.add((g, name))
    assert {n for _, n in seen} == set(fu.DEFECTS)
    for g in "cdef":
        assert (g, "swap_items") in seen
    assert ("d", "nyquist_twice") in seen and ("d", "quad_slot") in seen
