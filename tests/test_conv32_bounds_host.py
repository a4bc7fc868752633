"""CPU: the rows of tests/_conv32_ref.py run what they claim, their bounds are attainable and restated defects miss them.

1. Routes and forms.  flowse_op_conv_route (a host-only entry: no GPU is touched), asked with the bits the row's entry
   offers, names the row's route and slice count; the claims about the launch -- the halo kernel's N tile, conv_f43_wide,
   tiles per block, walk order, chunks per slice, the flat tiling and fast / generic path, the 1x1 kernel's k-block count,
   the cin4 kernels' Q and pixels per round, the border class -- equal the launchers' arithmetic restated in
   _conv32_ref.form_of.
2. Attainable.  An fp32 torch restatement of every row (direct rows an fp32 conv, F(4,3) rows the transform pipeline in
   fp32, GN rows the gn_quad form) meets both checks -- the sparse rows (above 8M output elements) included: their
   reference is gathers and takes 2 to 5 s; test_sparse_reference_is_the_dense_one holds those gathers to the dense
   convolution and pipeline on a small shape.
3. Sensitive.  Restated defects miss the bounds on the rows that claim to catch them; the bf16 operand misses rel-L2.
"""
import ctypes

import pytest
import torch

import _conv32_ref as R


def ask(r):
    from flowmse_amd import _lib
    buf = ctypes.create_string_buffer(96)
    assert _lib.lib.flowse_op_conv_route(0, 0, r.B, r.H, r.W, r.C1, r.C2, r.Cout, r.k * r.k, R.offer_bits(r), buf, 96) == 0
    return buf.value.decode()


@pytest.mark.parametrize("r", R.ROWS, ids=lambda r: r.name)
def test_row_runs_the_route_and_form_it_claims(r):
    text = ask(r)
    fields = dict(f.split("=") for f in text.split()[1:])
    assert text.split()[0] == r.route, (r.name, text)
    assert int(fields["ks"]) == (r.ks or 1), (r.name, text)
    assert (r.ks > 1) == r.route.endswith("_splitk")
    form = R.form_of(r)
    for claim, value in r.form:
        if claim == "stats":
            assert int(fields["stats"]) > 0, (r.name, text)     # the statistics-writing kernel runs inside the sink
        else:
            assert form[claim] == value, (r.name, claim, form[claim], value)
    M = r.B * r.H * r.W
    if r.route not in ("cin4", "cin4_stats", "flat"):
        assert M > 2048                                          # above the small-image kernels' limit
    # the size rules that keep the worst-case bounds sharp; rows whose subject is the chunk count (the sliced rows, the 32-row
    # tiling on the fast path) are exempt
    if r.route in R.WINO_ROUTES:
        assert r.H % 8 == 0 and (r.C1 + r.C2 <= 128 or r.ks)
    elif r.kind == "conv" and not r.ks and r.name != "flat-smallm-fast":
        assert R.k_of(r) <= 2048
    assert r.kind == "probe" or (r.kind == "sparse") == (M * r.Cout > R.BIG)     # (a probe needs no convolution)
    assert r.gn in R.GN_MODES[r.route] and (not r.sink or "stats" in dict(r.form))
    if r.kind == "probe":
        assert r.Cout == r.k * r.k * (r.C1 + r.C2) and r.route not in R.WINO_ROUTES


@pytest.mark.parametrize("r", R.CONV_ROWS, ids=lambda r: r.name)
def test_fp32_restatement_meets_the_bounds(r):
    if r.gn:
        assert not R.stats_guard(r, None)
    fails, report, _ = R.check(r, R.restate_fp32(r), R.reference(r))
    print(f"{r.name:28s} {r.route:12s} {report}")
    assert not fails, fails


@pytest.mark.parametrize("r", R.PROBE_ROWS, ids=lambda r: r.name)
def test_restated_probe(r):
    """what the probe rows assert of the kernels, asserted of the fp32 staging: the one-hot conv is an exact shift"""
    p = r.k // 2
    a = torch.nn.functional.pad(R.stage_fp32(r, R.gn_data(r), R.inputs(r).x), (p, p, p, p))
    got = torch.cat([a[:, :, t // r.k:t // r.k + r.H, t % r.k:t % r.k + r.W] for t in range(r.k * r.k)], 1)
    fails, report = R.check_probe(r, got)
    print(f"{r.name:28s} {report}")
    assert not fails, fails
    if r.gn:                                                  # padding before the activation leaves act(beta - m s) outside
        b = R.stage_fp32(r, R.gn_data(r), torch.nn.functional.pad(R.inputs(r).x, (p, p, p, p)))
        bad = torch.cat([b[:, :, t // r.k:t // r.k + r.H, t % r.k:t % r.k + r.W] for t in range(r.k * r.k)], 1)
        assert any("out-of-image" in f for f in R.check_probe(r, bad)[0])
    else:                                                     # one ulp anywhere is a failure
        got[0, 1, r.H // 2, r.W // 2] = torch.nextafter(got[0, 1, r.H // 2, r.W // 2], torch.tensor(9.0))
        assert R.check_probe(r, got)[0]


def test_sparse_reference_is_the_dense_one():
    """the gathers of the sparse rows (direct and Wabs) against the dense convolution / pipeline on a small shape"""
    r = R._r("sparse-small", "f43", "f", (2, 16, 32), 32, 64, C2=32, gn=2, kind="sparse")
    i = R.inputs(r)
    a64, tau = R.staged(r, R.gn_data(r))
    w = i.w.double()
    dense = torch.nn.functional.conv2d(a64, w, padding=1)
    assert torch.allclose(R.sparse_direct(a64, i.sparse), dense, rtol=1e-12, atol=1e-12)
    assert torch.allclose(R.sparse_wino(a64.abs(), i.sparse, True), R.wino(a64.abs(), w.abs(), True), rtol=1e-12, atol=1e-12)
    assert torch.allclose(R.sparse_wino(a64, i.sparse), dense, rtol=1e-10, atol=1e-10)
    fails, report, _ = R.check(r, R.restate_fp32(r), R.reference(r))
    assert not fails, fails
    assert R.check(r, R.restate_fp32(r, "tile_shift"), R.reference(r))[0]


def test_wabs_is_what_the_issue_measured():
    """S_w / S on a dense F(4,3) row: the Winograd allowance is a small multiple of the direct one (median well below
    the 4 x 2.25 x 1.x of the three absolute matrices' norms), so the bound still resolves one wrong operand"""
    r = R.BY_NAME["f43-strip-plain"]
    i = R.inputs(r)
    a, w = i.x.double().abs(), i.w.double().abs()
    ratio = R.wino(a, w, True) / torch.nn.functional.conv2d(a, w, padding=1)
    print(f"S_w / S: median {float(ratio.median()):.2f} max {float(ratio.max()):.2f}")
    assert 1.0 <= float(ratio.min()) and float(ratio.median()) < 12 and float(ratio.max()) < 40


SENSITIVE = {
    "pad_before_act": ("halo-3x6-gnsilu", "halo-3x6-gn", "head4-all4-gnsilu", "f43-all4", "f43sk-ks2-4-gn"),
    "drop_last_chunk": ("halo-3x6-plain", "f43sk-ks2-5-plain", "f43sk-ks3-7-gnsilu", "flatsk-1x1", "stream-12kb", "f43-wide-cat-64+32"),
    "second_from_first": ("halo-cat-64+64", "halo-cat-96+32", "f43-wide-cat-32+32", "f43sk-cat-64+64", "flatsk-cat-48+16",
                          "flatsk-1x1-cat", "stream-cat-32+32"),
    "tile_shift": ("halo-bn128-full", "head4-1x128x128", "f43-strip-plain", "f43-rowmajor", "flat-46x46-k3", "stream-ring4",
                   "cin4mfma-all4"),
    "swap_quads": ("halo-bn64-partial", "f43-wide-odd", "f43sk-ks2-4-plain", "flat-cout132", "stream-2x128x128", "cin4-5x7-k3",
                   "cin4stats-4rounds"),
    "bias2_sample0": ("halo-bn32-live4", "halo-all4", "f43-all4", "f43-wide-8x64x128", "f43sk-ks2-5-gn", "flatsk-1x1-cat",
                      "stream-ring4", "cin4-5x7-k1", "cin4stats-q256", "cin4mfma-all4"),
    "slice_twice": ("f43sk-ks2-4-plain", "f43sk-ks3-7-plain", "flatsk-1x1", "flatsk-1x1-cat"),
}


@pytest.mark.parametrize("defect,name", [(d, n) for d, ns in SENSITIVE.items() for n in ns])
def test_restated_defects_miss_the_element_bound(defect, name):
    r = R.BY_NAME[name]
    fails, report, _ = R.check(r, R.restate_fp32(r, defect), R.reference(r))
    print(f"{defect:18s} {name:24s} {report}")
    assert any("bound" in f for f in fails), (defect, name, report)


@pytest.mark.parametrize("name", ("halo-3x6-plain", "f43-strip-plain", "f43sk-ks2-4-gnsilu", "flat-46x46-k3", "stream-12kb",
                                  "head4-4x64x64-96", "cin4mfma-all4"))
def test_bf16_operand_misses_rel_l2(name):
    r = R.BY_NAME[name]
    fails, report, _ = R.check(r, R.restate_fp32(r, "bf16_operand"), R.reference(r))
    print(f"bf16_operand       {name:24s} {report}")
    assert any("rel-L2" in f for f in fails), (name, report)


def test_table_coverage():
    """the table names exactly the fp32 large-image routes and, per route, every GN mode its entry can reach; the forms
    the issue lists are each claimed by a row"""
    assert {r.route for r in R.ROWS} == set(R.ROUTES)
    for route in R.ROUTES:
        assert {r.gn for r in R.ROWS if r.route == route} == set(R.GN_MODES[route]), route
    form = lambda r: dict(r.form)
    has = lambda pred: any(pred(r, form(r)) for r in R.ROWS)
    assert {form(r).get("bn") for r in R.ROWS if r.route == "halo"} >= {32, 64, 128}
    assert {form(r).get("border") for r in R.ROWS if r.route == "halo"} >= {"all4", "strip_lr", "strip_tb", "interior"}
    assert {form(r).get("tpb") for r in R.ROWS if r.route == "f43"} == {1, 2, 4}
    assert has(lambda r, f: f.get("tpb") == 2 and f.get("walk") == "row") and has(lambda r, f: f.get("walk") == "strip")
    assert {f for r in R.ROWS if r.route == "f43_splitk" for f in [form(r).get("slices")]} >= {(2, 2), (3, 2), (3, 3, 1)}
    assert {form(r).get("tiling") for r in R.ROWS if r.route.startswith("flat")} >= {"2222", "2221", "4111", "1411"}
    assert has(lambda r, f: r.route == "flat_splitk" and f.get("fast") is False)
    assert {(f["rounds"] > 1, f["last"]) for r in R.ROWS if r.route == "cin4_stats" for f in [form(r)] if "last" in f} >= \
        {(False, 1), (False, 2), (False, 3), (True, 4)}
    assert has(lambda r, f: r.route == "head4" and r.gn == 1)
    assert has(lambda r, f: r.inplace)
    for route in ("f43_splitk", "flat_splitk", "1x1_stream", "cin4_stats"):
        assert has(lambda r, f: r.route == route and r.sink), route
    for tag in ("halo-epi", "f43-wide-epi", "stream-epi"):
        assert {r.name[len(tag) + 1:] for r in R.ROWS if r.name.startswith(tag)} == {t for t, _ in R.EPI}
    assert {R.BY_NAME[n].route for n in R.REPRO} == {"f43", "f43_splitk", "flat_splitk", "1x1_stream", "cin4_stats"}
