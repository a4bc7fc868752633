"""GPU: the large-image fp32 convolution kernels -- conv3x3_halo_kernel, conv3x3_head4_kernel, conv3x3_f43_kernel (64- and
128-channel blocks, 1 / 2 / 4 tiles per block, both tile walks, K slices), conv_mfma_kernel / conv_mfma_fast_kernel with
their K slices, the two plain reduction kernels, conv1x1_stream_kernel, conv_cin4_kernel, conv_cin4_stats_kernel and
conv3x3_cin4_mfma_kernel -- against float64, per element.  Rows, reference, tau and the bounds: tests/_conv32_ref.py
(tests/test_conv32_bounds_host.py shows on the CPU that every row reaches the route and form it names, that the bounds are
attainable and that restated defects miss them).

Every row goes through a per-op entry, first asserts that the launch ran the kernel the row names
(flowse_op_last_conv_route), then -- rows with fused GroupNorm -- that the (mean, scale) pair the entry staged with agrees
with the float64 statistics of the input, then the element bound on every element and rel-L2 < 2e-5.  A failure names
the worst element as (b, y % TH, x % TW, channel) with the kernel's tile TH x TW.  Rows marked "sink" run inside the
statistics sink, which is the only way to cin4_stats and the statistics-writing reduction kernel; the statistics
themselves are held to float64 in tests/test_gpu_fused_stats.py.  Probe rows (one-hot weights) are compared bit for bit
(within tau of the float64 staging where GroupNorm is fused) and must be exactly 0 at every out-of-image tap.

Out of scope: "w2d" (tests/test_gpu_w2d_epilogue.py), "halo_bf16x3" and splitk_reduce_gn_kernel (reachable only through a
model handle), "smallm" (tests/test_gpu_smallm.py).

Recorded on an MI355X (worst over the rows of a route; recorded, not asserted -- nothing here is fitted to them):
    route         rows  max|d|/bound  rel-L2    seconds (sum over the rows; slowest row)
    halo            23      1.15e-02  6.00e-07     2.1   0.4 (halo-bn128-full)
    head4            9      5.59e-03  3.59e-07     0.3   0.1 (head4-4x64x64-128)
    f43             22      7.64e-03  6.05e-07    20.4   2.9 (f43-tpb4-gnsilu)
    f43_splitk      13      7.53e-04  8.02e-07     0.2   < 0.05 each
    flat             9      4.22e-02  6.65e-07     0.1   < 0.05 each
    flat_splitk     11      5.52e-03  3.60e-07     0.2   0.1 (flatsk-64x64)
    1x1_stream      10      6.69e-02  1.54e-07     2.5   0.3 (stream-cat-32+32)
    cin4             3      7.68e-02  9.20e-08     0.1   < 0.05 each
    cin4_stats       7      9.99e-02  5.56e-08     0.1   < 0.05 each
    cin4_mfma        3      5.27e-02  1.02e-07     0.4   0.1 (cin4mfma-2x128x128)
  row times (wall, the launch with its copies, the float64 reference and the comparison): halo-bn32-plain 0.3, halo-bn128-last32 0.3,
  halo-bn128-full 0.4, f43-wide-odd 0.5, f43-wide-8x64x128 0.4, f43-wide-cat-32+32 0.5, f43-wide-cat-64+32 0.6,
  f43-wide-epi-* 0.3 to 0.4, stream-* 0.2 to 0.3, halo-probe-* 0.1 to 0.3 s, every other dense row <= 0.1 s; the
  sparse rows f43-tpb2-* 1.2 / 1.6 / 1.7 s, f43-tpb2row-* 1.2 / 1.5 / 1.5 s, f43-tpb4-* 2.4 / 2.9 / 2.8 s (plain / gnsilu /
  cat-gn; the 67M-element output's copies and the gathers dominate); the module 28 s.
  probe rows: halo, flat and 1x1_stream bit-exact without GN and exactly 0 at every out-of-image tap; halo with GroupNorm
  max |d| / tau 0.47, with GroupNorm + SiLU 0.21.
  (the F(4,3) figures against the wider S_w: the fp32 restatement on the CPU gives 3e-3 there, the kernel 4e-3 to 8e-3)
No row failed: no kernel was changed.
"""
import time

import pytest
import torch

import _conv32_ref as R

pytestmark = pytest.mark.gpu

_seen = {}                                   # row name -> (route, max |d| / bound or None, rel-L2 or None, seconds)


@pytest.fixture(scope="module")
def G():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    import _gpu
    return _gpu


def run_row(G, r):
    """-> (output NCHW cpu, route of the launch, (mean, scale) the entry staged with or None)"""
    i = R.inputs(r)
    x1 = i.x[:, :r.C1].contiguous()
    x2 = i.x[:, r.C1:].contiguous() if r.C2 else None
    staged = []

    def launch():
        if r.entry in ("c", "cs"):
            return G.conv2d(x1, i.w, i.bias, x2, i.bias2, i.res, r.scale, splitk=r.entry == "cs", res_in_place=r.inplace)
        if r.entry == "g":
            return G.conv3x3_gn(x1, i.gamma, i.beta, i.w, i.bias, x2, i.bias2, i.res, r.scale, silu=r.gn == 2, staged=staged)
        return G.conv3x3_f43(x1, i.w, i.gamma if r.gn else None, i.beta if r.gn else None, i.bias, x2, i.bias2, i.res,
                             r.scale, silu=r.gn == 2, staged=staged)
    if r.sink:
        with G.stats_sink(2 * r.B * r.Cout * max(1, r.H * r.W // 8)) as sink:
            got = launch()
        assert sink.blocks > 0, f"{r.name}: the launch wrote no statistics"
    else:
        got = launch()
    route = G.last_route()
    assert route == r.route, f"{r.name}: ran {route!r}, the row is written for {r.route!r}"
    assert bool(staged) == bool(r.gn)
    return got, route, tuple(staged) if staged else None


@pytest.mark.parametrize("r", R.CONV_ROWS, ids=lambda r: r.name)
def test_conv32_against_float64(G, r):
    t0 = time.time()
    got, route, stats = run_row(G, r)
    if r.gn:
        assert not R.stats_guard(r, stats), R.stats_guard(r, stats)
    fails, report, (ratio, rel) = R.check(r, got, R.reference(r, stats))
    dt = time.time() - t0
    _seen[r.name] = (route, ratio, rel, dt)
    print(f"{r.name:24s} route {route:12s} gn {r.gn}  {report}  {dt:5.1f} s")
    assert not fails, fails


@pytest.mark.parametrize("r", R.PROBE_ROWS, ids=lambda r: r.name)
def test_probe_is_exact(G, r):
    t0 = time.time()
    got, route, stats = run_row(G, r)
    if r.gn:
        assert not R.stats_guard(r, stats), R.stats_guard(r, stats)
    fails, report = R.check_probe(r, got, stats)
    dt = time.time() - t0
    _seen[r.name] = (route, None, None, dt)
    print(f"{r.name:24s} route {route:12s} gn {r.gn}  {report}  {dt:5.1f} s")
    assert not fails, fails


@pytest.mark.parametrize("name", R.REPRO)
def test_conv32_is_bit_reproducible(G, name):
    """f43 with two tiles per block, f43 over three K slices, flat over nine, the streaming 1x1, cin4_stats: two launches
    agree bit for bit"""
    r = R.BY_NAME[name]
    a, _, _ = run_row(G, r)
    b, _, _ = run_row(G, r)
    assert torch.equal(a, b), name


def test_route_coverage():
    """the table names exactly the fp32 large-image routes and, per route, every GN mode its entry can reach; every row that
    ran in this session ran the route it names (each row asserts its own above).  Prints the per-route figures."""
    assert {r.route for r in R.ROWS} == set(R.ROUTES)
    for route in R.ROUTES:
        assert {r.gn for r in R.ROWS if r.route == route} == set(R.GN_MODES[route]), route
    for name, (route, _, _, _) in _seen.items():
        assert route == R.BY_NAME[name].route, name
    print("    route         rows  max|d|/bound  rel-L2    seconds (sum, slowest row)")
    for route in R.ROUTES:
        rows = [(n, v) for n, v in _seen.items() if v[0] == route]
        if rows:
            figs = [v for _, v in rows if v[1] is not None]
            slow = max(rows, key=lambda nv: nv[1][3])
            print(f"    {route:12s} {len(rows):5d}  {max(v[1] for v in figs):12.2e}  {max(v[2] for v in figs):.2e}  "
                  f"{sum(v[3] for _, v in rows):6.1f}  {slow[1][3]:5.1f} ({slow[0]})")
