"""GPU: view handles on one set of weights and the multi-lane sampler call (flowse_model_view_create,
flowse_rk_sample_multi, NCSNpp.rk_sample_multi, get_white_box_solver_multi, evaluate --streams).

The claim under test is bit-identity: an item sampled on a lane, next to other lanes' work, equals the same item sampled
alone.  "Sequential" always means ``rk_sample`` on the parent handle, one item after the other, in this process.  No test
asserts a time.
"""
import ctypes as CT
import filecmp
import os
import subprocess
import sys

import pytest
import torch

import _cases as C
from flowmse_amd import _lib
from flowmse_amd.util import synth

pytestmark = pytest.mark.gpu
TIGHT = 1e-4        # as tests/test_gpu_model.py: what the fp32 MFMA path is expected to reach
L = _lib.lib
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_STATE = 3


def _model(cfg, seed=0):
    from flowmse_amd.model import VFModel
    m = VFModel(backbone="ncsnpp", ode="flowmatching", **cfg)
    m.dnn.load_state_dict({n: torch.from_numpy(synth.synth_param(n, tuple(p.shape), seed))
                           for n, p in m.dnn.named_parameters()})
    return m.cuda().eval()


@pytest.fixture(scope="module")
def tiny():
    assert torch.cuda.is_available()
    return _model(C.TINY)


@pytest.fixture(scope="module")
def full():
    return _model(C.FULL)


def _grid(N, T_rev=1.0, t_eps=0.03):
    from flowmse_amd.sampling import time_grid
    ts, dts = time_grid(T_rev, t_eps, N)
    return ts.tolist(), dts.tolist()


def _items(model, shapes, F, seed0=40):
    """[(x0, y, z)] on the device: y a synthetic spectrogram, x0 the prior sample for the explicit noise z."""
    out = []
    for i, (B, T) in enumerate(shapes):
        y = C.c64(synth.synth_spectrogram(seed0 + i, B, F, T)).cuda()
        z = C.c64(synth.synth_noise(seed0 + i, B, F, T)).cuda()
        out.append((model.ode.prior_sampling(y.shape, y, z)[0].contiguous(), y, z))
    return out


def _sequential(model, items, ts, dts, tableau="euler"):
    return [model.dnn.rk_sample(x0.clone(), y, ts, dts, tableau).clone() for x0, y, _ in items]


def _multi(model, items, ts, dts, tableau="euler", lanes=2, lane_of=None):
    xs = [x0.clone() for x0, _, _ in items]
    model.dnn.rk_sample_multi(xs, [y for _, y, _ in items], ts, dts, tableau, lanes=lanes, lane_of=lane_of)
    torch.cuda.synchronize()
    return xs


def _assert_equal(got, want, what):
    assert len(got) == len(want)
    for i, (a, b) in enumerate(zip(got, want)):
        assert a.shape == b.shape and torch.isfinite(torch.view_as_real(b)).all()
        assert torch.equal(a, b), f"{what}: item {i} differs from the sequential result"


# ---------------------------------------------------------------------------------------------------- 1
def test_tiny_three_lanes_equal_sequential_and_oracle(tiny):
    from oracle import ncsnpp_oracle as O
    from oracle import sampler_oracle as S
    ts, dts = _grid(5)
    items = _items(tiny, [(1, 64), (1, 128), (1, 192)], 64)
    want = _sequential(tiny, items, ts, dts)
    got = _multi(tiny, items, ts, dts, lanes=3)
    _assert_equal(got, want, "tiny, three lanes")
    t = C.param_tables()["tiny"]
    w = C.synth_weights(t["names"], t["shapes"])
    cfg = O.make_cfg(**C.TINY)
    for (x0, y, z), g in zip(items, got):
        ref, _ = S.euler_sample_net(w, cfg, y.cpu(), z.cpu(), N=5)
        err = C.rel_l2(g.cpu(), ref)
        print(f"tiny multi T={y.shape[-1]} rel-L2 vs oracle {err:.3e}")
        assert err < 5 * TIGHT          # the bound of test_tiny_sampler_golden


# ---------------------------------------------------------------------------------------------------- 2
@pytest.mark.parametrize("lanes", [2, 3, 4])
def test_full_mixed_lengths_equal_sequential(full, lanes):
    ts, dts = _grid(5)
    items = _items(full, [(1, 64), (1, 128), (1, 256), (1, 320)], 256)
    want = _sequential(full, items, ts, dts)
    _assert_equal(_multi(full, items, ts, dts, lanes=lanes), want, f"full net, {lanes} lanes")


def test_full_mixed_batch_sizes_equal_sequential(full):
    ts, dts = _grid(5)
    items = _items(full, [(2, 128), (1, 64)], 256, seed0=60)
    want = _sequential(full, items, ts, dts)
    _assert_equal(_multi(full, items, ts, dts, lanes=2), want, "full net, B = 2 beside B = 1")


# ---------------------------------------------------------------------------------------------------- 3
def test_five_items_two_lanes_planned_and_repeatable():
    """Lanes hold 2-3 items of different T: the lane's workspace, time table and scratch are sized up front.  A fresh
    model, so that the views start without any buffer."""
    from flowmse_amd.parallel import batch_cost, plan_lanes
    m = _model(C.TINY)
    ts, dts = _grid(5)
    shapes = [(1, 64), (1, 256), (1, 128), (2, 64), (1, 192)]
    items = _items(m, shapes, 64, seed0=70)
    lane_of, order = plan_lanes([batch_cost(T, B) for B, T in shapes], 2)
    assert sorted(len(o) for o in order) == [2, 3]
    first = _multi(m, items, ts, dts, lanes=2, lane_of=lane_of)       # before any sequential call: nothing is reserved yet
    want = _sequential(m, items, ts, dts)
    _assert_equal(first, want, "five items on two lanes")
    _assert_equal(_multi(m, items, ts, dts, lanes=2, lane_of=lane_of), first, "second identical call")


# ---------------------------------------------------------------------------------------------------- 4
@pytest.mark.parametrize("tableau,N", [("heun", 3), ("rk4", 2)])
def test_tiny_higher_order_equal_sequential(tiny, tableau, N):
    ts, dts = _grid(N)
    items = _items(tiny, [(1, 64), (2, 128), (1, 192)], 64, seed0=80)
    want = _sequential(tiny, items, ts, dts, tableau)
    _assert_equal(_multi(tiny, items, ts, dts, tableau, lanes=2), want, tableau)


@pytest.mark.parametrize("precision", ["fp16", "bf16"])
def test_full_16bit_modes_equal_sequential(precision):
    m = _model(C.FULL)
    m.dnn.set_precision(precision)
    ts, dts = _grid(5)
    items = _items(m, [(1, 64), (1, 128)], 256, seed0=90)
    want = _sequential(m, items, ts, dts)
    _assert_equal(_multi(m, items, ts, dts, lanes=2), want, precision)


# ---------------------------------------------------------------------------------------------------- 5
@pytest.mark.parametrize("side_stream", [True, False])
def test_exit_fence_orders_the_callers_stream(tiny, side_stream):
    """A copy enqueued on the caller's stream straight after the call, then ONE synchronise: the copy must see every
    lane's result."""
    ts, dts = _grid(5)
    items = _items(tiny, [(1, 192), (1, 64), (1, 128)], 64, seed0=100)
    want = _sequential(tiny, items, ts, dts)
    torch.cuda.synchronize()
    s = torch.cuda.Stream() if side_stream else torch.cuda.default_stream()
    xs = [x0.clone() for x0, _, _ in items]
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        tiny.dnn.rk_sample_multi(xs, [y for _, y, _ in items], ts, dts, "euler", lanes=3)
        outs = [x.clone() for x in xs]
    s.synchronize()
    _assert_equal(outs, want, "copy on the caller's stream after the call")


# ---------------------------------------------------------------------------------------------------- 6, 8
def _raw_handle(cfg, blob):
    from flowmse_amd.backbones.structure import create_handle
    h = create_handle(cfg)
    _lib.check(L.flowse_model_load_weights(h, CT.c_void_p(blob.data_ptr()), blob.numel()))
    return h


def _view(parent):
    v = CT.c_void_p()
    _lib.check(L.flowse_model_view_create(parent, CT.byref(v)))
    return v


def _raw_sample(h, x0, y, ts, dts):
    x = x0.clone()
    N = len(ts)
    B, _, F, T = x.shape
    _lib.check(L.flowse_rk_sample(h, _lib.ptr(x), _lib.ptr(y), (CT.c_float * N)(*ts), (CT.c_float * N)(*dts), N, 0, B, F, T,
                                  _lib.current_stream()))
    torch.cuda.synchronize()
    return x


def test_lifetime_of_a_shared_weight_set(tiny):
    blob = tiny.dnn.canonical_blob().contiguous()
    ts, dts = _grid(3)
    (x0, y, _), = _items(tiny, [(1, 128)], 64, seed0=110)
    parent = _raw_handle(C.TINY, blob)
    v1, v2 = _view(parent), _view(parent)
    try:
        before = _raw_sample(parent, x0, y, ts, dts)
        assert torch.equal(_raw_sample(v1, x0, y, ts, dts), before)
        # the weight set has three holders: it can be neither repacked nor switched to another precision
        assert L.flowse_model_load_weights(parent, CT.c_void_p(blob.data_ptr()), blob.numel()) == ERR_STATE
        assert "destroy the views first" in L.flowse_last_error().decode()
        assert L.flowse_model_load_weights(v1, CT.c_void_p(blob.data_ptr()), blob.numel()) == ERR_STATE
        assert L.flowse_model_set_precision(parent, 3) == ERR_STATE
        assert "destroy the views first" in L.flowse_last_error().decode()
        assert L.flowse_model_set_precision(v2, 3) == ERR_STATE
        assert L.flowse_model_set_precision(parent, 0) == 0                 # not a change
        assert torch.equal(_raw_sample(parent, x0, y, ts, dts), before)
        assert torch.equal(_raw_sample(v2, x0, y, ts, dts), before)
        L.flowse_model_destroy(parent)
        parent = None
        assert L.flowse_model_weight_holders(v1) == 2
        assert torch.equal(_raw_sample(v1, x0, y, ts, dts), before)
        assert torch.equal(_raw_sample(v2, x0, y, ts, dts), before)
    finally:
        for h in (v1, v2, parent):
            if h:
                L.flowse_model_destroy(h)


def test_views_share_weight_memory(full):
    blob = full.dnn.canonical_blob().contiguous()
    parent = _raw_handle(C.FULL, blob)
    views = []
    try:
        assert L.flowse_model_weight_holders(parent) == 1
        wbytes = L.flowse_model_device_bytes(parent, _lib.FLOWSE_BYTES_WEIGHTS)
        assert wbytes >= 4 * blob.numel()
        torch.cuda.synchronize()
        free0 = torch.cuda.mem_get_info()[0]
        views.append(_view(parent))
        free1 = torch.cuda.mem_get_info()[0]
        print(f"weight set {wbytes / 2**20:.1f} MiB; device memory taken by one view: {free0 - free1} bytes")
        assert abs(free0 - free1) < 0.01 * wbytes
        views.append(_view(parent))
        for h in [parent] + views:
            assert L.flowse_model_weight_holders(h) == 3
            assert L.flowse_model_device_bytes(h, _lib.FLOWSE_BYTES_WEIGHTS) == wbytes
        for v in views:
            assert 0 < L.flowse_model_device_bytes(v, _lib.FLOWSE_BYTES_OWNED) <= 4096       # its CallBlock, nothing else
        L.flowse_model_destroy(parent)
        parent = None
        for v in views:
            assert L.flowse_model_weight_holders(v) == 2
            assert L.flowse_model_device_bytes(v, _lib.FLOWSE_BYTES_WEIGHTS) == wbytes
    finally:
        for h in views + [parent]:
            if h:
                L.flowse_model_destroy(h)


# ---------------------------------------------------------------------------------------------------- 7
def test_facade_drops_views_when_weights_change():
    m = _model(C.TINY)
    ts, dts = _grid(5)
    items = _items(m, [(1, 64), (1, 128), (1, 192)], 64, seed0=120)
    first = _multi(m, items, ts, dts, lanes=3)
    assert len(m.dnn._views) == 2
    m.dnn.load_state_dict({n: torch.from_numpy(synth.synth_param(n, tuple(p.shape), 1))
                           for n, p in m.dnn.named_parameters()})
    assert m.dnn._views == []
    second = _multi(m, items, ts, dts, lanes=3)
    _assert_equal(second, _sequential(m, items, ts, dts), "after load_state_dict")
    assert all(not torch.equal(a, b) for a, b in zip(first, second))
    m.dnn.set_precision("bf16x3")
    assert m.dnn._views == []
    _assert_equal(_multi(m, items, ts, dts, lanes=2), _sequential(m, items, ts, dts), "after set_precision")


# ---------------------------------------------------------------------------------------------------- 9
def test_white_box_solver_multi_routing(tiny, monkeypatch):
    from flowmse_amd.sampling import ODEsolverRegistry, get_white_box_solver, get_white_box_solver_multi
    from flowmse_amd.sampling.odesolvers import EulerODEsolver

    @ODEsolverRegistry.register("euler_plugin_streams_test")
    class PluginEuler(EulerODEsolver):
        def update_fn(self, x, t, y, stepsize, *args):
            return super().update_fn(x, t, y, stepsize, *args)

    items = _items(tiny, [(1, 64), (2, 128), (1, 192)], 64, seed0=130)
    Ys, zs = [y for _, y, _ in items], [z for _, _, z in items]
    calls = []
    real = type(tiny).rk_sample_multi_

    def counted(self, *a, **k):
        calls.append(len(a[0]))
        return real(self, *a, **k)

    monkeypatch.setattr(type(tiny), "rk_sample_multi_", counted)
    # a plugin that overrides update_fn: the per-item path, the plugin's update is what runs
    got, n = get_white_box_solver_multi("euler_plugin_streams_test", tiny.ode, tiny, Ys, N=4, zs=zs, lanes=3)()
    assert n == 4 and calls == []
    for g, Y, z in zip(got, Ys, zs):
        assert torch.equal(g, get_white_box_solver("euler_plugin_streams_test", tiny.ode, tiny, Y, N=4, z=z)()[0])
    # the library's own solver: one fused multi call
    got, n = get_white_box_solver_multi("euler", tiny.ode, tiny, Ys, N=4, zs=zs, lanes=3)()
    torch.cuda.synchronize()
    assert n == 4 and calls == [3]
    for g, Y, z in zip(got, Ys, zs):
        assert torch.equal(g, get_white_box_solver("euler", tiny.ode, tiny, Y, N=4, z=z)()[0])


def test_enhance_entries_share_one_core(full):
    """One 1 s utterance (128 padded frames), N = 1, one key and seed: the three enhance entries give the same bytes, as
    numpy and as a device tensor."""
    import numpy as np
    from flowmse_amd.evaluate import _synthetic_pairs, enhance_batch, enhance_concurrent, enhance_waveform
    y = torch.from_numpy(_synthetic_pairs(1, seconds=1.0)[0][2])[None].cuda()
    kw = dict(N=1, noise_keys=[0x912975D344AF26C6], noise_seed=0x1F2E3D4C5B6A7988)
    one = enhance_waveform(full, y, **kw)
    assert isinstance(one, np.ndarray) and one.shape == (16000,) and one.dtype == np.float32 and np.isfinite(one).all()
    assert enhance_batch(full, [y], **kw)[0].tobytes() == one.tobytes()
    assert enhance_concurrent(full, [y], 1, **kw)[0].tobytes() == one.tobytes()
    t = enhance_batch(full, [y], as_tensor=True, **kw)[0]
    assert t.is_cuda and t.dim() == 1 and t.cpu().numpy().tobytes() == one.tobytes()


# ---------------------------------------------------------------------------------------------------- 10
@pytest.mark.timeout(900)
def test_evaluate_streams_writes_identical_files(tmp_path):
    """The CLI with three lanes and with one writes byte-identical wav files (child processes, each under its own time
    limit; the second one only starts when the first one ended well).  Both runs are seeded: the prior noise of an
    unseeded run differs from process to process (torch seeds its default device generator from the clock), with or
    without --streams."""
    outs = {}
    for k in (3, 1):
        out = tmp_path / f"streams{k}"
        r = subprocess.run(["timeout", "-k", "10", "400", sys.executable, "-m", "flowmse_amd.evaluate", "--synthetic", "3",
                            "--seed", "7", "--streams", str(k), "--folder_destination", str(out)], cwd=ROOT, capture_output=True,
                           text=True)
        assert r.returncode == 0, f"--streams {k} exited with {r.returncode}:\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}"
        outs[k] = out / "files"
    names = sorted(os.listdir(outs[1]))
    assert len(names) == 3 and names == sorted(os.listdir(outs[3]))
    for n in names:
        assert filecmp.cmp(outs[1] / n, outs[3] / n, shallow=False), f"{n} differs between --streams 1 and 3"


# ---------------------------------------------------------------------------------------------------- argument handling
def test_lanes_argument_and_views_on_demand():
    m = _model(C.TINY)
    ts, dts = _grid(2)
    items = _items(m, [(1, 64), (1, 128), (1, 64), (1, 128)], 64, seed0=140)
    xs, ys = [x0.clone() for x0, _, _ in items], [y for _, y, _ in items]
    for bad in (0, 5):
        with pytest.raises(ValueError, match="lanes must be"):
            m.dnn.rk_sample_multi(xs, ys, ts, dts, "euler", lanes=bad)
    with pytest.raises(ValueError, match="lane_of"):
        m.dnn.rk_sample_multi(xs, ys, ts, dts, "euler", lanes=2, lane_of=[0, 1, 2, 0])
    want = _sequential(m, items, ts, dts)
    _assert_equal(_multi(m, items, ts, dts, lanes=4, lane_of=[0, 1, 0, 1]), want, "four lanes allowed, two used")
    assert len(m.dnn._views) == 1               # no view for a lane that holds no item
