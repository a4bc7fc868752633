"""Host side of the multi-lane sampler: argument checks of the new C-ABI entries (no device is touched before they
fail), the lane planner, and the evaluate CLI's --streams argument.  None of this needs a GPU."""
import ctypes as C

import pytest

from flowmse_amd import _lib
from flowmse_amd.backbones.structure import create_handle

import _cases as Cs

L = _lib.lib
ERR_ARG, ERR_STATE = 1, 3


def _err():
    return L.flowse_last_error().decode()


def test_view_create_argument_errors():
    out = C.c_void_p()
    assert L.flowse_model_view_create(None, C.byref(out)) == ERR_ARG and _err()
    full = create_handle(Cs.TINY)
    try:
        assert L.flowse_model_view_create(full, None) == ERR_ARG and _err()
        # a full-network handle that has no weights yet: a view would share nothing
        assert L.flowse_model_view_create(full, C.byref(out)) == ERR_STATE and "weights" in _err()
        assert not out.value
        assert L.flowse_model_weight_holders(full) == 0
        assert L.flowse_model_device_bytes(full, _lib.FLOWSE_BYTES_WEIGHTS) == 0
        assert L.flowse_model_device_bytes(full, _lib.FLOWSE_BYTES_OWNED) == 0
    finally:
        L.flowse_model_destroy(full)
    blk = C.c_void_p()
    _lib.check(L.flowse_block_create(0, 32, 32, 0, 0, 64, C.byref(blk)))
    try:
        assert L.flowse_model_view_create(blk, C.byref(out)) == ERR_ARG and "single-module" in _err()
        assert not out.value
    finally:
        L.flowse_model_destroy(blk)


def test_rk_sample_multi_argument_errors():
    """Every check below fails before the first device call: it runs on a machine without a GPU."""
    hs = [create_handle(Cs.TINY) for _ in range(5)]
    try:
        n = 5
        ts = (C.c_float * 2)(1.0, 0.03)
        dts = (C.c_float * 2)(0.97, 0.03)
        h_a = (C.c_void_p * n)(*[h.value for h in hs])
        fake = (C.c_void_p * n)(*[0x1000] * n)          # never dereferenced: the call fails on its arguments
        B = (C.c_int * n)(*[1] * n)
        T = (C.c_int * n)(*[64] * n)
        assert _lib.FLOWSE_MAX_LANES == 4
        assert L.flowse_rk_sample_multi(h_a, 0, fake, fake, B, T, 64, ts, dts, 2, 0, None) == ERR_ARG and _err()
        assert L.flowse_rk_sample_multi(None, 2, fake, fake, B, T, 64, ts, dts, 2, 0, None) == ERR_ARG and _err()
        assert L.flowse_rk_sample_multi(h_a, 2, None, fake, B, T, 64, ts, dts, 2, 0, None) == ERR_ARG and _err()
        assert L.flowse_rk_sample_multi(h_a, 2, fake, fake, None, T, 64, ts, dts, 2, 0, None) == ERR_ARG and _err()
        assert L.flowse_rk_sample_multi(h_a, 2, fake, fake, B, T, 64, None, dts, 2, 0, None) == ERR_ARG and _err()
        assert L.flowse_rk_sample_multi(h_a, 2, fake, fake, B, T, 64, ts, dts, 2, 7, None) == ERR_ARG and _err()
        # five distinct handles are five lanes
        assert L.flowse_rk_sample_multi(h_a, 5, fake, fake, B, T, 64, ts, dts, 2, 0, None) == ERR_ARG
        assert "distinct handles" in _err()
        # a null handle inside the table
        h_bad = (C.c_void_p * 2)(hs[0].value, None)
        assert L.flowse_rk_sample_multi(h_bad, 2, fake, fake, B, T, 64, ts, dts, 2, 0, None) == ERR_ARG and _err()
    finally:
        for h in hs:
            L.flowse_model_destroy(h)


def _check_plan(costs, k):
    from flowmse_amd.parallel import plan_lanes
    lane_of, order = plan_lanes(costs, k)
    assert len(lane_of) == len(costs) and len(order) == k
    assert sorted(i for o in order for i in o) == list(range(len(costs)))          # every item exactly once
    assert all(lane_of[i] == l for l, o in enumerate(order) for i in o)
    assert all(o == sorted(o) for o in order)                                      # input order inside a lane
    loads = [sum(costs[i] for i in o) for o in order]
    mean = sum(costs) / k
    if costs:
        assert max(loads) <= mean + max(costs) + 1e-9
    assert plan_lanes(costs, k) == (lane_of, order)                                # same input -> same plan
    return max(loads) / mean if costs else 1.0


def test_plan_lanes_properties():
    from flowmse_amd.parallel import batch_cost, plan_lanes
    costs = [batch_cost(64 * t, b) for t, b in [(2, 1), (10, 1), (3, 2), (3, 1), (7, 1), (5, 8), (5, 1), (8, 1), (2, 4)]]
    for k in (1, 2, 3, 4):
        _check_plan(costs, k)
    assert plan_lanes(costs, 1) == ([0] * len(costs), [list(range(len(costs)))])   # k = 1: the input order
    assert plan_lanes([], 3) == ([], [[], [], []])
    assert plan_lanes([5.0, 5.0, 5.0], 2)[0] == [0, 1, 0]                          # ties: earlier item, lower lane
    with pytest.raises(ValueError):
        plan_lanes(costs, 0)


def test_plan_lanes_balance_on_the_standin_set():
    """The 824-utterance stand-in set of test_plan_shards_config3_partition: modelled imbalance (max / mean lane load)
    of a longest-processing-time deal, for single utterances and for the equal-length batches of up to 8."""
    import bench
    from flowmse_amd.parallel import batch_cost, plan_batches
    padded = [((t + 63) // 64) * 64 for t in bench.vbdmd_lengths(bench.VBDMD_UTTS)]
    assert len(padded) == 824
    items = [batch_cost(T, 1) for T in padded]
    batches = plan_batches(range(len(padded)), padded, 8)
    assert len(batches) == 106
    bcosts = [batch_cost(T, len(ids)) for T, ids in batches]
    for k in (2, 3, 4):
        a, b = _check_plan(items, k), _check_plan(bcosts, k)
        print(f"k={k}: imbalance items {a:.4f} batches {b:.4f}")
        assert a <= 1.01 and b <= 1.01


def test_evaluate_streams_argument():
    from flowmse_amd.evaluate import build_parser
    ap = build_parser()
    assert ap.parse_args(["--folder_destination", "o"]).streams == 1
    assert ap.parse_args(["--folder_destination", "o", "--streams", "3"]).streams == 3
    for bad in ("0", "5"):
        with pytest.raises(SystemExit):
            ap.parse_args(["--folder_destination", "o", "--streams", bad])
