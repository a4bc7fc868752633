"""GPU: the device buffers of a model handle, pinned.

Which buffers a handle and its weight set hold after each call -- what grows, what is kept across a precision change,
what a view owns -- is visible from outside as two numbers, flowse_model_device_bytes(FLOWSE_BYTES_WEIGHTS / _OWNED).
tests/handle_buffer_pins.json holds both after every step of one sequence of calls on one handle (SEQUENCE below), and
the scratch size each 16-bit per-op entry asks for at one small shape (SCRATCH_CASES).  Comparison is exact equality.
A change that does not mean to alter when a buffer is allocated, grown or freed leaves the file untouched; one that
does regenerates it:

    python tests/test_gpu_handle_buffers.py --write

(FLOWSE_LIB_PATH=<another build's libflowse_hip.so> reproduces the file from that build.)

Every model test runs the WIDE configuration at [B, 1, 64, 64]: nf = 32 is the smallest width that enters 16-bit
storage, so bf16 and fp16 keep the 16-bit twin and the fragment-order copies, bf16x3 and fp32 do not.
"""
import ctypes as CT
import json
import os
import re
import sys

import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
PINS = os.path.join(HERE, "handle_buffer_pins.json")
F = T = 64
MODES = {"fp32": 0, "bf16x3": 1, "bf16": 2, "fp16": 3}
ERR_ARG = 1
SEQUENCE = ["load fp32", "reserve B=1", "reserve B=2", "reserve B=1 again", "heun N=2", "rk45 capped", "bf16 + load",
            "fp16 + load", "bf16x3 + load", "fp32 + load"]
# one smallest shape each entry's kernel takes: (B, H, W, Cin, Cout); attention: (B, L, C)
SCRATCH_CASES = {"conv2d_16_3x3": (1, 8, 8, 32, 32), "conv2d_16_1x1": (1, 8, 8, 32, 32),
                 "resblock_tail_16": (1, 128, 128, 128, 128), "attention_16": (1, 64, 32)}


def _env():
    import torch
    import _cases as C
    from flowmse_amd import _lib
    from flowmse_amd.backbones.structure import create_handle, handle_param_table
    from flowmse_amd.util import synth
    return torch, C, _lib, _lib.lib, create_handle, handle_param_table, synth


def _blob():
    """The WIDE network's parameters, synthetic, in the library's blob order."""
    torch, C, _lib, L, create_handle, handle_param_table, synth = _env()
    h = create_handle(C.WIDE)
    try:
        names, shapes, offsets = handle_param_table(h)
        blob = torch.zeros(int(L.flowse_model_blob_numel(h)))
    finally:
        L.flowse_model_destroy(h)
    for n, shp, off in zip(names, shapes, offsets):
        w = torch.from_numpy(synth.synth_param(n, tuple(shp)))
        blob[off:off + w.numel()] = w.reshape(-1)
    return blob.contiguous()


def _load(h, blob, mode=None):
    torch, C, _lib, L = _env()[:4]
    if mode is not None:
        _lib.check(L.flowse_model_set_precision(h, MODES[mode]))
    _lib.check(L.flowse_model_load_weights(h, CT.c_void_p(blob.data_ptr()), blob.numel()))


def _fresh(blob, mode="fp32"):
    torch, C, _lib, L, create_handle = _env()[:5]
    h = create_handle(C.WIDE)
    _load(h, blob, mode)
    return h


def _bytes(h):
    _lib, L = _env()[2:4]
    return [int(L.flowse_model_device_bytes(h, _lib.FLOWSE_BYTES_WEIGHTS)),
            int(L.flowse_model_device_bytes(h, _lib.FLOWSE_BYTES_OWNED))]


def _reserve(h, B):
    _lib, L = _env()[2:4]
    n = CT.c_int64()
    _lib.check(L.flowse_model_reserve(h, B, F, T, CT.byref(n)))
    return int(n.value)


def _inputs(B=1):
    torch, C, _lib, L, _, _, synth = _env()
    x = C.c64(synth.complex_normal(17, 1, (B, 1, F, T), 0.5)).cuda()
    y = C.c64(synth.synth_spectrogram(17, B, F, T)).cuda()
    return x, y


def _forward(h, B=1):
    torch, C, _lib, L = _env()[:4]
    x, y = _inputs(B)
    t = torch.full((B,), 0.515, device="cuda")
    out = torch.empty_like(x)
    _lib.check(L.flowse_vf_forward(h, _lib.ptr(x), _lib.ptr(y), _lib.ptr(t), _lib.ptr(out), B, F, T, 0, _lib.current_stream()))
    torch.cuda.synchronize()
    assert torch.isfinite(torch.view_as_real(out)).all()
    return out


def _heun(h):
    torch, C, _lib, L = _env()[:4]
    from flowmse_amd.sampling import time_grid
    ts, dts = (v.tolist() for v in time_grid(1.0, 0.03, 2))
    x, y = _inputs()
    _lib.check(L.flowse_rk_sample(h, _lib.ptr(x), _lib.ptr(y), (CT.c_float * 2)(*ts), (CT.c_float * 2)(*dts), 2, 1, 1, F, T,
                                  _lib.current_stream()))
    torch.cuda.synchronize()


def _rk45(h):
    """scipy's first-step selection (2 evaluations) and one attempted step (6): the cap ends the solve with status -2"""
    torch, C, _lib, L = _env()[:4]
    x, y = _inputs()
    times = (CT.c_double * 4)()
    nfev, status, nacc = CT.c_int64(), CT.c_int(), CT.c_int()
    _lib.check(L.flowse_rk45_sample(h, _lib.ptr(x), _lib.ptr(y), 1.0, 0.03, 1e-5, 1e-5, 0.0, float("inf"), 8, 1, F, T,
                                    CT.byref(nfev), CT.byref(status), times, 4, CT.byref(nacc), _lib.current_stream()))
    torch.cuda.synchronize()
    assert 2 <= nfev.value <= 8


def _sequence(blob):
    """SEQUENCE on one new handle -> (the handle, [[step, weight bytes, owned bytes]])."""
    torch, C, _lib, L, create_handle = _env()[:5]
    h = create_handle(C.WIDE)
    steps = [lambda: _load(h, blob), lambda: _reserve(h, 1), lambda: _reserve(h, 2), lambda: _reserve(h, 1),
             lambda: _heun(h), lambda: _rk45(h), lambda: _load(h, blob, "bf16"), lambda: _load(h, blob, "fp16"),
             lambda: _load(h, blob, "bf16x3"), lambda: _load(h, blob, "fp32")]
    rec = []
    try:
        for name, step in zip(SEQUENCE, steps):
            step()
            rec.append([name] + _bytes(h))
    except Exception:
        L.flowse_model_destroy(h)
        raise
    return h, rec


def _scratch_call(case, nbytes, scratch=None):
    """One call of the entry with `nbytes` declared -> (return code, last error)."""
    torch, C, _lib, L = _env()[:4]
    p, s = _lib.ptr, _lib.current_stream()
    g = torch.Generator().manual_seed(5)
    rnd = lambda *shape: (0.1 * torch.randn(*shape, generator=g)).cuda()
    if scratch is None:
        scratch = torch.empty(max(nbytes, 256), dtype=torch.uint8, device="cuda")
    assert scratch.numel() >= nbytes
    if case == "attention_16":
        B, Lt, Cc = SCRATCH_CASES[case]
        qkv, out = rnd(B, Lt, 3 * Cc), torch.empty(B, Lt, Cc, device="cuda")
        rc = L.flowse_op_attention_16(p(qkv), p(out), B, Lt, Cc, 1, p(scratch), nbytes, s)
    elif case == "resblock_tail_16":
        B, H, W, Cc, Cout = SCRATCH_CASES[case]
        h, x1, out = rnd(B, H, W, Cc), rnd(B, H, W, Cc), torch.empty(B, H, W, Cout, device="cuda")
        w1, w2, b1, b2 = rnd(Cout, 9, Cc), rnd(Cout, 1, Cc), rnd(Cout), rnd(Cout)
        rc = L.flowse_op_resblock_tail_16(p(h), Cc, None, None, None, 0, p(w1), p(b1), p(x1), Cc, None, 0, p(w2), p(b2),
                                          p(out), B, H, W, Cout, 0.7071, 1, p(scratch), nbytes, s)
    else:
        taps = 9 if case.endswith("3x3") else 1
        B, H, W, Cc, Cout = SCRATCH_CASES[case]
        x, w, b, out = rnd(B, H, W, Cc), rnd(Cout, taps, Cc), rnd(Cout), torch.empty(B, H, W, Cout, device="cuda")
        rc = L.flowse_op_conv2d_16(p(x), Cc, None, 0, p(w), p(b), None, None, None, None, 0, p(out), B, H, W, Cout, taps,
                                   1.0, 1, p(scratch), nbytes, s)
    torch.cuda.synchronize()
    return rc, L.flowse_last_error().decode()


def _scratch_need(case):
    """The size the entry itself names when it is offered nothing."""
    rc, msg = _scratch_call(case, 0)
    m = re.search(r"scratch needs (\d+) bytes", msg)
    assert rc == ERR_ARG and m, (case, rc, msg)
    return int(m.group(1))


@pytest.fixture(scope="module")
def blob():
    import torch
    assert torch.cuda.is_available()
    return _blob()


@pytest.fixture(scope="module")
def pins():
    with open(PINS) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def tripped(blob):
    """(handle, record): the handle after SEQUENCE, back in fp32"""
    h, rec = _sequence(blob)
    yield h, rec
    _env()[3].flowse_model_destroy(h)


def test_pinned_sequence(tripped, pins):
    _, rec = tripped
    for name, w, o in rec:
        print(f"{name:>18}: weights {w} bytes, owned {o} bytes")
    assert rec[3][1:] == rec[2][1:], "reserve at the smaller batch moved the bytes"
    assert rec[2][2] > rec[1][2], "the workspace did not grow with the batch"
    assert rec == pins["sequence"], "device bytes moved (meant? regenerate with --write)"


@pytest.mark.parametrize("mode", list(MODES))
def test_forward_after_round_trip_equals_fresh_handle(tripped, blob, mode):
    torch, C, _lib, L = _env()[:4]
    h, _ = tripped
    fresh = _fresh(blob, mode)
    view = CT.c_void_p()
    try:
        want = _forward(fresh)
        _load(h, blob, mode)
        got = _forward(h)
        assert torch.equal(torch.view_as_real(got), torch.view_as_real(want)), f"{mode}: differs from a fresh handle"
        _lib.check(L.flowse_model_view_create(h, CT.byref(view)))
        vw, vo = _bytes(view)
        assert vw == _bytes(h)[0] and 0 < vo <= 4096
        assert torch.equal(torch.view_as_real(_forward(view)), torch.view_as_real(want)), f"{mode}: the view differs"
    finally:
        if view:
            L.flowse_model_destroy(view)
        L.flowse_model_destroy(fresh)
        _load(h, blob, "fp32")


def test_destroy_views_then_parent_then_again(blob):
    torch, C, _lib, L = _env()[:4]

    def life():
        parent = _fresh(blob)
        views = [CT.c_void_p(), CT.c_void_p()]
        try:
            for v in views:
                _lib.check(L.flowse_model_view_create(parent, CT.byref(v)))
            outs = [_forward(parent, 2), _forward(views[0], 1), _forward(views[1], 2)]
            return [_bytes(x) for x in [parent] + views], outs
        finally:
            for x in views + [parent]:          # the views first, the set's last holder last
                if x:
                    L.flowse_model_destroy(x)

    bytes0, outs0 = life()
    bytes1, outs1 = life()
    assert bytes0 == bytes1
    assert bytes0[0][0] == bytes0[1][0] == bytes0[2][0] and bytes0[0][1] == bytes0[2][1] > bytes0[1][1]
    assert torch.equal(torch.view_as_real(outs0[0]), torch.view_as_real(outs0[2]))
    for a, b in zip(outs0, outs1):
        assert torch.equal(torch.view_as_real(a), torch.view_as_real(b))


@pytest.mark.parametrize("case", list(SCRATCH_CASES))
def test_scratch_threshold(pins, case):
    torch = _env()[0]
    need = pins["scratch"][case]
    scratch = torch.empty(need, dtype=torch.uint8, device="cuda")
    rc, msg = _scratch_call(case, need - 1, scratch)
    assert rc == ERR_ARG and f"scratch needs {need} bytes" in msg, (rc, msg)
    rc, msg = _scratch_call(case, need, scratch)
    assert rc == 0, (rc, msg)


def _write():
    sys.path.insert(0, os.path.dirname(HERE))
    L = _env()[3]
    h, rec = _sequence(_blob())
    L.flowse_model_destroy(h)
    scratch = {case: _scratch_need(case) for case in SCRATCH_CASES}
    with open(PINS, "w") as f:                     # one step per line: a change reads as a diff of steps
        f.write("{\n \"sequence\": [\n" + ",\n".join("  " + json.dumps(r) for r in rec) + "\n ],\n")
        f.write(" \"scratch\": " + json.dumps(scratch) + "\n}\n")
    for r in rec:
        print(r)
    print(scratch)
    print("wrote", PINS)


if __name__ == "__main__":
    if sys.argv[1:] != ["--write"]:
        sys.exit("usage: python tests/test_gpu_handle_buffers.py --write")
    _write()
