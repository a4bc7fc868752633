"""GPU: the launch plans themselves, pinned.

Builder (csrc/model_plan.hip) turns the network into the flat launch list every sampler step replays.  Which kernel a
conv gets, whether it runs split over K, whose reduction finishes a GroupNorm, where a shortcut rides: all of it shows
in that list and in the arena's peak.  tests/plan_pins.json holds, per (precision mode, B, T) at F = 256 with the released
architecture: the plan's workspace_bytes; the launch / flop / issued-flop totals of one forward; and per label, in order
of first appearance in the launch list, [label, launches, flops, bytes, issued].  Comparison is exact equality of the
parsed values (times are not pinned).  A change that does not mean to alter a plan leaves the file untouched; one that
does regenerates it and the diff of the file is the diff of the launches:

    python tests/test_gpu_plan_pins.py --write

(FLOWSE_LIB_PATH=<another build's libflowse_hip.so> reproduces the file from that build.)

The cases reach every branch of Builder::resblock and Builder::conv: small-image kernels up to 2048 pixels, the 2049-8191
pixel range where convs run split over K with merged and GroupNorm-finishing reductions, the low-resolution shortcut of
fp32 up blocks, the folded shortcut of the 16-bit modes, the bf16 planes.
"""
import json
import os
import sys

import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
PINS = os.path.join(HERE, "plan_pins.json")
F = 256
# mode -> [(B, T)]
CASES = {"fp32": [(1, 64), (3, 128), (1, 256), (8, 256)],
         "bf16": [(1, 256), (8, 256)],
         "fp16": [(8, 256)],
         "bf16x3": [(8, 256)]}


def _key(mode, B, T):
    return f"{mode}:B{B}xT{T}"


def _model():
    """The released architecture with synthetic weights (= test_gpu_model.py's `full` fixture)."""
    import torch
    import _cases as C
    from flowmse_amd.model import VFModel
    from flowmse_amd.util import synth
    m = VFModel(backbone="ncsnpp", ode="flowmatching", **C.FULL)
    m.dnn.load_state_dict({n: torch.from_numpy(synth.synth_param(n, tuple(p.shape))) for n, p in m.dnn.named_parameters()})
    return m.cuda().eval()


def _measure(dnn, B, T):
    """One forward of the current precision mode at [B, 2, F, T] -> the pinned record."""
    import torch
    import _cases as C
    from flowmse_amd.util import synth
    ws = dnn.reserve(B, F, T)
    x = C.c64(synth.complex_normal(41, 1, (B, 1, F, T), 0.5))
    y = C.c64(synth.synth_spectrogram(41, B, F, T))
    inp = torch.cat([x, y], 1).cuda()
    t = torch.full((B,), 0.515, device="cuda")
    dnn.profile_begin(1)
    try:
        dnn(inp, t)
    finally:
        prof = dnn.profile_end()
    tot = prof.pop("_all_launches")
    return {"workspace_bytes": ws,
            "launches": tot["launches"], "flops": tot["flops"], "issued": tot["issued"],
            "ops": [[k, v["launches"], v["flops"], v["bytes"], v["issued"]] for k, v in prof.items()]}


def _measure_mode(dnn, mode):
    dnn.set_precision(mode)
    try:
        return {_key(mode, B, T): _measure(dnn, B, T) for B, T in CASES[mode]}
    finally:
        dnn.set_precision("fp32")


def _diff(key, want, got):
    """Readable account of what moved (empty: nothing)."""
    out = [f"{key}: {f} {want[f]!r} -> {got[f]!r}" for f in ("workspace_bytes", "launches", "flops", "issued")
           if want[f] != got[f]]
    if want["ops"] != got["ops"]:
        n = next((i for i, (a, b) in enumerate(zip(want["ops"], got["ops"])) if a != b), min(len(want["ops"]), len(got["ops"])))
        a = want["ops"][n] if n < len(want["ops"]) else None
        b = got["ops"][n] if n < len(got["ops"]) else None
        out.append(f"{key}: {len(want['ops'])} -> {len(got['ops'])} labels; first difference at #{n}: {a} -> {b}")
    return out


@pytest.fixture(scope="module")
def full():
    import torch
    assert torch.cuda.is_available()
    return _model()


@pytest.fixture(scope="module")
def pins():
    with open(PINS) as f:
        return json.load(f)


@pytest.mark.parametrize("mode", list(CASES))
def test_plan_pins(full, pins, mode):
    got = _measure_mode(full.dnn, mode)
    assert full.dnn.precision == "fp32"
    bad = []
    for key, rec in got.items():
        print(f"{key}: {rec['launches']} launches per forward, {len(rec['ops'])} labels, workspace {rec['workspace_bytes']} bytes")
        assert key in pins, f"{key} is not in {os.path.basename(PINS)}"
        bad += _diff(key, pins[key], json.loads(json.dumps(rec)))
    assert not bad, "the launch plan moved (meant? regenerate with --write):\n" + "\n".join(bad)


def _write():
    sys.path.insert(0, os.path.dirname(HERE))
    dnn = _model().dnn
    rec = {}
    for mode in CASES:
        rec.update(_measure_mode(dnn, mode))
    with open(PINS, "w") as f:                     # one label per line: a plan change reads as a diff of launches
        f.write("{\n")
        for i, (key, r) in enumerate(rec.items()):
            head = {k: v for k, v in r.items() if k != "ops"}
            f.write(f" {json.dumps(key)}: {{{json.dumps(head)[1:-1]}, \"ops\": [\n")
            f.write(",\n".join("  " + json.dumps(o) for o in r["ops"]))
            f.write("\n ]}" + (",\n" if i + 1 < len(rec) else "\n"))
        f.write("}\n")
    for key, r in rec.items():
        print(f"{key}: {r['launches']} launches per forward, {len(r['ops'])} labels, workspace {r['workspace_bytes']} bytes")
    print("wrote", PINS)


if __name__ == "__main__":
    if sys.argv[1:] != ["--write"]:
        sys.exit("usage: python tests/test_gpu_plan_pins.py --write")
    _write()
