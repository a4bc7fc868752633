"""CPU: the conv routing decision, pinned.

conv_route (csrc/conv_dispatch.hip) decides which kernel a convolution runs, over how many K slices, whether a reduction
launch follows and in what geometry the GroupNorm statistics leave it.  The plan builder stores its answer per conv and
launch_conv switches on it, so this table -- asked through flowse_op_conv_route, a host-only entry: no GPU is touched --
is the routing of every model the library runs.  tests/conv_route_pins.txt holds it; a change that does not mean to alter
a route leaves the file untouched, one that does regenerates it and the diff of the file is the diff of the routes:

    python tests/test_conv_route_host.py --write

File format.  One line per shape, storage type and answer: "HxW C1+C2>Cout/taps dt B<batches>" and, per distinct answer, the
offers that get it, "names: answer".  An answer is the entry's text with the field names dropped, "kernel ks stats gn issued"
(`reduce` is left out: it is ks > 1, which test_route_properties asserts for every query; `reads` too: the kernel decides
it, test_route_reads holds every query to that mapping), or "error <status>".  dt "16"
stands for bf16 and fp16 where their answers are equal; "f32>bf16" is an fp32 input stored as bf16 (the convs of the
4-channel input in the 16-bit modes); batches that give the same answers share a line.  The first
section is the library as loaded by default; a section "[HOOK=value]" is the same list of queries asked in a fresh process
with that environment variable set (the hooks are read when the library loads) and holds only what differs from the first.

The queries: every distinct conv of tests/plan_pins.json (LEVELS x CASES below, concat inputs as their two parts) at the
batch of its case and at B = 2 and 4, in all three storage types, offering what a model handle holds / nothing / the
former plus normalise-on-load -- the convs of the 4-channel input (IN4_LEVELS) with fp32 in and each storage type out, with
and without statistics asked for --; and EDGES, the two sides of every threshold the policy has.
"""
import ctypes
import os
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
PINS = os.path.join(HERE, "conv_route_pins.txt")

# FLOWSE_OFFER_* of include/flowse_hip.h
WINO, WINO2, WSM, WFRAG, WQ, WQ3, WQF16, SLAB, GN, BIAS2, STATS, FOLD = (1 << i for i in range(12))
F32, BF16, F16 = 0, 1, 2
DT_NAME = {F32: "f32", BF16: "bf16", F16: "f16"}
# what a model handle holds for a conv, per storage type (fp32 weights only: the bf16-plane modes are among the EDGES)
HANDLE = {F32: WINO | WINO2 | WSM | SLAB, BF16: WQ | WFRAG | SLAB, F16: WQ | WQF16 | WFRAG | SLAB}

# ---- the convs of the pinned plans: tests/plan_pins.json, F = 256, labels "name@HxW:Cin>Cout"
# (B, T) of the cases, each also at B = 2 and 4
CASES = [(1, 64), (3, 128), (1, 256), (8, 256)]
# image height of a level -> (C1, C2, Cout, taps) of the convs that run there; inputs of 384 and 512 channels, and the 256
# of the two full-size levels, are concats of a block's input and its skip
LEVELS = {
    256: [(128, 0, 4, 9), (128, 0, 128, 9), (128, 128, 128, 1), (128, 128, 128, 9)],
    128: [(128, 0, 4, 9), (128, 0, 128, 1), (128, 0, 128, 9), (128, 128, 128, 1), (128, 128, 128, 9),
          (256, 0, 256, 1), (256, 0, 256, 9), (256, 128, 128, 1), (256, 128, 128, 9)],
    64: [(128, 0, 128, 1), (128, 0, 128, 9), (128, 0, 256, 1), (128, 0, 256, 9), (256, 0, 4, 9),
         (256, 0, 256, 1), (256, 0, 256, 9), (256, 128, 256, 1), (256, 128, 256, 9), (256, 256, 256, 1), (256, 256, 256, 9)],
    32: [(256, 0, 4, 9), (256, 0, 256, 1), (256, 0, 256, 9), (256, 256, 256, 1), (256, 256, 256, 9)],
    16: [(256, 0, 4, 9), (256, 0, 256, 1), (256, 0, 256, 9), (256, 0, 768, 1), (256, 256, 256, 1),
         (256, 256, 256, 9)],
    8: [(256, 0, 4, 9), (256, 0, 256, 1), (256, 0, 256, 9), (256, 256, 256, 1), (256, 256, 256, 9)],
    4: [(256, 0, 4, 9), (256, 0, 256, 1), (256, 0, 256, 9), (256, 0, 768, 1), (256, 256, 256, 1),
        (256, 256, 256, 9)],
}
# the convs of the 4-channel input (labels conv_in and combine_1x1): fp32 in, every storage type out
IN4_LEVELS = {256: [(4, 0, 128, 9)], 128: [(4, 0, 128, 1)], 64: [(4, 0, 128, 1)], 32: [(4, 0, 256, 1)], 16: [(4, 0, 256, 1)],
              8: [(4, 0, 256, 1)], 4: [(4, 0, 256, 1)]}
IN4 = (F32, (F32, BF16), (F32, F16))                  # a pair: (in_dt, out_dt) where the two differ by design
IN4_OFFERS = [("h", 0), ("+stats", STATS), ("0", None), ("g", GN)]
# offers: (name, bits added to HANDLE[dt]; None: no bits at all).  h = what a handle holds, 0 = nothing, g = h + normalise-on-load
PLAN_OFFERS = [("h", 0), ("0", None), ("g", GN)]

# ---- the edges: (B, H, W, C1, C2, Cout, taps), storage types, [(offer name, bits added to HANDLE[dt] | None)]
ALL = (F32, BF16, F16)
STD = [("h", 0), ("g", GN)]
EDGES = []
# pixels over the batch: 64 | 65 (32-row tiles), 256 | 257 (16 x 16-tile small-image kernel), 2048 | 2049 (small-image
# kernels), 8191 | 8192 (the sliced range ends where 128-row tiles fill the chip)
for B, H, W in [(1, 8, 8), (5, 13, 1), (1, 16, 16), (257, 1, 1), (8, 16, 16), (3, 683, 1), (1, 8191, 1), (8, 32, 32)]:
    EDGES += [((B, H, W, 256, 0, 256, t), ALL, STD) for t in (9, 1)]
# (8 x 16-pixel tile, 64-channel block) pairs of the F(4,3) kernel: 15 | 16 (too small even sliced), 255 | 256 (whole K);
# (16 x 16, 64) blocks of the 2-D kernel: 127 | 128; the same counts of 128-channel items: 63 | 64 producer / consumer
# kernel, 127 | 128 16-bit halo kernel
for B in (15, 16, 63, 64, 127, 128, 255, 256):
    EDGES += [((B, 8, 16, 128, 0, 64, 9), ALL, STD), ((B, 16, 16, 128, 0, 64, 9), ALL, STD),
              ((B, 8, 16, 128, 0, 128, 9), ALL, STD), ((B, 16, 16, 128, 0, 128, 9), ALL, STD)]
# H a multiple of 16, of 8 only, of neither; W = 8
EDGES += [((8, H, 64, 128, 0, 128, 9), ALL, STD) for H in (32, 24, 20)]
EDGES += [((8, 64, 8, 128, 0, 128, 9), ALL, STD), ((64, 64, 8, 128, 0, 128, 9), ALL, STD)]
# output widths, 3x3 and 1x1, large and small images
for Cout in (4, 32, 64, 96, 128, 384):
    EDGES += [((B, H, W, 128, 0, Cout, t), ALL, STD) for B, H, W in ((8, 64, 64), (1, 16, 16)) for t in (9, 1)]
# input widths that are 4-aligned only; a concat whose parts are not 32-aligned though their sum is
for C1, C2 in ((36, 0), (48, 16)):
    EDGES += [((B, H, W, C1, C2, 128, t), ALL, STD) for B, H, W in ((8, 64, 64), (1, 16, 16)) for t in (9, 1)]
# a folded shortcut, offered and not: on the producer / consumer kernel's shapes, without its weights, on a small image, in fp32
FOLDS = [("g", GN), ("fold+gn", FOLD | GN), ("fold-wfrag", FOLD | GN), ("fold", FOLD)]
EDGES += [((8, 64, 64, 128, 0, 128, 9), ALL, FOLDS), ((1, 32, 32, 256, 0, 256, 9), ALL, FOLDS), ((8, 64, 64, 128, 0, 256, 1), ALL, FOLDS)]
# per-sample bias and statistics on a 4-channel head (the head kernel has neither)
HEAD = [("h", 0), ("g", GN), ("+bias2", BIAS2), ("+stats", STATS), ("+bias2+stats+gn", BIAS2 | STATS | GN)]
EDGES += [((8, 128, 128, 128, 0, 4, 9), ALL, HEAD), ((1, 32, 32, 256, 0, 4, 9), ALL, HEAD)]
# fp32 storage with 16-bit weight planes next to the Winograd weights (precision modes bf16x3 / bf16 / fp16 operands)
PLANES = [("+bf16x3", WQ | WQ3), ("+bf16x3+gn", WQ | WQ3 | GN), ("+bf16", WQ), ("+f16", WQ | WQF16), ("+f16x3", WQ | WQ3 | WQF16)]
EDGES += [((B, H, W, 128, 0, Co, 9), (F32,), PLANES) for B, H, W in ((8, 256, 256), (1, 64, 64), (1, 16, 16)) for Co in (128, 64)]
# the kernels of a 4-channel fp32 input.  Matrix-core kernel: 32768 | 32640 pixels over the batch, H W a multiple of 128 or
# not, Cout 128 | 64, 256 (those run the VALU kernel)
EDGES += [((B, 8, 16, 4, 0, 128, 9), IN4, IN4_OFFERS) for B in (256, 255)]
EDGES += [((B, H, W, 4, 0, 128, 9), IN4, IN4_OFFERS) for B, H, W in ((64, 32, 16), (64, 33, 16))]
EDGES += [((2, 128, 128, 4, 0, Co, 9), IN4, IN4_OFFERS) for Co in (128, 64, 256)]
# VALU kernels: Cout / 4 divides 256 or not (96 | 64); weights of 72 KB | 36 KB | 8 KB in LDS (Cout 512 at taps 9 | 256 at
# taps 9 | 512 at taps 1); what they refuse runs the flat kernel, whole K, without statistics
EDGES += [((B, H, W, 4, 0, Co, t), IN4, IN4_OFFERS) for B, H, W in ((8, 64, 64), (1, 16, 16))
          for Co, t in ((96, 9), (96, 1), (64, 9), (64, 1), (512, 9), (256, 9), (512, 1))]
# statistics kernel: blocks of min(128, H W) pixels -- H W = 64, 128, 192 (not whole blocks); a block's pixels a multiple of the
# 256 / (Cout / 4) pixel rows or not (H W = 128: Cout 8 | 4); 3x3 with statistics asked for
EDGES += [((2, H, 8, 4, 0, 32, 1), IN4, IN4_OFFERS) for H in (8, 16, 24)]
EDGES += [((2, 16, 8, 4, 0, Co, 1), IN4, IN4_OFFERS) for Co in (8, 4)]
EDGES += [((2, 8, 8, 4, 0, 32, 9), IN4, IN4_OFFERS)]
# not the family: a second input part, 16-bit input
EDGES += [((2, 8, 8, 4, 4, 32, t), ALL, IN4_OFFERS) for t in (9, 1)]
EDGES += [((B, H, W, 4, 0, Co, t), (BF16, F16), IN4_OFFERS) for B, H, W, Co, t in ((8, 256, 256, 128, 9), (2, 8, 8, 32, 1))]

HOOKS = ["FLOWSE_NO_WINOGRAD=1", "FLOWSE_NO_HALO_CONV=1", "FLOWSE_FORCE_GENERIC_CONV=1", "FLOWSE_W2D=0", "FLOWSE_NO_SMALLM=1"]


def rows():
    """[(shape, storage types, offers)], duplicates removed, in listing order"""
    out, seen = [], set()
    for Bc, T in CASES:
        for B in (Bc, 2, 4):
            for lv, (H, convs) in enumerate(LEVELS.items()):
                for c in convs:
                    shape = (B, H, T >> lv) + c
                    if shape not in seen:
                        seen.add(shape)
                        out.append((shape, ALL, PLAN_OFFERS))
    for Bc, T in CASES:
        for B in (Bc, 2, 4):
            for lv, (H, convs) in enumerate(IN4_LEVELS.items()):
                for c in convs:
                    shape = (B, H, T >> lv) + c
                    if shape not in seen:
                        seen.add(shape)
                        out.append((shape, IN4, IN4_OFFERS))
    return out + EDGES


def queries():
    """[(key = (shape without B, dt, B), offer name, the entry's ten integer arguments)] in listing order"""
    out = []
    for shape, dts, offers in rows():
        B, H, W, C1, C2, Cout, taps = shape
        for dt in dts:
            in_dt, out_dt = dt if isinstance(dt, tuple) else (dt, dt)
            if Cout == 4:
                out_dt = F32                           # the 4-channel pyramids stay fp32 in every mode
            for name, add in offers:
                bits = 0 if add is None else (HANDLE[in_dt] | add) & ~(WFRAG if name == "fold-wfrag" else 0)
                out.append(((shape[1:], dt, B), name, (in_dt, out_dt, B, H, W, C1, C2, Cout, taps, bits)))
    return out


def ask(L, args):
    buf = ctypes.create_string_buffer(96)
    assert L.flowse_op_conv_route(*args, buf, 96) == 0, args
    return buf.value.decode()


def short(text):
    """the entry's line without its field names, and without `reduce` -- it is ks > 1 (test_route_properties holds every query to
    that) -- and `reads`: the kernel decides it (test_route_reads)"""
    return " ".join(f.split("=")[-1] for f in text.split() if not f.startswith(("reduce=", "reads=")))


def entries():
    """{key: "names: answer | names: answer ..."} from the library loaded into this process (offers that get one answer share it)"""
    from flowmse_amd import _lib
    per_key = {}
    for key, name, args in queries():
        per_key.setdefault(key, {}).setdefault(short(ask(_lib.lib, args)), []).append(name)
    return {k: "; ".join(",".join(names) + ": " + ans for ans, names in v.items()) for k, v in per_key.items()}


def render_section(ent):
    """Lines for a set of entries: per shape and answer, the storage types ("16": bf16 and fp16 alike) and batches that give it."""
    by_shape = {}
    for (shape, dt, B), body in ent.items():
        by_shape.setdefault(shape, {})[(dt, B)] = body
    lines = []
    for (H, W, C1, C2, Cout, taps), cell in by_shape.items():
        groups = {}
        for (dt, B), body in cell.items():
            pre, odt = (DT_NAME[dt[0]] + ">", dt[1]) if isinstance(dt, tuple) else ("", dt)
            twin = {BF16: F16, F16: BF16}.get(odt)
            both = twin is not None and cell.get(((dt[0], twin) if pre else twin, B)) == body
            if odt == F16 and both:
                continue
            groups.setdefault((pre + ("16" if both else DT_NAME[odt]), body), []).append(B)
        for (dtn, body), Bs in groups.items():
            lines.append(f"{H}x{W} {C1}+{C2}>{Cout}/{taps} {dtn} B{','.join(map(str, Bs))} {body}")
    return lines


def child_entries(hook):
    k, v = hook.split("=")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--dump"], env=dict(os.environ, **{k: v}),
                       capture_output=True, text=True, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    return eval(r.stdout)                                  # repr of entries(), printed by this file


def section(hook, base):
    """Lines of a hook's section: the entries that differ from the default library's"""
    got = child_entries(hook)
    assert list(got) == list(base), hook
    return render_section({k: v for k, v in got.items() if v != base[k]})


def read_pins():
    secs, name = {}, None
    with open(PINS) as f:
        for ln in f.read().splitlines():
            if ln.startswith("["):
                name = ln[1:-1]
                secs[name] = []
            else:
                secs[name].append(ln)
    return secs


def _compare(want, got, what):
    if got != want:
        moved = [ln for ln in got if ln not in set(want)]
        pytest.fail(f"the routes {what} moved: {len(want)} -> {len(got)} lines (meant? regenerate with --write); new lines:\n" +
                    "\n".join(moved[:20]))


def test_route_table_default():
    _compare(read_pins()["default"], render_section(entries()), "of the default library")


@pytest.mark.parametrize("hook", HOOKS)
def test_route_table_under_hook(hook):
    _compare(read_pins()[hook], section(hook, entries()), "under " + hook)


@pytest.fixture(scope="module")
def answers():
    from flowmse_amd import _lib
    return [(args, ask(_lib.lib, args)) for _, _, args in queries()]


def test_route_properties(answers):
    """What holds for every query, pinned or not."""
    kernels = set()
    for args, text in answers:
        dt, out_dt, B, H, W, C1, C2, Cout, taps, bits = args
        family = dt == F32 and (C1, C2) == (4, 0)         # the kernels of a 4-channel fp32 input ...
        # ... take the widths whose channel quads divide a block of 256 threads and whose weights fit 64 KB of LDS
        takes = family and Cout // 4 <= 256 and 256 % (Cout // 4) == 0 and Cout * taps * 16 <= 64 * 1024
        assert family or out_dt in (F32, dt), args
        if text.startswith("error"):
            assert text in ("error 1", "error 4"), (args, text)
            assert not family or bits & GN, (args, text)
            continue
        assert text.split()[0].startswith("cin4") == takes, (args, text)
        f = dict(kv.split("=") for kv in text.split()[1:])
        kernels.add(text.split()[0])
        ks, nblk = int(f["ks"]), int(f["stats"])
        assert ks >= 1 and (ks == 1 or bits & SLAB), (args, text)                  # K slices need the slab
        assert f["reduce"] == ("1" if ks > 1 else "0"), (args, text)
        assert f["gn"] == "1" or not bits & GN, (args, text)                       # never a kernel that would ignore the request
        assert nblk == 0 or (H * W) % nblk == 0, (args, text)
        assert f["issued"] in ("1/3", "1/2", "1", "3"), (args, text)
        if family:                                         # whole K whatever is offered; no kernel of theirs normalises on load
            kernel = text.split()[0]
            assert (ks, f["gn"], f["issued"]) == (1, "0", "1") and not bits & GN, (args, text)
            if not takes:                                  # refused: the flat kernel, whole K, no statistics
                assert text == "flat ks=1 reduce=0 stats=0 gn=0 issued=1 reads=-", (args, text)
            else:                                          # statistics: the matrix-core kernel's, or asked for
                assert (nblk > 0) == (kernel in ("cin4_mfma", "cin4_stats")) and (kernel != "cin4_stats" or bits & STATS), (args, text)
    assert kernels == {"head4", "head4_16", "smallm", "1x1_stream", "w2d", "f43", "f43_splitk", "halo", "halo_bf16x3",
                       "halo16", "pc16", "smallm16b", "flat", "flat_splitk", "flat16", "flat16_splitk", "cin4", "cin4_stats",
                       "cin4_mfma"}, kernels


# the weight pointers a kernel dereferences next to the packed fp32 weights, by kernel name ("smallm": computed from the shape)
READS = {"f43": {"wino"}, "f43_splitk": {"wino"}, "w2d": {"wino2"}, "1x1_stream": {"wsm"}, "halo_bf16x3": {"wq"},
         "halo16": {"wq"}, "flat16": {"wq"}, "flat16_splitk": {"wq"}, "pc16": {"wq", "wfrag"}, "smallm16b": {"wq", "wfrag"}}
NO_READS = ("head4", "head4_16", "halo", "flat", "flat_splitk", "cin4", "cin4_stats", "cin4_mfma")


def test_route_reads(answers):
    """`reads`, the weight copies the chosen kernel dereferences: for every query that has a route it is what the kernel's
    name says, and nothing the query did not offer.

    One exemption from "offered": the `wq` of a 16-bit input.  There the weights in the storage type are the conv's operand
    itself -- every 16-bit kernel but head4_16 reads them -- and conv_route has never looked at the WQ bit of such a query (the
    pinned answers of the "0" offers, which this change leaves untouched, name halo16 / flat16 with nothing offered).  For an
    fp32 input, where `wq` is an optional copy like the others, it has to be offered."""
    seen = set()
    for args, text in answers:
        dt, out_dt, B, H, W, C1, C2, Cout, taps, bits = args
        if text.startswith("error"):
            continue
        kernel = text.split()[0]
        f = dict(kv.split("=") for kv in text.split()[1:])
        names = [] if f["reads"] == "-" else f["reads"].split("+")
        reads = set(names)
        assert names == [n for n in ("wq", "wino", "wino2", "wsm", "wsm16", "wfrag") if n in reads], (args, text)   # one spelling per set
        if kernel == "smallm":                             # the 16 x 16-tile form: <= 256 pixels over the batch, whole 16-pixel blocks
            want = {"wsm16"} if B * H * W <= 256 and (H * W) % 16 == 0 else {"wsm"}
        elif kernel in NO_READS:
            want = set()
        else:
            want = READS[kernel]
        assert reads == want, (args, text)
        offered = {n for n, bit in (("wino", WINO), ("wino2", WINO2), ("wsm", WSM), ("wsm16", WSM), ("wfrag", WFRAG), ("wq", WQ))
                   if bits & bit}
        if dt != F32:
            offered.add("wq")
        assert reads <= offered, (args, text, sorted(offered))
        seen |= reads
    assert seen == {"wq", "wino", "wino2", "wsm", "wsm16", "wfrag"}, seen


def test_route_entry_is_declared_and_checks_its_arguments():
    import re
    from flowmse_amd import _lib
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "flowse_hip.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+flowse_op_conv_route\s*\(", header) and "flowse_op_conv_route" in _lib.SIGNATURES
    assert _lib.lib.flowse_abi_version() == 3 and re.search(r"#define\s+FLOWSE_ABI_VERSION\s+3\b", header)
    for i, name in enumerate(("WINO", "WINO2", "WSM", "WFRAG", "WQ", "WQ_SPLIT3", "WQ_F16", "SLAB", "GN", "BIAS2", "STATS", "FOLD")):
        assert re.search(r"\bFLOWSE_OFFER_%s\s*=\s*%d\b" % (name, 1 << i), header), name
    buf = ctypes.create_string_buffer(96)
    L = _lib.lib
    assert L.flowse_op_conv_route(0, 0, 1, 16, 16, 32, 0, 32, 9, 0, None, 96) == 1
    assert L.flowse_op_conv_route(0, 0, 1, 16, 16, 32, 0, 32, 9, 0, buf, 8) == 1
    assert L.flowse_op_conv_route(3, 0, 1, 16, 16, 32, 0, 32, 9, 0, buf, 96) == 1
    assert L.flowse_op_conv_route(0, 1, 1, 16, 16, 32, 0, 32, 9, 0, buf, 96) == 1
    assert L.flowse_op_conv_route(0, 0, 0, 16, 16, 32, 0, 32, 9, 0, buf, 96) == 1
    assert b"flowse_op_conv_route" in L.flowse_last_error()
    # launch_conv's shape checks answer as they do there
    for args in ((0, 0, 1, 16, 16, 30, 0, 32, 9, 0), (0, 0, 1, 16, 16, 32, 0, 32, 3, 0), (0, 0, 1, 16, 16, 32, 0, 34, 1, 0),
                 (0, 0, 4, 16384, 16384, 32, 0, 32, 1, 0)):
        assert ask(L, args) == "error 4", args
        assert L.flowse_last_error().startswith(b"conv: "), args


def _write():
    base = entries()
    secs = {"default": render_section(base)}
    for hook in HOOKS:
        secs[hook] = section(hook, base)
    text = "".join(f"[{name}]\n" + "".join(ln + "\n" for ln in lines) for name, lines in secs.items())
    with open(PINS, "w") as f:
        f.write(text)
    print(f"wrote {PINS}: {len(text)} bytes, {text.count(chr(10))} lines")


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    if sys.argv[1:] == ["--dump"]:
        print(repr(entries()))
    elif sys.argv[1:] == ["--write"]:
        _write()
    else:
        sys.exit("usage: python tests/test_conv_route_host.py --write")
