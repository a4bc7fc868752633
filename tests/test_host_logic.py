"""CPU: host-side logic, the C-ABI surface and the parameter-table contract (no GPU compute calls)."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import _cases as Cs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cabi_exports_every_declared_symbol():
    from flowmse_amd import _lib
    header = open(os.path.join(ROOT, "include", "flowse_hip.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    declared = set(re.findall(r"\b(flowse_[a-z0-9_]+)\s*\(", header))
    assert len(declared) >= 20
    for name in sorted(declared):
        assert hasattr(_lib.lib, name), f"{name} declared in flowse_hip.h but not exported"
    assert declared == set(_lib.SIGNATURES), declared ^ set(_lib.SIGNATURES)
    assert _lib.lib.flowse_abi_version() == 3
    assert _lib.lib.flowse_device_count() >= 0


@pytest.mark.parametrize("tag", ["tiny", "full"])
def test_param_table_matches_reference(tag):
    """Keys, shapes and parameters() order of the C-ABI table == the reference NCSNpp's state_dict."""
    from flowmse_amd.backbones.structure import param_table
    t = Cs.param_tables()[tag]
    names, shapes = param_table(t["cfg"])
    assert names == t["names"] == t["parameters_order"]
    assert shapes == t["shapes"]
    assert sum(int(np.prod(s)) for s in shapes) == t["n_params"]


def test_facade_state_dict_and_registry():
    from flowmse_amd.backbones import BackboneRegistry, NCSNpp
    from flowmse_amd.odes import ODERegistry
    from flowmse_amd.sampling import ODEsolverRegistry
    t = Cs.param_tables()["tiny"]
    assert BackboneRegistry.get_by_name("ncsnpp") is NCSNpp
    assert "flowmatching" in ODERegistry.get_all_names()
    assert "euler" in ODEsolverRegistry.get_all_names()
    with pytest.raises(ValueError):
        BackboneRegistry.get_by_name("dcunet")
    m = NCSNpp(**t["cfg"])
    sd = m.state_dict()
    assert list(sd.keys()) == t["names"]
    assert [list(v.shape) for v in sd.values()] == t["shapes"]
    assert [n for n, _ in m.named_parameters()] == t["parameters_order"]
    assert not dict(m.named_parameters())["all_modules.0.W"].requires_grad
    # reference init rules: init_scale=0 tensors ~1e-10 variance, zero biases
    assert float(sd["all_modules.4.Conv_1.weight"].abs().max()) < 1e-4
    assert float(sd["all_modules.4.Conv_0.bias"].abs().max()) == 0.0
    blob = m.canonical_blob()
    assert blob.numel() == t["n_params"]
    assert torch.equal(blob[:8], sd["output_layer.weight"].reshape(-1))
    # the cached parameter list follows a replaced parameter AND a replaced submodule (an orphaned owner must not
    # keep serving the old tensor): same identity scan as the upload's
    import copy
    new_out = copy.deepcopy(m.output_layer)
    with torch.no_grad():
        new_out.weight.fill_(0.25)
    m.output_layer = new_out
    assert m._params_in_order()[0] is new_out.weight and float(m.canonical_blob()[0]) == 0.25
    m.output_layer.weight = torch.nn.Parameter(torch.full_like(new_out.weight, 0.5))
    assert float(m.canonical_blob()[0]) == 0.5


def test_unsupported_configs_fail_loudly():
    from flowmse_amd.backbones import NCSNpp
    from flowmse_amd._lib import FlowseError
    with pytest.raises(NotImplementedError):
        NCSNpp(resblock_type="ddpm")
    with pytest.raises(NotImplementedError):
        NCSNpp(progressive="none")
    with pytest.raises(FlowseError):
        NCSNpp(nf=6)
    m = NCSNpp(nf=16, ch_mult=(1, 2), image_size=32)
    x = torch.zeros(1, 2, 32, 32, dtype=torch.complex64)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m(x, torch.ones(1))


def test_time_grid_matches_reference_rule():
    from flowmse_amd.sampling import time_grid
    g = Cs.gold("tiny_sampler")
    ts, steps = time_grid(1.0, 0.03, 5)
    assert np.array_equal(ts.numpy(), g["timesteps_N5"])
    assert np.array_equal(steps[:-1].numpy(), (ts[:-1] - ts[1:]).numpy())
    assert float(steps[-1]) == float(ts[-1])            # last step integrates to t = 0
    ts1, st1 = time_grid(1.0, 0.03, 1)
    assert float(ts1[0]) == 1.0 and float(st1[0]) == 1.0


def test_pad_spec():
    from flowmse_amd.util.other import pad_spec
    g = Cs.gold("op_pad_spec")
    Y = torch.zeros(1, 1, 256, 501, dtype=torch.complex64)
    assert list(pad_spec(Y).shape) == list(g["shape"])
    assert pad_spec(torch.zeros(1, 1, 256, 512)).shape[-1] == 512
    assert pad_spec(torch.zeros(1, 1, 256, 1)).shape[-1] == 64


def test_prior_sampling_cpu_semantics():
    from flowmse_amd.odes import FLOWMATCHING
    ode = FLOWMATCHING()
    y = torch.randn(2, 1, 4, 4, dtype=torch.complex64)
    z = torch.randn(2, 1, 4, 4, dtype=torch.complex64)
    x, z2 = ode.prior_sampling(y.shape, y, z)
    assert torch.allclose(x, y + z * 0.487) and z2 is z
    assert abs(ode.prior_std() - 0.487) < 1e-7
    assert float(ode._std(torch.tensor([0.5]))) == pytest.approx(0.2435)


def test_generic_white_box_solver_on_cpu_callable():
    """The plugin loop accepts any callable VF_fn (reference semantics), e.g. a closed-form field."""
    from flowmse_amd.odes import FLOWMATCHING
    from flowmse_amd.sampling import get_white_box_solver
    ode = FLOWMATCHING()
    Y = torch.ones(1, 1, 2, 2, dtype=torch.complex64)
    z = torch.zeros_like(Y)
    vf = lambda x, t, y: torch.ones_like(x)            # dx/dt = 1 -> x(0) = x(1) - 1
    x, n = get_white_box_solver("euler", ode, vf, Y=Y, N=7, z=z)()
    assert n == 7 and torch.allclose(x, torch.zeros_like(x), atol=1e-6)
    x, _ = get_white_box_solver("rk4", ode, vf, Y=Y, N=3, z=z)()
    assert torch.allclose(x, torch.zeros_like(x), atol=1e-6)


@pytest.mark.parametrize("solver", ["heun", "rk4"])
def test_higher_order_solvers_never_leave_the_field_domain(solver):
    """The field is only defined on [t_eps, T] (h / t and log t, ncsnpp.py:259,398): a solver must never query
    below t_eps.  dx/dt = x / t is singular at t = 0 (exact solution x(t) = x(1) t); the last step, which lands on
    t = 0, must be the reference's Euler step."""
    from flowmse_amd.odes import FLOWMATCHING
    from flowmse_amd.sampling import get_white_box_solver, time_grid
    from oracle import sampler_oracle as S
    ode = FLOWMATCHING()
    Y = torch.full((2, 1, 2, 2), 1.0 + 0.5j, dtype=torch.complex64)
    z = torch.zeros_like(Y)
    seen = []

    def vf(x, t, y):
        seen.append(float(t.min()))
        return x / t.reshape(-1, 1, 1, 1)

    N, t_eps = 4, 0.03
    x, n = get_white_box_solver(solver, ode, vf, Y=Y, N=N, z=z, t_eps=t_eps)()
    assert n == N and min(seen) >= t_eps - 1e-7, seen
    assert torch.isfinite(torch.view_as_real(x)).all()
    want = S.rk_sample(lambda xx, tt, yy: xx / tt.reshape(-1, 1, 1, 1), Y, z, tableau=solver, N=N, t_eps=t_eps)
    assert torch.allclose(x, want, rtol=1e-5, atol=1e-7)
    # interior steps integrate x / t almost exactly, the Euler step from t_eps lands on exactly 0 for this field
    assert float(x.abs().max()) < 1e-3
    ts, steps = time_grid(1.0, t_eps, N)
    assert float(steps[-1]) == float(ts[-1])


def test_ema_swap_semantics():
    """eval(no_ema=False) swaps the EMA shadow weights in, train() restores (model.py:92-103)."""
    from flowmse_amd.model import VFModel
    m = VFModel(nf=16, ch_mult=(1, 2), image_size=32)
    params = list(m.parameters())
    shadow = [torch.full_like(p, 0.25) for p in params if p.requires_grad]
    m.load_ema_shadow(shadow)
    w0 = params[0].detach().clone()
    m.eval()
    assert float(params[0].flatten()[0]) == 0.25
    m.train(True)
    assert torch.equal(params[0].detach(), w0)
    m.eval(no_ema=True)
    assert torch.equal(params[0].detach(), w0)
    with pytest.raises(ValueError):
        m.load_ema_shadow(shadow[:-1])


def test_shard_utterances_balance():
    from flowmse_amd.parallel import batches_by_length, shard_utterances
    lengths = [64 * k for k in [2, 10, 3, 3, 7, 5, 5, 8, 2, 9, 4, 6]]
    shards = shard_utterances(lengths, 4)
    assert sorted(i for s in shards for i in s) == list(range(len(lengths)))
    loads = [sum(lengths[i] for i in s) for s in shards]
    assert max(loads) - min(loads) <= max(lengths)
    assert shard_utterances([], 3) == [[], [], []]
    b = batches_by_length(shards[0], lengths, 2)
    assert all(len(ids) <= 2 and all(lengths[i] == T for i in ids) for T, ids in b)


def test_plan_shards_config3_partition():
    """BASELINE config[3]'s stand-in set dealt to 2 / 4 / 8 ranks (host only): every utterance exactly once, batches of one
    padded length (no promotion by default: results stay those of the per-utterance path), balanced modelled time, and
    well-filled batches -- the numbers DESIGN section 6 quotes and `bench.py --workload vbdmd --plan` prints."""
    import bench
    from flowmse_amd.parallel import plan_batches, plan_shards, plan_summary, shard_utterances, batches_by_length, batch_cost
    true_len = bench.vbdmd_lengths(bench.VBDMD_UTTS)
    padded = [((t + 63) // 64) * 64 for t in true_len]
    ideal = sum(p * (65.0 / 8 + 48.0) for p in padded) / 1e3
    for world in (1, 2, 4, 8):
        plan = plan_shards(padded, world, 8)
        assert sorted(i for b in plan for _, ids in b for i in ids) == list(range(len(padded)))
        assert all(len(ids) <= 8 and all(padded[i] == T for i in ids) for b in plan for T, ids in b)
        s = plan_summary(plan, padded, 8)
        assert s["promotion_padding_frames"] == 0
        assert s["model_time_imbalance_max_over_mean"] <= 1.01, s
        assert s["frame_imbalance_max_over_mean"] <= 1.01, s
        assert s["batch_fill"] >= 0.9, s
        # within 1.5 % of the all-batches-full bound, and never worse than round 3's deal-utterances-then-batch scheme
        makespan = max(r["model_ms"] for r in s["per_rank"])
        assert makespan <= 1.015 * ideal / world, (world, makespan, ideal / world)
        old = max(sum(batch_cost(T, len(ids)) for T, ids in batches_by_length(m, padded, 8)) / 1e3
                  for m in shard_utterances(padded, world))
        assert makespan <= old + 1e-6, (world, makespan, old)
    # degenerate sets: fewer batches than ranks get split, empty ranks are fine
    assert plan_shards([], 3, 8) == [[], [], []]
    assert plan_shards([64], 3, 8) == [[(64, [0])], [], []]
    two = plan_shards([128, 128, 128], 2, 8)
    assert sorted(len(ids) for b in two for _, ids in b) == [1, 2]
    # promotion (opt-in) only ever pads upwards and only merges when the cost model says so
    pr = plan_batches(range(4), [640, 128, 128, 64], 8, promote=True)
    assert all(max(([640, 128, 128, 64][i]) for i in ids) == T for T, ids in pr)
    assert (640, [0]) in pr                                  # 512 frames of padding per member: never worth it
    assert plan_batches(range(3), [192, 128, 128], 8, promote=True) == [(192, [0, 1, 2])]
    assert plan_batches(range(3), [192, 128, 128], 8) == [(192, [0]), (128, [1, 2])]


def test_bench_dump_outputs(tmp_path):
    """bench.py --dump-outputs: float32 .npy per array (complex as its real view); above the size cap a seeded sample
    that is the same in every run and keeps the whole under the cap."""
    import bench
    x = torch.view_as_complex(torch.arange(2 * 3 * 4 * 2, dtype=torch.float32).reshape(2, 3, 4, 2))
    info = bench.dump_outputs(str(tmp_path / "a"), {"enhanced": x})
    got = np.load(tmp_path / "a" / "enhanced.npy")
    assert got.dtype == np.float32 and got.shape == (2, 3, 4, 2) and info["enhanced"]["sampled_elements"] is None
    assert np.array_equal(got, torch.view_as_real(x).numpy())
    big = {"u": torch.linspace(-1, 1, 50000, dtype=torch.float64), "v": torch.ones(30000)}
    cap = 64 * 1024
    i1 = bench.dump_outputs(str(tmp_path / "b"), big, max_bytes=cap)
    i2 = bench.dump_outputs(str(tmp_path / "c"), big, max_bytes=cap)
    assert i1 == i2 and i1["u"]["sampled_elements"] and i1["v"]["sampled_elements"]
    files = [tmp_path / d / (n + ".npy") for d in "bc" for n in "uv"]
    assert sum(os.path.getsize(f) for f in files[:2]) <= cap
    for n in "uv":
        a, b = np.load(tmp_path / "b" / (n + ".npy")), np.load(tmp_path / "c" / (n + ".npy"))
        assert a.dtype == np.float32 and np.array_equal(a, b)
    u = np.load(tmp_path / "b" / "u.npy")
    assert np.all(np.diff(u) > 0) and np.isin(u, big["u"].float().numpy()).all()    # sorted indices into the array


def test_bench_options():
    """--full and --dump-outputs exist; --steps sets the timed steps and must be at least one (checked before any GPU
    work)."""
    import subprocess
    import sys
    h = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--help"], capture_output=True, text=True,
                       timeout=120)
    assert h.returncode == 0 and "--full" in h.stdout and "--dump-outputs" in h.stdout
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "0"], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 2 and "--steps" in r.stderr


def test_gather_staging_buffer_is_reused_not_aliased():
    """Rank 0's host staging of the final gather (parallel._acquire_stage): two consecutive gathers reuse ONE buffer
    (no per-call allocation / page-locking) -- unless a result of the first is still alive, which must never be aliased."""
    from flowmse_amd import parallel as P
    P._STAGE_POOL.clear()
    a = P._acquire_stage(1000)
    res1 = [torch.view_as_complex(a[:64].view(4, 8, 2))]           # what gather_spectrograms hands out: views
    b = P._acquire_stage(900)
    assert b is not a and P.stage_pool_stats()[0] == 2             # first result alive: a second buffer
    del res1
    c = P._acquire_stage(900)
    assert (c is a or c is b) and P.stage_pool_stats()[0] == 2     # released: reused, nothing new allocated
    del b, c
    d = P._acquire_stage(1000)
    assert d is a                                                  # the larger free buffer serves it
    e_id = id(d)
    del d
    assert id(P._acquire_stage(10)) == e_id
    P._STAGE_POOL.clear()


def test_gather_staging_pool_is_capped():
    """A caller that held several result sets alive at once leaves several buffers behind: once they are unreferenced the pool
    drops all but _STAGE_POOL_MAX of them (the largest), and without torch's storage use count nothing is pooled at all."""
    from flowmse_amd import parallel as P
    P._STAGE_POOL.clear()
    held = []
    for n in (100, 200, 300, 400):
        buf = P._acquire_stage(n)
        held.append(buf[:8].view(2, 4))                            # a live result per call: four buffers
        del buf
    assert P.stage_pool_stats()[0] == 4
    del held
    x = P._acquire_stage(50)
    assert P.stage_pool_stats()[0] <= P._STAGE_POOL_MAX and x.numel() >= 400      # the largest one serves, the rest is gone
    del x
    saved = getattr(torch._C, "_storage_Use_Count")
    try:
        del torch._C._storage_Use_Count                            # "the private API moved"
        n0 = P.stage_pool_stats()[0]
        y, z = P._acquire_stage(10), P._acquire_stage(10)
        assert y is not z and P.stage_pool_stats()[0] == n0        # fresh buffers, never pooled
    finally:
        torch._C._storage_Use_Count = saved
    P._STAGE_POOL.clear()


def test_fused_sampler_only_for_classes_that_opt_in_themselves():
    """A plugin that subclasses a built-in solver and overrides update_fn must go through the plugin loop (its update_fn
    is what runs); only the built-in classes themselves map to the library's fused loop."""
    from flowmse_amd.sampling import ODEsolverRegistry, _fused_tableau, get_white_box_solver
    from flowmse_amd.sampling.odesolvers import EulerODEsolver, HeunODEsolver, RK4ODEsolver
    from flowmse_amd.odes import FLOWMATCHING
    assert (_fused_tableau(EulerODEsolver), _fused_tableau(HeunODEsolver), _fused_tableau(RK4ODEsolver)) == \
        ("euler", "heun", "rk4")

    class Doubling(EulerODEsolver):
        calls = 0

        def update_fn(self, x, t, y, stepsize, *args):
            type(self).calls += 1
            return x * 2

    class Inheriting(RK4ODEsolver):
        pass

    assert _fused_tableau(Doubling) is None and _fused_tableau(Inheriting) is None
    name = "_doubling_test"
    ODEsolverRegistry.register(name)(Doubling)
    try:

        class Field:                                  # looks like a HIP-backed model: has rk_sample_
            def rk_sample_(self, *a):
                raise AssertionError("fused loop taken for a subclass with its own update_fn")

            def __call__(self, x, t, y):
                return x

        y = torch.ones(1, 1, 4, 64, dtype=torch.complex64)
        x, n = get_white_box_solver(name, FLOWMATCHING(), Field(), y, N=3, z=torch.zeros_like(y))()
        assert Doubling.calls == 3 and n == 3 and torch.allclose(x, y * 8)
    finally:
        ODEsolverRegistry._registry.pop(name, None)


def test_spec_transform_roundtrip():
    from flowmse_amd.data_module import SpecTransform
    st = SpecTransform()
    sig = torch.randn(1, 16000)
    S = st.stft(sig)
    assert S.shape[1] == 256
    back = st.spec_back(st.spec_fwd(S))
    assert torch.allclose(back, S, atol=1e-4, rtol=1e-3)
    assert torch.allclose(st.istft(S, 16000), sig, atol=1e-4)


def test_black_box_solver_closed_form():
    """scipy RK45 wrapper (reference sampling/__init__.py:64-114): dx/dt = x integrates to x(t_eps) = x(1) e^{t_eps-1}."""
    from flowmse_amd.odes import FLOWMATCHING
    from flowmse_amd.sampling import get_black_box_solver
    ode = FLOWMATCHING()
    y = torch.ones(1, 1, 2, 3, dtype=torch.complex64) * (1 + 2j)
    z = torch.zeros_like(y)
    x, nfe = get_black_box_solver(ode, lambda x, t, yy: x, y, T_rev=1.0, t_eps=0.03, device="cpu", z=z)()
    assert nfe > 0 and x.dtype == torch.complex64
    assert torch.allclose(x, y * float(np.exp(0.03 - 1.0)), rtol=1e-4)


def test_config0_cpu_plumbing_with_oracle_field():
    """BASELINE config[0]: one synthetic 4 s utterance (256 bins, 501 -> 512 frames), N=1 Euler step, the whole
    evaluate.py flow (normalise -> STFT -> spec_fwd -> pad_spec -> sampler -> spec_back -> iSTFT) on CPU, with the
    oracle vector field of a tiny-width full-height net standing in for the checkpoint."""
    from flowmse_amd.evaluate import enhance_waveform, energy_ratios
    from flowmse_amd.model import VFModel
    from flowmse_amd.backbones.structure import param_table
    from oracle import ncsnpp_oracle as O
    cfg = dict(nf=8, ch_mult=(1, 1, 1, 1, 1, 1, 1), num_res_blocks=1, attn_resolutions=(16,), image_size=256)
    names, shapes = param_table(cfg)
    w = Cs.synth_weights(names, shapes)
    ocfg = O.make_cfg(**cfg)
    host = VFModel(nf=8, ch_mult=(1, 1, 1, 1, 1, 1, 1), num_res_blocks=1, image_size=256)   # spec transforms + ode only
    sig = torch.from_numpy(Cs.synth.normal(3, 9, (1, 64000), 0.1))
    z = None
    torch.manual_seed(0)
    out = enhance_waveform(host, sig, N=1, VF_fn=lambda x, t, y: O.vf_forward(w, ocfg, x, t, y), device="cpu")
    assert out.shape == (64000,) and np.isfinite(out).all()
    r = energy_ratios(out + 1e-3, sig[0].numpy(), sig[0].numpy() * 0.1 + 1e-3)
    assert all(np.isfinite(v) for v in r)


def _valid_set(tmp_path, n, seconds=1.0):
    """n clean/noisy wav pairs on disk + the data_module.valid_set view evaluate_model reads."""
    import types
    from scipy.io import wavfile
    from flowmse_amd.evaluate import _synthetic_pairs
    clean, noisy = [], []
    for name, c, y in _synthetic_pairs(n, seconds=seconds):
        for kind, sig, lst in (("clean", c, clean), ("noisy", y, noisy)):
            path = str(tmp_path / f"{kind}_{name}")
            wavfile.write(path, 16000, sig)
            lst.append(path)
    return types.SimpleNamespace(clean_files=clean, noisy_files=noisy)


def test_evaluate_model_hook_cpu(tmp_path):
    """util/inference.py:15-71 contract: picks files uniformly, returns (pesq, si_sdr, estoi) means; with a zero
    vector field and sigma -> 0 the 'enhanced' signal is the noisy one, so SI-SDR equals the mixture's."""
    from flowmse_amd.model import VFModel
    from flowmse_amd.util.inference import evaluate_model
    from flowmse_amd.util.other import read_wav, si_sdr
    host = VFModel(nf=8, ch_mult=(1, 1, 1, 1, 1, 1, 1), num_res_blocks=1, image_size=256, sigma_min=0.0, sigma_max=1e-6)
    host.data_module.valid_set = _valid_set(tmp_path, 4)
    p, s, e = evaluate_model(host, 2, inference_N=3, VF_fn=lambda x, t, y: torch.zeros_like(x))
    vs = host.data_module.valid_set
    want = np.mean([si_sdr(read_wav(vs.clean_files[i])[0][0].numpy(), read_wav(vs.noisy_files[i])[0][0].numpy())
                    for i in (0, 3)])
    assert abs(s - want) < 0.05, (s, want)
    assert np.isnan(p) or np.isfinite(p)
    assert np.isnan(e) or np.isfinite(e)


def test_spec_transform_matches_reference_golden():
    """STFT / spec_fwd / spec_back / iSTFT against the reference's SpecsDataModule (tests/golden/op_spec.npz)."""
    from flowmse_amd.data_module import SpecTransform
    g = Cs.gold("op_spec")
    st = SpecTransform()
    sig = torch.from_numpy(Cs.synth.normal(5, 8, (1, 4000), 0.1))
    S = st.stft(sig)
    assert S.shape == tuple(g["stft"].shape) and S.shape[1] == 256
    assert Cs.rel_l2(S, g["stft"]) < 1e-6
    Sf = st.spec_fwd(S)
    assert Cs.rel_l2(Sf, g["fwd"]) < 1e-6
    assert Cs.rel_l2(st.spec_back(Sf), g["back"]) < 1e-5
    assert Cs.rel_l2(st.istft(st.spec_back(Sf), 4000), g["istft"]) < 1e-5


def test_product_never_imports_the_oracle():
    """The oracle is test infrastructure: nothing under flowmse_amd/ (the product) may import or execute it."""
    import ast
    pkg = os.path.join(ROOT, "flowmse_amd")
    offenders = []
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if not f.endswith(".py"):
                continue
            path = os.path.join(dirpath, f)
            tree = ast.parse(open(path).read())
            for node in ast.walk(tree):
                names = []
                if isinstance(node, ast.Import):
                    names = [a.name for a in node.names]
                elif isinstance(node, ast.ImportFrom):
                    names = [node.module or ""]
                if any(n == "oracle" or n.startswith("oracle.") for n in names):
                    offenders.append(path)
    assert not offenders, offenders
    for f in os.listdir(os.path.join(pkg, "csrc")):
        assert "oracle" not in open(os.path.join(pkg, "csrc", f), errors="ignore").read()


def test_missing_library_fails_loudly(tmp_path):
    """Without libflowse_hip.so the package refuses to import (no silent CPU / PyTorch fallback)."""
    import subprocess
    import sys
    code = ("import importlib.util, sys, os\n"
            "spec = importlib.util.spec_from_file_location('lib_copy', sys.argv[1])\n"
            "m = importlib.util.module_from_spec(spec)\n"
            "try:\n    spec.loader.exec_module(m)\nexcept ImportError as e:\n    print('IMPORTERROR', e); sys.exit(0)\n"
            "sys.exit(1)\n")
    src = open(os.path.join(ROOT, "flowmse_amd", "_lib.py")).read()
    copy = tmp_path / "_lib_copy.py"
    copy.write_text(src)                      # same module, but its directory holds no .so
    r = subprocess.run([sys.executable, "-c", code, str(copy)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "IMPORTERROR" in r.stdout and "no CPU fallback" in r.stdout, r.stdout + r.stderr


def test_graft_entry_build_passes():
    """The driver's build check (`__graft_entry__.build()`): compiles (a no-op when the in-tree library is current) and
    asserts the loaded library's ABI version against include/flowse_hip.h -- a stale literal there would fail every round's
    build check while all other tests stay green."""
    import __graft_entry__ as g
    g.build()
