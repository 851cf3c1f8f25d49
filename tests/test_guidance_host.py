"""The LTX Sigma Advanced guider without a GPU: csrc/vrg_guidance_math.hpp compiled for the host against torch run live (fp32 and the fp64
truth), the schedules, the index lookup and the fp32 contract against the reference's own functions, the node's surface and control flow
with stub seams, the operator's refusals and the host side of the ABI."""
import ast
import ctypes as C
import importlib
import json
import math
import os
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

import guidance_support as S
from conftest import GOLDEN, PKG_NAME, ROOT

REFERENCE_FILE = os.path.join(os.environ.get("VRGDG_REFERENCE_ROOT", "/root/reference"), "CustomLTXNodes.py")
needs_reference = pytest.mark.skipif(not os.path.isfile(REFERENCE_FILE), reason="no reference checkout")
SCHEDULE_FUNCTIONS = ("_sigma_tensor", "_interpolation_factor", "_build_transition_values", "_runtime_schedule_offset",
                      "_current_transition_index", "_schedule_index")


@pytest.fixture(scope="module")
def ops(pkg):
    from comfyui_vrgamedevgirl_amd import _hip, build_ext, ops
    if not os.path.exists(_hip.LIB_PATH):
        build_ext.build(verbose=False)
    return ops


@pytest.fixture(scope="module")
def host(ops, tmp_path_factory):
    from comfyui_vrgamedevgirl_amd import _hip
    return S.build_host_lib(tmp_path_factory.mktemp("guidance_host"), _hip.GuidanceDesc)


@pytest.fixture(scope="module")
def results(tmp_path_factory):
    return S.torch_results(S.CASES, tmp_path_factory.mktemp("guidance_torch"))


@pytest.fixture()
def node(pkg):
    return importlib.import_module(PKG_NAME + ".CustomLTXNodes")


@pytest.fixture(scope="module")
def reference():
    """the reference's schedule functions and its guider class (without its ComfyUI base), taken from its source by the AST and executed"""
    with open(REFERENCE_FILE, encoding="utf-8") as fh:
        tree = ast.parse(fh.read(), filename=REFERENCE_FILE)
    body = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name in SCHEDULE_FUNCTIONS]
    for n in tree.body:
        if isinstance(n, ast.ClassDef) and n.name in ("_LTXSigmaAdvancedGuider", "VRGDGLTXSigmaAdvancedGuider"):
            n.bases = []
            body.append(n)
    ns = {"torch": torch, "math": math}
    exec(compile(ast.Module(body=body, type_ignores=[]), REFERENCE_FILE, "exec"), ns)
    return types.SimpleNamespace(**{k: v for k, v in ns.items() if not k.startswith("__")})


def test_span_constant(ops):
    from comfyui_vrgamedevgirl_amd import _hip
    text = open(os.path.join(ROOT, "include", "vrgdg_hip.h")).read()
    assert f"#define VRG_GUIDANCE_SPAN {S.SPAN}\n" in text and _hip.GUIDANCE_SPAN == S.SPAN == ops.GUIDANCE_SPAN


# ---- the header against torch ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("i", range(len(S.CASES)), ids=[c["name"] for c in S.CASES])
def test_header_reproduces_the_truth(ops, host, results, i):
    """every output of every step: bit for bit where there is no reduction, within the bar elsewhere"""
    c = S.CASES[i]
    average = None
    for step, (p, n, q) in enumerate(results.latents(i)):
        p, n, q = (None if t is None else S.guidance_view(c, w, t).numpy() for w, t in (("positive", p), ("negative", n), ("perturbed", q)))
        got = S.host_step(host, ops, c, p, n, q, average)
        average = got["average"]
        for name in S.OUTPUTS:
            fp32, truth = results.part(i, "fp32", step, name), results.part(i, "truth", step, name)
            assert (got[name] is None) == (truth is None), (c["name"], step, name)
            if truth is None:
                continue
            if S.is_exact(c):
                assert np.array_equal(got[name].view(np.uint32), fp32.view(np.uint32)), (c["name"], step, name)
            e_kernel, e_ref = S.error(got[name], truth), S.error(fp32, truth)
            print(f"{c['name']} step {step} {name}: E_header {e_kernel:.3e} E_ref {e_ref:.3e}")
            assert e_kernel <= S.bar(e_ref), (c["name"], step, name, e_kernel, e_ref)


def test_the_cases_reach_what_they_are_for(results):
    """fp32 torch is off the truth by a finite, nonzero amount wherever there is a reduction; the degenerate inputs hit their clamps"""
    by_name = {c["name"]: i for i, c in enumerate(S.CASES)}
    for i, c in enumerate(S.CASES):
        if S.is_exact(c) or c["special"]:
            continue
        if c["shape"] == [3, 1, 1, 1] and c["mode"] == "APG" and c["eta"] == 0.0 and c["rescale"] == 0.0:
            continue                    # a row of one element is parallel to itself: orth is exactly 0 and guided is p, in any arithmetic
        for step in range(c["steps"]):
            e = S.error(results.part(i, "fp32", step, "guided"), results.part(i, "truth", step, "guided"))
            assert math.isfinite(e) and 0.0 < e < 1e-4, (c["name"], step, e)
    i = by_name["zero-negative/star"]
    assert not results.part(i, "truth", 0, "negative").any() and np.isfinite(results.part(i, "truth", 0, "guided")).all()
    i = by_name["constant-guided/rescale"]
    p, _, q = results.latents(i)[0]
    assert float((p + 1.0 * (p - q)).std()) == 0.0 and float(p.std()) > 0.5
    assert np.abs(results.part(i, "truth", 0, "guided")).max() > 1e10                        # std(guided) clamped to 1e-12
    i = by_name["zero-positive-row/apg"]
    p, n, _ = results.latents(i)[0]
    row = results.part(i, "truth", 0, "guided")[1, 2]                     # normalize's eps: u = 0, nothing is parallel, guided = 3 * g'
    assert not p[1, 2].any() and np.isfinite(row).all() and row.any()
    i = by_name["zero-guidance-row/apg"]
    p, n, _ = results.latents(i)[0]
    assert torch.equal(p[0, 1], n[0, 1]) and np.array_equal(results.part(i, "truth", 0, "guided")[0, 1], p[0, 1].double().numpy())
    # the thresholds cut some rows and leave others
    for name, thr in (("rows70/apg-threshold", 5.0), ("rows128/apg-threshold", 5.0)):
        p, n, _ = results.latents(by_name[name])[0]
        norms = (p - n).norm(p=2, dim=[-1, -2, -3]).flatten()
        assert (norms > thr).any() and (norms < thr).any(), name


def test_moments_merge_like_one_pass_and_a_constant_has_none(host):
    rng = np.random.default_rng(5)
    x = (rng.standard_normal(10000) * 3.0 + 100.0).astype(np.float32).astype(np.float64)
    parts = []
    for chunk in np.array_split(x, 37):
        d = chunk - chunk[0]
        parts.append([chunk.size, chunk[0], d.sum(), (d * d).sum()])
    out = np.zeros(3)
    host.hm_gd_merge(np.ascontiguousarray(parts, dtype=np.float64), len(parts), out)
    assert out[0] == x.size and abs(out[1] - x.mean()) < 1e-12 * 100 and abs(out[2] - ((x - x.mean()) ** 2).sum()) < 1e-11 * out[2]
    constant = [[n, 0.3, 0.0, 0.0] for n in (4096, 1, 70)] + [[0, 0.0, 0.0, 0.0]]
    host.hm_gd_merge(np.ascontiguousarray(constant, dtype=np.float64), len(constant), out)
    assert out[0] == 4167 and out[1] == 0.3 and out[2] == 0.0


# ---- the reference's own functions -----------------------------------------------------------------------------------------------------------

SIGMAS = [1.0, 0.99375, 0.9875, 0.98125, 0.975, 0.909375, 0.725, 0.421875, 0.0]


@needs_reference
def test_schedules_equal_the_reference(node, reference):
    percents = (0.0, 0.1, 0.25, 0.5, 0.75, 0.99, 1.0)
    for sigmas in (SIGMAS, SIGMAS[:2], torch.linspace(1.0, 0.0, 31), np.linspace(14.6, 0.03, 12)):
        for interpolation in ("linear", "ease_in", "ease_out"):
            for start in percents:
                for end in percents:
                    for a, b, outside in ((4.0, 1.5, 1.0), (0.0, 1.0, 0.0), (1.0, 0.0, None), (0.7, 0.7, 0.0)):
                        args = (sigmas, a, b, interpolation, start, end)
                        if start > end:
                            with pytest.raises(ValueError) as mine:
                                node._build_transition_values(*args, outside_value=outside)
                            with pytest.raises(ValueError) as theirs:
                                reference._build_transition_values(*args, outside_value=outside)
                            assert str(mine.value) == str(theirs.value)
                            continue
                        got, want = node._build_transition_values(*args, outside_value=outside), reference._build_transition_values(*args, outside_value=outside)
                        assert torch.equal(got[0], want[0]) and got[0].dtype == want[0].dtype and got[1] == want[1], (args, outside)
    for bad, kw in (([1.0], {}), ([1.0, float("nan")], {}), (SIGMAS, {"interpolation": "cubic"})):
        args = (bad, 1.0, 2.0, kw.get("interpolation", "linear"), 0.0, 1.0)
        with pytest.raises(ValueError) as mine:
            node._build_transition_values(*args, outside_value=1.0)
        with pytest.raises(ValueError) as theirs:
            reference._build_transition_values(*args, outside_value=1.0)
        assert str(mine.value) == str(theirs.value)


@needs_reference
def test_index_lookup_equals_the_reference_on_its_three_routes(node, reference):
    """split sigma ranges (the runtime schedule is a contiguous part of the connected one) x timesteps that match a sigma exactly, lie
    inside an interval, or lie outside every interval (nearest)"""
    full = torch.tensor(SIGMAS, dtype=torch.float32)
    routes = set()
    for lo, hi in ((0, 9), (0, 5), (4, 9), (2, 4), (7, 9)):
        runtime = full[lo:hi]
        steps = [float(v) for v in runtime] + [float(v) * (1 + 5e-6) for v in runtime[:-1]]                          # exact (within isclose)
        steps += [float((runtime[k] + runtime[k + 1]) / 2) for k in range(len(runtime) - 1)]                          # inside an interval
        steps += [float(runtime[0]) + 0.5, float(runtime[-1]) - 0.25, 7.0]                                             # outside: nearest
        for t in steps:
            for timestep in (t, torch.tensor([t, 0.5]), torch.tensor([[t]], dtype=torch.float64)):
                got, want = node._schedule_index(SIGMAS, runtime, timestep), reference._schedule_index(SIGMAS, runtime, timestep)
                assert got == want, (lo, hi, t)
                assert node._current_transition_index(runtime, timestep) == reference._current_transition_index(runtime, timestep)
            inside = float(runtime.min()) <= t <= float(runtime.max())
            exact = bool(torch.isclose(runtime[:-1].double(), torch.tensor(t, dtype=torch.float64), rtol=1e-5, atol=1e-7).any())
            routes.add("exact" if exact else "interval" if inside else "nearest")
    assert routes == {"exact", "interval", "nearest"}
    for runtime in ([0.5, 0.25], SIGMAS + [0.0], [1.0, 0.9875]):
        with pytest.raises(ValueError) as mine:
            node._runtime_schedule_offset(SIGMAS, runtime)
        with pytest.raises(ValueError) as theirs:
            reference._runtime_schedule_offset(SIGMAS, runtime)
        assert str(mine.value) == str(theirs.value)


@needs_reference
def test_the_fp32_contract_equals_the_reference_bit_for_bit(reference):
    """guidance_contract -- what the child runs -- against _cfg_star_negative, _project and _apg of the reference's guider, same process,
    same CPU kernels"""
    cls = reference._LTXSigmaAdvancedGuider
    checked = set()
    for c in S.CASES:
        if not c["negative"]:
            continue
        guider = object.__new__(cls)
        guider.apg_momentum, guider.apg_norm_threshold, guider.apg_eta = c["momentum"], c["threshold"], c["eta"]
        guider.apg_running_average, guider.previous_sigma = None, None
        plain = dict(c, stg=None, rescale=0.0)                      # STG and the rescale are inline in predict_noise: compared below
        average = None
        for step, (p, n, q) in enumerate(S.guidance_latents(c)):
            p, n = S.guidance_view(c, "positive", p), S.guidance_view(c, "negative", n)
            mine = S.guidance_contract(plain, p, n, None, average)
            average = mine.get("average")
            theirs_n = cls._cfg_star_negative(p, n) if c["star"] else n
            if c["star"]:
                assert torch.equal(mine["negative"], theirs_n), c["name"]
                checked.add("star")
            if c["mode"] == "APG":
                theirs = guider._apg(p, theirs_n, c["cfg"], torch.tensor([1.0 - 0.1 * step]))
                assert torch.equal(mine["guided"], theirs), (c["name"], step)
                if c["momentum"] != 0.0:
                    assert torch.equal(mine["average"], guider.apg_running_average), (c["name"], step)
                    checked.add("momentum")
                par, orth = cls._project(p - theirs_n, p)
                assert par.dtype == torch.float32 and torch.equal(par + orth, orth + par)
                checked.add("apg")
            else:
                assert torch.equal(mine["guided"], p + (c["cfg"] - 1.0) * (p - theirs_n)), c["name"]
    assert checked == {"star", "apg", "momentum"}


# ---- the node --------------------------------------------------------------------------------------------------------------------------------

def _fixture():
    with open(os.path.join(GOLDEN, "guider_surface.json")) as fh:
        return json.load(fh)


def test_surface_equals_the_fixture(node, pkg):
    want = _fixture()
    cls = getattr(node, want["class"])
    assert json.loads(json.dumps(cls.INPUT_TYPES())) == want["INPUT_TYPES"]
    assert list(cls.INPUT_TYPES()["required"]) == list(want["INPUT_TYPES"]["required"])
    assert [list(cls.RETURN_TYPES), list(cls.RETURN_NAMES), cls.FUNCTION, cls.CATEGORY, cls.DESCRIPTION] == \
        [want["RETURN_TYPES"], want["RETURN_NAMES"], want["FUNCTION"], want["CATEGORY"], want["DESCRIPTION"]]
    assert node.NODE_CLASS_MAPPINGS == {want["key"]: cls}
    assert node.NODE_DISPLAY_NAME_MAPPINGS == {want["key"]: want["display_name"]}
    assert want["key"] not in pkg.NODE_CLASS_MAPPINGS and want["key"] not in pkg.NODE_DISPLAY_NAME_MAPPINGS      # the pinned package surface


@needs_reference
def test_the_fixture_equals_the_reference(reference):
    want = _fixture()
    cls = getattr(reference, want["class"])
    assert json.loads(json.dumps(cls.INPUT_TYPES())) == want["INPUT_TYPES"]
    assert [list(cls.RETURN_TYPES), list(cls.RETURN_NAMES), cls.FUNCTION, cls.CATEGORY, cls.DESCRIPTION] == \
        [want["RETURN_TYPES"], want["RETURN_NAMES"], want["FUNCTION"], want["CATEGORY"], want["DESCRIPTION"]]


def test_module_imports_without_comfyui(pkg):
    code = ("import sys; sys.path.insert(0, %r); import conftest; conftest.load_package(); import importlib; "
            "m = importlib.import_module(conftest.PKG_NAME + '.CustomLTXNodes'); "
            "assert not [n for n in sys.modules if n.split('.')[0] in ('comfy', 'comfy_extras', 'folder_paths')]; "
            "assert len(m.NODE_CLASS_MAPPINGS) == 1 and callable(m.comfy_samplers) and callable(m.ltx_stg_module)") % os.path.join(ROOT, "tests")
    ran = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True)
    assert ran.returncode == 0, ran.stderr


class Seams:
    """stub comfy.samplers and ComfyUI-LTXVideo stg: count the model evaluations, note the perturbation flags each one saw"""

    def __init__(self, shape=(1, 2, 1, 2, 3), fail_perturbed=False):
        self.calls, self.shape, self.fail_perturbed, self.patches = [], shape, fail_perturbed, []
        seams = self

        class CFGGuider:
            def __init__(self, model):
                self.inner_model, self.conds = model, {}

            def inner_set_conds(self, conds):
                self.conds = dict(conds)

        class STGFlag:
            def __init__(self, do_skip, skip_layers):
                self.do_skip, self.skip_layers = do_skip, skip_layers
                seams.flag = self

        class STGGuider:
            @staticmethod
            def get_transformer_blocks(model):
                return ["block"] * 24

        self.samplers = types.SimpleNamespace(CFGGuider=CFGGuider, calc_cond_batch=self.calc_cond_batch)
        self.stg = types.SimpleNamespace(STGFlag=STGFlag, STGGuider=STGGuider, STGBlockWrapper=lambda block, flag, index: (block, index))

    def calc_cond_batch(self, model, conds, x, timestep, model_options):
        kind = "perturbed" if self.flag.do_skip else conds[0]
        self.calls.append((kind, model_options["transformer_options"].get("ptb_index")))
        if kind == "perturbed" and self.fail_perturbed:
            raise RuntimeError("the perturbed evaluation failed")
        g = torch.Generator().manual_seed(len(self.calls))
        return [torch.randn(self.shape, generator=g)]

    def model(self):
        seams = self

        class Model:
            def clone(self):
                return self

            def set_model_patch_replace(self, patch, *where):
                seams.patches.append(where)
        return Model()


def _stub_operator(ops, log):
    """ops.ltx_guidance on the CPU: the contract in plain torch (there is no GPU here), with the operator's keywords recorded"""
    def ltx_guidance(positive, negative=None, perturbed=None, **kw):
        log.append(dict(kw, has_negative=negative is not None, has_perturbed=perturbed is not None))
        c = {"star": kw["cfg_star"], "mode": kw["mode"], "cfg": kw["cfg"], "eta": kw["eta"], "threshold": kw["norm_threshold"],
             "momentum": kw["momentum"], "stg": kw["stg_scale"], "rescale": kw["rescale"]}
        out = S.guidance_contract(c, positive, negative, perturbed, kw["average"])
        return ops.GuidanceResult(out["guided"], out.get("negative") if kw["want_negative"] else None, out.get("average"))
    return ltx_guidance


def _guider(node, seams, monkeypatch, ops, log, **kw):
    monkeypatch.setattr(node, "comfy_samplers", lambda: seams.samplers)
    monkeypatch.setattr(node, "ltx_stg_module", lambda: seams.stg)
    monkeypatch.setattr(node, "ops", types.SimpleNamespace(ltx_guidance=_stub_operator(ops, log)))
    args = dict(model=seams.model(), positive="P", negative="N", sigmas=SIGMAS, cfg_start=4.0, cfg_end=4.0, stg_start=1.0, stg_end=1.0,
                rescale_start=0.7, rescale_end=0.7, interpolation="linear", start_percent=0.0, end_percent=1.0, stg_blocks="14, 19",
                guidance_mode="CFG", cfg_star=False, apg_eta=1.0, apg_norm_threshold=5.0, apg_momentum=0.0)
    args.update(kw)
    (guider,) = node.VRGDGLTXSigmaAdvancedGuider().get_guider(**args)
    return guider


def _options(**extra):
    return dict({"transformer_options": {"sample_sigmas": torch.tensor(SIGMAS)}}, **extra)


def test_guider_control_flow_with_stub_seams(node, ops, monkeypatch):
    x = torch.zeros(1, 2, 1, 2, 3)
    # every evaluation; the hook dictionary
    seams, log, seen = Seams(), [], []
    guider = _guider(node, seams, monkeypatch, ops, log, cfg_star=True)
    assert isinstance(guider, seams.samplers.CFGGuider) and guider.raw_conds == ("P", "N") and guider.conds == {"positive": "P", "negative": "N"}
    assert len(seams.patches) == 24 and seams.flag.skip_layers == [14, 19]
    options = _options(sampler_post_cfg_function=[lambda args: seen.append(args) or args["denoised"] + 1.0])
    out = guider.predict_noise(x, torch.tensor([1.0]), options)
    assert seams.calls == [("P", None), ("N", None), ("perturbed", 0)]
    assert seams.flag.do_skip is False and "ptb_index" not in options["transformer_options"]
    assert sorted(seen[0]) == sorted(["denoised", "cond", "uncond", "model", "uncond_denoised", "cond_denoised", "sigma", "model_options", "input",
                                      "perturbed_cond", "perturbed_cond_denoised"])
    assert log[0]["want_negative"] and log[0]["cfg"] == 4.0 and log[0]["stg_scale"] == 1.0 and log[0]["rescale"] == 0.7 and log[0]["mode"] == "CFG"
    assert torch.equal(out, seen[0]["denoised"] + 1.0) and seen[0]["cond"] == "P" and seen[0]["uncond"] == "N" and seen[0]["input"] is x
    assert not torch.equal(seen[0]["uncond_denoised"], seen[0]["cond_denoised"])                # the CFG-star negative, not positive
    # cfg == 1: no negative evaluation; stg == 0: no perturbed one; the hook then sees positive in their places
    seams, log, seen = Seams(), [], []
    guider = _guider(node, seams, monkeypatch, ops, log, cfg_start=1.0, cfg_end=1.0, stg_start=0.0, stg_end=0.0, guidance_mode="APG")
    out = guider.predict_noise(x, torch.tensor([0.975]), _options(sampler_post_cfg_function=[lambda args: seen.append(args) or args["denoised"]]))
    assert seams.calls == [("P", None)] and not log[0]["has_negative"] and not log[0]["has_perturbed"] and log[0]["mode"] == "CFG"
    assert seen[0]["uncond_denoised"] is seen[0]["cond_denoised"] is seen[0]["perturbed_cond_denoised"]
    # outside the window cfg is 1 and stg / rescale are 0
    seams, log = Seams(), []
    guider = _guider(node, seams, monkeypatch, ops, log, start_percent=0.5, end_percent=1.0)
    guider.predict_noise(x, torch.tensor([1.0]), _options())
    assert seams.calls == [("P", None)] and log[0]["rescale"] == 0.0
    # an exception in the perturbed evaluation leaves the flags as they were
    seams, log = Seams(fail_perturbed=True), []
    guider = _guider(node, seams, monkeypatch, ops, log)
    options = _options()
    with pytest.raises(RuntimeError, match="perturbed evaluation failed"):
        guider.predict_noise(x, torch.tensor([1.0]), options)
    assert seams.flag.do_skip is False and "ptb_index" not in options["transformer_options"] and not log
    # texts
    with pytest.raises(ValueError, match="could not find the sampler sigma schedule"):
        guider.predict_noise(x, torch.tensor([1.0]), {})
    for kw, text in ((dict(stg_blocks="14, x"), "stg_blocks must be comma-separated integers"),
                     (dict(stg_blocks=" "), "At least one stg_blocks index is required when STG is active"),
                     (dict(stg_blocks="3, 24"), r"stg_blocks contains invalid indices \[24\]; this LTX model has 24 transformer blocks")):
        with pytest.raises(ValueError, match=text):
            _guider(node, Seams(), monkeypatch, ops, [], **kw)


def test_the_running_average_is_fed_back_and_forgotten_when_sigma_rises(node, ops, monkeypatch):
    x = torch.zeros(1, 2, 1, 2, 3)
    seams, log = Seams(), []
    guider = _guider(node, seams, monkeypatch, ops, log, guidance_mode="APG", apg_momentum=-0.5, stg_start=0.0, stg_end=0.0)
    for sigma in (1.0, 0.99375, 0.9875, 1.0, 0.99375):
        guider.predict_noise(x, torch.tensor([sigma]), _options())
    assert [entry["average"] is None for entry in log] == [True, False, False, True, False]
    assert all(entry["mode"] == "APG" and entry["momentum"] == -0.5 for entry in log)
    assert guider.apg_running_average is not None and guider.previous_sigma == pytest.approx(0.99375)
    # without a momentum nothing is kept
    seams, log = Seams(), []
    guider = _guider(node, seams, monkeypatch, ops, log, guidance_mode="APG", stg_start=0.0, stg_end=0.0)
    guider.predict_noise(x, torch.tensor([1.0]), _options())
    assert guider.apg_running_average is None


# ---- the operator's refusals and the host side of the ABI --------------------------------------------------------------------------------------

def test_operator_refusals_name_the_argument(ops):
    p = torch.zeros(2, 3, 2, 5, 7)
    for kw, text in ((dict(positive=p.double()), "positive must be float32"),
                     (dict(positive=p, negative=p.half()), "negative must be float32"),
                     (dict(positive=p, perturbed=p.to(torch.int32)), "perturbed must be float32"),
                     (dict(positive=p[0, 0]), "positive must have 4 or 5 dimensions, got 3"),
                     (dict(positive=p[None]), "positive must have 4 or 5 dimensions, got 6"),
                     (dict(positive=p, negative=p[:1]), "negative is shaped"),
                     (dict(positive=p, negative=p, average=p[:, :2], mode="APG", momentum=0.5), "average is shaped"),
                     (dict(positive=p, negative=torch.zeros(p.shape, device="meta")), "negative lives on meta, positive on cpu"),
                     (dict(positive=p, perturbed=torch.zeros(p.shape, device="meta")), "perturbed lives on meta"),
                     (dict(positive=torch.zeros(1, 1, 1, 1), rescale=0.5), "fewer than two elements"),
                     (dict(positive=p, negative=p, mode="PAG"), "mode must be one of"),
                     (dict(positive=torch.zeros(0, 3, 2, 5, 7)), "positive is empty"),
                     (dict(positive="p"), "positive must be a tensor"),
                     (dict(positive=p), "positive lives on cpu")):                       # no CPU form
        with pytest.raises(ValueError, match=text):
            ops.ltx_guidance(**kw)
    assert ops.ltx_guidance.__wrapped__ is not None                                     # wrapped in _on_device like the other operators


def test_record_and_host_checks(ops, host):
    from comfyui_vrgamedevgirl_amd import _hip
    lib = _hip.host_library()
    d = ops.guidance_desc((1, 128, 33, 22, 38), has_negative=True, has_perturbed=True, cfg=4.0, stg_scale=1.0, rescale=0.7, cfg_star=True,
                          mode="APG", eta=-0.5, norm_threshold=5.0, momentum=0.1, has_average=True, want_negative=True)
    assert (d.rows, d.row_len, d.batch) == (128, 33 * 22 * 38, 1) and d.mode == _hip.GUIDANCE_APG
    assert [d.has_negative, d.has_perturbed, d.cfg_star, d.has_average, d.has_momentum, d.has_threshold, d.has_rescale, d.want_negative] == [1] * 8
    # Python doubles, rounded to fp32 once
    assert d.cfg_m1 == 3.0 and d.rescale == np.float32(0.7) and d.one_minus_rescale == np.float32(1.0 - 0.7) and d.momentum == np.float32(0.1)
    segments = -(-d.row_len // S.SPAN)
    want = 128 * segments * 64 + 128 * 8 + 8 + 128 * 4 + 8
    assert lib.vrg_guidance_scratch_bytes(C.byref(d)) == want == host.hm_gd_scratch_bytes(C.byref(d))
    assert lib.vrg_guidance_check(C.byref(d)) == 0 == host.hm_gd_check(C.byref(d))
    # flags that say nothing without a negative or outside APG are dropped by the operator's record ...
    d0 = ops.guidance_desc((3, 1, 1, 1), has_negative=False, has_perturbed=False, cfg_star=True, mode="APG", momentum=0.5, norm_threshold=2.0,
                           want_negative=True, has_average=True)
    assert [d0.cfg_star, d0.has_average, d0.has_momentum, d0.has_threshold, d0.want_negative] == [0] * 5
    # ... and refused by the library where a caller sets them all the same
    def refused(**fields):
        bad = _hip.GuidanceDesc.from_buffer_copy(d)
        for k, v in fields.items():
            setattr(bad, k, v)
        rc = lib.vrg_guidance_check(C.byref(bad))
        assert rc == host.hm_gd_check(C.byref(bad)) and lib.vrg_guidance_scratch_bytes(C.byref(bad)) == 0
        return rc
    for fields in (dict(rows=0), dict(row_len=0), dict(batch=3), dict(mode=2), dict(cfg_star=2), dict(has_negative=0), dict(mode=0),
                   dict(has_momentum=0), dict(threshold=0.0), dict(threshold=float("nan")), dict(rows=1, row_len=1, batch=1)):
        assert refused(**fields) == 1, fields
    assert refused(rows=1 << 41, batch=1) == 2
    # every entry point checks the record, the scratch buffer and its operands before it touches a device
    one, two, null = C.c_void_p(1 << 20), C.c_void_p(1 << 30), C.c_void_p(0)
    size = lib.vrg_guidance_scratch_bytes(C.byref(d))
    scratch = C.c_void_p(1 << 40)
    assert lib.vrg_guidance_sums_f32(one, two, C.byref(d), null, size, null) == 1                         # no scratch buffer
    assert lib.vrg_guidance_sums_f32(one, two, C.byref(d), scratch, size - 1, null) == 1                  # too small
    assert lib.vrg_guidance_sums_f32(one, two, C.byref(d), C.c_void_p((1 << 40) + 4), size, null) == 1    # off the 8-byte grid
    assert lib.vrg_guidance_sums_f32(null, two, C.byref(d), scratch, size, null) == 1
    assert lib.vrg_guidance_rows_f32(one, two, null, null, C.byref(d), scratch, size, null) == 1           # the record has an average
    assert lib.vrg_guidance_rows_f32(one, two, C.c_void_p(1 << 32), one, C.byref(d), scratch, size, null) == 1    # average_out overlaps positive
    assert lib.vrg_guidance_combine_f32(one, two, null, null, C.c_void_p(1 << 33), null, C.byref(d), scratch, size, null) == 1   # operands missing
    assert lib.vrg_guidance_rescale_f32(C.c_void_p((1 << 20) + 2), C.byref(d), scratch, size, null) == 1   # off the 4-byte grid
    plain = ops.guidance_desc((2, 3, 2, 5, 7), has_negative=True, has_perturbed=False, cfg=4.0)
    size = lib.vrg_guidance_scratch_bytes(C.byref(plain))
    assert lib.vrg_guidance_sums_f32(one, two, C.byref(plain), scratch, size, null) == 1                  # no star: no such phase
    assert lib.vrg_guidance_rescale_f32(one, C.byref(plain), scratch, size, null) == 1
    assert lib.vrg_guidance_combine_f32(one, two, null, null, one, null, C.byref(plain), scratch, size, null) == 1      # guided == positive
