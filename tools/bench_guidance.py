"""Time ops.ltx_guidance against the reference guider's expressions run by eager torch on the same GPU.

    python tools/bench_guidance.py [--iters 200] [--warmup 20] [--json PATH]

Shapes: the working latent 1 x 128 x 33 x 22 x 38 and 1 x 128 x 65 x 34 x 60.  Modes: plain CFG, and APG with CFG-star, a norm threshold,
momentum, STG and the variance rescale.  The eager side restates _LTXSigmaAdvancedGuider.predict_noise between its model evaluations
(CFG-star, _apg with _project, STG, rescale) as the reference writes them; nothing is read from a reference checkout.  Device time by
events around `iters` calls after `warmup` calls of each side, the two sides alternating in blocks so that a drift of the clocks hits both;
launches of the fused side are the operator's own count, those of the eager side are counted by the profiler over one call.  Prints one
JSON line per (shape, mode); there is no CPU form: without a GPU the tool fails.
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
SHAPES = ((1, 128, 33, 22, 38), (1, 128, 65, 34, 60))
MODES = {"cfg": dict(cfg=4.0),
         "apg-all": dict(cfg=4.0, cfg_star=True, mode="APG", eta=-0.5, norm_threshold=5.0, momentum=0.25, stg_scale=1.0, rescale=0.7)}


def eager(p, n, q, average, cfg=1.0, cfg_star=False, mode="CFG", eta=1.0, norm_threshold=0.0, momentum=0.0, stg_scale=0.0, rescale=0.0):
    """the reference's expressions, op by op; returns (guided, new average)"""
    dims = [-1, -2, -3]
    if cfg_star:
        b = p.shape[0]
        pf, nf = p.reshape(b, -1), n.reshape(b, -1)
        alpha = torch.sum(pf * nf, dim=1, keepdim=True) / (torch.sum(nf.square(), dim=1, keepdim=True) + 1e-8)
        n = n * alpha.reshape(b, *([1] * (n.ndim - 1)))
    if mode == "APG":
        g = p - n
        if momentum != 0.0:
            average = g if average is None else momentum * average + g
            g = average
        if norm_threshold > 0:
            norm = g.norm(p=2, dim=dims, keepdim=True).clamp_min(1e-12)
            g = g * torch.minimum(torch.ones_like(norm), norm_threshold / norm)
        g64 = g.double()
        u = torch.nn.functional.normalize(p.double(), dim=dims)
        par64 = (g64 * u).sum(dim=dims, keepdim=True) * u
        par, orth = par64.to(g.dtype), (g64 - par64).to(g.dtype)
        guided = p + (cfg - 1.0) * (orth + eta * par)
    else:
        guided = p + (cfg - 1.0) * (p - n)
    if q is not None:
        guided = guided + stg_scale * (p - q)
    if rescale != 0.0:
        guided_std = guided.std().clamp_min(1e-12)
        guided = guided * (rescale * (p.std() / guided_std) + (1.0 - rescale))
    return guided, average


def timed(fn, iters):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) / iters


def eager_launches(fn):
    from torch.profiler import ProfilerActivity, profile
    fn()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return sum(e.count for e in prof.key_averages() if e.device_type == torch.autograd.DeviceType.CUDA)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--blocks", type=int, default=3)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_guidance: no GPU visible; a timing needs one")
    from conftest import load_package
    load_package()
    from comfyui_vrgamedevgirl_amd import ops
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    lines = []
    for shape in SHAPES:
        g = torch.Generator().manual_seed(7)
        p, n, q, avg = ((torch.rand(shape, generator=g) * 4.0 - 2.0).to(dev) for _ in range(4))
        for name, kw in MODES.items():
            full = name != "cfg"
            def fused():
                return ops.ltx_guidance(p, n, q if full else None, average=avg if full else None, **kw)

            def plain():
                return eager(p, n, q if full else None, avg if full else None, **kw)
            for _ in range(args.warmup):
                fused(), plain()
            torch.cuda.synchronize()
            a, b = fused().guided, plain()[0]
            difference = float((a.double() - b.double()).abs().max() / b.double().abs().max())
            fused_ms, eager_ms = [], []
            for _ in range(args.blocks):
                fused_ms.append(timed(fused, args.iters))
                eager_ms.append(timed(plain, args.iters))
            try:
                launches_eager = eager_launches(plain)
            except Exception as exc:                      # the profiler is optional: the timing stands without the count
                launches_eager = f"not measured ({type(exc).__name__})"
            elements = p.numel()
            tensors = (3 if full else 2) + (3 if full else 1)          # read once + written once, the least any implementation moves
            line = {"shape": list(shape), "mode": name, "device": torch.cuda.get_device_name(dev), "iters": args.iters, "blocks": args.blocks,
                    "fused_ms": min(fused_ms), "fused_ms_blocks": fused_ms, "eager_ms": min(eager_ms), "eager_ms_blocks": eager_ms,
                    "ratio_eager_over_fused": min(eager_ms) / min(fused_ms), "launches_fused": fused().launches,
                    "launches_eager": launches_eager, "max_rel_difference": difference,
                    "least_bytes": elements * 4 * tensors, "fused_least_bytes_per_s": elements * 4 * tensors / (min(fused_ms) * 1e-3)}
            print(json.dumps(line), flush=True)
            lines.append(line)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as fh:
            json.dump(lines, fh, indent=1)


if __name__ == "__main__":
    main()
