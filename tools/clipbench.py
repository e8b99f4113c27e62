#!/usr/bin/env python3
"""The gradient-clipped graph step against the default step ("Clipped step").

    python3 tools/clipbench.py [--out clip_bench.json]

VanillaVAE, InfoVAE and the ae_big Autoencoder at B = 64, bf16: the default (deferred) step, the same
step without deferral (TrainStep(defer_reductions=False)) and the clipped step (max_grad_norm = 0.8),
each a HIP graph, timed alternately between device events — 5 windows of 200 replays after 50
warm-up replays.  Then, on the clipped step's own buffers, back-to-back launches of vae_grad_sumsq,
of vae_adam_step and of the clipped pair."""
import argparse
import ctypes
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "pytorch-vae_amd")]

import torch  # noqa: E402

from vae_amd import _lib as L  # noqa: E402
from vae_amd import engine, models  # noqa: E402

B, M_N, LR, CLIP = 64, 2.5e-4, 0.005, 0.8
WARM, WINDOWS, REPLAYS = 50, 5, 200


def make(name):
    kw = dict(dtype=torch.bfloat16, device="cuda", seed=1265)
    if name == "vanilla":
        return models.VanillaVAE(3, 128, **kw), dict(device_eps=7)
    if name == "infovae":
        return (models.InfoVAE(3, 128, reg_weight=110, kernel_type="imq", alpha=-9.0, beta=10.5, **kw),
                dict(device_eps=7, device_prior=7))
    return models.Autoencoder(3, 128, hidden_dims=[128, 256, 512, 1024, 2048], **kw), {}


def build(name, variant):
    model, kw = make(name)
    if variant == "nodefer":
        real = engine.TrainStep
        engine.TrainStep = lambda *a, **k: real(*a, **dict(k, defer_reductions=False))
        try:
            step = model.fused_train_step(B, M_N, lr=LR, graph=True, **kw)
        finally:
            engine.TrainStep = real
    elif variant == "clip":
        step = model.fused_train_step(B, M_N, lr=LR, graph=True, max_grad_norm=CLIP, **kw)
    else:
        step = model.fused_train_step(B, M_N, lr=LR, graph=True, **kw)
    step.plan.x.uniform_()
    if getattr(step.plan, "prior", None) is not None and not step.device_prior:
        step.plan.prior.normal_()
    return model, step


def window(step, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        step()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / n


def ops(step):
    """Back-to-back launches on the step's own buffers: the sum of squares alone, Adam alone, clipped Adam."""
    net, g, fa = step.net, step.plan.grads, step.opt
    st = L.stream_ptr()
    plain = engine.FusedAdam(net, lr=LR, m=fa.m, v=fa.v)
    plain.step.fill_(5)
    n = net.params.numel()

    def sumsq():
        L.call("vae_grad_sumsq", n, g.data_ptr(), fa._partials.data_ptr(), ctypes.byref(fa._nparts), st)
    out = {"n": n, "parts": None}
    for tag, fn in (("sumsq", sumsq), ("adam", lambda: plain.apply(g, st, refresh_swaps=False)),
                    ("sumsq+adam_clip", lambda: fa.apply(g, st, refresh_swaps=False))):
        for _ in range(20):
            fn()
        w = [window(fn, 200) for _ in range(5)]
        out[tag] = {"median_us": statistics.median(w), "min_us": min(w), "max_us": max(w)}
    out["parts"] = fa._nparts.value
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="clip_bench.json")
    args = ap.parse_args()
    res = {}
    for name in ("vanilla", "infovae", "ae_big"):
        steps = {v: build(name, v) for v in ("default", "nodefer", "clip")}
        assert steps["default"][1].deferred and not steps["nodefer"][1].deferred and not steps["clip"][1].deferred
        for _, s in steps.values():
            for _ in range(WARM):
                s()
        torch.cuda.synchronize()
        t = {v: [] for v in steps}
        for _ in range(WINDOWS):
            for v, (_, s) in steps.items():
                t[v].append(window(s, REPLAYS))
        r = {v: {"median_us": statistics.median(w), "min_us": min(w), "max_us": max(w)} for v, w in t.items()}
        r["adam_split"] = steps["default"][1]._adam_split
        r["ops"] = ops(steps["clip"][1])
        res[name] = r
        print(name, json.dumps(r), flush=True)
        del steps
        torch.cuda.empty_cache()
    json.dump(res, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
