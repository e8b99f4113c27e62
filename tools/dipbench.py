"""Step time of the graph-replayed DIP-VAE step beside the VanillaVAE step (the same network, the
loss DIP-VAE's extends), on one build, in one process:

    python tools/dipbench.py [--batch 64] [--rounds 5] [--iters 400] [--out profiles/NAME.json]

Both steps are bf16 engine.TrainStep graphs with eps drawn on the device, as bench.py times the other
models; DIP-VAE takes configs/vae/dip_vae.yaml's parameters.  The two are timed alternately, `rounds`
windows of `iters` replays each between device events (a window is > 0.1 s), after warm-up replays
of both; the JSON carries every window, the medians and the spread, so a difference is read against
the noise.  DIP-VAE adds three launches per step over VanillaVAE: the two of vae_dip_fwd, and a
stand-alone vae_elbo_fwd (VanillaVAE's loss is evaluated inside the head backward).

    python tools/dipbench.py --trace-steps 20 --batch 64

runs only `trace-steps` DIP-VAE replays (plus warm-up) — the command to put behind
`rocprofv3 --kernel-trace --stats --` for the kernels' own durations."""
import argparse
import json
import os
import statistics
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "pytorch-vae_amd")]

YAML = dict(lambda_diag=0.05, lambda_offdiag=0.1)        # configs/vae/dip_vae.yaml
M_N = 1.0


def make_step(name, batch):
    from vae_amd.models import vae_models
    kw = YAML if name == "DIPVAE" else {}
    model = vae_models[name](3, 128, **kw, dtype=torch.bfloat16, device="cuda", seed=1265)
    step = model.fused_train_step(batch, M_N, lr=0.001, graph=True, device_eps=11)
    step.plan.x.copy_(torch.rand(step.plan.x.shape, generator=torch.Generator().manual_seed(3)))
    return model, step


def window(step, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        step()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters             # us per step


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=400)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--trace-steps", type=int, default=0)
    ap.add_argument("--out")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("dipbench: no GPU (a step time is only ever measured on one)")
    from vae_amd import _lib as L
    if a.trace_steps:
        _, step = make_step("DIPVAE", a.batch)
        for _ in range(a.warmup + a.trace_steps):
            step()
        torch.cuda.synchronize()
        print(f"traced {a.trace_steps} DIPVAE steps at B={a.batch} after {a.warmup} warm-up replays")
        return
    steps = {n: make_step(n, a.batch) for n in ("VanillaVAE", "DIPVAE")}
    for _, s in steps.values():
        for _ in range(a.warmup):
            s()
    torch.cuda.synchronize()
    times = {n: [] for n in steps}
    for _ in range(a.rounds):
        for n, (_, s) in steps.items():                   # alternate: both see the same machine state
            times[n].append(window(s, a.iters))
    props = torch.cuda.get_device_properties(0)
    dip = steps["DIPVAE"][1]
    res = {"tool": "dipbench", "batch": a.batch, "dtype": "bf16", "iters": a.iters, "rounds": a.rounds,
           "digest": L.load().vae_build_digest().decode(), "device": torch.cuda.get_device_name(0),
           "gcn_arch": getattr(props, "gcnArchName", None), "compute_units": props.multi_processor_count,
           "hbm_gib": round(props.total_memory / 2 ** 30, 1),
           "us_per_step": times,
           "median_us": {n: statistics.median(v) for n, v in times.items()},
           "spread_us": {n: max(v) - min(v) for n, v in times.items()},
           "launches": {n: len(s.plan.fwd_calls) + len(s.plan.bwd_calls) for n, (_, s) in steps.items()},
           "dipvae_terms": dip.loss_terms() + [dip.extra_term()[1]]}
    res["delta_us"] = res["median_us"]["DIPVAE"] - res["median_us"]["VanillaVAE"]
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
