"""Step time of the graph-replayed InfoVAE step beside the BetaVAE-H step (the same network, the
loss InfoVAE's extends), on one build, in one process:

    python tools/infobench.py [--batch 64] [--rounds 5] [--iters 400] [--out profiles/NAME.json]

Both steps are bf16 engine.TrainStep graphs with eps (and InfoVAE's prior) drawn on the device, as
bench.py times the other models.  The two are timed alternately, `rounds` windows of `iters`
replays each between device events (a window is > 0.1 s), after warm-up replays of both; the
JSON carries every window, the medians and the spread, so a difference is read against the noise.
InfoVAE adds two launches per step over BetaVAE-H: vae_mmd_fwd, and a stand-alone vae_elbo_fwd
(BetaVAE-H's loss is evaluated inside the head backward).

    python tools/infobench.py --trace-steps 20 --batch 64

runs only `trace-steps` InfoVAE replays (plus warm-up) — the command to put behind
`rocprofv3 --kernel-trace --stats --` for the kernels' own durations."""
import argparse
import json
import os
import statistics
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "pytorch-vae_amd")]

YAML = dict(alpha=-9.0, beta=10.5, reg_weight=110, kernel_type="imq")      # configs/vae/infovae.yaml
M_N = 2.5e-4


def make_step(name, batch):
    from vae_amd.models import vae_models
    kw = YAML if name == "InfoVAE" else dict(loss_type="H", beta=4)
    model = vae_models[name](3, 128, **kw, dtype=torch.bfloat16, device="cuda", seed=1265)
    step = model.fused_train_step(batch, M_N, lr=0.005, graph=True, device_eps=11,
                                  device_prior=11 if name == "InfoVAE" else None)
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
        raise SystemExit("infobench: no GPU (a step time is only ever measured on one)")
    from vae_amd import _lib as L
    if a.trace_steps:
        _, step = make_step("InfoVAE", a.batch)
        for _ in range(a.warmup + a.trace_steps):
            step()
        torch.cuda.synchronize()
        print(f"traced {a.trace_steps} InfoVAE steps at B={a.batch} after {a.warmup} warm-up replays")
        return
    steps = {n: make_step(n, a.batch) for n in ("BetaVAE", "InfoVAE")}
    for _, s in steps.values():
        for _ in range(a.warmup):
            s()
    torch.cuda.synchronize()
    times = {n: [] for n in steps}
    for _ in range(a.rounds):
        for n, (_, s) in steps.items():                   # alternate: both see the same machine state
            times[n].append(window(s, a.iters))
    props = torch.cuda.get_device_properties(0)
    res = {"tool": "infobench", "batch": a.batch, "dtype": "bf16", "iters": a.iters, "rounds": a.rounds,
           "digest": L.load().vae_build_digest().decode(), "device": torch.cuda.get_device_name(0),
           "gcn_arch": getattr(props, "gcnArchName", None), "compute_units": props.multi_processor_count,
           "hbm_gib": round(props.total_memory / 2 ** 30, 1),
           "us_per_step": times,
           "median_us": {n: statistics.median(v) for n, v in times.items()},
           "spread_us": {n: max(v) - min(v) for n, v in times.items()},
           "launches": {n: len(s.plan.fwd_calls) + len(s.plan.bwd_calls) for n, (_, s) in steps.items()},
           "infovae_terms": steps["InfoVAE"][1].loss_terms() + [steps["InfoVAE"][1].mmd_term()]}
    res["delta_us"] = res["median_us"]["InfoVAE"] - res["median_us"]["BetaVAE"]
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
