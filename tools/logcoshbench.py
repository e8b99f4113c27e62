"""Step time of the graph-replayed LogCoshVAE step (configs/vae/logcosh_vae.yaml: alpha 10, beta 1)
beside the VanillaVAE step — the same network, the loss on vae_logcosh_loss instead of inside the head
backward — on one build, in one process:

    python tools/logcoshbench.py [--batch 64] [--rounds 5] [--iters 400] [--out profiles/NAME.json]

Both steps are bf16 engine.TrainStep graphs with eps drawn on the device, as bench.py times the other
models.  The two are timed alternately, `rounds` windows of `iters` replays each between device events
(a window is > 0.1 s), after warm-up replays of both; the JSON carries every window, the medians and
the spread, so a difference is read against the noise.  After the steps, the LogCoshVAE plan's
vae_logcosh_loss is called alone, `loss-iters` calls back to back between device events on the step's
own buffers: the time of one call (two launches) in a full queue — the kernels' own durations are the
tracer's.  `loss_bytes` is the algorithmic traffic of the streaming launch, from the shapes: recon and
target read, grad written; `loss_call_gbps` that over the call's time (a lower bound of the streaming
launch's own rate: the call's time includes the one-workgroup second launch).

    python tools/logcoshbench.py --trace-steps 20 --batch 64

runs only `trace-steps` LogCoshVAE replays (plus warm-up) — the command to put behind
`rocprofv3 --kernel-trace --stats --` for the kernels' own durations."""
import argparse
import json
import os
import statistics
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "pytorch-vae_amd")]

M_N = 0.00025                                            # configs/vae/logcosh_vae.yaml
CTOR = {"VanillaVAE": dict(), "LogCoshVAE": dict(alpha=10.0, beta=1.0)}


def make_step(name, batch):
    from vae_amd.models import vae_models
    model = vae_models[name](3, 128, **CTOR[name], dtype=torch.bfloat16, device="cuda", seed=1265)
    step = model.fused_train_step(batch, M_N, lr=0.005, graph=True, device_eps=11)
    step.plan.x.copy_(torch.rand(step.plan.x.shape, generator=torch.Generator().manual_seed(3)))
    return model, step


def window(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters             # us per call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=400)
    ap.add_argument("--loss-iters", type=int, default=20000)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--only", choices=sorted(CTOR))
    ap.add_argument("--trace-steps", type=int, default=0)
    ap.add_argument("--out")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("logcoshbench: no GPU (a step time is only ever measured on one)")
    from vae_amd import _lib as L
    if a.trace_steps:
        _, step = make_step("LogCoshVAE", a.batch)
        for _ in range(a.warmup + a.trace_steps):
            step()
        torch.cuda.synchronize()
        print(f"traced {a.trace_steps} LogCoshVAE steps at B={a.batch} after {a.warmup} warm-up replays")
        return
    steps = {n: make_step(n, a.batch) for n in ([a.only] if a.only else ["VanillaVAE", "LogCoshVAE"])}
    for _, s in steps.values():
        for _ in range(a.warmup):
            s()
    torch.cuda.synchronize()
    times = {n: [] for n in steps}
    for _ in range(a.rounds):
        for n, (_, s) in steps.items():                   # alternate: both see the same machine state
            times[n].append(window(s, a.iters))
    terms = {n: s.loss_terms() for n, (_, s) in steps.items()}
    props = torch.cuda.get_device_properties(0)
    res = {"tool": "logcoshbench", "batch": a.batch, "dtype": "bf16", "iters": a.iters, "rounds": a.rounds,
           "loss_iters": a.loss_iters, "library": os.path.basename(L.LIB_PATH),
           "digest": L.load().vae_build_digest().decode(), "device": torch.cuda.get_device_name(0),
           "gcn_arch": getattr(props, "gcnArchName", None), "compute_units": props.multi_processor_count,
           "hbm_gib": round(props.total_memory / 2 ** 30, 1),
           "us_per_step": times,
           "median_us": {n: statistics.median(v) for n, v in times.items()},
           "spread_us": {n: max(v) - min(v) for n, v in times.items()},
           "launches": {n: len(s.plan.fwd_calls) + len(s.plan.bwd_calls) for n, (_, s) in steps.items()},
           "terms": terms}
    if "LogCoshVAE" in steps:
        # the loss call alone, on the last step's recon / x / mu | log_var (its outputs are rewritten in place)
        plan = steps["LogCoshVAE"][1].plan
        arg = next(ref for fn, ref in plan.fwd_calls if fn == "vae_logcosh_loss")
        st = L.stream_ptr()
        calls = [window(lambda: L.call("vae_logcosh_loss", arg, st), a.loss_iters) for _ in range(a.rounds)]
        loss_bytes = 3 * plan.recon.numel() * 4           # recon + target read, grad written (fp32)
        res.update(loss_call_us=calls, loss_call_median_us=statistics.median(calls), loss_bytes=loss_bytes,
                   loss_workgroups=L.logcosh_workspace(arg._obj) // 8,
                   loss_call_gbps=loss_bytes / (statistics.median(calls) * 1e-6) / 1e9)
    if not a.only:
        res["delta_us"] = res["median_us"]["LogCoshVAE"] - res["median_us"]["VanillaVAE"]
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
