"""Step time of the graph-replayed MIWAE step (M x K = 3 x 5, configs/vae/miwae.yaml) beside the IWAE
step at S = 15 — the same rows through every kernel but the one-workgroup loss — on one build, in one
process:

    python tools/miwaebench.py [--batch 64] [--rounds 5] [--iters 400] [--out profiles/NAME.json]

Both steps are bf16 engine.TrainStep graphs with eps drawn on the device, as bench.py times the other
models.  The two are timed alternately, `rounds` windows of `iters` replays each between device events
(a window is > 0.1 s), after warm-up replays of both; the JSON carries every window, the medians and
the spread, so a difference is read against the noise.  After the steps, each plan's vae_elbo_fwd is
called alone, `elbo-iters` calls back to back between device events on the step's own buffers: the
time of one call of the loss launch in a full queue (the kernel's own duration is the tracer's).

    python tools/miwaebench.py --only IWAE

times one model alone; with VAE_HIP_LIB naming another build of the library (vae_amd/_lib.py) that is
the IWAE step of that build, for a comparison across builds and the run-to-run spread.

    python tools/miwaebench.py --trace-steps 20 --batch 64

runs only `trace-steps` MIWAE replays (plus warm-up) — the command to put behind
`rocprofv3 --kernel-trace --stats --` for the kernels' own durations."""
import argparse
import ctypes
import json
import os
import statistics
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "pytorch-vae_amd")]

M, K = 3, 5                                              # configs/vae/miwae.yaml
M_N = 1e-8
CTOR = {"IWAE": dict(num_samples=M * K), "MIWAE": dict(num_samples=K, num_estimates=M)}


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
    ap.add_argument("--elbo-iters", type=int, default=20000)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--only", choices=sorted(CTOR))
    ap.add_argument("--trace-steps", type=int, default=0)
    ap.add_argument("--out")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("miwaebench: no GPU (a step time is only ever measured on one)")
    from vae_amd import _lib as L
    if a.trace_steps:
        _, step = make_step("MIWAE", a.batch)
        for _ in range(a.warmup + a.trace_steps):
            step()
        torch.cuda.synchronize()
        print(f"traced {a.trace_steps} MIWAE steps at B={a.batch} after {a.warmup} warm-up replays")
        return
    steps = {n: make_step(n, a.batch) for n in ([a.only] if a.only else ["IWAE", "MIWAE"])}
    for _, s in steps.values():
        for _ in range(a.warmup):
            s()
    torch.cuda.synchronize()
    times = {n: [] for n in steps}
    for _ in range(a.rounds):
        for n, (_, s) in steps.items():                   # alternate: both see the same machine state
            times[n].append(window(s, a.iters))
    terms = {n: s.loss_terms() for n, (_, s) in steps.items()}
    # the loss launch alone, on the last step's SSE and mu | log_var (its outputs are rewritten in place)
    elbo = {n: [] for n in steps}
    st = L.stream_ptr()
    for _ in range(a.rounds):
        for n, (_, s) in steps.items():
            e = s.plan.elbo_args
            elbo[n].append(window(lambda: L.call("vae_elbo_fwd", ctypes.byref(e), st), a.elbo_iters))
    props = torch.cuda.get_device_properties(0)
    res = {"tool": "miwaebench", "batch": a.batch, "rows": a.batch * M * K, "dtype": "bf16", "iters": a.iters,
           "rounds": a.rounds, "elbo_iters": a.elbo_iters, "library": os.path.basename(L.LIB_PATH),
           "digest": L.load().vae_build_digest().decode(), "device": torch.cuda.get_device_name(0),
           "gcn_arch": getattr(props, "gcnArchName", None), "compute_units": props.multi_processor_count,
           "hbm_gib": round(props.total_memory / 2 ** 30, 1),
           "us_per_step": times,
           "median_us": {n: statistics.median(v) for n, v in times.items()},
           "spread_us": {n: max(v) - min(v) for n, v in times.items()},
           "elbo_call_us": elbo,
           "elbo_call_median_us": {n: statistics.median(v) for n, v in elbo.items()},
           "launches": {n: len(s.plan.fwd_calls) + len(s.plan.bwd_calls) for n, (_, s) in steps.items()},
           "terms": terms}
    if not a.only:
        res["delta_us"] = res["median_us"]["MIWAE"] - res["median_us"]["IWAE"]
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
