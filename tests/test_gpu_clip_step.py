"""Gradient-norm clipping inside the fused training step (engine.TrainStep on
FusedAdam(max_grad_norm=...), model.fused_train_step(..., max_grad_norm=v)): eager launches, the
one-graph replay and the bucketed exchange routes all clip by the global norm of the complete
gradient and leave plan.grads unclipped.

The mirror is teacher-forced: after each step the step's own (unclipped) gradient buffer goes through
clip_grad_norm_ + torch.optim.Adam in fp64 on the CPU (clip_ref), started from the same parameters."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

import clip_ref as R

pytestmark = pytest.mark.gpu

SEED, M_N, LR = 1265, 2.5e-4, 0.005


def _model(dtype):
    from vae_amd.models import VanillaVAE
    return VanillaVAE(3, 128, dtype=dtype, device="cuda", seed=SEED)


def _inputs(B):
    g = torch.Generator().manual_seed(SEED + B)
    return torch.rand(B, 3, 64, 64, generator=g).cuda(), torch.randn(B, 128, generator=g).cuda()


def _unclipped_norm(dtype, B):
    """The gradient norm of the first step as the parent's engine computes it (no clipping, the
    non-deferred route)."""
    from vae_amd.engine import FusedAdam, TrainStep
    from vae_amd.net import StepPlan
    model = _model(dtype)
    plan = StepPlan(model.net, B, kld_weight=M_N)
    step = TrainStep(model.net, plan, FusedAdam(model.net, lr=LR), graph=False, defer_reductions=False)
    step(*_inputs(B))
    torch.cuda.synchronize()
    return float(plan.grads.double().norm())


def _run(dtype, B, v, graph, steps):
    model = _model(dtype)
    p0 = model.net.params.clone()
    step = model.fused_train_step(B, M_N, lr=LR, graph=graph, max_grad_norm=v)
    assert not step.deferred and step.opt.max_grad_norm is not None
    assert step.plan.grads.numel() == model.net.params.numel()
    x, eps = _inputs(B)
    rec = []
    for _ in range(steps):
        step(x, eps)
        torch.cuda.synchronize()
        rec.append(dict(G=step.plan.grads.clone(), p=model.net.params.clone(), m=step.opt.m.clone(),
                        v=step.opt.v.clone(), norm=step.opt.grad_norm.clone()))
    return p0, rec, step


def _check_against_mirror(p0, rec, v, moments=True):
    want, bars = R.trajectory(p0, [r["G"] for r in rec], v, lr=LR), R.BARS
    for k, (r, (p, m, mv, norm, coef)) in enumerate(zip(rec, want)):
        dp = float((r["p"].cpu().double() - p).abs().max())
        dm = float((r["m"].cpu().double() - m).abs().max() / m.abs().max())
        dv = float((r["v"].cpu().double() - mv).abs().max() / mv.abs().max())
        gn, gc = r["norm"].tolist()
        print(f"step {k}: |dp| {dp:.3e} |dm|/max {dm:.3e} |dv|/max {dv:.3e} norm {gn:.9g} vs {norm:.12g} "
              f"coef {gc:.9g}")
        assert dp <= bars[0], (k, dp, bars)
        if moments:
            assert dm <= bars[1] and dv <= bars[2], (k, dm, dv, bars)
        assert abs(gn - norm) <= 2.0 ** -23 * norm, (k, gn, norm)
        # coef = fp32(fp32(v) / fp32(norm + 1e-6)): four roundings of 2^-24 each; twice that allowed
        assert abs(gc - coef) <= 4 * 2.0 ** -23 * coef, (k, gc, coef)
    assert rec[0]["norm"][1] < 1.0                     # v is half the first step's norm: clipping is active


def test_clipped_step_eager_and_graph_match_the_fp64_mirror_and_each_other():
    """Default VanillaVAE net, fp32, B = 4, three steps with v = half the first step's unclipped norm.
    Bars: clip_ref.BARS (those of test_gpu_adam.py, held against fp64), the norm to one fp32 rounding.
    Measured on an MI355X, worst step: parameters 1.7e-7, moments 6.1e-8 and 1.7e-7 of their maximum."""
    B = 4
    v = 0.5 * _unclipped_norm(torch.float32, B)
    runs = {}
    for graph in (False, True):
        p0, rec, step = _run(torch.float32, B, v, graph, 3)
        _check_against_mirror(p0, rec, v)
        runs[graph] = rec
        if graph:
            # the threshold is a device scalar: a new value needs no new capture
            g = step.graphs[0]
            step.opt.set_max_grad_norm(1e30)
            step(*_inputs(B))
            torch.cuda.synchronize()
            assert step.graphs[0] is g and float(step.opt.grad_norm[1]) == 1.0
    for k, (a, b) in enumerate(zip(runs[False], runs[True])):
        for key in ("G", "p", "m", "v", "norm"):
            assert torch.equal(a[key], b[key]), (k, key)


def test_clipped_bf16_step_updates_the_fp32_master_parameters():
    """bf16 throughput mode, B = 8, graph replay: the update arithmetic is fp32 whatever the dtype, so
    the fp32 master parameters follow the fp64 mirror of the step's own gradients."""
    B = 8
    v = 0.5 * _unclipped_norm(torch.bfloat16, B)
    p0, rec, step = _run(torch.bfloat16, B, v, True, 3)
    _check_against_mirror(p0, rec, v, moments=False)
    assert torch.equal(step.net.lowp, step.net.params.to(torch.bfloat16))


def test_constructor_keeps_deferral_without_a_threshold():
    from vae_amd.engine import FusedAdam
    model = _model(torch.bfloat16)
    assert model.fused_train_step(4, M_N, lr=LR, graph=False).deferred
    model = _model(torch.bfloat16)
    step = model.fused_train_step(4, M_N, lr=LR, graph=False, max_grad_norm=1.0)
    assert not step.deferred and step._adam_split == 0
    with pytest.raises(ValueError):
        FusedAdam(model.net, lr=LR, max_grad_norm=0)


# ------------------------------------------------------------------ the bucketed routes, world size 1
def _port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _bucketed(B, v, force, graph_comm):
    from vae_amd.engine import FusedAdam, TrainStep
    from vae_amd.net import StepPlan
    model = _model(torch.float32)
    plan = StepPlan(model.net, B, kld_weight=M_N)
    step = TrainStep(model.net, plan, FusedAdam(model.net, lr=LR, max_grad_norm=v), graph=True, nbuckets=2,
                     force_buckets=force, graph_comm=graph_comm)
    assert step.graph_comm == graph_comm and (step.comm is not None) == force and not step.deferred
    x, eps = _inputs(B)
    norms = []
    for _ in range(2):
        step(x, eps)
        norms.append(step.opt.grad_norm.cpu().numpy())
    return model.net.params.cpu().numpy(), np.stack(norms), len(step.buckets)


def _worker(port, q):
    try:
        import torch.distributed as dist
        os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        torch.cuda.set_device(0)
        dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda:0"))
        B, v = 4, 1.6             # (the first step's norm at these seeds is 3.24: asserted clipped below)
        out = [_bucketed(B, v, False, False), _bucketed(B, v, True, True), _bucketed(B, v, True, False)]
        dist.barrier()
        dist.destroy_process_group()
        q.put(out)
    except Exception:
        import traceback
        q.put(traceback.format_exc())


def test_bucketed_routes_clip_like_the_one_rank_step():
    """force_buckets at world size 1 over RCCL (as tests/test_gpu_zz_rccl.py): the norm launch sits
    behind the last bucket's all-reduce, in the one captured graph and on the host-issued path alike.
    After two clipped steps the parameters are bit-identical to the plain one-rank clipped step's —
    the fp32 parity mode's guarantee, now with the clip in it."""
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    p = ctx.Process(target=_worker, args=(_port(), q))
    p.start()
    out = q.get(timeout=240)
    p.join(timeout=60)
    assert not isinstance(out, str), out
    (p_one, n_one, _), (p_graph, n_graph, nb), (p_host, n_host, _) = out
    assert nb >= 2 and float(n_one[0][1]) < 1.0             # (the first step is clipped)
    assert np.array_equal(p_graph, p_one) and np.array_equal(n_graph, n_one)
    assert np.array_equal(p_host, p_one) and np.array_equal(n_host, n_one)
