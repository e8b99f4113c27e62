"""MIWAE through the training engines (engine.TrainStep via MIWAE.fused_train_step, experiment.fit,
python -m vae_amd.run): the graph replay equals the eager launch sequence bit for bit in fp32 at
(B, M, K) = (4, 3, 5), the bucketed data-parallel path at one rank equals the one-graph step, fit()
logs the three terms, a YAML with name: 'MIWAE' trains with its num_samples / num_estimates passed
straight through, and two ranks over RCCL average the shards' gradients.

The one-rank process group lives in a spawned child (the set-up of tests/test_gpu_dp_infovae.py), so
no test that runs after this file in the same process finds torch.distributed initialised."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

import miwae_ref as R
from test_gpu_dp import _port

pytestmark = pytest.mark.gpu

B, M, K, LR, M_N = 4, 3, 5, 0.005, 2.5e-4


def _model(dtype, device="cuda"):
    from oracle import vae_oracle as O
    from vae_amd.models import MIWAE
    m = MIWAE(3, 128, num_samples=K, num_estimates=M, dtype=dtype, device=device)
    m.load_reference_state_dict(O.make_params(O.vanilla_param_spec(), 1265))
    return m


def _inputs(seed=5):
    from oracle import vae_oracle as O
    return O.make_inputs(B, 128, seed, samples=M * K)


def _three_steps(**step_kw):
    x, eps = _inputs()
    model = _model(torch.float32)
    step = model.fused_train_step(B, M_N, lr=LR, **step_kw)
    assert step.plan.S == M * K and step.extra_term() is None       # no fourth term
    terms = []
    for _ in range(3):
        step(x.cuda(), eps.reshape(B * M * K, 128).cuda())
        torch.cuda.synchronize()
        terms.append(step.loss_terms())
    return step, terms, model.net.params.clone(), model.net.running.clone()


def test_graph_replay_equals_eager_over_three_adam_steps():
    res = [_three_steps(graph=g) for g in (True, False)]
    assert res[0][1] == res[1][1]
    assert torch.equal(res[0][2], res[1][2]) and torch.equal(res[0][3], res[1][3])
    terms = res[0][1]
    assert all(np.isfinite(v) for t in terms for v in t)
    assert terms[0] != terms[1] != terms[2]                # Adam moved the parameters
    from oracle import vae_oracle as O
    x, eps = _inputs()
    ref = R.train_step(O.make_params(O.vanilla_param_spec(), 1265), x, eps, M_N=M_N, M=M, K=K)
    for got, k in zip(terms[0], R.TERMS):
        assert abs(got - ref["loss"][k]) <= 1e-4 * abs(ref["loss"][k]), (k, got, ref["loss"][k])
    assert tuple(res[0][0].plan.loss_dict()) == R.TERMS


def _bucket_worker(port, q):
    try:
        import torch.distributed as dist
        os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        torch.cuda.set_device(0)
        dist.init_process_group("gloo", rank=0, world_size=1)
        from vae_amd.engine import FusedAdam, TrainStep
        from vae_amd.net import StepPlan
        x, eps = _inputs()
        out = []
        for force in (False, True):
            model = _model(torch.float32)
            plan = StepPlan(model.net, B, loss="miwae", samples=K, estimates=M, kld_weight=M_N)
            step = TrainStep(model.net, plan, FusedAdam(model.net, lr=LR), graph=True, nbuckets=4, force_buckets=force)
            assert (step.comm is not None) == force
            terms = []
            for _ in range(3):
                step(x.cuda(), eps.reshape(B * M * K, 128).cuda())
                torch.cuda.synchronize()
                terms.append(step.loss_terms())
            out.append((terms, model.net.params.cpu().numpy(), model.net.running.cpu().numpy()))
        q.put(out)
        dist.barrier()
        dist.destroy_process_group()
    except Exception:
        import traceback
        q.put(traceback.format_exc())


def test_bucketed_step_over_a_one_rank_group_equals_the_one_graph_step():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    p = ctx.Process(target=_bucket_worker, args=(_port(), q))
    p.start()
    out = q.get(timeout=240)
    p.join(timeout=60)
    assert not isinstance(out, str), out
    one, bucketed = out
    assert one[0] == bucketed[0]
    assert np.array_equal(one[1], bucketed[1]) and np.array_equal(one[2], bucketed[2])


def test_fit_logs_the_three_terms_and_scores_images_over_their_rows():
    from vae_amd.experiment import VAEXperiment, fit
    model = _model(torch.bfloat16)
    exp = VAEXperiment(model, {"LR": LR, "weight_decay": 0.0, "kld_weight": M_N, "manual_seed": 1265})
    g = torch.Generator().manual_seed(3)
    batches = [(torch.rand(8, 3, 64, 64, generator=g).cuda(), torch.zeros(8), [f"i{j}" for j in range(8)])
               for _ in range(2)]
    for engine in ("graph", "eager"):
        hist = fit(exp, batches, epochs=1, engine=engine)
        assert set(hist[0]) >= set(R.TERMS) and "DIP_Loss" not in hist[0] and "MMD" not in hist[0], (engine, hist)
        assert all(np.isfinite(hist[0][k]) for k in R.TERMS)
    # per-image scores: an image's M*K rows averaged (experiment.per_image_mse on [B,M,K,C,H,W])
    recon, x = torch.rand(2, M, K, 3, 8, 8), torch.rand(2, 3, 8, 8)
    want = ((recon - x[:, None, None]) ** 2).flatten(1).mean(1)
    torch.testing.assert_close(VAEXperiment.per_image_mse(recon, x), want)
    assert exp.ensure_4_dims(recon).shape == (2, 3, 8, 8)              # the first row of every image


def test_run_cli_trains_miwae_from_a_yaml(tmp_path):
    import yaml
    cfg = {"model_params": dict(name="MIWAE", in_channels=3, latent_dim=128, num_samples=5, num_estimates=3),
           "data_params": {"data_path": "Data/", "train_batch_size": 8, "val_batch_size": 8, "patch_size": 64},
           "exp_params": {"LR": 0.005, "weight_decay": 0.0, "scheduler_gamma": 0.95, "kld_weight": 0.00000001,
                          "manual_seed": 1265},
           "trainer_params": {"gpus": [0], "max_epochs": 1},
           "logging_params": {"save_dir": str(tmp_path / "logs"), "name": "MIWAE"}}
    p = tmp_path / "miwae.yaml"
    p.write_text(yaml.safe_dump(cfg))
    pkg = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "pytorch-vae_amd")
    env = dict(os.environ, PYTHONPATH=pkg + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-m", "vae_amd.run", "-c", str(p), "--synthetic", "24", "--dtype", "bf16"],
                       capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "Reconstruction_Loss=" in r.stdout and "Successfully completed" in r.stdout


# ---- two ranks over RCCL, one device each
WORLD, BR = 2, 4


def _shard(rank):
    from oracle import vae_oracle as O
    return O.make_inputs(BR, 128, 300 + rank, samples=M * K)


def _rccl_worker(rank, port, q):
    try:
        import torch.distributed as dist
        os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        torch.cuda.set_device(rank)
        dist.init_process_group("nccl", rank=rank, world_size=WORLD, device_id=torch.device(f"cuda:{rank}"))
        from vae_amd.engine import FusedAdam, TrainStep
        from vae_amd.net import StepPlan
        model = _model(torch.float32, device=f"cuda:{rank}")
        net = model.net
        plan = StepPlan(net, BR, loss="miwae", samples=K, estimates=M, kld_weight=M_N)
        step = TrainStep(net, plan, FusedAdam(net, lr=LR), graph=True, nbuckets=4)
        x, eps = _shard(rank)
        step(x.cuda(), eps.reshape(BR * M * K, 128).cuda())
        torch.cuda.synchronize()
        grads = {k: v.cpu().numpy() for k, v in net.layout.export_reference(plan.grads).items()}
        q.put((rank, grads, step.loss_terms(), plan.loss_dict()))
        dist.barrier()
        dist.destroy_process_group()
    except Exception:
        import traceback
        q.put((rank, traceback.format_exc(), None, None))


@pytest.mark.skipif(torch.cuda.device_count() < 2, reason="two ranks over RCCL need two GPUs")
def test_two_ranks_over_rccl_average_the_shards():
    from oracle import vae_oracle as O
    from parity_util import grad_bar
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _port()
    procs = [ctx.Process(target=_rccl_worker, args=(r, port, q)) for r in range(WORLD)]
    for p in procs:
        p.start()
    res = {}
    for _ in range(WORLD):
        r, grads, terms, local = q.get(timeout=240)
        assert not isinstance(grads, str), grads
        res[r] = ({k: torch.from_numpy(v) for k, v in grads.items()}, terms, local)
    for p in procs:
        p.join(timeout=60)
    sd = O.make_params(O.vanilla_param_spec(), 1265)
    shards, spreads = zip(*[R.with_spread(sd, *_shard(r), M_N=M_N, M=M, K=K) for r in range(WORLD)])
    spread = {k: max(sp[k] for sp in spreads) for k in spreads[0]}
    for k in res[0][0]:
        assert torch.equal(res[0][0][k], res[1][0][k]), k             # both ranks hold the averaged gradient
    for r in range(WORLD):
        for i, t in enumerate(R.TERMS):
            want = sum(s["loss"][t] for s in shards) / WORLD
            assert abs(res[r][1][i] - want) <= 1e-4 * abs(want), (r, t, res[r][1][i], want)
            own = shards[r]["loss"][t]
            assert abs(res[r][2][t] - own) <= 1e-4 * abs(own), (r, t, res[r][2][t], own)
    gmean = {k: sum(s["grads"][k] for s in shards) / WORLD for k in shards[0]["grads"]}
    for name, gr in gmean.items():
        if R.pre_bn_bias(name):
            continue                                                  # analytically zero under train-mode BN
        err = float((res[0][0][name].double() - gr.double()).norm() / gr.double().norm())
        assert err < grad_bar(name, spread), (name, err, grad_bar(name, spread))
