"""DIP-VAE through the training engines (engine.TrainStep via DIPVAE.fused_train_step, experiment.fit,
python -m vae_amd.run): the graph replay equals the eager launch sequence bit for bit in fp32, the
DIP_Loss metric is reported, the bucketed data-parallel path at one rank equals the one-graph step,
and a YAML with name: 'DIPVAE' trains.

The one-rank process group lives in a spawned child (the set-up of tests/test_gpu_dp_infovae.py), so
no test that runs after this file in the same process finds torch.distributed initialised."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

import dipvae_ref as R
from test_gpu_dipvae_step import M_N, YAML
from test_gpu_dp import _port

pytestmark = pytest.mark.gpu

B, LR = 16, 0.001


def _model(dtype):
    from oracle import vae_oracle as O
    from vae_amd.models import DIPVAE
    m = DIPVAE(3, 128, **YAML, dtype=dtype, device="cuda")
    m.load_reference_state_dict(O.make_params(O.vanilla_param_spec(), 1265))
    return m


def _three_steps(**step_kw):
    from oracle import vae_oracle as O
    x, eps = O.make_inputs(B, 128, 5)
    model = _model(torch.float32)
    step = model.fused_train_step(B, M_N, lr=LR, **step_kw)
    terms = []
    for _ in range(3):
        step(x.cuda(), eps.cuda())
        torch.cuda.synchronize()
        name, dip = step.extra_term()
        assert name == "DIP_Loss"
        terms.append(step.loss_terms() + [dip])
    return step, terms, model.net.params.clone(), model.net.running.clone()


def test_graph_replay_equals_eager_over_three_adam_steps():
    res = [_three_steps(graph=g) for g in (True, False)]
    assert res[0][1] == res[1][1]
    assert torch.equal(res[0][2], res[1][2]) and torch.equal(res[0][3], res[1][3])
    terms = res[0][1]
    assert all(np.isfinite(v) for t in terms for v in t)
    assert terms[0] != terms[1] != terms[2]                # Adam moved the parameters
    # the reported DIP_Loss is the restatement's, on the first step's (initial) parameters
    from oracle import vae_oracle as O
    x, eps = O.make_inputs(B, 128, 5)
    ref = R.train_step(O.make_params(O.vanilla_param_spec(), 1265), x, eps, M_N=M_N, **YAML)
    for got, k in zip(terms[0], R.TERMS):
        assert abs(got - ref["loss"][k]) <= 1e-4 * abs(ref["loss"][k]), (k, got, ref["loss"][k])
    assert res[0][0].plan.loss_dict()["DIP_Loss"] == terms[2][3]


def _bucket_worker(port, q):
    try:
        import torch.distributed as dist
        os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        torch.cuda.set_device(0)
        dist.init_process_group("gloo", rank=0, world_size=1)
        from vae_amd.engine import FusedAdam, TrainStep
        from vae_amd.net import StepPlan
        from oracle import vae_oracle as O
        x, eps = O.make_inputs(B, 128, 5)
        out = []
        for force in (False, True):
            model = _model(torch.float32)
            plan = StepPlan(model.net, B, loss="dip", kld_weight=M_N, **YAML)
            step = TrainStep(model.net, plan, FusedAdam(model.net, lr=LR), graph=True, nbuckets=4, force_buckets=force)
            assert (step.comm is not None) == force
            terms = []
            for _ in range(3):
                step(x.cuda(), eps.cuda())
                torch.cuda.synchronize()
                terms.append(step.loss_terms() + [step.extra_term()[1]])
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
    assert one[0] == bucketed[0]                           # loss terms and DIP_Loss (metrics[3]: the rank mean)
    assert np.array_equal(one[1], bucketed[1]) and np.array_equal(one[2], bucketed[2])


def test_fit_logs_dip_loss_beside_the_other_terms():
    from vae_amd.experiment import VAEXperiment, fit
    model = _model(torch.bfloat16)
    exp = VAEXperiment(model, {"LR": LR, "weight_decay": 0.0, "kld_weight": M_N, "manual_seed": 1265})
    g = torch.Generator().manual_seed(3)
    batches = [(torch.rand(16, 3, 64, 64, generator=g).cuda(), torch.zeros(16), [f"i{j}" for j in range(16)])
               for _ in range(2)]
    for engine in ("graph", "eager"):
        hist = fit(exp, batches, epochs=1, engine=engine)
        assert set(hist[0]) >= set(R.TERMS), (engine, hist)
        assert all(np.isfinite(hist[0][k]) for k in R.TERMS)


def test_run_cli_trains_dipvae_from_a_yaml(tmp_path):
    import yaml
    cfg = {"model_params": dict(name="DIPVAE", in_channels=3, latent_dim=128, lambda_diag=0.05, lambda_offdiag=0.1),
           "data_params": {"data_path": "Data/", "train_batch_size": 16, "val_batch_size": 16, "patch_size": 64},
           "exp_params": {"LR": 0.001, "weight_decay": 0.0, "scheduler_gamma": 0.97, "kld_weight": 1,
                          "manual_seed": 1265},
           "trainer_params": {"gpus": [0], "max_epochs": 1},
           "logging_params": {"save_dir": str(tmp_path / "logs"), "name": "DIPVAE"}}
    p = tmp_path / "dip_vae.yaml"
    p.write_text(yaml.safe_dump(cfg))
    pkg = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "pytorch-vae_amd")
    env = dict(os.environ, PYTHONPATH=pkg + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-m", "vae_amd.run", "-c", str(p), "--synthetic", "40", "--dtype", "bf16"],
                       capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "DIP_Loss=" in r.stdout and "Successfully completed" in r.stdout
