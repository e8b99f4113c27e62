"""InfoVAE through the training engines (engine.TrainStep via InfoVAE.fused_train_step, experiment.fit,
python -m vae_amd.run): the captured step draws eps and the MMD prior on the device at every replay,
the graph replay equals the eager launch sequence, and a YAML with name: 'InfoVAE' trains."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import infovae_ref as R
from test_gpu_infovae_step import M_N, YAML

pytestmark = pytest.mark.gpu


def _model(dtype):
    from oracle import vae_oracle as O
    from vae_amd.models import InfoVAE
    m = InfoVAE(3, 128, **YAML, dtype=dtype, device="cuda")
    m.load_reference_state_dict(O.make_params(O.vanilla_param_spec(), 1265))
    return m


def test_graphed_step_draws_eps_and_prior_per_replay():
    model = _model(torch.bfloat16)
    step = model.fused_train_step(64, M_N, lr=0.005, graph=True, device_eps=7, device_prior=7)
    assert step.device_eps and step.device_prior
    plan = step.plan
    plan.x.uniform_()
    seen = []
    for _ in range(3):
        step()
        torch.cuda.synchronize()
        terms = step.loss_terms() + [step.mmd_term()]
        assert all(np.isfinite(v) for v in terms), terms
        seen.append((plan.eps.clone(), plan.prior.clone(), terms[3]))
    for a, b in zip(seen, seen[1:]):
        assert not torch.equal(a[0], b[0]) and not torch.equal(a[1], b[1]) and a[2] != b[2]
    # the prior is another stream of the generator: uncorrelated with the same step's eps
    for e, p, _ in seen:
        assert abs(float(np.corrcoef(e.flatten().cpu().numpy(), p.flatten().cpu().numpy())[0, 1])) < 0.03
        assert abs(float(p.mean())) < 0.05 and abs(float(p.std()) - 1) < 0.05
    # the logged MMD is the MMD of what was drawn (z in fp32 from the step's own mu | log_var)
    mulv, eps, prior = plan.mulv.cpu().double(), plan.eps.cpu().double(), plan.prior.cpu().double()
    m = float(R.compute_mmd(mulv[:, :128] + eps * torch.exp(0.5 * mulv[:, 128:]), prior, "imq", 2.0))
    assert abs(seen[-1][2] - m) <= 1e-4 * abs(m)


def test_graph_replay_equals_eager_with_injected_noise():
    from oracle import vae_oracle as O
    x, eps = O.make_inputs(16, 128, 5)
    prior = R.make_prior(16, 128, 5)
    res = []
    for graph in (True, False):
        model = _model(torch.float32)
        step = model.fused_train_step(16, M_N, lr=0.005, graph=graph)
        step.plan.prior.copy_(prior)
        terms = []
        for _ in range(2):
            step(x.cuda(), eps.cuda())
            torch.cuda.synchronize()
            terms.append(step.loss_terms() + [step.mmd_term()])
        res.append((terms, model.net.params.clone(), model.net.running.clone()))
    assert res[0][0] == res[1][0]
    assert torch.equal(res[0][1], res[1][1]) and torch.equal(res[0][2], res[1][2])


def test_fit_logs_mmd_beside_the_other_terms():
    from vae_amd.experiment import VAEXperiment, fit
    model = _model(torch.bfloat16)
    exp = VAEXperiment(model, {"LR": 0.005, "weight_decay": 0.0, "kld_weight": M_N, "manual_seed": 1265})
    g = torch.Generator().manual_seed(3)
    batches = [(torch.rand(16, 3, 64, 64, generator=g).cuda(), torch.zeros(16), [f"i{j}" for j in range(16)])
               for _ in range(2)]
    for engine in ("graph", "eager"):
        hist = fit(exp, batches, epochs=1, engine=engine)
        assert set(hist[0]) >= {"loss", "Reconstruction_Loss", "MMD", "KLD"}, (engine, hist)
        assert all(np.isfinite(hist[0][k]) for k in ("loss", "Reconstruction_Loss", "MMD", "KLD"))


def test_run_cli_trains_infovae_from_a_yaml(tmp_path):
    import yaml
    cfg = {"model_params": dict(name="InfoVAE", in_channels=3, latent_dim=128, reg_weight=110, kernel_type="imq",
                                alpha=-9.0, beta=10.5),
           "data_params": {"data_path": "Data/", "train_batch_size": 16, "val_batch_size": 16, "patch_size": 64},
           "exp_params": {"LR": 0.005, "weight_decay": 0.0, "scheduler_gamma": 0.95, "kld_weight": M_N,
                          "manual_seed": 1265},
           "trainer_params": {"gpus": [0], "max_epochs": 1, "gradient_clip_val": 0.8},
           "logging_params": {"save_dir": str(tmp_path / "logs"), "name": "InfoVAE"}}
    p = tmp_path / "infovae.yaml"
    p.write_text(yaml.safe_dump(cfg))
    pkg = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "pytorch-vae_amd")
    env = dict(os.environ, PYTHONPATH=pkg + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-m", "vae_amd.run", "-c", str(p), "--synthetic", "40", "--dtype", "bf16"],
                       capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "MMD=" in r.stdout and "Successfully completed" in r.stdout
    assert r.stderr.count("UserWarning: trainer_params.gradient_clip_val is set but not applied") == 1
