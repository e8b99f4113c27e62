"""LogCoshVAE through the training engines: experiment.fit on the graph engine against the eager
drop-in path, python -m vae_amd.run on a YAML with name: 'LogCoshVAE', and gradient-norm clipping
inside the fused step."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import logcosh_ref as R

pytestmark = pytest.mark.gpu

YAML = dict(alpha=10.0, beta=1.0)                       # configs/vae/logcosh_vae.yaml
M_N, LR = 0.00025, 0.005


def test_fit_graph_engine_follows_the_eager_path():
    """experiment.fit(engine='graph') takes LogCoshVAE onto GraphedSteps (no eager fallback), and its
    loss follows the eager drop-in path's on the same three batches (both engines draw eps from torch's
    device generator, seeded alike), as the MS-SSIM Autoencoder's does."""
    from vae_amd.experiment import VAEXperiment, _fusable, fit
    from vae_amd.models import vae_models
    g = torch.Generator(device="cuda").manual_seed(3)
    batches = [(torch.rand(8, 3, 64, 64, generator=g, device="cuda"), torch.zeros(8, device="cuda"),
                [f"{i}.png" for i in range(8)]) for _ in range(3)]
    out = {}
    for engine in ("graph", "eager"):
        torch.manual_seed(0)
        model = vae_models["LogCoshVAE"](in_channels=3, latent_dim=128, **YAML, dtype=torch.float32, device="cuda",
                                         seed=5)
        assert _fusable(model) and hasattr(model, "fused_train_step")
        exp = VAEXperiment(model, {"LR": 0.001, "weight_decay": 0.0, "kld_weight": M_N})
        torch.manual_seed(0)
        hist = fit(exp, batches, epochs=1, engine=engine)[0]
        assert set(hist) >= set(R.TERMS), (engine, hist)
        out[engine] = hist["loss"]
    print(out)
    assert np.isfinite(out["graph"]) and 0.0 < out["graph"] < 2.0
    assert abs(out["graph"] - out["eager"]) <= 1e-3 * abs(out["eager"]), out


def test_run_cli_trains_logcosh_from_a_yaml(tmp_path):
    import yaml
    # configs/vae/logcosh_vae.yaml's values
    cfg = {"model_params": dict(name="LogCoshVAE", in_channels=3, latent_dim=128, alpha=10.0, beta=1.0),
           "data_params": {"data_path": "Data/", "train_batch_size": 16, "val_batch_size": 16, "patch_size": 64},
           "exp_params": {"LR": 0.005, "weight_decay": 0.0, "scheduler_gamma": 0.95, "kld_weight": 0.00025,
                          "manual_seed": 1265},
           "trainer_params": {"gpus": [0], "max_epochs": 1},
           "logging_params": {"save_dir": str(tmp_path / "logs"), "name": "LogCoshVAE"}}
    p = tmp_path / "logcosh_vae.yaml"
    p.write_text(yaml.safe_dump(cfg))
    pkg = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "pytorch-vae_amd")
    env = dict(os.environ, PYTHONPATH=pkg + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-m", "vae_amd.run", "-c", str(p), "--synthetic", "40", "--dtype", "bf16"],
                       capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "Successfully completed" in r.stdout and "Reconstruction_Loss=" in r.stdout


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_clipped_step_reports_the_norm_of_the_unclipped_gradient(dtype):
    """fused_train_step(max_grad_norm=1.0): plan.grads stays unclipped, and the norm the optimizer reports
    is its fp64 norm to one fp32 rounding (the bar of tests/test_gpu_clip_step.py)."""
    from oracle import vae_oracle as O
    from vae_amd.models import vae_models
    B = 8
    x, eps = O.make_inputs(B, 128, 77)
    model = vae_models["LogCoshVAE"](in_channels=3, latent_dim=128, **YAML, dtype=dtype, device="cuda")
    model.load_reference_state_dict(O.make_params(O.vanilla_param_spec(), 1265))
    step = model.fused_train_step(B, M_N, lr=LR, graph=True, max_grad_norm=1.0)
    assert not step.deferred and step.opt.max_grad_norm is not None
    step(x.cuda(), eps.cuda())
    torch.cuda.synchronize()
    norm = float(step.plan.grads.double().norm())
    gn, gc = step.opt.grad_norm.tolist()
    print(f"{dtype}: reported norm {gn:.9g}, fp64 {norm:.12g}, coefficient {gc:.6g}")
    assert np.isfinite(norm) and norm > 0
    assert abs(gn - norm) <= 2.0 ** -23 * norm, (gn, norm)
    assert gc == pytest.approx(min(1.0, 1.0 / (norm + 1e-6)), rel=4 * 2.0 ** -23)
    assert all(np.isfinite(v) for v in step.loss_terms())


def test_bf16_graph_step_defers_and_draws_eps_on_the_device():
    """The one-rank bf16 step as fit() runs it: reductions deferred to the optimizer launch, eps drawn
    in the bottleneck kernel; three replays stay finite and move the loss."""
    from oracle import vae_oracle as O
    from vae_amd.models import vae_models
    B = 8
    x, _ = O.make_inputs(B, 128, 78)
    model = vae_models["LogCoshVAE"](in_channels=3, latent_dim=128, **YAML, dtype=torch.bfloat16, device="cuda")
    model.load_reference_state_dict(O.make_params(O.vanilla_param_spec(), 1265))
    step = model.fused_train_step(B, M_N, lr=LR, graph=True, device_eps=1265)
    assert step.deferred and step.device_eps
    terms = []
    for _ in range(3):
        step(x.cuda())
        torch.cuda.synchronize()
        terms.append(step.loss_terms())
    print(terms)
    assert all(np.isfinite(v) for t in terms for v in t)
    assert terms[0] != terms[1] != terms[2]
    per = step.plan.per_img.cpu()
    want = ((step.plan.recon.cpu() - x) ** 2).mean(dim=[1, 2, 3])
    torch.testing.assert_close(per, want, rtol=1e-3, atol=1e-6)
