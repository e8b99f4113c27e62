"""trainer_params.gradient_clip_val through the training loops: experiment.fit(gradient_clip_val=v)
on both engines — torch.nn.utils.clip_grad_norm_ before optimizer.step() on the eager one, the fused
step's own clip (FusedAdam(max_grad_norm=v)) on the graph one — and `python -m vae_amd.run
--clip_gradients` on a YAML that sets it."""
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

PARAMS = {"LR": 0.005, "weight_decay": 0.0, "kld_weight": 2.5e-4, "manual_seed": 1265}


def _batches():
    g = torch.Generator().manual_seed(3)
    return [(torch.rand(8, 3, 64, 64, generator=g).cuda(), torch.zeros(8), [f"i{k}_{j}" for j in range(8)])
            for k in range(2)]


def _fit(engine, clip, batches):
    """One epoch from the seeded parameters: (parameter update, exp_avg, exp_avg_sq) of the flat parameter."""
    from vae_amd.experiment import VAEXperiment, fit
    from vae_amd.models import vae_models
    model = vae_models["Autoencoder"](in_channels=3, latent_dim=128, dtype=torch.float32, device="cuda", seed=1265)
    model.train()
    p0 = model.flat.detach().clone()
    exp = VAEXperiment(model, PARAMS)
    made, configure = [], exp.configure_optimizers
    exp.configure_optimizers = lambda: made.append(configure()) or made[-1]      # (fit builds its own optimizer)
    fit(exp, batches, epochs=1, engine=engine, gradient_clip_val=clip)
    torch.cuda.synchronize()
    st = made[0][0].state[model.flat]
    return (model.flat.detach() - p0).double(), st["exp_avg"].double(), st["exp_avg_sq"].double()


def _first_norm(batches):
    from vae_amd.experiment import VAEXperiment
    from vae_amd.models import vae_models
    model = vae_models["Autoencoder"](in_channels=3, latent_dim=128, dtype=torch.float32, device="cuda", seed=1265)
    model.train()
    VAEXperiment(model, PARAMS).training_step(batches[0], 0).backward()
    return float(model.flat.grad.double().norm())


def _rel(a, b):
    return float((a - b).norm() / b.norm())


def test_fit_clips_alike_on_both_engines():
    """fp32 Autoencoder (no noise: both engines see the same step), two batches of 8, v = half the
    first step's gradient norm.  The eager and graph runs may differ under clipping by four times what
    they differ by without it (the parent's behaviour, measured here; floor 1e-6) — relative L2
    distance of the parameter update and of both moment buffers.  And the clip is not ignored: the
    moments of a clipped run differ from the unclipped run's, on either engine.
    Measured on an MI355X, unclipped / clipped: update 1.3e-4 / 2.3e-4, exp_avg 4.3e-8 / 6.8e-8,
    exp_avg_sq 7.4e-8 / 7.9e-8."""
    batches = _batches()
    v = 0.5 * _first_norm(batches)
    plain = {e: _fit(e, None, batches) for e in ("eager", "graph")}
    clipped = {e: _fit(e, v, batches) for e in ("eager", "graph")}
    for i, name in enumerate(("update", "exp_avg", "exp_avg_sq")):
        base = _rel(plain["eager"][i], plain["graph"][i])
        got = _rel(clipped["eager"][i], clipped["graph"][i])
        print(f"{name}: eager vs graph {base:.3e} unclipped, {got:.3e} clipped (v = {v:.6g})")
        assert got <= max(4 * base, 1e-6), (name, got, base)
    for e in ("eager", "graph"):
        assert _rel(clipped[e][1], plain[e][1]) > 0.1, e        # exp_avg scales with the coefficient (<= 0.5 at step 1)
        assert _rel(clipped[e][2], plain[e][2]) > 0.1, e


def test_run_cli_applies_the_clip_with_the_flag(tmp_path):
    """The YAML of test_gpu_infovae_engine.py's CLI test (gradient_clip_val: 0.8) with --clip_gradients:
    the run completes and the `not applied` warning is gone."""
    import yaml
    cfg = {"model_params": dict(name="InfoVAE", in_channels=3, latent_dim=128, reg_weight=110, kernel_type="imq",
                                alpha=-9.0, beta=10.5),
           "data_params": {"data_path": "Data/", "train_batch_size": 16, "val_batch_size": 16, "patch_size": 64},
           "exp_params": {"LR": 0.005, "weight_decay": 0.0, "scheduler_gamma": 0.95, "kld_weight": 2.5e-4,
                          "manual_seed": 1265},
           "trainer_params": {"gpus": [0], "max_epochs": 1, "gradient_clip_val": 0.8},
           "logging_params": {"save_dir": str(tmp_path / "logs"), "name": "InfoVAE"}}
    p = tmp_path / "infovae.yaml"
    p.write_text(yaml.safe_dump(cfg))
    pkg = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "pytorch-vae_amd")
    env = dict(os.environ, PYTHONPATH=pkg + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-m", "vae_amd.run", "-c", str(p), "--synthetic", "40", "--dtype", "bf16",
                        "--clip_gradients"], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "MMD=" in r.stdout and "Successfully completed" in r.stdout
    assert "is set but not applied" not in r.stderr
