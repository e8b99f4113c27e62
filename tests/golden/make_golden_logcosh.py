"""Generate the LogCoshVAE golden vectors by running the REFERENCE's own module.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_logcosh.py <reference root> [case ...]

The recipe of make_golden.py (the reference is imported read-only, nothing of it is copied):
parameters from oracle.vae_oracle.make_params(vanilla_param_spec()) loaded with strict=True (LogCoshVAE
has the VanillaVAE network), inputs from make_inputs.  torch.randn_like is swapped for the duration of
forward: its one call (reparameterize, models/logcosh_vae.py:117) returns eps.
One step = forward, loss_function(M_N=...), backward, Adam(lr).step().

The reference's reconstruction term overflows in fp32 once -2*alpha*t > 88.7 (inf loss, NaN
gradients): with |t| < 2 on these inputs it is finite for alpha < 22.  A case whose loss is not finite
is refused, so the fixtures hold only what the reference can compute.

Outputs: tests/golden/<case>.npz — data only: the summaries of the other fixtures."""
from __future__ import annotations

import copy
import json
import math
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [REPO, os.path.dirname(HERE), HERE]

from make_golden import HEAD, SEED, import_reference, summary  # noqa: E402
from oracle import vae_oracle as O  # noqa: E402

CASES = {
    # configs/vae/logcosh_vae.yaml's model_params, kld_weight and LR
    "logcosh_b8": (8, dict(in_channels=3, latent_dim=128, alpha=10.0, beta=1.0), 0.00025, 0.005),
    # a steeper alpha still inside the reference's fp32 range, and a heavier KL term
    "logcosh_b16": (16, dict(in_channels=3, latent_dim=128, alpha=20.0, beta=10.0), 0.00025, 0.005),
}


def run_case(models, name):
    B, kw, M_N, lr = CASES[name]
    torch.manual_seed(0)
    model = models.vae_models["LogCoshVAE"](**copy.deepcopy(kw))
    sd = O.make_params(O.vanilla_param_spec(latent_dim=kw["latent_dim"]), SEED)
    model.load_state_dict(sd, strict=True)
    model.train()
    x, eps = O.make_inputs(B, kw["latent_dim"], SEED)
    queue = [eps]
    real_randn_like = torch.randn_like

    def fake_randn_like(t, *a, **k):
        v = queue.pop(0)
        assert tuple(t.shape) == tuple(v.shape), (t.shape, v.shape)
        return v.clone()

    torch.randn_like = fake_randn_like
    try:
        results = model(x, labels=torch.zeros(B))
        ld = model.loss_function(*results, M_N=M_N, optimizer_idx=0, batch_idx=0)
    finally:
        torch.randn_like = real_randn_like
    assert not queue
    loss = {k: float(v.detach().reshape(-1)[0]) for k, v in ld.items()}
    assert all(math.isfinite(v) for v in loss.values()), (
        f"{name}: the reference's loss is not finite ({loss}): exp(-2*alpha*t) overflowed at alpha={kw['alpha']}")
    ld["loss"].reshape(()).backward()

    arrays = {}
    t = (results[0] - x).detach()
    meta = {"case": name, "arch": "LogCoshVAE", "batch": B, "ctor": kw, "M_N": M_N, "lr": lr, "seed": SEED,
            "samples": None, "x_sha": O.sha256_of([x]), "eps_sha": O.sha256_of([eps]),
            "params_sha": O.sha256_of([sd[k] for k in sd]), "loss": loss, "t_range": [float(t.min()), float(t.max())],
            "torch": torch.__version__}
    recon = results[0].detach()
    arrays["recon_head"] = recon[:min(B, 4)].numpy()
    flat = recon.reshape(B, -1)
    arrays["recon_sum"] = flat.double().sum(1).numpy()
    arrays["recon_sq"] = (flat.double() ** 2).sum(1).numpy()
    arrays["per_img_mse"] = torch.nn.functional.mse_loss(recon, x, reduction="none").mean(dim=[1, 2, 3]).numpy()
    arrays["mu"], arrays["log_var"] = results[2].detach().numpy(), results[3].detach().numpy()
    names = []
    for k, p in model.named_parameters():
        g = p.grad if p.grad is not None else torch.zeros_like(p)
        assert bool(torch.isfinite(g).all()), (name, k)
        arrays[f"grad_stats/{k}"] = summary(g)
        arrays[f"grad_head/{k}"] = g.detach().flatten()[:HEAD].numpy()
        names.append(k)
    meta["param_names"] = names
    for k, t in model.state_dict().items():
        if k.endswith("running_mean") or k.endswith("running_var"):
            arrays[f"running/{k}"] = t.numpy()
    torch.optim.Adam(model.parameters(), lr=lr, weight_decay=0.0).step()
    for k, p in model.named_parameters():
        arrays[f"new_stats/{k}"] = summary(p)
        arrays[f"new_head/{k}"] = p.detach().flatten()[:HEAD].numpy()
    arrays["meta"] = np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8)
    out = os.path.join(HERE, f"{name}.npz")
    np.savez_compressed(out, **arrays)
    print(f"wrote {out} ({os.path.getsize(out) / 1024:.0f} KiB) loss={meta['loss']} t in {meta['t_range']}")


def main():
    if len(sys.argv) < 2:
        raise SystemExit(__doc__)
    torch.set_num_threads(8)
    models = import_reference(sys.argv[1])
    for name in sys.argv[2:] or list(CASES):
        run_case(models, name)


if __name__ == "__main__":
    main()
