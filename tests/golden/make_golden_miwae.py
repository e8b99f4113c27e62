"""Generate the MIWAE golden vectors by running the REFERENCE's own module.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_miwae.py <reference root> [case ...]

The recipe of make_golden.py (the reference is imported read-only, nothing of it is copied):
parameters from oracle.vae_oracle.make_params(vanilla_param_spec()) loaded with strict=True (MIWAE has
the VanillaVAE network), inputs from make_inputs(samples=M*K).  torch.randn_like is swapped for the
duration of forward: its one call (reparameterize, models/miwae.py:121) has shape [B, M, K, D] and
returns eps viewed so.
One step = forward, loss_function(M_N=...), backward, Adam(lr).step().

Outputs: tests/golden/<case>.npz — data only: the summaries of the other fixtures, the reconstructions
summarised per decoder row (B*M*K of them, row-major b, m, k)."""
from __future__ import annotations

import copy
import json
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
    # configs/vae/miwae.yaml's model_params (num_samples 5, num_estimates 3), kld_weight and LR
    "miwae_b4": (4, dict(in_channels=3, latent_dim=128, num_samples=5, num_estimates=3), 1e-8, 0.005),
    # the constructor's defaults (5 x 5)
    "miwae_b2": (2, dict(in_channels=3, latent_dim=128), 2.5e-4, 0.005),
}


def run_case(models, name):
    B, kw, M_N, lr = CASES[name]
    torch.manual_seed(0)
    model = models.vae_models["MIWAE"](**copy.deepcopy(kw))
    M, K, D = model.num_estimates, model.num_samples, kw["latent_dim"]
    sd = O.make_params(O.vanilla_param_spec(latent_dim=D), SEED)
    model.load_state_dict(sd, strict=True)
    model.train()
    x, eps = O.make_inputs(B, D, SEED, samples=M * K)
    queue = [eps.view(B, M, K, D)]
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
    ld["loss"].reshape(()).backward()

    arrays = {}
    meta = {"case": name, "arch": "MIWAE", "batch": B, "ctor": kw, "M_N": M_N, "lr": lr, "seed": SEED,
            "samples": M * K, "estimates": M, "x_sha": O.sha256_of([x]), "eps_sha": O.sha256_of([eps]),
            "params_sha": O.sha256_of([sd[k] for k in sd]),
            "loss": {k: float(v.detach().reshape(-1)[0]) for k, v in ld.items()}, "torch": torch.__version__}
    recon = results[0].detach()
    assert tuple(recon.shape[:3]) == (B, M, K)
    rows = recon.reshape(B * M * K, *recon.shape[3:])
    arrays["recon_head"] = rows[:4].numpy()
    flat = rows.reshape(B * M * K, -1)
    arrays["recon_sum"] = flat.double().sum(1).numpy()
    arrays["recon_sq"] = (flat.double() ** 2).sum(1).numpy()
    arrays["per_row_mse"] = ((rows - x.repeat_interleave(M * K, 0)) ** 2).mean(dim=[1, 2, 3]).numpy()
    arrays["mu"], arrays["log_var"] = results[2][:, 0, 0].detach().numpy(), results[3][:, 0, 0].detach().numpy()
    names = []
    for k, p in model.named_parameters():
        g = p.grad if p.grad is not None else torch.zeros_like(p)
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
    print(f"wrote {out} ({os.path.getsize(out) / 1024:.0f} KiB) loss={meta['loss']}")


def main():
    if len(sys.argv) < 2:
        raise SystemExit(__doc__)
    torch.set_num_threads(8)
    models = import_reference(sys.argv[1])
    for name in sys.argv[2:] or list(CASES):
        run_case(models, name)


if __name__ == "__main__":
    main()
