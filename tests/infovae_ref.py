"""InfoVAE restated on the CPU oracle's functional pieces (oracle/vae_oracle.py), for the tests.

The reference's InfoVAE (models/info_vae.py) has the VanillaVAE network, so the forward is the
oracle's vanilla_encode / reparameterize / vanilla_decode; what is restated here is its loss,
info_vae.py:128-229, with the two random draws (eps of reparameterize, :120; the prior sample of
compute_mmd, :220) injected so a step is a function of its inputs.  Quirks kept: the imq kernel
sums k over i != j for ALL three matrices (the diagonal of prior-vs-z is dropped too) and the
`.mean()` calls of compute_mmd then act on scalars; the rbf kernel is the mean over all B*B entries.
`train_step` returns what oracle.vae_oracle.train_step returns (loss terms, z, gradients in the
reference layout, running statistics)."""
from collections import OrderedDict

import torch
from torch.nn import functional as F

from oracle import vae_oracle as O


def compute_kernel(x1, x2, kernel_type="imq", latent_var=2.0, eps=1e-7):
    """info_vae.py:150-216: [N,D] x [N,D] -> the scalar (imq) or the N x N matrix (rbf)."""
    D = x1.size(1)
    a = x1.unsqueeze(-2)
    b = x2.unsqueeze(-3)
    if kernel_type == "rbf":
        sigma = 2.0 * D * latent_var
        return torch.exp(-((a - b).pow(2).mean(-1) / sigma))
    if kernel_type == "imq":
        C = 2 * D * latent_var
        kernel = C / (eps + C + (a - b).pow(2).sum(dim=-1))
        return kernel.sum() - kernel.diag().sum()
    raise ValueError("Undefined kernel type.")


def compute_mmd(z, prior, kernel_type="imq", latent_var=2.0):
    """info_vae.py:218-229 with the prior sample given."""
    return (compute_kernel(prior, prior, kernel_type, latent_var).mean()
            + compute_kernel(z, z, kernel_type, latent_var).mean()
            - 2 * compute_kernel(prior, z, kernel_type, latent_var).mean())


def info_loss(recons, x, z, mu, log_var, prior, M_N, alpha=-0.5, beta=5.0, reg_weight=100, kernel_type="imq",
              latent_var=2.0):
    """info_vae.py:128-148."""
    B = x.size(0)
    bias_corr = B * (B - 1)
    recons_loss = F.mse_loss(recons, x)
    mmd_loss = compute_mmd(z, prior, kernel_type, latent_var)
    kld_loss = torch.mean(-0.5 * torch.sum(1 + log_var - mu ** 2 - log_var.exp(), dim=1), dim=0)
    loss = beta * recons_loss + (1. - alpha) * M_N * kld_loss + (alpha + reg_weight - 1.) / bias_corr * mmd_loss
    return {"loss": loss, "Reconstruction_Loss": recons_loss, "MMD": mmd_loss, "KLD": -kld_loss}


def make_prior(batch, latent_dim=128, seed=1265):
    """The prior sample of a case: N(0,1) from a generator of its own (seed + 1), [B,D]."""
    return torch.randn(batch, latent_dim, generator=torch.Generator().manual_seed(seed + 1))


def train_step(sd, x, eps, prior, *, M_N, hidden_dims=None, training=True, **loss_kw):
    """forward -> loss_function -> backward on a copy of ``sd`` (the dtype of ``sd`` / inputs)."""
    kinds = O._kinds_of("VanillaVAE", sd, hidden_dims)
    P = OrderedDict()
    for k, t in sd.items():
        t = t.detach().clone()
        if kinds[k] in O.TRAINABLE_KINDS:
            t.requires_grad_(True)
        P[k] = t
    stats = {}
    hd = list(hidden_dims or O.DEFAULT_HIDDEN)
    mu, log_var = O.vanilla_encode(P, x, hd, training, stats)
    z = O.reparameterize(mu, log_var, eps)
    recon = O.vanilla_decode(P, z, hd, training, stats)
    ld = info_loss(recon, x, z, mu, log_var, prior, M_N, **loss_kw)
    ld["loss"].backward()
    grads = OrderedDict((k, (P[k].grad.detach().clone() if P[k].grad is not None else torch.zeros_like(P[k])))
                        for k in P if kinds[k] in O.TRAINABLE_KINDS)
    per_img = F.mse_loss(recon.detach(), x, reduction="none").mean(dim=[1, 2, 3])
    return dict(recon=recon.detach(), mu=mu.detach(), log_var=log_var.detach(), z=z.detach(),
                loss={k: float(v.detach()) for k, v in ld.items()}, per_img_mse=per_img, grads=grads, running=stats)


def with_spread(sd, x, eps, prior, threads=1, **kw):
    """(the fp32 step at the default thread count, its per-gradient relative-norm spread): the larger
    of the thread-count spread and the fp32-vs-fp64 error — the recipe of parity_util.oracle_with_spread."""
    from parity_util import _rel
    o = train_step(sd, x, eps, prior, **kw)
    n0 = torch.get_num_threads()
    try:
        torch.set_num_threads(threads)
        o1 = train_step(sd, x, eps, prior, **kw)
    finally:
        torch.set_num_threads(n0)
    sd64 = {k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()}
    o64 = train_step(sd64, x.double(), eps.double(), prior.double(), **kw)
    spread = {k: max(_rel(o["grads"][k], o1["grads"][k]), _rel(o["grads"][k], o64["grads"][k])) for k in o["grads"]}
    return o, spread
