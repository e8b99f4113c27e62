"""DIP-VAE restated on the CPU oracle's functional pieces (oracle/vae_oracle.py), for the tests.

The reference's DIPVAE (models/dip_vae.py) has the VanillaVAE network, so the forward is the oracle's
vanilla_encode / reparameterize / vanilla_decode; what is restated here is its loss,
dip_vae.py:125-164, with the eps of reparameterize (:117) injected so a step is a function of its
inputs.  Quirks kept: the reconstruction term and the KL term are SUMS over the batch; the means are
centred over the latent axis (each row loses its own mean), not over the batch; the covariance is a
plain sum over the batch (no 1/B); the "variance" added for DIP loss II is ONE scalar — the mean of
the main diagonal of the [B, D] matrix exp(2 log_var), min(B, D) entries — and it is added to every
entry of the covariance, off-diagonals included.
`train_step` returns what oracle.vae_oracle.train_step returns (loss terms, gradients in the
reference layout, running statistics)."""
from collections import OrderedDict

import torch
from torch.nn import functional as F

from oracle import vae_oracle as O

TERMS = ("loss", "Reconstruction_Loss", "KLD", "DIP_Loss")


def pre_bn_bias(name):
    """A conv / convT bias followed by train-mode BatchNorm: its gradient is analytically zero."""
    return name.endswith(".0.bias") and not name.startswith("final_layer.3")


def dip_term(mu, log_var, lambda_diag=10.0, lambda_offdiag=5.0):
    """dip_vae.py:146-158 ("DIP loss II"): the penalty on the covariance of the latent means."""
    c = mu - mu.mean(dim=1, keepdim=True)
    cov = c.t().matmul(c)
    n = min(mu.shape)
    idx = torch.arange(n)
    cov_z = cov + (2.0 * log_var[idx, idx]).exp().mean()
    diag = torch.diagonal(cov_z)
    off = cov_z - torch.diag_embed(diag)
    return lambda_offdiag * (off ** 2).sum() + lambda_diag * ((diag - 1) ** 2).sum()


def dip_grad64(mu, log_var, lambda_diag, lambda_offdiag):
    """(dip, d dip/d mu, d dip/d log_var) by fp64 autograd of dip_term."""
    m = mu.detach().double().requires_grad_(True)
    lv = log_var.detach().double().requires_grad_(True)
    d = dip_term(m, lv, lambda_diag, lambda_offdiag)
    gm, gl = torch.autograd.grad(d, (m, lv))
    return float(d.detach()), gm, gl


def dip_loss(recons, x, mu, log_var, M_N, lambda_diag=10.0, lambda_offdiag=5.0):
    """dip_vae.py:125-164."""
    recons_loss = F.mse_loss(recons, x, reduction="sum")
    kld_loss = torch.sum(-0.5 * torch.sum(1 + log_var - mu ** 2 - log_var.exp(), dim=1), dim=0)
    dip = dip_term(mu, log_var, lambda_diag, lambda_offdiag)
    loss = recons_loss + M_N * kld_loss + dip
    return {"loss": loss, "Reconstruction_Loss": recons_loss, "KLD": -kld_loss, "DIP_Loss": dip}


def train_step(sd, x, eps, *, M_N, hidden_dims=None, training=True, **loss_kw):
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
    ld = dip_loss(recon, x, mu, log_var, M_N, **loss_kw)
    ld["loss"].backward()
    grads = OrderedDict((k, (P[k].grad.detach().clone() if P[k].grad is not None else torch.zeros_like(P[k])))
                        for k in P if kinds[k] in O.TRAINABLE_KINDS)
    per_img = F.mse_loss(recon.detach(), x, reduction="none").mean(dim=[1, 2, 3])
    return dict(recon=recon.detach(), mu=mu.detach(), log_var=log_var.detach(), z=z.detach(),
                loss={k: float(v.detach()) for k, v in ld.items()}, per_img_mse=per_img, grads=grads, running=stats)


def with_spread(sd, x, eps, threads=1, **kw):
    """(the fp32 step at the default thread count, its per-gradient relative-norm spread): the larger
    of the thread-count spread and the fp32-vs-fp64 error — the recipe of parity_util.oracle_with_spread."""
    from parity_util import _rel
    o = train_step(sd, x, eps, **kw)
    n0 = torch.get_num_threads()
    try:
        torch.set_num_threads(threads)
        o1 = train_step(sd, x, eps, **kw)
    finally:
        torch.set_num_threads(n0)
    sd64 = {k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()}
    o64 = train_step(sd64, x.double(), eps.double(), **kw)
    spread = {k: max(_rel(o["grads"][k], o1["grads"][k]), _rel(o["grads"][k], o64["grads"][k])) for k in o["grads"]}
    return o, spread


# ---- the golden cases (tests/golden/dipvae_*.npz, written by tests/golden/make_golden_dipvae.py)
CASES = ["dipvae_b16", "dipvae_b8"]


def case_inputs(meta):
    """(params, x, eps) from the recipe, checked against the fixture's SHA-256s."""
    D = meta["ctor"]["latent_dim"]
    sd = O.make_params(O.vanilla_param_spec(latent_dim=D), meta["seed"])
    x, eps = O.make_inputs(meta["batch"], D, meta["seed"])
    assert O.sha256_of([x]) == meta["x_sha"], "input recipe drifted"
    assert O.sha256_of([eps]) == meta["eps_sha"], "eps recipe drifted"
    assert O.sha256_of([sd[k] for k in sd]) == meta["params_sha"], "param recipe drifted"
    return sd, x, eps


def loss_kwargs(meta):
    """Keyword arguments of train_step / StepPlan(loss='dip') for a case (the reference
    constructor's defaults where the case leaves them out)."""
    kw = meta["ctor"]
    return dict(lambda_diag=kw.get("lambda_diag", 10.0), lambda_offdiag=kw.get("lambda_offdiag", 5.0))
