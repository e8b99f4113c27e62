"""LogCoshVAE restated on the CPU oracle's functional pieces (oracle/vae_oracle.py), for the tests.

The reference's LogCoshVAE (models/logcosh_vae.py) has the VanillaVAE network, so the forward is the
oracle's vanilla_encode / reparameterize / vanilla_decode; what is restated here is its loss,
logcosh_vae.py:125-155, with the eps of reparameterize (:118) injected so a step is a function of its
inputs.  The reconstruction term comes in two forms:
  * `literal`: the reference's own expression, alpha*t + log(1 + exp(-2*alpha*t)) - log 2.  In fp32
    exp overflows to inf once -2*alpha*t > 88.7 (alpha = 100, the constructor default: t < -0.44);
  * `stable`:  a + (log1p(exp(-2*alpha*a)) - log 2) / alpha with a = |t| — what the kernel
    (vaehip.h vae_logcosh_loss) and models.LogCoshVAE evaluate: the same function, finite for every t.
`train_step` returns what oracle.vae_oracle.train_step returns (loss terms, gradients in the
reference layout, running statistics)."""
import math
from collections import OrderedDict

import torch
from torch.nn import functional as F

from oracle import vae_oracle as O

TERMS = ("loss", "Reconstruction_Loss", "KLD")


def pre_bn_bias(name):
    """A conv / convT bias followed by train-mode BatchNorm: its gradient is analytically zero."""
    return name.endswith(".0.bias") and not name.startswith("final_layer.3")


def recon_literal(t, alpha):
    """logcosh_vae.py:146-150, operation for operation."""
    r = alpha * t + torch.log(1. + torch.exp(- 2 * alpha * t)) - torch.log(torch.tensor(2.0))
    return (1. / alpha) * r.mean()


def logcosh_stable(t, alpha):
    """(1/alpha) log cosh(alpha t) per element, in the dtype of t."""
    a = t.abs()
    return a + (torch.log1p(torch.exp(-2.0 * alpha * a)) - math.log(2.0)) / alpha


def recon_stable(t, alpha):
    return logcosh_stable(t, alpha).mean()


def kld_rows(mu, log_var):
    return -0.5 * torch.sum(1 + log_var - mu ** 2 - log_var.exp(), dim=1)


def logcosh_loss(recons, x, mu, log_var, M_N, alpha=100.0, beta=10.0, form="literal"):
    """logcosh_vae.py:125-155 (form='stable': the reconstruction term in the stable form)."""
    t = recons - x
    recons_loss = recon_literal(t, alpha) if form == "literal" else recon_stable(t, alpha)
    kld_loss = torch.mean(kld_rows(mu, log_var), dim=0)
    loss = recons_loss + beta * M_N * kld_loss
    return {"loss": loss, "Reconstruction_Loss": recons_loss, "KLD": -kld_loss}


def terms64(recon, x, mulv, alpha, kl_weight):
    """What vae_logcosh_loss writes, in fp64 from fp32 tensors: (Reconstruction_Loss, kld, loss,
    tanh(alpha t) / N) with the stable form; mulv = [mu | log_var] or None."""
    t = recon.double() - x.double()
    rl = float(recon_stable(t, float(alpha)))
    seed = torch.tanh(float(alpha) * t) / t.numel()
    kld = 0.0
    if mulv is not None:
        D = mulv.shape[1] // 2
        kld = float(kld_rows(mulv[:, :D].double(), mulv[:, D:].double()).mean())
    return rl, kld, rl + float(kl_weight) * kld, seed


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
    ld = logcosh_loss(recon, x, mu, log_var, M_N, **loss_kw)
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


# ---- the golden cases (tests/golden/logcosh_*.npz, written by tests/golden/make_golden_logcosh.py)
CASES = ["logcosh_b8", "logcosh_b16"]


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
    """Keyword arguments of train_step / StepPlan(loss='logcosh') for a case (the reference
    constructor's defaults where the case leaves them out)."""
    kw = meta["ctor"]
    return dict(alpha=float(kw.get("alpha", 100.0)), beta=float(kw.get("beta", 10.0)))
