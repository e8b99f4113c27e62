"""MIWAE restated on the CPU oracle's functional pieces (oracle/vae_oracle.py), for the tests.

The reference's MIWAE (models/miwae.py) has the VanillaVAE network.  Its forward (:124-130) repeats
mu | log_var to [B, M, K, D], draws one eps of that shape and decodes the B*M*K latents in row-major
order (b, then m, then k: `.contiguous().view`, :105-106) — which is the oracle's IWAE forward at
S = M*K, so that is what runs here.  What is restated is the loss, :148-164: IWAE's self-normalised
weighting inside each group of K samples, averaged over the M estimates and the batch; the weights
are not detached.
`train_step` returns what oracle.vae_oracle.train_step returns (loss terms, gradients in the
reference layout, running statistics)."""
from collections import OrderedDict

import torch
from torch.nn import functional as F

from oracle import vae_oracle as O

TERMS = ("loss", "Reconstruction_Loss", "KLD")


def pre_bn_bias(name):
    """A conv / convT bias followed by train-mode BatchNorm: its gradient is analytically zero."""
    return name.endswith(".0.bias") and not name.startswith("final_layer.3")


def miwae_loss(recons, x, mu, log_var, M_N):
    """miwae.py:148-164.  recons [B,M,K,C,H,W], x [B,C,H,W], mu / log_var [B,M,K,D]."""
    B, M, K = recons.shape[:3]
    xr = x[:, None, None].expand(-1, M, K, -1, -1, -1)
    log_p_x_z = ((recons - xr) ** 2).flatten(3).mean(-1)
    kld_loss = -0.5 * torch.sum(1 + log_var - mu ** 2 - log_var.exp(), dim=3)
    log_weight = log_p_x_z + M_N * kld_loss
    weight = F.softmax(log_weight, dim=-1)
    loss = torch.mean(torch.mean(torch.sum(weight * log_weight, dim=-1), dim=-2), dim=0)
    return {"loss": loss, "Reconstruction_Loss": log_p_x_z.mean(), "KLD": -kld_loss.mean()}


def kld_rows(mulv):
    """kld_b of every row of mulv = [mu | log_var]."""
    D = mulv.shape[1] // 2
    mu, lv = mulv[:, :D], mulv[:, D:]
    return -0.5 * torch.sum(1 + lv - mu ** 2 - lv.exp(), dim=1)


def miwae_elbo64(sse, mulv, M, K, M_N, img, grouping="bmk"):
    """What vae_elbo_fwd (VAE_LOSS_MIWAE) computes, in fp64, from the per-row SSE [B*M*K] and
    mulv [B, 2D]: (out [4], per_img, head_coef, kl_coef), the coefficients by autograd of the loss.
    grouping: 'bmk' — the reference's (softmax over k inside row b*M*K + m*K + k); the two wrong ones a
    kernel could implement instead: 'all' — one softmax over an image's M*K rows (IWAE at S = M*K),
    'kmajor' — groups of rows m + k*M (the k index running slowest)."""
    sse = sse.detach().double().reshape(-1)
    mulv = mulv.detach().double()
    B = mulv.shape[0]
    mse = (sse / img).requires_grad_(True)
    kld = kld_rows(mulv).requires_grad_(True)
    lw = mse.view(B, M * K) + M_N * kld.view(B, 1)
    if grouping == "bmk":
        lw = lw.view(B, M, K)
    elif grouping == "all":
        lw = lw.view(B, 1, M * K)
    elif grouping == "kmajor":
        lw = lw.view(B, K, M).transpose(1, 2)
    else:
        raise ValueError(grouping)
    w = F.softmax(lw, dim=-1)
    loss = (w * lw).sum(-1).mean(-1).mean(0)
    g_mse, = torch.autograd.grad(loss, mse, retain_graph=True)
    # dL/dsse_r = g_r / img; the head backward's seed is dL/drecon = head_coef * (recon - x), so
    # head_coef = 2 g_r / img; kl_coef[r] = g_r * M_N (the row's share of dL/dkld_b)
    out = torch.stack([loss.detach(), mse.detach().mean(), -kld.detach().mean(), kld.detach().mean()])
    return out, mse.detach().clone(), g_mse * 2.0 / img, g_mse * M_N


def train_step(sd, x, eps, *, M_N, M, K, hidden_dims=None, training=True):
    """forward -> loss_function -> backward on a copy of ``sd`` (the dtype of ``sd`` / inputs).
    eps: [B, M*K, D] (or [B, M, K, D]), the one randn_like of miwae.py:121."""
    kinds = O._kinds_of("VanillaVAE", sd, hidden_dims)
    P = OrderedDict()
    for k, t in sd.items():
        t = t.detach().clone()
        if kinds[k] in O.TRAINABLE_KINDS:
            t.requires_grad_(True)
        P[k] = t
    stats = {}
    hd = list(hidden_dims or O.DEFAULT_HIDDEN)
    B, D = x.shape[0], eps.shape[-1]
    recon, mu_s, lv_s, z = O.iwae_forward(P, x, eps.reshape(B, M * K, D), hd, training, stats)
    recon6 = recon.view(B, M, K, *recon.shape[2:])
    ld = miwae_loss(recon6, x, mu_s.reshape(B, M, K, D), lv_s.reshape(B, M, K, D), M_N)
    ld["loss"].backward()
    grads = OrderedDict((k, (P[k].grad.detach().clone() if P[k].grad is not None else torch.zeros_like(P[k])))
                        for k in P if kinds[k] in O.TRAINABLE_KINDS)
    rows = recon.detach().reshape(B * M * K, *recon.shape[2:])
    per_row = ((rows - x.repeat_interleave(M * K, 0)) ** 2).mean(dim=[1, 2, 3])
    return dict(recon=rows, mu=mu_s[:, 0].detach(), log_var=lv_s[:, 0].detach(), z=z.detach(),
                loss={k: float(v.detach()) for k, v in ld.items()}, per_row_mse=per_row,
                per_img_mse=per_row.view(B, M * K).mean(1), grads=grads, running=stats)


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


# ---- the golden cases (tests/golden/miwae_*.npz, written by tests/golden/make_golden_miwae.py)
CASES = ["miwae_b4", "miwae_b2"]


def case_mk(meta):
    """(M, K) of a case (the reference constructor's defaults, 5 x 5, where the case leaves them out)."""
    return meta["ctor"].get("num_estimates", 5), meta["ctor"].get("num_samples", 5)


def case_inputs(meta):
    """(params, x, eps [B, M*K, D]) from the recipe, checked against the fixture's SHA-256s."""
    D = meta["ctor"]["latent_dim"]
    M, K = case_mk(meta)
    sd = O.make_params(O.vanilla_param_spec(latent_dim=D), meta["seed"])
    x, eps = O.make_inputs(meta["batch"], D, meta["seed"], samples=M * K)
    assert O.sha256_of([x]) == meta["x_sha"], "input recipe drifted"
    assert O.sha256_of([eps]) == meta["eps_sha"], "eps recipe drifted"
    assert O.sha256_of([sd[k] for k in sd]) == meta["params_sha"], "param recipe drifted"
    return sd, x, eps
