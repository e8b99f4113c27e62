"""The loss terms that couple the rows of a batch through the latents, beside reconstruction and KL:
InfoVAE's MMD (models/info_vae.py:128-229, vae_mmd_fwd) and DIP-VAE's covariance penalty
(models/dip_vae.py:125-164, vae_dip_fwd).  A training StepPlan whose loss has one holds it as
`plan.term` (TERMS: loss name -> class); everything the term needs lives here.

A term owns its buffers — `value` (the one-element loss-dict entry, written by vae_elbo_fwd from the
tile partials in `ws`) and `grad` (the term's unscaled gradient) — its argument struct `args` and
tile count `tiles`.  In a fused-loss plan its call is part of the forward (queue) and adds its share
of d[mu | log_var] itself; in a drop-in plan it runs at loss_function time (run, from
StepPlan.run_elbo) and the backward applies a copy of `grad` scaled by dL/dloss (seed / apply_seed,
models._HipELBO), next to the two seeds StepPlan.seed_fused switches on."""
from __future__ import annotations

import torch

from . import _lib as L

MMD_KINDS = {"imq": L.MMD_IMQ, "rbf": L.MMD_RBF}


class LatentTerm:
    name = None             # the term's loss-dict key
    before = None           # the key it goes in front of (None: last)
    fn = None               # the kernel that evaluates it
    recon_sum = False       # the loss's reconstruction term is the batch sum, not the mean
    prior = None            # a noise input of the term, for the step to fill or use_device_prior to draw

    def __init__(self, plan, args, grad: torch.Tensor, query, pad: int = 0):
        self.plan, self.args, self.grad = plan, args, grad
        self.value = torch.zeros(1, dtype=torch.float32, device=grad.device)
        nbytes, self.tiles = query(args)
        self.ws = torch.zeros(nbytes // 8 + pad, dtype=torch.float64, device=grad.device)
        args.workspace, args.workspace_bytes = self.ws.data_ptr(), self.ws.numel() * 8

    def queue(self, F):
        """Fused-loss plan: the call joins the forward and adds into dmulv itself."""
        if self.plan.fused_loss:
            self.args.dmulv = self.plan.dmulv.data_ptr()
            self.plan._add(F, self.fn, self.args)

    def fill_elbo(self, e):
        """What vae_elbo_fwd reads of the term (the partials travel in the mmd_* fields for every term)."""
        e.mmd_tiles, e.mmd_partials, e.mmd_out = self.tiles, self.ws.data_ptr(), self.value.data_ptr()

    def run(self, e, stream, **loss_kw):
        """Drop-in plan: the term of this forward — `grad` unscaled, the partials the loss adds."""
        L.call(self.fn, self.args, stream)

    def place(self, d: dict, value):
        """Put the term's entry where the reference's loss dict has it."""
        d[self.name] = value
        if self.before is not None:
            d[self.before] = d.pop(self.before)

    def seed(self):
        """What a repeated drop-in backward restarts from (apply_seed's first argument)."""
        return self.grad.clone()

    def apply_seed(self, seed, g_loss: torch.Tensor, stream):
        """dmulv += dL/dloss * the term's gradient.  dmulv is zero here (the step head or
        reset_backward) and the backward accumulates onto it."""
        raise NotImplementedError


class MmdTerm(LatentTerm):
    """The MMD of the step's latents (recomputed in fp32 from mu | log_var and eps) against a prior
    sample, right behind the reparameterization; `grad` is dmmd/dz.  The fused call's coefficient
    is a constant of the plan."""
    name, before, fn = "MMD", "KLD", "vae_mmd_fwd"          # info_vae.py:148: MMD before KLD

    def __init__(self, plan, *, alpha, reg_weight, kernel_type, latent_var, **_):
        B, D = plan.B, plan.net.latent_dim
        f32 = dict(dtype=torch.float32, device=plan.net.device)
        self.alpha, self.reg_weight = alpha, reg_weight
        self.prior = torch.zeros(B, D, **f32)       # an input, or drawn on the device (use_device_prior)
        self._scale = torch.zeros(1, **f32)         # drop-in backward: dL/dloss * mmd_coef
        a = L.MmdArgs(kind=MMD_KINDS[kernel_type], batch=B, latent=D, latent_var=latent_var)
        a.mulv, a.eps, a.prior = plan.mulv.data_ptr(), plan.eps.data_ptr(), self.prior.data_ptr()
        a.grad_scale = (alpha + reg_weight - 1.0) / (B * (B - 1)) if plan.fused_loss else 1.0
        grad = torch.zeros(B, D, **f32)
        a.dz = grad.data_ptr()
        super().__init__(plan, a, grad, L.mmd_workspace)

    def weights(self, e, beta: float, alpha: float, reg_weight: float):
        """The weights of info_vae.py:145-147 in vae_elbo_args."""
        B = self.plan.B
        e.recon_weight, e.kl_factor = beta, 1.0 - alpha
        e.mmd_coef = (alpha + reg_weight - 1.0) / (B * (B - 1))

    def fill_elbo(self, e):
        super().fill_elbo(e)
        self.weights(e, self.plan.beta, self.alpha, self.reg_weight)

    def run(self, e, stream, beta, alpha, reg_weight, prior=None, **_):
        if prior is not None:
            self.prior.copy_(prior.detach().reshape(self.prior.shape))
        self.weights(e, beta, alpha, reg_weight)
        super().run(e, stream)

    def seed(self):
        return self.grad.clone(), self.plan.elbo_args.mmd_coef

    def apply_seed(self, seed, g_loss, stream):
        """Through the reparameterization backward of (dL/dloss * mmd_coef) * dz (vae_mmd_reseed)."""
        p, (dz, coef) = self.plan, seed
        self.grad.copy_(dz)
        torch.mul(g_loss.reshape(1).to(self._scale), coef, out=self._scale)
        L.call("vae_mmd_reseed", p.B, p.net.latent_dim, self.grad.data_ptr(), self._scale.data_ptr(),
               p.mulv.data_ptr(), p.eps.data_ptr(), p.dmulv.data_ptr(), stream)

    def use_device_prior(self, step, seed):
        """Draw the prior sample of compute_mmd (torch.randn_like(z), info_vae.py:220) inside
        vae_mmd_fwd, every step: the generator of StepPlan.use_device_eps on another stream word, keyed
        by `seed` and the device step counter `step`; the draw is written to self.prior.  Works on both
        bottleneck routes."""
        a = self.args
        a.prior_gen, a.prior_step, a.prior_seed = 1, step.data_ptr(), seed & 0xFFFFFFFFFFFFFFFF
        self._prior_step = step                     # keep the counter alive with the plan
        return True


class DipTerm(LatentTerm):
    """The covariance penalty of the step's latent means, as soon as mu | log_var are final (it needs
    neither eps nor z); `grad` is d dip/d[mu | log_var].  The term's weight in the loss is 1, and the
    lambdas are the plan's."""
    name, fn, recon_sum = "DIP_Loss", "vae_dip_fwd", True   # dip_vae.py:161-164: DIP_Loss last; :141

    def __init__(self, plan, *, lambda_diag, lambda_offdiag, **_):
        B, D = plan.B, plan.net.latent_dim
        self.lambdas = (lambda_diag, lambda_offdiag)
        a = L.DipArgs(batch=B, latent=D, lambda_diag=lambda_diag, lambda_offdiag=lambda_offdiag, grad_scale=1.0)
        grad = torch.zeros(B, 2 * D, dtype=torch.float32, device=plan.net.device)
        a.mulv, a.dmulv_dip = plan.mulv.data_ptr(), grad.data_ptr()
        super().__init__(plan, a, grad, L.dip_workspace, pad=1)

    def apply_seed(self, seed, g_loss, stream):
        self.plan.dmulv.view(seed.shape).addcmul_(seed, g_loss.reshape(1, 1).to(seed))


TERMS = {"info": MmdTerm, "dip": DipTerm}
